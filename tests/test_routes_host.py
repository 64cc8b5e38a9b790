"""The route log on the host (no GPU, and the library need not load): the CRW_ROUTE sites of csrc/ against tests/routes_ref.py and
DESIGN.md's table, every CRW_* environment switch of the sources against `routes_ref.SWITCHES` (a new switch fails here until
somebody decides how it is proven live), every live switch against the test that proves it, and include/crw_hip_routes.h against
the binding, the way tests/test_conv_chain_host.py holds crw_hip_chain.h."""
import ctypes
import glob
import os
import re

import routes_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radar-sounder-crw_amd", "csrc")
PY_SOURCES = (os.path.join(ROOT, "radar-sounder-crw_amd", "crw_hip.py"), os.path.join(ROOT, "radar-sounder-crw_amd", "imported", "labelprop.py"))


def _read(path):
    with open(path) as f:
        return f.read()


def _csrc():
    return {p: _read(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) +
                                        glob.glob(os.path.join(CSRC, "*.cpp")))}


def route_literals(sources):
    """every CRW_ROUTE("name") of the given {path: text}, in order (the macro's own definition takes `name`, no literal)"""
    return [m for text in sources.values() for m in re.findall(r'CRW_ROUTE\(\s*"([^"]*)"\s*\)', text)]


def switch_names(c_sources, py_sources):
    names = {m for text in c_sources.values() for m in re.findall(r'getenv\(\s*"(CRW_[A-Z0-9_]+)"', text)}
    names |= {m for text in py_sources.values() for m in re.findall(r'environ(?:\.get\(|\[)\s*"(CRW_[A-Z0-9_]+)"', text)}
    return names


def _design_table():
    """the rows `| \\`name\\` | selector | rule |` of DESIGN.md's route table"""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    start = text.index("## 8. The route log")
    end = text.find("\n## ", start + 1)
    return re.findall(r"^\| `([a-z0-9_.]+)` \|", text[start:end if end > 0 else None], flags=re.M)


def test_route_sites_equal_the_table_and_design():
    found = route_literals(_csrc())
    assert found, "no CRW_ROUTE site found"
    dup = sorted({n for n in found if found.count(n) > 1})
    assert not dup, f"a route name stands at more than one site: {dup}"
    assert len(set(rr.ROUTES)) == len(rr.ROUTES)
    assert set(found) == set(rr.ROUTES), sorted(set(found) ^ set(rr.ROUTES))
    assert all(re.fullmatch(r"[a-z0-9_]+\.[a-z0-9_]+", n) and len(n) < 100 for n in found)
    assert len(found) <= 256                                            # MAX_ROUTES of csrc/crw_common.h
    assert "constexpr int MAX_ROUTES = 256;" in _read(os.path.join(CSRC, "crw_common.h"))
    table = _design_table()
    assert len(set(table)) == len(table) and set(table) == set(rr.ROUTES), sorted(set(table) ^ set(rr.ROUTES))


def test_the_scan_notices_a_deleted_site_and_a_new_switch():
    """the two scans on doctored copies of the sources: one CRW_ROUTE line less, one getenv more"""
    src = _csrc()
    walk = os.path.join(CSRC, "walk.hip")
    less = dict(src)
    less[walk] = src[walk].replace('CRW_ROUTE("walk.fwd_gemm");', "", 1)
    assert less[walk] != src[walk] and set(route_literals(less)) == set(rr.ROUTES) - {"walk.fwd_gemm"}
    more = dict(src)
    more[walk] = src[walk] + '\nstatic const char *x = getenv("CRW_X");\n'
    py = {p: _read(p) for p in PY_SOURCES}
    assert switch_names(more, py) == set(rr.SWITCHES) | {"CRW_X"}


def test_every_switch_of_the_sources_is_decided():
    found = switch_names(_csrc(), {p: _read(p) for p in PY_SOURCES})
    assert found == set(rr.SWITCHES), sorted(found ^ set(rr.SWITCHES))
    allowed = ("CRW_CONV_STAMPS-only diagnostic", "the library path", "host-only batching knob", "the route log's own file name")
    for name, entry in rr.SWITCHES.items():
        if entry[0] == "none":
            assert entry[1].startswith(allowed), (name, entry[1])
        else:
            kind, routes, proof = entry
            assert kind == "routes" and routes and set(routes) <= set(rr.ROUTES), (name, routes)
    # a diagnostic that claims to be CRW_CONV_STAMPS-only is read between #ifdef CRW_CONV_STAMPS and #endif, nowhere else
    for name, entry in rr.SWITCHES.items():
        if entry[0] == "none" and entry[1] == rr.DIAG:
            for text in _csrc().values():
                guarded = "".join(re.findall(r"#ifdef CRW_CONV_STAMPS(.*?)#endif", text, flags=re.S))
                assert text.count(f'"{name}"') == guarded.count(f'"{name}"'), name


def _function_source(path, name):
    text = _read(os.path.join(ROOT, path))
    m = re.search(rf"^def {name}\(.*?(?=^(?:def |@pytest|class |[A-Z_]+ = )|\Z)", text, flags=re.M | re.S)
    assert m, f"{path} has no test {name}"
    return m.group(0)


def test_every_live_switch_has_its_proof():
    import test_variants
    rows = test_variants.VARIANTS
    assert all(isinstance(env, dict) and env and must_run and set(must_run) <= set(rr.ROUTES) for env, must_run, _, _, _ in rows)
    for name, entry in rr.SWITCHES.items():
        if entry[0] != "routes":
            continue
        _, routes, proof = entry
        if proof == rr.VARIANT:
            proven = {r for env, must_run, _, _, _ in rows if name in env for r in must_run}
            assert set(routes) <= proven, (name, "no VARIANTS row sets it and names", sorted(set(routes) - proven))
        else:
            path, test = proof.split("::")
            body = _function_source(path, test)
            assert name in body and ("routes()" in body or "took(hip" in body), (name, proof, "does not set the switch inside crw_hip.routes()")
            assert all(f'"{r}"' in body for r in routes), (name, proof, routes)
    named = {r for e in rr.SWITCHES.values() if e[0] == "routes" and e[2] == rr.VARIANT for r in e[1]}
    assert set(rr.VARIANT_ONLY) <= named and len(set(rr.VARIANT_ONLY)) == len(rr.VARIANT_ONLY)


def _declared():
    header = re.sub(r"/\*.*?\*/", "", _read(os.path.join(ROOT, "include", "crw_hip_routes.h")), flags=re.S)
    return dict(re.findall(r"\b(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header))


def test_routes_header_and_binding_agree():
    import crw_hip
    decls = _declared()
    assert set(decls) == set(crw_hip.ROUTES_SIGNATURES) == {"crw_routes_clear", "crw_routes_read"}
    assert not set(decls) & (set(crw_hip.SIGNATURES) | set(crw_hip.CHAIN_SIGNATURES) | set(crw_hip.RESTART_SIGNATURES))   # one header each
    for name, params in decls.items():
        res, args = crw_hip.ROUTES_SIGNATURES[name]
        assert res is ctypes.c_int, name
        want = [] if params.strip() == "void" else [ctypes.c_void_p if "*" in p else ctypes.c_int for p in params.split(",")]
        assert args == want, name                                          # type by type, in the header's order
    text = _read(os.path.join(ROOT, "include", "crw_hip.h"))
    assert "#define CRW_ABI_VERSION 8" in text and crw_hip.ABI_VERSION == 8  # added without a bump
    assert not any(name in text for name in decls)                        # outside crw_hip.h: tests/stale_ref.py's tables stand
    names = crw_hip.ROUTES_ENTRY_POINTS
    assert set(names) == set(decls) and crw_hip.OPTIONAL_ENTRY_POINTS["routes"] is names
    assert crw_hip.has_routes.__name__ == "has_routes" and callable(crw_hip.routes)
    rs = _read(os.path.join(CSRC, "routes.hip"))
    assert all(re.search(rf'extern "C" int {name}\(', rs) for name in decls)
    assert crw_hip.MAX_ROUTES == 256


def test_library_exports_and_counts_when_it_is_built(tmp_path):
    """where libcrw_hip.so stands (a build here, or `build()`): the entry points on the host, no GPU -- nothing has launched, so the
    table is empty, and clearing is harmless"""
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name in crw_hip.ROUTES_ENTRY_POINTS:
        assert hasattr(handle, name), f"{name} declared in crw_hip_routes.h but not exported"
    assert crw_hip.has_routes() is True
    with crw_hip.routes() as hit:
        pass
    assert hit == {} and isinstance(hit, dict)
    assert crw_hip.lib().crw_routes_read(None, None, 0) >= 0
