"""include/crw_hip_novelty.h (context novelty, a companion of include/crw_hip.h) against the binding and the library, the way
tests/test_restart_host.py holds crw_hip_restart.h: the declaration is exported and mirrored in `crw_hip.NOVELTY_SIGNATURES`, the
entry point forms the optional group `novelty`, and it is run over stale memory and between guard bands by
tests/test_novelty_gpu.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crw_hip_novelty.h")).read(), flags=re.S)
    return dict(re.findall(r"\b(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header))


def test_novelty_header_binding_and_library_agree():
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    decls = _declared()
    assert len(decls) == 1 and set(decls) == set(crw_hip.NOVELTY_SIGNATURES), set(decls) ^ set(crw_hip.NOVELTY_SIGNATURES)
    others = set(crw_hip.SIGNATURES) | set(crw_hip.CHAIN_SIGNATURES) | set(crw_hip.RESTART_SIGNATURES) | set(crw_hip.ROUTES_SIGNATURES)
    assert not set(decls) & others                                                          # one header each
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name, params in decls.items():
        assert hasattr(handle, name), f"{name} declared in crw_hip_novelty.h but not exported"
        res, args = crw_hip.NOVELTY_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == params.count(",") + 1, name
        kinds = [ctypes.c_void_p if "*" in p or "crw_stream_t" in p else ctypes.c_size_t if "size_t" in p else
                 ctypes.c_float if "float" in p else ctypes.c_int for p in params.split(",")]
        assert args == kinds, name                                                          # type by type, in the header's order
        assert getattr(crw_hip.lib(), name).argtypes == args
    text = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert "#define CRW_ABI_VERSION 8" in text and crw_hip.ABI_VERSION == 8                 # added without a bump
    assert not any(name in text for name in decls)


def test_the_novelty_entry_point_is_banded():
    """it takes device pointers; tests/test_novelty_gpu.py calls it by its C name under `run_twice` and `run_banded`"""
    text = open(os.path.join(ROOT, "tests", "test_novelty_gpu.py")).read()
    for name, params in _declared().items():
        assert "*" in params, name
        assert "run_banded" in text and "run_twice" in text and re.search(rf"\blib\.{name}\b", text), name


def test_novelty_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.NOVELTY_ENTRY_POINTS
    assert names and set(names) == set(crw_hip.NOVELTY_SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS["novelty"] is names
    assert crw_hip.has_novelty() is True and crw_hip._novelty_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "novelty", False)              # a library from before the entry point
    assert crw_hip.has_novelty() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._novelty_lib()
    assert all(name in str(err.value) for name in names)
