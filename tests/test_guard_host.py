"""include/crw_hip_guard.h (the guarded Adam step, a companion of include/crw_hip.h) against the binding and the library, the way
tests/test_align_host.py holds crw_hip_align.h: every declaration is exported and mirrored in `crw_hip.GUARD_SIGNATURES`, the control
block's layout in the binding and in tests/guard_ref.py is the header's, and what the entry point refuses before any launch.  No GPU."""
import ctypes
import os
import re
import struct

import pytest
import torch

import guard_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crw_hip_guard.h")


def _declared():
    """{name: (result type, parameter text)} of the header's prototypes"""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t)\s+(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header)}


def test_guard_header_binding_and_library_agree():
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    decls = _declared()
    assert set(decls) == set(crw_hip.GUARD_SIGNATURES) == {"crw_adam_guard_ws_bytes", "crw_adam_step_guarded"}
    others = (crw_hip.SIGNATURES, crw_hip.CHAIN_SIGNATURES, crw_hip.RESTART_SIGNATURES, crw_hip.LONGMEM_SIGNATURES, crw_hip.NOVELTY_SIGNATURES,
              crw_hip.ALIGN_SIGNATURES, crw_hip.REACH_SIGNATURES, crw_hip.SWEEPMEM_SIGNATURES, crw_hip.ROUTES_SIGNATURES)
    assert not any(set(decls) & set(o) for o in others)                                    # one header each
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name, (result, params) in decls.items():
        assert hasattr(handle, name), f"{name} declared in crw_hip_guard.h but not exported"
        res, args = crw_hip.GUARD_SIGNATURES[name]
        assert res is (ctypes.c_size_t if result == "size_t" else ctypes.c_int), name
        kinds = [ctypes.c_void_p if "*" in p or "crw_stream_t" in p else ctypes.c_size_t if "size_t" in p else
                 ctypes.c_float if "float" in p else ctypes.c_long if re.search(r"\blong\b", p) else ctypes.c_int for p in params.split(",")]
        assert args == kinds, name                                                          # type by type, in the header's order
        assert getattr(crw_hip.lib(), name).argtypes == args and getattr(crw_hip.lib(), name).restype is res
    # crw_adam_step's arguments, then max_norm, ctl, ws and its size in front of the stream
    plain = crw_hip.SIGNATURES["crw_adam_step"][1]
    assert crw_hip.GUARD_SIGNATURES["crw_adam_step_guarded"][1] == plain[:-1] + [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + plain[-1:]
    text = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert "#define CRW_ABI_VERSION 8" in text and crw_hip.ABI_VERSION == 8                 # added without a bump
    assert not any(name in text for name in decls)                                          # tests/stale_ref.py's tables stand
    src = open(os.path.join(ROOT, "radar-sounder-crw_amd", "csrc", "guard.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")                                    # the sums are joined in a fixed order
    assert "asm" not in src and "CRW_ROUTE(" not in src                                     # plain C++; one route, so no name in the log
    assert all(re.search(rf'extern "C" (?:int|size_t) {name}\(', src) for name in decls)
    names = crw_hip.GUARD_ENTRY_POINTS
    assert set(names) == set(decls) and crw_hip.OPTIONAL_ENTRY_POINTS["guard"] is names and crw_hip.has_guard.__name__ == "has_guard"


def test_the_entry_point_is_banded_and_takes_no_host_pointer():
    """tests/test_guard_gpu.py calls it by its C name under `run_twice` and `run_banded`; the header calls every pointer a device one"""
    text = open(os.path.join(ROOT, "tests", "test_guard_gpu.py")).read()
    _, params = _declared()["crw_adam_step_guarded"]
    assert params.count("*") == 6
    assert "run_banded" in text and "run_twice" in text and re.search(r"\blib\.crw_adam_step_guarded\b", text)
    words = open(HEADER).read()
    assert "HOST pointer" not in words and "DEVICE memory" in words


def test_ctl_layout_in_the_binding_is_the_headers():
    """the header's table `offset  type  name` against GUARD_CTL_FORMAT / GUARD_CTL_FIELDS of the binding and tests/guard_ref.py"""
    import crw_hip
    text = open(HEADER).read()
    rows = re.findall(r"^ \*\s+(\d+)\s+(int64|double|float|int32)\s+([a-z_]+)\b", text, flags=re.M)
    assert [(int(o), t, n) for o, t, n in rows] == [(0, "int64", "applied"), (8, "int64", "skipped"), (16, "double", "norm"), (24, "float", "scale"),
                                                    (28, "int32", "last_applied")]
    assert re.search(r"^ \*\s+32\s+\.\.\.\s+reserved", text, flags=re.M) and "#define CRW_GUARD_CTL_BYTES 64" in text
    code = {"int64": "q", "double": "d", "float": "f", "int32": "i"}
    fmt = "<" + "".join(code[t] for _, t, _ in rows)
    assert crw_hip.GUARD_CTL_FORMAT == fmt == gr.CTL_FORMAT and crw_hip.GUARD_CTL_BYTES == gr.CTL_BYTES == 64
    assert crw_hip.GUARD_CTL_FIELDS == tuple(n for _, _, n in rows)
    offs, at = {}, 0
    for _, t, n in rows:                                            # natural alignment, no padding: the offsets the header prints
        size = struct.calcsize("<" + code[t])
        assert at % size == 0
        offs[n], at = at, at + size
    assert offs == {n: int(o) for o, _, n in rows} == {k: v for k, v in gr.CTL_OFFSETS.items() if k != "reserved"} and at == gr.CTL_OFFSETS["reserved"] == 32
    assert f"#define CRW_GUARD_BLOCK_ELEMS {gr.BLOCK_ELEMS}" in text
    raw = struct.pack(fmt, 7, 2, 1.5, 0.25, 1).ljust(64, b"\0")
    want = dict(applied=7, skipped=2, norm=1.5, scale=0.25, last_applied=1)
    assert crw_hip.guard_ctl_unpack(raw) == want and crw_hip.guard_ctl_unpack(torch.tensor(list(raw), dtype=torch.uint8)) == want
    ref = gr.GuardRef([0.0])
    ref.ctl.update(want)
    assert ref.ctl_bytes() == raw
    with pytest.raises(ValueError, match="64 bytes"):
        crw_hip.guard_ctl_unpack(raw[:32])


def test_the_size_query_and_the_argument_checks_run_on_the_host():
    """what the entry point refuses before any launch (no GPU is touched: every call returns at its checks)"""
    import crw_hip
    lib = crw_hip.lib()
    assert crw_hip.has_guard() is True
    q = lib.crw_adam_guard_ws_bytes
    assert [q(n) for n in (0, 1, 4096, 4097, 3 * 4096 + 3, 263088, 4971468)] == [16, 24, 24, 32, 48, 65 * 8 + 16, 1214 * 8 + 16]
    assert crw_hip.adam_guard_ws_bytes(4097) == 32
    EINVAL, EWORKSPACE = 1, 2
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)           # never dereferenced: the checks come first

    def call(n=100, step=1, b1=0.9, b2=0.999, max_norm=0.0, ptrs=(p, p, p, p), ctl=p, ws=p, nbytes=1 << 20):
        return lib.crw_adam_step_guarded(*ptrs, n, 1e-3, b1, b2, 1e-8, step, max_norm, ctl, ws, nbytes, None)

    # whatever crw_adam_step refuses
    assert call(n=0) == EINVAL and call(step=0) == EINVAL and call(b1=1.0) == EINVAL and call(b2=-0.1) == EINVAL and call(b1=float("nan")) == EINVAL
    for k in range(4):
        assert call(ptrs=tuple(None if i == k else p for i in range(4))) == EINVAL
        assert call(ptrs=tuple(ctypes.c_void_p(4104) if i == k else p for i in range(4))) == EINVAL      # 8-byte, not 16-byte aligned
        plain = lib.crw_adam_step(*tuple(None if i == k else p for i in range(4)), 100, 1e-3, 0.9, 0.999, 1e-8, 1, None)
        assert plain == EINVAL
    # its own: the bound, the control block, the workspace
    assert call(max_norm=-1.0) == EINVAL and call(max_norm=float("nan")) == EINVAL and call(max_norm=-float("inf")) == EINVAL
    assert call(ctl=None) == EINVAL and call(ctl=odd) == EINVAL and call(ws=None) == EINVAL and call(ws=odd) == EINVAL
    assert call(nbytes=q(100) - 1) == EWORKSPACE and call(n=4097, nbytes=q(4097) - 1) == EWORKSPACE and call(nbytes=0) == EWORKSPACE
    assert call(max_norm=-1.0, nbytes=0) == EINVAL                  # the caller's data first


def test_guard_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.GUARD_ENTRY_POINTS
    assert crw_hip.has_guard() is True and crw_hip._guard_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "guard", False)         # a library from before the entry points
    assert crw_hip.has_guard() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._guard_lib()
    assert all(name in str(err.value) for name in names)


def test_the_binding_checks_the_bound_before_the_library(monkeypatch):
    import crw_hip
    called = []
    monkeypatch.setattr(crw_hip, "_guard_lib", lambda: called.append(1))
    for bad in (-1, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="max_grad_norm must be None or a number >= 0"):
            crw_hip.check_max_norm(bad)
    assert crw_hip.check_max_norm(None) == 0.0 and crw_hip.check_max_norm(2) == 2.0 and crw_hip.check_max_norm(float("inf")) == float("inf")
    t = torch.zeros(8)
    with pytest.raises(ValueError, match="max_grad_norm"):
        crw_hip.adam_step_guarded(t, t, t, t, 1, 1e-3, torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), max_norm=-2)
    with pytest.raises(ValueError, match="ctl must hold 64 bytes"):
        crw_hip.adam_step_guarded(t, t, t, t, 1, 1e-3, torch.zeros(32, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))
    assert not called
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # and a host tensor is refused like everywhere else
        crw_hip.adam_step_guarded(t, t, t, t, 1, 1e-3, torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))
