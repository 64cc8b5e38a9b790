"""include/crw_hip_reach.h (one confusion matrix per group of columns, a companion of include/crw_hip.h) against the binding and the
library, the way tests/test_align_host.py holds crw_hip_align.h, and what the entry point refuses before any launch.  No GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"crw_confusion_grouped_ws_bytes", "crw_confusion_grouped"}


def _declared():
    """{name: (result type, parameter text)} of the header's prototypes"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crw_hip_reach.h")).read(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t)\s+(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header)}


def test_reach_header_binding_and_library_agree():
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    decls = _declared()
    assert set(decls) == set(crw_hip.REACH_SIGNATURES) == NAMES
    others = (crw_hip.SIGNATURES, crw_hip.CHAIN_SIGNATURES, crw_hip.RESTART_SIGNATURES, crw_hip.LONGMEM_SIGNATURES, crw_hip.NOVELTY_SIGNATURES,
              crw_hip.ALIGN_SIGNATURES, crw_hip.ROUTES_SIGNATURES)
    assert not any(set(decls) & set(o) for o in others)                                    # one header each
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name, (result, params) in decls.items():
        assert hasattr(handle, name), f"{name} declared in crw_hip_reach.h but not exported"
        res, args = crw_hip.REACH_SIGNATURES[name]
        assert res is (ctypes.c_size_t if result == "size_t" else ctypes.c_int), name
        kinds = [ctypes.c_void_p if "*" in p or "crw_stream_t" in p else ctypes.c_size_t if "size_t" in p else ctypes.c_int
                 for p in params.split(",")]
        assert args == kinds, name                                                          # type by type, in the header's order
        assert getattr(crw_hip.lib(), name).argtypes == args and getattr(crw_hip.lib(), name).restype is res
    text = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert "#define CRW_ABI_VERSION 8" in text and crw_hip.ABI_VERSION == 8                 # added without a bump
    assert not any(name in text for name in decls)                                          # crw_hip.h declares neither
    header = open(os.path.join(ROOT, "include", "crw_hip_reach.h")).read()
    assert "#define CRW_REACH_MAX_GROUPS 64" in header and crw_hip.REACH_MAX_GROUPS == 64
    src = open(os.path.join(ROOT, "radar-sounder-crw_amd", "csrc", "reach.hip")).read()
    assert '#include "labelmap.h"' in src and "code_f32" in src                            # labelmap.h's loaders and codes
    assert not re.search(r"atomic\w*\(\s*&?\s*c\.", src) and "CRW_ROUTE(" not in src and "getenv" not in src   # LDS atomics only; one route


def test_the_entry_point_is_banded():
    """tests/test_reach_gpu.py calls it by its C name under `run_twice` and `run_banded`"""
    text = open(os.path.join(ROOT, "tests", "test_reach_gpu.py")).read()
    assert "run_banded" in text and "run_twice" in text and re.search(r"\blib\.crw_confusion_grouped\b", text)


def test_the_size_query_and_the_argument_checks_run_on_the_host():
    """what the entry point refuses before any launch (no GPU is touched: every call returns at its checks)"""
    import crw_hip
    lib = crw_hip.lib()
    assert crw_hip.has_reach() is True
    q = lib.crw_confusion_grouped_ws_bytes
    # per strip of 64 columns: groups * K * K counts, 4 drop counts and groups confidence sums, 8 bytes each
    assert q(410, 24576, 5, 12) == 384 * (12 * 25 + 4 + 12) * 8 and q(7, 33, 16, 64) == 1 * (64 * 256 + 4 + 64) * 8 and q(1, 65, 2, 1) == 2 * 9 * 8
    assert q(0, 100, 5, 12) == q(100, 0, 5, 12) == 0
    assert q(10, 10, 1, 1) == q(10, 10, 17, 1) == q(10, 10, 5, 0) == q(10, 10, 5, 65) == q(-1, 10, 5, 1) == q(10, -1, 5, 1) == 0
    EINVAL, EWORKSPACE, F32, I8 = 1, 2, 0, 1
    p = ctypes.c_void_p(256)                                                                 # never dereferenced: the checks come first
    args = dict(gt=p, dg=F32, pred=p, dp=I8, aux=None, da=I8, conf=None, rows=10, cols=20, ld=20, grp=p, groups=12, K=5, ig=-1, ip=-1, ia=-1,
                counts=p, conf_sum=None, dropped=p, ws=p, nbytes=1 << 20)
    call = lambda **kw: lib.crw_confusion_grouped(*{**args, **kw}.values(), None)
    for bad in (dict(K=1), dict(K=17), dict(groups=0), dict(groups=65), dict(rows=-1), dict(cols=-1), dict(ld=19), dict(dg=2), dict(dp=-1),
                dict(aux=p, da=7), dict(gt=None), dict(pred=None), dict(grp=None), dict(counts=None), dict(dropped=None), dict(ws=None),
                dict(conf=p), dict(conf_sum=p),                                              # conf_sum is NULL exactly when conf is
                dict(ig=-2), dict(ip=-2), dict(ia=-2), dict(ia=4),                           # ignore_aux without aux
                dict(gt=ctypes.c_void_p(258)), dict(conf=ctypes.c_void_p(258), conf_sum=p), dict(counts=ctypes.c_void_p(260)),
                dict(dropped=ctypes.c_void_p(260)), dict(conf=p, conf_sum=ctypes.c_void_p(260)), dict(ws=ctypes.c_void_p(260))):
        assert call(**bad) == EINVAL, bad
    assert call(nbytes=q(10, 20, 5, 12) - 1) == EWORKSPACE
    assert call(pred=ctypes.c_void_p(257), rows=-1) == EINVAL                                # (an int8 operand may sit at any address)


def test_reach_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.REACH_ENTRY_POINTS
    assert names and set(names) == set(crw_hip.REACH_SIGNATURES) == NAMES and crw_hip.OPTIONAL_ENTRY_POINTS["reach"] is names
    assert crw_hip.has_reach() is True and crw_hip._reach_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "reach", False)       # a library from before the entry points
    assert crw_hip.has_reach() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._reach_lib()
    assert all(name in str(err.value) for name in names)
