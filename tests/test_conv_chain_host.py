"""include/crw_hip_chain.h (the conv-trunk chain, a companion of include/crw_hip.h) against the binding and the library, the way
tests/test_host.py holds crw_hip.h: every declaration is exported and mirrored in `crw_hip.CHAIN_SIGNATURES`, the entry points form
the optional group `conv_chain`, and each one is run over stale memory and between guard bands by tests/test_conv_chain_gpu.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crw_hip_chain.h")).read(), flags=re.S)
    return dict(re.findall(r"\b(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header))


def test_chain_header_binding_and_library_agree():
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    decls = _declared()
    assert decls and set(decls) == set(crw_hip.CHAIN_SIGNATURES), set(decls) ^ set(crw_hip.CHAIN_SIGNATURES)
    assert not set(decls) & set(crw_hip.SIGNATURES)                      # one header each
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name, params in decls.items():
        assert hasattr(handle, name), f"{name} declared in crw_hip_chain.h but not exported"
        assert len(crw_hip.CHAIN_SIGNATURES[name][1]) == params.count(",") + 1, name
    assert crw_hip.lib().crw_enc_conv_fwd_chain.argtypes == crw_hip.CHAIN_SIGNATURES["crw_enc_conv_fwd_chain"][1]


def test_every_chain_entry_point_is_banded():
    """each takes device pointers; tests/test_conv_chain_gpu.py calls it by its C name under `run_twice` and `run_banded`"""
    text = open(os.path.join(ROOT, "tests", "test_conv_chain_gpu.py")).read()
    for name, params in _declared().items():
        assert "*" in params, name
        assert "run_banded" in text and "run_twice" in text and re.search(rf"\blib\.{name}\b", text), name


def test_chain_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.CONV_CHAIN_ENTRY_POINTS
    assert names and set(names) == set(crw_hip.CHAIN_SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS["conv_chain"] is names
    assert crw_hip.has_conv_chain() is True and crw_hip._conv_chain_lib() is crw_hip.lib()
    monkeypatch.delenv("CRW_CONV_CHAIN", raising=False)
    assert crw_hip.conv_chain_on() is True
    monkeypatch.setenv("CRW_CONV_CHAIN", "0")
    assert crw_hip.conv_chain_on() is False
    monkeypatch.delenv("CRW_CONV_CHAIN")
    monkeypatch.setitem(crw_hip._present, "conv_chain", False)           # a library from before the chain: per-layer, not an error
    assert crw_hip.has_conv_chain() is False and crw_hip.conv_chain_on() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._conv_chain_lib()
    assert all(name in str(err.value) for name in names)
