"""include/crw_hip_align.h (segment-centred features and the bias on the long-term keys, a companion of include/crw_hip.h) against the
binding and the library, the way tests/test_longmem_host.py holds crw_hip_longmem.h; the option checks of the host path
(`crw_hip`, `LabelPropVOS_CRW.propagate_all`, `utils.propagate`, `inference.segment`, `segment_sweep`, scripts/segment_all.py); and the
hand-over of the two options from the command line down to the binding, with stubs in place of the device.  No GPU."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    """{name: (result type, parameter text)} of the header's prototypes"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crw_hip_align.h")).read(), flags=re.S)
    return {name: (res, params) for res, name, params in re.findall(r"\b(int|size_t)\s+(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header)}


def test_align_header_binding_and_library_agree():
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    decls = _declared()
    assert set(decls) == set(crw_hip.ALIGN_SIGNATURES) == {"crw_center_normalize_ws_bytes", "crw_center_normalize", "crw_labelprop_topk_long_bias"}
    others = (crw_hip.SIGNATURES, crw_hip.CHAIN_SIGNATURES, crw_hip.RESTART_SIGNATURES, crw_hip.LONGMEM_SIGNATURES, crw_hip.NOVELTY_SIGNATURES)
    assert not any(set(decls) & set(o) for o in others)                                    # one header each
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name, (result, params) in decls.items():
        assert hasattr(handle, name), f"{name} declared in crw_hip_align.h but not exported"
        res, args = crw_hip.ALIGN_SIGNATURES[name]
        assert res is (ctypes.c_size_t if result == "size_t" else ctypes.c_int), name
        kinds = [ctypes.c_void_p if "*" in p or "crw_stream_t" in p else ctypes.c_size_t if "size_t" in p else
                 ctypes.c_float if "float" in p else ctypes.c_int for p in params.split(",")]
        assert args == kinds, name                                                          # type by type, in the header's order
        assert getattr(crw_hip.lib(), name).argtypes == args and getattr(crw_hip.lib(), name).restype is res
    # the biased lists take crw_labelprop_topk_long's arguments and the bias in front of the stream
    long_args = crw_hip.LONGMEM_SIGNATURES["crw_labelprop_topk_long"][1]
    assert crw_hip.ALIGN_SIGNATURES["crw_labelprop_topk_long_bias"][1] == long_args[:-1] + [ctypes.c_float] + long_args[-1:]
    text = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert "#define CRW_ABI_VERSION 8" in text and crw_hip.ABI_VERSION == 8                 # added without a bump
    assert not any(name in text for name in decls)
    src = open(os.path.join(ROOT, "radar-sounder-crw_amd", "csrc", "align.hip")).read()
    assert "atomic" not in src.replace("no atomics", "").replace("nothing is atomic", "")   # the sums are joined in a fixed order


def test_every_align_entry_point_is_banded():
    """each takes device pointers; tests/test_align_gpu.py calls it by its C name under `run_twice` and `run_banded`"""
    text = open(os.path.join(ROOT, "tests", "test_align_gpu.py")).read()
    for name, (_, params) in _declared().items():
        if name.endswith("_ws_bytes"):
            continue
        assert "*" in params, name
        assert "run_banded" in text and "run_twice" in text and re.search(rf"\blib\.{name}\b", text), name


def test_the_size_query_and_the_argument_checks_run_on_the_host():
    """what the entry points refuse before any launch (no GPU is touched: every call returns at its checks)"""
    import crw_hip
    lib = crw_hip.lib()
    assert crw_hip.has_align() is True
    q = lib.crw_center_normalize_ws_bytes
    assert q(100, 8, 2) == 2 * 4 * 8 * 8 + 8 and q(13000, 128, 2) == 2 * 64 * 128 * 8 + 8 and q(1, 1, 1) == 16     # ceil(rows / 32) slabs, 64 at most
    assert q(0, 8, 2) == q(8, 0, 2) == q(8, 8, 0) == 8
    EINVAL, EWORKSPACE = 1, 2
    p = ctypes.c_void_p(256)                                                                 # never dereferenced: the checks come first
    seg = lambda *b: (ctypes.c_int32 * len(b))(*b)
    call = lambda rows, C, dev, host, S, ws=p, nbytes=1 << 20, mean=None: lib.crw_center_normalize(p, rows, C, dev, host, S, ws, nbytes, p, mean, None)
    assert call(10, 4, None, seg(0, 10), 0) == EINVAL                                        # S < 1
    assert call(10, 4, None, None, 1) == EINVAL and call(10, 4, p, seg(0, 10), 1) == EINVAL  # exactly one of the two offset arguments
    assert call(10, 4, None, seg(1, 10), 1) == EINVAL and call(10, 4, None, seg(0, 9), 1) == EINVAL
    assert call(10, 4, None, seg(0, 7, 5, 10), 3) == EINVAL                                  # not monotone
    assert call(10, 4, None, seg(*range(0, 10)), 9) == EINVAL                                # more than 8 segments by value
    assert call(10, 4, p, None, 1025) == EINVAL and call(10, 4097, None, seg(0, 10), 1) == EINVAL
    assert call(10, 4, None, seg(0, 10), 1, mean=ctypes.c_void_p(260)) == EINVAL             # mean is fp64: 8-byte aligned
    assert call(10, 4, None, seg(0, 10), 1, nbytes=q(10, 4, 1) - 1) == EWORKSPACE
    bias = lambda b, **kw: lib.crw_labelprop_topk_long_bias(p, kw.get("T", 6), 5, 4, 2, kw.get("n_long", 2), 2, 0.1, 2, 2, p, p, 0, kw.get("route", 0),
                                                            b, None)
    for b in (float("nan"), float("inf"), -float("inf")):
        assert bias(b) == EINVAL
    assert bias(0.1, n_long=0) == EINVAL and bias(0.1, n_long=6) == EINVAL and bias(0.1, route=3) == EINVAL


def test_align_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.ALIGN_ENTRY_POINTS
    assert names and set(names) == set(crw_hip.ALIGN_SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS["align"] is names
    assert crw_hip.has_align() is True and crw_hip._align_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "align", False)       # a library from before the entry points
    assert crw_hip.has_align() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._align_lib()
    assert all(name in str(err.value) for name in names)


def test_the_binding_checks_the_options_before_the_library(monkeypatch):
    import crw_hip
    called = []
    monkeypatch.setattr(crw_hip, "_align_lib", lambda: called.append(1))
    for bad in ("centre", "mean", 1, ""):
        with pytest.raises(ValueError, match="memory_align must be None or 'center'"):
            crw_hip.check_memory_align(bad)
    assert crw_hip.check_memory_align(None) is None and crw_hip.check_memory_align("center") == "center"
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="memory_bias must be a finite number"):
            crw_hip.check_memory_bias(bad)
    assert crw_hip.check_memory_bias(0) == 0.0 and crw_hip.check_memory_bias(-0.25) == -0.25
    assert not called


class _Recorder:
    """stands in for `crw_hip.labelprop_topk` / `labelprop_gather`: remembers the top-k call, fills every later frame with class 1"""

    def __init__(self):
        self.topk = []

    def labelprop_topk(self, ehat, cxt, radius, temp, knn, **kw):
        self.topk.append(kw)
        F, N, _ = ehat.shape
        ff = kw["first_frame"]
        return torch.full((F - ff, knn, N), 1.0 / knn), torch.zeros(F - ff, knn, N, dtype=torch.int32)

    def labelprop_gather(self, seed, W, I, T, N, M, **kw):
        ff = kw["first_frame"]
        kw["L"][ff * N:] = torch.eye(M)[1]
        kw["pred"][:, ff:] = 1
        return kw["L"], kw["pred"]


def test_propagate_all_hands_the_bias_to_the_lists_and_refuses_it_without_a_bank(monkeypatch):
    import crw_hip
    from imported.labelprop import LabelPropVOS_CRW
    T, N, C, M, B = 6, 5, 4, 3, 2
    rec = _Recorder()
    monkeypatch.setattr(crw_hip, "labelprop_topk", rec.labelprop_topk)
    monkeypatch.setattr(crw_hip, "labelprop_gather", rec.labelprop_gather)
    feats, seed = torch.zeros(T, N, C), torch.zeros(N)
    mem = (torch.zeros(B, N, C), torch.zeros(B, N, dtype=torch.int8))
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding"))
    lp.propagate_all(feats, seed, M, memory=mem)
    lp.propagate_all(feats, seed, M, memory=mem, memory_bias=0.0)
    lp.propagate_all(feats, seed, M, memory=mem, memory_bias=0.1)
    lp.propagate_all(feats, None, M, memory=mem, memory_bias=-0.05)
    assert ["long_bias" in kw for kw in rec.topk] == [False, False, True, True]             # 0: the call as it is without the option
    assert rec.topk[2]["long_bias"] == 0.1 and rec.topk[2]["n_long"] == B + 1 and rec.topk[3]["long_bias"] == -0.05 and rec.topk[3]["n_long"] == B
    with pytest.raises(ValueError, match="memory_bias needs memory"):
        lp.propagate_all(feats, seed, M, memory_bias=0.1)
    with pytest.raises(ValueError, match="finite"):
        lp.propagate_all(feats, seed, M, memory=mem, memory_bias=float("nan"))
    assert len(rec.topk) == 4


def _synthetic_case():
    from dataset import RGDataset
    from test_confidence import Flatten
    H, Wd, T, patch, overlap = 48, 160, 5, (16, 16), (0, 0)
    ds = RGDataset.synthetic(H, Wd, T, patch, overlap)
    seg = (torch.arange(H)[:, None] * 3 // H).expand(H, Wd).contiguous().to(torch.int8)
    return ds, seg, Flatten(), T, patch, overlap


def test_propagate_centres_the_two_segments_and_passes_the_bias_on(monkeypatch):
    """`utils.propagate`: with memory_align='center' the encoder's raw output goes through `crw_hip.center_normalize` with the
    segments [0, B * N, (B + T) * N] (here on its CPU route) where it otherwise goes through `crw_hip.normalize`"""
    import crw_hip
    import utils
    from imported.labelprop import LabelPropVOS_CRW
    ds, seg, enc, T, patch, overlap = _synthetic_case()
    bank = utils.bank_from_columns(ds, seg, [0, 32, 70])
    seq = ds[0]
    N = seq.shape[1]
    seen = []
    real = crw_hip.center_normalize
    monkeypatch.setattr(crw_hip, "center_normalize", lambda emb, segments, **kw: seen.append(("center", list(segments))) or real(emb, segments, **kw))
    monkeypatch.setattr(crw_hip, "normalize", lambda emb: seen.append(("plain",)) or torch.nn.functional.normalize(emb, dim=-1))
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding"))
    got = []

    def propagate_all(feats, seed, nclasses, **kw):
        got.append(dict(feats=feats, **kw))
        return torch.zeros(N, T), torch.zeros(T * N, nclasses)

    monkeypatch.setattr(lp, "propagate_all", propagate_all)
    monkeypatch.setattr(crw_hip, "xent_metric", lambda feats: torch.zeros(N, T - 1))     # the device work around the propagation
    monkeypatch.setattr(utils, "column_diffs_async", lambda xent: None)
    monkeypatch.setattr(utils, "change_point", lambda xent, diffs=None: None)
    run = lambda **kw: utils.propagate(seq, seg[:, :16], enc, lp, 3, False, False, **kw)
    pred, xent, change = run(memory=bank, memory_align="center", memory_bias=0.1)
    assert pred.shape == (N, T) and change is None
    assert seen == [("center", [0, 3 * N, (3 + T) * N])] and got[0]["memory_bias"] == 0.1
    mem_feats, feats = got[0]["memory"][0], got[0]["feats"]
    assert mem_feats.shape[0] == 3 and feats.shape[0] == T
    raw = enc(torch.cat([bank.patches, seq]).reshape(-1, 16, 16).unsqueeze(1)).reshape(3 + T, N, -1).float()
    for part, rows in ((mem_feats, raw[:3]), (feats, raw[3:])):          # each segment centred by its own mean, then normalised
        y = rows.double() - rows.double().reshape(-1, rows.shape[-1]).mean(0)
        assert torch.allclose(part.double(), y / y.norm(dim=-1, keepdim=True).clamp_min(1e-12), atol=1e-6)
    del seen[:], got[:]
    run(memory=bank)
    assert seen == [("plain",)] and "memory_bias" not in got[0]                  # without the options the call is what it was
    for kw, msg in ((dict(memory_align="center"), "need memory"), (dict(memory_bias=0.1), "need memory"),
                    (dict(memory=bank, memory_align="mean"), "memory_align must be None or 'center'"),
                    (dict(memory=bank, memory_bias=float("inf")), "finite")):
        with pytest.raises(ValueError, match=msg):
            run(**kw)


def test_segment_hands_the_same_settings_to_both_passes_and_refuses_what_it_must(monkeypatch, capsys):
    import inference as crw_inference
    import utils
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    ds, seg, enc, T, patch, overlap = _synthetic_case()
    capsys.readouterr()
    calls = []

    def stub(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, confidence=None, memory=None, **kw):
        calls.append(dict(use_last=use_last, memory=memory, kw=kw))
        Tn, N = seq.shape[:2]
        return (torch.zeros(N, Tn), torch.zeros(N, max(Tn - 1, 0)), None)

    monkeypatch.setattr(crw_inference, "propagate", stub)
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding"))
    bank = utils.bank_from_columns(ds, seg, [0, 32])
    run = lambda **kw: crw_inference.segment(ds, seg, enc, lp, 3, T, patch, overlap, device="cpu", dataset_id=0, **kw)
    out = run(use_last=True, memory=bank, memory_align="center", memory_bias=0.1)
    assert out["memory_align"] == "center" and out["memory_bias"] == 0.1 and out["memory_traces"] == 2
    assert calls and {c["use_last"] for c in calls} == {False, True}
    assert all(c["kw"].get("memory_align") == "center" and c["kw"].get("memory_bias") == 0.1 and c["memory"] is bank for c in calls)
    del calls[:]
    plain = run(use_last=True, memory=bank)
    assert plain["memory_align"] is None and plain["memory_bias"] == 0.0
    assert calls and not any("memory_align" in c["kw"] or "memory_bias" in c["kw"] for c in calls)     # the calls are what they were
    del calls[:]
    none = run(use_last=True)
    assert "memory_align" not in none and "memory_bias" not in none
    # refused with a message: either option without a bank, an unknown alignment; unchanged: sweeps, suggest, restart
    for kw, msg in ((dict(memory_align="center"), "memory_align and memory_bias need memory"), (dict(memory_bias=0.1), "need memory"),
                    (dict(memory=bank, memory_align="whiten"), "memory_align must be None or 'center'"),
                    (dict(memory=bank, memory_bias=float("nan")), "finite"),
                    (dict(memory=bank, memory_align="center", suggest=2), "memory and suggest"),
                    (dict(memory=bank, memory_bias=0.1, anchors=(seg, [16]), anchor_context="restart"), "memory and anchor_context='restart'")):
        with pytest.raises(ValueError, match=msg):
            run(**kw)
    sweep = LabelPropSweep(2, [2], [0.1], [2], context="sliding")
    for kw in (dict(memory=bank), dict(memory=bank, memory_align="center"), dict(memory_bias=0.1)):
        with pytest.raises(ValueError, match="memory is not offered in segment_sweep"):
            crw_inference.segment_sweep(ds, seg, enc, sweep, 3, T, patch, overlap, device="cpu", **kw)


def test_segment_all_flags_reach_segment(monkeypatch, capsys, tmp_path):
    """scripts/segment_all.py: the flag checks, what `inference.segment` is given, the printed line and the json keys"""
    import inference as crw_inference
    from test_confidence import _cli, Flatten
    cli = _cli()
    parse = cli.get_args_parser().parse_args
    base = ["--synthetic", "48", "160", "--seq_length", "5", "--patch_size", "16", "16", "--overlap", "0", "0", "--dataset", "0", "-c", "2", "-r", "2",
            "-k", "2", "-t", "0.1", "--model", "0"]
    for extra, msg in ((["--memory_align", "center"], "need --memory_cols or --memory_bank"),
                       (["--memory_bias", "0.1"], "need --memory_cols or --memory_bank"),
                       (["--context", "sliding", "--memory_cols", "3", "--memory_bias", "nan"], "finite")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_memory_flags(cli.with_defaults(parse(base + extra)))
    with pytest.raises(SystemExit):
        parse(base + ["--memory_align", "mean"])                                  # argparse: 'center' is the one choice
    capsys.readouterr()
    given = []
    real = crw_inference.segment
    monkeypatch.setattr(crw_inference, "segment", lambda *a, **kw: given.append(kw) or real(*a, **kw))
    seen = []

    def stub(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, confidence=None, memory=None, **kw):
        seen.append(kw)
        Tn, N = seq.shape[:2]
        return (torch.zeros(N, Tn), torch.zeros(N, max(Tn - 1, 0)), None)

    monkeypatch.setattr(crw_inference, "propagate", stub)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    js = tmp_path / "r.json"
    common = ["--context", "sliding", "--memory_cols", "3", "40", "--output_folder", str(tmp_path / "out"), "--report_json", str(js)]
    cli.main(parse(base + common + ["--memory_align", "center", "--memory_bias", "0.1"]))
    text = capsys.readouterr().out
    assert "memory_align='center'" in text and "memory_bias=0.1" in text
    assert given[-1]["memory_align"] == "center" and given[-1]["memory_bias"] == 0.1
    assert seen and all(kw.get("memory_align") == "center" and kw.get("memory_bias") == 0.1 for kw in seen)
    d = json.load(open(js))
    assert d["memory_align"] == "center" and d["memory_bias"] == 0.1 and d["memory_traces"] == 2
    del seen[:]
    cli.main(parse(base + common))                                                # a bank without the two flags: as it was
    text = capsys.readouterr().out
    assert "memory_align" not in text and "memory_bias" not in text
    assert "memory_align" not in given[-1] and "memory_bias" not in given[-1] and not any("memory_align" in kw or "memory_bias" in kw for kw in seen)
    d = json.load(open(js))
    assert d["memory_align"] is None and d["memory_bias"] == 0.0
    cli.main(parse(base + ["--output_folder", str(tmp_path / "out"), "--report_json", str(js)]))
    assert "memory_align" not in json.load(open(js))
