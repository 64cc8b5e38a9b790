"""include/crw_hip_longmem.h (the sliding rule with a bank of long-term frames, a companion of include/crw_hip.h) against the binding
and the library, the way tests/test_restart_host.py holds crw_hip_restart.h; the option checks of the host path (`crw_hip`,
`LabelPropVOS_CRW.propagate_all`, `utils.propagate`, `inference.segment`, `segment_sweep`, scripts/segment_all.py); and the hand-over
-- anchors moved B frames down, outputs cut to the item, the same bank in both passes -- with stubs in place of the device.  No GPU."""
import ctypes
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crw_hip_longmem.h")).read(), flags=re.S)
    return dict(re.findall(r"\b(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header))


def test_longmem_header_binding_and_library_agree():
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    decls = _declared()
    assert len(decls) == 2 and set(decls) == set(crw_hip.LONGMEM_SIGNATURES), set(decls) ^ set(crw_hip.LONGMEM_SIGNATURES)
    assert not set(decls) & (set(crw_hip.SIGNATURES) | set(crw_hip.CHAIN_SIGNATURES) | set(crw_hip.RESTART_SIGNATURES))   # one header each
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name, params in decls.items():
        assert hasattr(handle, name), f"{name} declared in crw_hip_longmem.h but not exported"
        res, args = crw_hip.LONGMEM_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == params.count(",") + 1, name
        kinds = [ctypes.c_void_p if "*" in p or "crw_stream_t" in p else ctypes.c_size_t if "size_t" in p else
                 ctypes.c_float if "float" in p else ctypes.c_int for p in params.split(",")]
        assert args == kinds, name                                                          # type by type, in the header's order
        assert getattr(crw_hip.lib(), name).argtypes == args
    text = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert "#define CRW_ABI_VERSION 8" in text and crw_hip.ABI_VERSION == 8                 # added without a bump
    assert not any(name in text for name in decls)


def test_every_longmem_entry_point_is_banded():
    """each takes device pointers; tests/test_longmem_gpu.py calls it by its C name under `run_twice` and `run_banded`"""
    text = open(os.path.join(ROOT, "tests", "test_longmem_gpu.py")).read()
    for name, params in _declared().items():
        assert "*" in params, name
        assert "run_banded" in text and "run_twice" in text and re.search(rf"\blib\.{name}\b", text), name


def test_long_memory_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.LONG_MEMORY_ENTRY_POINTS
    assert names and set(names) == set(crw_hip.LONGMEM_SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS["long_memory"] is names
    assert crw_hip.has_long_memory() is True and crw_hip._long_memory_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "long_memory", False)       # a library from before the entry points
    assert crw_hip.has_long_memory() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._long_memory_lib()
    assert all(name in str(err.value) for name in names)


def test_the_binding_checks_n_long_before_the_library(monkeypatch):
    import crw_hip
    T, N, C, M, knn = 6, 5, 4, 3, 2
    ehat, W, I = torch.zeros(T, N, C), torch.zeros(T - 1, knn, N), torch.zeros(T - 1, knn, N, dtype=torch.int32)
    called = []
    monkeypatch.setattr(crw_hip, "_long_memory_lib", lambda: called.append(1))
    for bad in (0, T, -1):
        with pytest.raises(ValueError, match="n_long must be in 1"):
            crw_hip.labelprop_topk(ehat, 2, 2, 0.1, knn, n_long=bad)
    with pytest.raises(ValueError, match="origin"):
        crw_hip.labelprop_topk(ehat, 2, 2, 0.1, knn, n_long=2, origin=torch.zeros(T, dtype=torch.int32))
    with pytest.raises(ValueError, match="N x 1"):
        crw_hip.labelprop_topk_scores(ehat, 2, 2, 0.1, knn, n_long=2, grid_w=5)
    with pytest.raises(ValueError, match="first_frame"):
        crw_hip.labelprop_topk(ehat, 2, 2, 0.1, knn, first_frame=T, n_long=2)
    with pytest.raises(ValueError, match="n_long needs context='sliding'.*consistently"):
        crw_hip.labelprop_gather(None, W, I, T, N, M, cxt_size=2, n_long=2)
    assert not called


class _Recorder:
    """stands in for `crw_hip.labelprop_topk` / `labelprop_gather`: remembers the calls, fills every later frame with class 1"""

    def __init__(self):
        self.topk, self.gather = None, None

    def labelprop_topk(self, ehat, cxt, radius, temp, knn, **kw):
        self.topk = dict(ehat=ehat.clone(), **kw)
        F, N, _ = ehat.shape
        ff = kw["first_frame"]
        return torch.full((F - ff, knn, N), 1.0 / knn), torch.zeros(F - ff, knn, N, dtype=torch.int32)

    def labelprop_gather(self, seed, W, I, T, N, M, **kw):
        self.gather = dict(seed=seed, W=W.clone(), I=I.clone(), T=T, L_in=kw["L"].clone(), pred_in=kw["pred"].clone(),
                           **{k: v for k, v in kw.items() if k not in ("L", "pred")})
        ff = kw["first_frame"]
        kw["L"][ff * N:] = torch.eye(M)[1]
        kw["pred"][:, ff:] = 1
        return kw["L"], kw["pred"]


@pytest.mark.parametrize("seeded", (True, False))
def test_propagate_all_puts_the_bank_in_front_and_returns_the_item(monkeypatch, seeded):
    import crw_hip
    from imported.labelprop import LabelPropVOS_CRW
    T, N, C, M, B, knn = 7, 5, 4, 3, 2, 2
    rec = _Recorder()
    monkeypatch.setattr(crw_hip, "labelprop_topk", rec.labelprop_topk)
    monkeypatch.setattr(crw_hip, "labelprop_gather", rec.labelprop_gather)
    g = torch.Generator().manual_seed(0)
    feats, mem_feats = torch.randn(T, N, C, generator=g), torch.randn(B, N, C, generator=g)
    mem_labels = torch.tensor([[0, 0, 1, 2, 2], [0, 1, 1, 1, 2]], dtype=torch.int8)
    seed = torch.tensor([2.0, 2, 0, 0, 1]) if seeded else None
    anchors = torch.full((T, N), -1, dtype=torch.int8)
    anchors[0], anchors[3, 1], anchors[5] = 2, 0, torch.tensor([0, 1, 2, 0, 1], dtype=torch.int8)
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=knn, CONTEXT="sliding"))
    pred, L = lp.propagate_all(feats, seed, M, anchors=anchors, memory=(mem_feats, mem_labels))
    K = B + 1 if seeded else B
    assert rec.topk["n_long"] == K and rec.topk["first_frame"] == K and rec.gather["n_long"] == K and rec.gather["first_frame"] == K
    assert rec.gather["T"] == B + T and rec.gather["context"] == "sliding" and rec.gather["cxt_size"] == 2 and rec.gather["seed"] is None
    assert torch.equal(rec.topk["ehat"], torch.cat([mem_feats, feats]))
    front = torch.cat([mem_labels.long(), seed.long()[None]]) if seeded else mem_labels.long()
    assert torch.equal(rec.gather["L_in"][:K * N], torch.eye(M)[front.reshape(-1)])           # the rows in front: one-hot
    assert torch.equal(rec.gather["pred_in"][:, :K], front.t().float())
    # the anchors moved B frames down: the item's frame f is the lists' entry B + f - K; row 0 is ignored under a seed, live without
    marked = torch.isinf(rec.gather["W"][:, 0]) & (rec.gather["W"][:, 0] < 0)                 # [F - K, N]
    want = torch.zeros(B + T - K, N, dtype=torch.bool)
    want[B + 3 - K, 1], want[B + 5 - K] = True, True
    if not seeded:
        want[0] = True
    assert torch.equal(marked, want)
    assert rec.gather["I"][B + 5 - K, 0].tolist() == [0, 1, 2, 0, 1] and int(rec.gather["I"][B + 3 - K, 0, 1]) == 0
    # the item's part alone comes back
    assert pred.shape == (N, T) and L.shape == (T * N, M)
    if seeded:
        assert torch.equal(pred[:, 0], seed) and torch.equal(L[:N], torch.eye(M)[seed.long()])
    assert bool((pred[:, 1:] == 1).all())


def _synthetic_case():
    from dataset import RGDataset
    from test_confidence import Flatten
    H, Wd, T, patch, overlap = 48, 160, 5, (16, 16), (0, 0)
    ds = RGDataset.synthetic(H, Wd, T, patch, overlap)
    seg = (torch.arange(H)[:, None] * 3 // H).expand(H, Wd).contiguous().to(torch.int8)
    return ds, seg, Flatten(), T, patch, overlap


def test_segment_hands_the_same_bank_to_both_passes_and_seeds_nothing_when_seedless(monkeypatch, capsys):
    import inference as crw_inference
    import utils
    from imported.labelprop import LabelPropVOS_CRW
    ds, seg, enc, T, patch, overlap = _synthetic_case()
    capsys.readouterr()
    calls = []

    def stub(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, confidence=None, memory=None, **kw):
        calls.append(dict(seg_ref=seg_ref, use_last=use_last, memory=memory, kw=kw))
        Tn, N = seq.shape[:2]
        return (torch.zeros(N, Tn), torch.zeros(N, max(Tn - 1, 0)), None)

    monkeypatch.setattr(crw_inference, "propagate", stub)
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding"))
    cols = [3, 40, 150]                                                 # 150: clipped to the last full patch column, 144
    run = lambda **kw: crw_inference.segment(ds, seg, enc, lp, 3, T, patch, overlap, device="cpu", dataset_id=0, **kw)
    plain = run(use_last=True)
    assert "memory_traces" not in plain and "seedless" not in plain and all(c["memory"] is None for c in calls)
    n_plain = len(calls)
    del calls[:]
    out = run(use_last=True, memory=(seg, cols), seedless=True)
    assert out["memory_traces"] == 3 and out["seedless"] is True and len(calls) == n_plain
    banks = {id(c["memory"]) for c in calls}
    assert len(banks) == 1 and all(c["seg_ref"] is None for c in calls) and {c["use_last"] for c in calls} == {False, True}
    bank = calls[0]["memory"]
    N = ds[0].shape[1]
    assert isinstance(bank, utils.MemoryBank) and bank.patches.shape == (3, N, 16, 16) and bank.labels.dtype == torch.int8
    for k, x in enumerate((3, 40, 144)):
        assert torch.equal(bank.patches[k], torch.stack([ds.T[n * 16:(n + 1) * 16, x:x + 16] for n in range(N)]).float())
        assert bank.labels[k].tolist() == [int(seg[n * ds.pxh // N, x]) for n in range(N)]       # `seed_labels`' row rule
    del calls[:]
    seeded = run(memory=bank)
    assert seeded["memory_traces"] == 3 and seeded["seedless"] is False and all(c["seg_ref"] is not None and c["memory"] is bank for c in calls)


def test_every_refusal_has_its_message(monkeypatch, capsys, tmp_path):
    import inference as crw_inference
    import utils
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    ds, seg, enc, T, patch, overlap = _synthetic_case()
    capsys.readouterr()
    sliding = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding"))
    reference = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2))
    bank = utils.bank_from_columns(ds, seg, [0, 32])
    run = lambda lp, **kw: crw_inference.segment(ds, seg, enc, lp, 3, T, patch, overlap, device="cpu", **kw)
    with pytest.raises(ValueError, match="memory needs CONTEXT 'sliding'.*never reads.*consistently"):
        run(reference, memory=bank)
    with pytest.raises(ValueError, match="memory and anchor_context='restart'"):
        run(sliding, memory=bank, anchors=(seg, [16]), anchor_context="restart")
    with pytest.raises(ValueError, match="memory and suggest"):
        run(sliding, memory=bank, suggest=2)
    with pytest.raises(ValueError, match="seedless=True and correction=True"):
        run(sliding, memory=bank, seedless=True, correction=True)
    with pytest.raises(ValueError, match="seedless=True needs memory"):
        run(sliding, seedless=True)
    other = utils.memory_bank(torch.zeros(2, ds[0].shape[1] + 1, 16, 16), torch.zeros(2, ds[0].shape[1] + 1, dtype=torch.int8))
    with pytest.raises(ValueError, match="a bank serves items of its own N"):
        run(sliding, memory=other)
    with pytest.raises(ValueError, match="memory is not offered in segment_sweep"):
        crw_inference.segment_sweep(ds, seg, enc, LabelPropSweep(2, [2], [0.1], [2], context="sliding"), 3, T, patch, overlap, device="cpu",
                                    memory=bank)
    with pytest.raises(ValueError, match="fully labelled traces only"):
        utils.memory_bank(torch.zeros(1, 3, 16, 16), torch.tensor([[0, -1, 1]], dtype=torch.int8))
    with pytest.raises(ValueError, match="int8"):
        utils.memory_bank(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, dtype=torch.int64))
    # `propagate` itself, before the encoder runs
    seq = ds[0]
    for kw, msg in ((dict(memory=bank, novelty=True), "memory and novelty"), (dict(memory=bank, anchor_context="restart", anchors=torch.zeros(T, 3, dtype=torch.int8)),
                                                                              "memory and anchor_context='restart'")):
        with pytest.raises(ValueError, match=msg):
            utils.propagate(seq, seg[:, :16], enc, sliding, 3, False, False, **kw)
    with pytest.raises(ValueError, match="memory needs CONTEXT 'sliding'"):
        utils.propagate(seq, seg[:, :16], enc, reference, 3, False, False, memory=bank)
    with pytest.raises(ValueError, match="seg_ref=None .* needs memory"):
        utils.propagate(seq, None, enc, sliding, 3, False, False)
    # a bank survives its file
    bank.save(str(tmp_path / "bank.npz"))
    again = utils.MemoryBank.load(str(tmp_path / "bank.npz"))
    assert torch.equal(again.patches, bank.patches) and torch.equal(again.labels, bank.labels) and len(again) == 2 and again.nodes == bank.nodes


def test_segment_all_flags(monkeypatch, capsys, tmp_path):
    """scripts/segment_all.py: the flag checks, the printed line, the two json keys -- `propagate` stubbed, CPU"""
    import inference as crw_inference
    from test_confidence import _cli, Flatten
    cli = _cli()
    parse = cli.get_args_parser().parse_args
    base = ["--synthetic", "48", "160", "--seq_length", "5", "--patch_size", "16", "16", "--overlap", "0", "0", "--dataset", "0", "-c", "2", "-r", "2",
            "-k", "2", "-t", "0.1", "--model", "0"]
    for extra, msg in ((["--seedless"], "need --memory_cols or --memory_bank"),
                       (["--memory_cols", "3"], "need --context sliding"),
                       (["--context", "sliding", "--memory_cols", "3", "--memory_bank", "x.npz"], "one of the two"),
                       (["--context", "sliding", "--memory_cols", "3", "--seedless", "--correction", "true"], "do not combine"),
                       (["--context", "sliding", "--memory_cols", "3", "--suggest_anchors", "2"], "do not combine")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_memory_flags(cli.with_defaults(parse(base + extra)))
    assert cli.check_memory_flags(cli.with_defaults(parse(base))) is False
    seen = []

    def stub(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, confidence=None, memory=None, **kw):
        seen.append((seg_ref is None, None if memory is None else len(memory)))
        Tn, N = seq.shape[:2]
        return (torch.zeros(N, Tn), torch.zeros(N, max(Tn - 1, 0)), None)

    monkeypatch.setattr(crw_inference, "propagate", stub)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    js, bank_file = tmp_path / "r.json", tmp_path / "bank.npz"
    cli.main(parse(base + ["--context", "sliding", "--memory_cols", "3", "40", "--seedless", "--save_memory_bank", str(bank_file),
                           "--output_folder", str(tmp_path / "out"), "--report_json", str(js)]))
    text = capsys.readouterr().out
    assert "Memory bank traces: 2 (no item is seeded)" in text and seen and all(s == (True, 2) for s in seen)
    d = json.load(open(js))
    assert d["memory_traces"] == 2 and d["seedless"] is True
    del seen[:]
    cli.main(parse(base + ["--context", "sliding", "--memory_bank", str(bank_file), "--output_folder", str(tmp_path / "out"), "--report_json", str(js)]))
    assert "Memory bank traces: 2" in capsys.readouterr().out and all(s == (False, 2) for s in seen)
    d = json.load(open(js))
    assert d["memory_traces"] == 2 and d["seedless"] is False
    cli.main(parse(base + ["--output_folder", str(tmp_path / "out"), "--report_json", str(js)]))
    assert "Memory" not in capsys.readouterr().out and "memory_traces" not in json.load(open(js))
