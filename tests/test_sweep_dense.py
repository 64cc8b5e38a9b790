"""Bilinear maps, confidence and calibration in the parameter sweep, host side: the CPU route of `crw_hip.labelmap_dense_batch`
against the loop of `labelmap_dense`, the contract of `utils.propagate_sweep(confidence=, soft=)`, `inference.segment_sweep` with
its new options against `inference.segment` per configuration (the fp32 oracle standing in for the kernels), `calibration_sweep`
against `calibration`, the ABI tables and the command line.  Nothing here has a counterpart in the reference: correctness is
equality with the per-configuration path, which is itself pinned to the reference's fixtures and the fp64 helper.  The kernel's
twins are in test_sweep_dense_gpu.py."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dense_ref as dr
from conftest import PKG, ROOT
from oracle import crw_oracle as orc
from test_confidence import Flatten, oracle_soft_labels, synthetic_case
from test_dense import oracle_propagate_soft

KINDS = (None,) + dr.KINDS
BATCH_SHAPES = [(5, 7, 3, 37, 61), (1, 1, 2, 5, 9)]


def distinct_soft_labels(G, T, N, M, seed=0):
    """L [G, T*N, M]: every slice its own softmax of random logits."""
    g = torch.Generator().manual_seed(100 + seed)
    return torch.softmax(2.0 * torch.randn(G, T * N, M, generator=g), -1).contiguous()


# ---- 1. the batch against the loop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("shape", BATCH_SHAPES, ids=str)
def test_cpu_batch_is_the_loop_of_labelmap_dense(shape, G):
    import crw_hip
    T, N, M, rows, cols = shape
    L = distinct_soft_labels(G, T, N, M)
    for kind in KINDS:
        for dtype in (torch.float32, torch.int8):
            for flip in (False, True):
                lab, conf = crw_hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, confidence=kind, flip=flip, dtype=dtype)
                assert lab.shape == (G, rows, cols) and lab.dtype == dtype and (conf is None) == (kind is None)
                wide = torch.full((G, rows, cols + 7), -7, dtype=dtype)
                widec = torch.full((G, rows, cols + 7), -7.0) if kind else None
                out, outc = crw_hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, confidence=kind, flip=flip, dtype=dtype,
                                                         out=wide[:, :, 3:3 + cols], out_conf=None if kind is None else widec[:, :, 3:3 + cols])
                assert out.data_ptr() == wide[:, :, 3:].data_ptr()
                for g in range(G):
                    one, onec = crw_hip.labelmap_dense(L[g], T, N, M, rows, cols, confidence=kind, flip=flip, dtype=dtype)
                    assert torch.equal(lab[g], one) and torch.equal(wide[g, :, 3:3 + cols], one)
                    if kind:
                        assert torch.equal(conf[g], onec) and torch.equal(widec[g, :, 3:3 + cols], onec)
                for m in (wide,) + ((widec,) if kind else ()):
                    assert (m[:, :, :3] == -7).all() and (m[:, :, 3 + cols:] == -7).all()  # the guard cells
    if G > 1 and rows * cols > 50:
        assert not torch.equal(conf[0], conf[1])
    assert inspect.signature(crw_hip.labelmap_dense_batch).parameters["dtype"].default is torch.int8


def test_cpu_batch_refuses_targets_that_are_no_windows():
    import crw_hip
    G, (T, N, M, rows, cols) = 3, BATCH_SHAPES[0]
    L = distinct_soft_labels(G, T, N, M)
    call = lambda **kw: crw_hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, **kw)
    with pytest.raises(ValueError):
        call(out=torch.zeros(G, cols, rows, dtype=torch.int8).transpose(1, 2))  # transposed
    with pytest.raises(ValueError, match="contiguous along its columns"):
        call(out=torch.zeros(G, rows, 2 * cols, dtype=torch.int8)[:, :, ::2])  # strided
    with pytest.raises(ValueError, match="overlap"):
        call(out=torch.zeros(rows, cols, dtype=torch.int8)[None].expand(G, rows, cols))  # the G maps on top of each other
    with pytest.raises(ValueError, match="overlap"):
        call(out=torch.zeros(G * rows * cols, dtype=torch.int8).as_strided((G, rows, cols), (rows * cols - 1, cols, 1)))
    with pytest.raises(ValueError, match="overlap"):
        call(out=torch.zeros(G, rows * cols, dtype=torch.int8).as_strided((G, rows, cols), (rows * cols, cols - 1, 1)))
    wide = torch.zeros(G, rows, cols + 7, dtype=torch.int8)
    with pytest.raises(ValueError, match="one pitch"):
        call(confidence="margin", out=wide[:, :, :cols], out_conf=torch.zeros(G, rows, cols))
    with pytest.raises(ValueError, match="one map stride"):
        call(confidence="margin", out=torch.zeros(G, rows + 1, cols, dtype=torch.int8)[:, :rows], out_conf=torch.zeros(G, rows, cols))
    with pytest.raises(ValueError):
        call(out=torch.zeros(G, rows, cols))  # float32 target, int8 asked
    with pytest.raises(ValueError):
        call(out_conf=torch.zeros(G, rows, cols))  # no kind
    for bad in (dict(G=0), dict(G=65536), dict(M=17), dict(rows=0), dict(T=0)):
        a = dict(G=G, T=T, N=N, M=M, rows=rows, cols=cols)
        a.update(bad)
        with pytest.raises(ValueError):
            crw_hip.labelmap_dense_batch(L, **a)


# ---- 2. propagate_sweep's contract ------------------------------------------------------------------------------------------------
class TwoConfigs:
    configs = [dict(CXT_SIZE=4, RADIUS=4, TEMP=0.1, KNN=5), dict(CXT_SIZE=4, RADIUS=2, TEMP=0.01, KNN=3)]

    def propagate_all(self, feats, seed, nclasses, grid_w=1, soft=False):
        T, N, _ = feats.shape
        g = torch.Generator().manual_seed(5)
        L = torch.softmax(torch.randn(2, T * N, nclasses, generator=g), -1)
        L[:, :N] = torch.nn.functional.one_hot(seed.long(), nclasses).float()
        pred = L.view(2, T, N, nclasses).argmax(-1).permute(0, 2, 1).float()
        return (pred, L) if soft else pred


def test_propagate_sweep_contract_on_the_cpu(monkeypatch):
    import crw_hip
    import utils as crw_utils
    sig = inspect.signature(crw_utils.propagate_sweep)
    for name, default in (("confidence", None), ("soft", False)):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is default
    assert list(sig.parameters)[:7] == ["seq", "seg_ref", "model", "sweep", "nclasses", "do_pos_embed", "use_last"]
    N, M = 6, 4
    seed = torch.tensor([0., 0., 1., 3., 3., 2.])
    monkeypatch.setattr(crw_utils, "_features_and_seed", lambda seq, *a: (torch.zeros(seq.shape[0], N, 8), seed))
    monkeypatch.setattr(crw_hip, "xent_metric", lambda feats: torch.zeros(N, feats.shape[0] - 1))
    monkeypatch.setattr(crw_utils, "column_diffs_async", lambda xent: None)
    monkeypatch.setattr(crw_utils, "change_point", lambda xent, diffs=None: None)
    sweep = TwoConfigs()
    one = torch.zeros(1, N, 4, 4)  # a one-frame item: G copies of the one-hot seed, a confidence of ones
    assert len(crw_utils.propagate_sweep(one, None, None, sweep, M, False, False)) == 3
    out = crw_utils.propagate_sweep(one, None, None, sweep, M, False, False, confidence="margin", soft=True)
    assert len(out) == 5 and out[0].shape == (2, N, 1) and torch.equal(out[0][1, :, 0], seed)
    assert out[3].shape == (2, N, 1) and (out[3] == 1).all() and out[4].shape == (2, N, M)
    for g in range(2):
        assert torch.equal(out[4][g], torch.nn.functional.one_hot(seed.long(), M).float())
    assert len(crw_utils.propagate_sweep(one, None, None, sweep, M, False, False, soft=True)) == 4
    seq = torch.zeros(5, N, 4, 4)
    three = crw_utils.propagate_sweep(seq, None, None, sweep, M, False, False)
    four = crw_utils.propagate_sweep(seq, None, None, sweep, M, False, False, confidence="entropy")
    fours = crw_utils.propagate_sweep(seq, None, None, sweep, M, False, False, soft=True)
    five = crw_utils.propagate_sweep(seq, None, None, sweep, M, False, False, confidence="maxprob", soft=True)
    assert [len(o) for o in (three, four, fours, five)] == [3, 4, 4, 5]
    L = five[4]
    assert L.shape == (2, 5 * N, M) and torch.equal(fours[3], L) and torch.equal(three[0], five[0]) and five[0].shape == (2, N, 5)
    for g in range(2):  # conf[g] is the one-pass call on L[g]: the stack read as G*T frames changes nothing
        assert torch.equal(five[3][g], crw_hip.labelprop_confidence(L[g], 5, N, M, "maxprob"))
        assert torch.equal(four[3][g], crw_hip.labelprop_confidence(L[g], 5, N, M, "entropy"))
        assert (five[3][g][:, 0] == 1).all()
    with pytest.raises(ValueError, match="confidence must be None or one of"):
        crw_utils.propagate_sweep(seq, None, None, sweep, M, False, False, confidence="softmax")


# ---- 3. segment_sweep on the oracle -----------------------------------------------------------------------------------------------
def oracle_propagate_sweep_soft(seq, seg_ref, model, sweep, ncls, do_pos_embed, use_last, confidence=None, soft=False):
    """`utils.propagate_sweep`'s contract on the CPU: ONE encoder call, then the fp32 oracle per configuration."""
    import crw_hip
    from imported.labelprop import LabelPropVOS_CRW
    T, N = seq.shape[:2]
    emb = model(seq.reshape(T * N, 1, *seq.shape[2:])).reshape(T, N, -1).numpy()
    if use_last:
        emb = emb[::-1].copy()
    seed = orc.seed_labels(seg_ref.numpy(), N)
    L = torch.stack([torch.tensor(oracle_soft_labels(emb, seed, ncls, LabelPropVOS_CRW(c))) for c in sweep.configs])
    G = L.shape[0]
    out = (L.view(G, T, N, ncls).argmax(-1).permute(0, 2, 1).float(), torch.tensor(orc.xent_metric(emb)) if T > 1 else torch.zeros(N, 0), None)
    if confidence is not None:
        out += (torch.stack([crw_hip.labelprop_confidence(l, T, N, ncls, confidence) for l in L]),)
    return out + (L,) if soft else out


def forced(fn, changes, T):
    """`fn` with the change points of the whole-length forward items forced."""
    it = iter(changes)

    def wrapped(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, **k):
        out = fn(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, **k)
        return out[:2] + ((next(it, None) if (seq.shape[0] == T and not use_last) else None),) + out[3:]
    return wrapped


SWEEP_GRID = dict(cxt_size=4, radii=[4, 2], temps=[0.1, 0.01], knns=[5, 3])
OUTPUTS = ("pred", "forward", "conf", "forward_conf")


@pytest.mark.parametrize("merge", ["rule", "confidence"])
@pytest.mark.parametrize("upsample", ["nearest", "bilinear"])
def test_segment_sweep_equals_segment_per_configuration_with_all_options(monkeypatch, upsample, merge):
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    M, T = 5, 8
    changes = [5, None]
    sweep = LabelPropSweep(SWEEP_GRID["cxt_size"], SWEEP_GRID["radii"], SWEEP_GRID["temps"], SWEEP_GRID["knns"])
    assert len(sweep.configs) == 8
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cpu", confidence="maxprob", merge=merge, upsample=upsample)
    ds, seg, _, _, _ = synthetic_case(n_rg=2)
    monkeypatch.setattr(crw_inference, "propagate_sweep", forced(oracle_propagate_sweep_soft, changes, T))
    out = crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), **kw)
    assert set(out) == {"pred", "forward", "conf", "forward_conf", "xent", "change_idx", "configs"} and out["change_idx"] == changes
    G, rows, cols = 8, seg.shape[0], 2 * T * 8
    for k in OUTPUTS:
        assert out[k].shape == (G, rows, cols) and out[k].dtype == (torch.float32 if "conf" in k else torch.int8)
    for g, cfg in enumerate(sweep.configs):
        ds, seg, _, _, _ = synthetic_case(n_rg=2)  # a fresh dataset: the correction shortens it for good
        monkeypatch.setattr(crw_inference, "propagate", forced(oracle_propagate_soft, changes, T))
        one = crw_inference.segment(ds, seg, Flatten(), LabelPropVOS_CRW(cfg), M, T, (8, 8), (4, 0), **kw)
        assert one["change_idx"] == changes
        for k in ("pred", "forward"):
            assert torch.equal(out[k][g], one[k].to(torch.int8)), (cfg, k)
        for k in ("conf", "forward_conf"):
            assert torch.equal(out[k][g], one[k]), (cfg, k)
    assert len({m.numpy().tobytes() for m in out["forward"]}) >= 2 and len({m.numpy().tobytes() for m in out["conf"]}) >= 2
    assert not torch.equal(out["pred"], out["forward"])  # the reverse pass took pixels
    if upsample == "bilinear":
        ds, seg, _, _, _ = synthetic_case(n_rg=2)
        near = crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), **dict(kw, upsample="nearest"))
        assert not torch.equal(near["forward"], out["forward"])  # the boundaries left the node grid


def test_segment_sweep_argument_errors_are_segments(monkeypatch):
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep
    ds, seg, _, M, T = synthetic_case(n_rg=1)
    sweep = LabelPropSweep(4, [4], [0.1], [5, 3])
    run = lambda **kw: crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), device="cpu", **kw)
    with pytest.raises(ValueError, match=r"merge must be 'rule' or 'confidence' \(got 'vote'\)"):
        run(merge="vote")
    with pytest.raises(ValueError, match=r"upsample must be 'nearest' or 'bilinear' \(got 'bicubic'\)"):
        run(upsample="bicubic")
    with pytest.raises(ValueError, match=r"confidence must be None or one of maxprob, margin, entropy \(got 'softmax'\)"):
        run(confidence="softmax")
    with pytest.raises(ValueError, match="merge='confidence' needs a confidence kind"):
        run(merge="confidence")
    with pytest.raises(ValueError, match="no merge rule for dataset id 2"):
        run(merge="rule", dataset_id=2, use_last=True)
    with pytest.raises(ValueError, match="no merge rule for dataset id 2"):
        run(merge="rule", dataset_id=2, use_last=True, confidence="margin", upsample="bilinear")
    monkeypatch.setattr(crw_inference, "propagate_sweep", oracle_propagate_sweep_soft)
    for upsample in ("nearest", "bilinear"):  # the merge by confidence needs no class rule: any dataset id
        out = run(merge="confidence", confidence="margin", dataset_id=2, use_last=True, upsample=upsample)
        assert out["pred"].shape == out["conf"].shape == (2, seg.shape[0], T * 8)
    sig = inspect.signature(crw_inference.segment_sweep).parameters
    assert (sig["confidence"].default, sig["merge"].default, sig["upsample"].default) == (None, "rule", "nearest")


# ---- 4. calibration_sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset_id", [0, 1, 3])
def test_calibration_sweep_equals_calibration_per_map(dataset_id):
    import crw_hip
    import inference as crw_inference
    K = crw_inference.NCLASSES[dataset_id]
    gen = torch.Generator().manual_seed(dataset_id + 21)
    seg = torch.randint(0, K, (20, 64), generator=gen).float()
    pred = torch.randint(0, K, (5, 20, 64), generator=gen).to(torch.int8)
    pred[:, ::2] = seg[::2].to(torch.int8)  # half right
    conf = torch.rand(5, 20, 64, generator=gen)
    unc = seg.clone()
    unc[8:11] = 4
    kw = dict(unc_seg=unc) if dataset_id == 0 else {}
    for remove_unc in (True, False):
        for bins in (10, 7):
            got = crw_inference.calibration_sweep(pred, conf, seg, dataset_id, remove_unc=remove_unc, bins=bins, **kw)
            want = [crw_inference.calibration(p, c, seg, dataset_id, remove_unc=remove_unc, bins=bins, **kw) for p, c in zip(pred, conf)]
            assert len(got) == 5
            for a, b in zip(got, want):
                assert np.array_equal(a.count, b.count) and np.array_equal(a.correct, b.correct) and a.dropped == b.dropped
                assert np.array_equal(a.conf_sum, b.conf_sum) and a.ece == b.ece and a.aurc == b.aurc and str(a) == str(b)
            if remove_unc and dataset_id in (0, 1):
                assert got[0].dropped[0] > 0
    assert len({c.ece for c in got}) > 1
    if dataset_id == 0:
        with pytest.raises(ValueError, match="unc_seg"):
            crw_inference.calibration_sweep(pred, conf, seg, 0)
    with pytest.raises(ValueError):
        crw_inference.calibration_sweep(pred, conf, seg[:, :60], dataset_id, remove_unc=False)
    with pytest.raises(ValueError):
        crw_inference.calibration_sweep(pred, conf[:4], seg, dataset_id, remove_unc=False)
    with pytest.raises(ValueError):
        crw_inference.calibration_sweep(pred, conf, seg, 2)
    bad = pred.clone()
    bad[3, 0, 0] = 9 if dataset_id != 1 else 7  # a planted label outside 0 ... K-1
    with pytest.raises(crw_hip.LabelError):
        crw_inference.calibration_sweep(bad, conf, seg, dataset_id, remove_unc=False)


# ---- 5. command line and ABI ------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("segment_sweep", os.path.join(PKG, "scripts", "segment_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_selection():
    cli = _cli()
    p = cli.get_args_parser()
    base = ["--synthetic", "40", "192"]
    a = p.parse_args(base)
    assert (a.upsample, a.confidence, a.merge, a.bins, a.select) == ("nearest", None, "rule", 10, "macro_f1")
    a = p.parse_args(base + ["--upsample", "bilinear", "--confidence", "margin", "--merge", "confidence", "--bins", "5", "--select", "aurc"])
    assert (a.upsample, a.confidence, a.merge, a.bins, a.select) == ("bilinear", "margin", "confidence", 5, "aurc")
    assert cli.check_confidence_flags(cli.with_defaults(a)) is a
    choices = next(x for x in p._actions if x.dest == "select").choices
    assert {"ece", "aurc", "macro_f1", "weighted_f1", "accuracy", "mean_iou"} == set(choices)
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--upsample", "bicubic"])
    with pytest.raises(SystemExit, match="--merge confidence needs --confidence"):
        cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + ["--merge", "confidence"])))
    with pytest.raises(SystemExit, match="--select ece needs --confidence"):
        cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + ["--select", "ece"])))
    with pytest.raises(SystemExit, match="--bins"):
        cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + ["--confidence", "maxprob", "--bins", "65"])))
    nan = float("nan")
    assert cli.pick_best([0.3, 0.1, 0.1, 0.2], lower_is_better=True) == 1  # the minimum, the first of equals
    assert cli.pick_best([nan, 0.4, 0.2], lower_is_better=True) == 2 and cli.pick_best([nan, nan], lower_is_better=True) == 0
    assert cli.pick_best([0.3, 0.5, 0.5]) == 1


def test_header_and_binding_declare_the_batch_entry_point_at_abi_8():
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^int\s+crw_labelmap_dense_batch\(const float \*L, int G, int T, int N, int M, int rows, int cols, int flip, "
                     r"int conf_kind, void \*labels,\s+int label_dtype, float \*conf, size_t ld, size_t map_stride, crw_stream_t stream\);",
                     header, re.M)
    assert int(re.search(r"^#define\s+CRW_ABI_VERSION\s+(\d+)", header, re.M).group(1)) == crw_hip.ABI_VERSION == 8
    assert "crw_labelmap_dense_batch\n * (crw_hip.has_dense_batch())" in header
    assert crw_hip.DENSE_BATCH_ENTRY_POINTS == ("crw_labelmap_dense_batch",) and len(crw_hip.SIGNATURES["crw_labelmap_dense_batch"][1]) == 15
    lib = crw_hip.lib()
    assert lib.crw_abi_version() == 8 and crw_hip.has_dense_batch() and crw_hip.has_dense()
    # argument errors are refused before anything is launched (no device needed); 16 is a pointer that is never followed
    ok = dict(L=16, G=3, T=4, N=4, M=4, rows=8, cols=8, flip=0, kind=-1, labels=16, dt=0, conf=None, ld=8, ms=64)
    for bad in (dict(G=0), dict(G=65536), dict(ms=63), dict(ld=9, ms=7 * 9 + 7), dict(L=None), dict(labels=None), dict(T=0), dict(M=1),
                dict(M=17), dict(rows=0), dict(cols=(1 << 22) + 1), dict(kind=3), dict(kind=0), dict(conf=16), dict(dt=2), dict(ld=7),
                dict(labels=18)):
        a = dict(ok, **bad)
        assert lib.crw_labelmap_dense_batch(a["L"], a["G"], a["T"], a["N"], a["M"], a["rows"], a["cols"], a["flip"], a["kind"], a["labels"],
                                            a["dt"], a["conf"], a["ld"], a["ms"], None) == crw_hip.CRW_EINVAL, bad


def test_a_library_without_the_batch_entry_point_is_named_stale(monkeypatch):
    import crw_hip
    crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "dense_batch", False)
    assert not crw_hip.has_dense_batch()
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*crw_labelmap_dense_batch.*rebuild"):
        crw_hip._dense_batch_lib()
