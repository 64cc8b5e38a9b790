"""Posterior confidence and horizon error bars in the parameter sweep, host side: the CPU route of the batched posterior calls
against the loop of the one-map calls, `inference.segment_sweep(..., posterior=True)` against `inference.segment(...,
posterior=True)` per configuration (the fp32 oracle standing in for the kernels; geometry and fixtures of test_sweep_dense.py),
the option checks, `horizon_bars_sweep` against `horizon_bars`, the ABI tables and status codes, and the command line.  Nothing here
has a counterpart in the reference: correctness is equality with the per-configuration path, which test_posterior.py holds to the
fp64 definition.  The kernel's twins are in test_sweep_posterior_gpu.py."""
import ctypes
import importlib.util
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import dense_ref as dr
import joint_ref as jr
from conftest import PKG, ROOT
from test_confidence import Flatten, synthetic_case
from test_dense import oracle_propagate_soft
from test_sweep_dense import SWEEP_GRID, distinct_soft_labels, forced, oracle_propagate_sweep_soft

ORDER = (0, 1, 2, 3, 4)


def _cli(name="segment_sweep"):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the batch against the loop, CPU route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
def test_cpu_batch_is_the_loop_of_the_single_calls(G):
    import crw_hip
    T, N, M, rows, cols = dr.SHAPES[2]
    order = (2, 0, 1)
    L = distinct_soft_labels(G, T, N, M, seed=4)
    lab = crw_hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, flip=True)[0]
    assert lab.dtype == torch.int8
    post, hz = crw_hip.labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, lab, flip=True, floor=1e-3)
    assert post.shape == (G, rows, cols) and hz.shape == (G, 3, 2, cols) and post.dtype == hz.dtype == torch.float32
    wide_lab = torch.full((G, rows, cols + 7), -7, dtype=torch.int8)
    wide_lab[:, :, 3:3 + cols] = lab
    wide, wide_hz = torch.full((G, rows, cols + 7), -7.0), torch.full((G, 3, 2, cols + 9), -7.0)
    out, out_hz = crw_hip.labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, wide_lab[:, :, 3:3 + cols], flip=True, floor=1e-3,
                                                           out=wide[:, :, 3:3 + cols], out_hz=wide_hz[:, :, :, 5:5 + cols])
    assert out.data_ptr() == wide[:, :, 3:].data_ptr() and out_hz.data_ptr() == wide_hz[:, :, :, 5:].data_ptr()
    for g in range(G):
        one, one_hz = crw_hip.labelmap_ordered_posterior(L[g], T, N, M, rows, cols, order, lab[g], flip=True, floor=1e-3)
        assert torch.equal(post[g], one) and torch.equal(hz[g], one_hz)
        assert torch.equal(wide[g, :, 3:3 + cols], one) and torch.equal(wide_hz[g, :, :, 5:5 + cols], one_hz)
    assert (wide[:, :, :3] == -7).all() and (wide[:, :, 3 + cols:] == -7).all()
    assert (wide_hz[..., :5] == -7).all() and (wide_hz[..., 5 + cols:] == -7).all()
    c = jr.case(2)
    Ls = [distinct_soft_labels(G, Tk, c.N, c.M, seed=5 + k) for k, (Tk, _, _, _) in enumerate(c.geo)]
    a, b = c.source(0, Ls[0]), c.source(1, Ls[1])
    labj = crw_hip.labelmap_ordered_joint_batch(a, b, G, *c.shared, confidence="margin")[0]
    post, hz = crw_hip.labelmap_ordered_joint_posterior_batch(a, b, G, *c.shared, labj, confidence="margin")
    for g in range(G):
        one, one_hz = crw_hip.labelmap_ordered_joint_posterior(c.source(0, Ls[0][g]), c.source(1, Ls[1][g]), *c.shared, labj[g], confidence="margin")
        assert torch.equal(post[g], one) and torch.equal(hz[g], one_hz)
    if G > 1:
        assert not torch.equal(post[0], post[1])


def test_batch_argument_errors_in_python():
    import crw_hip
    G, (T, N, M, rows, cols) = 3, dr.SHAPES[2]
    order = (0, 1, 2)
    L = distinct_soft_labels(G, T, N, M)
    lab = crw_hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order)[0]
    run = lambda labels=lab, order=order, G=G, **kw: crw_hip.labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, labels, **kw)
    for floor in (0.0, 2.0 ** -21, 0.26, float("nan")):  # the single calls' checks and messages
        with pytest.raises(ValueError, match="floor must lie in"):
            run(floor=floor)
    with pytest.raises(ValueError, match="order"):
        run(order=(0, 0))
    with pytest.raises(ValueError, match="labels must be torch.float32 or torch.int8"):
        run(labels=lab.long())
    with pytest.raises(ValueError, match="labels must be"):
        run(labels=lab[0])
    with pytest.raises(ValueError, match="share one pitch"):
        run(out=torch.zeros(G, rows, cols + 1)[:, :, :cols])
    with pytest.raises(ValueError, match="share one map stride"):
        run(out=torch.zeros(G, rows + 1, cols)[:, :rows])
    with pytest.raises(ValueError, match="out_hz must be"):
        run(out_hz=torch.zeros(3, 2, cols))
    with pytest.raises(ValueError, match="out_hz must be"):
        run(out_hz=torch.zeros(G, 3, 2, 2 * cols)[..., ::2])
    with pytest.raises(ValueError, match="overlap"):
        run(out_hz=torch.zeros(3, 2, cols)[None].expand(G, 3, 2, cols))
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="G must be in"):
            run(G=bad)
    src = (L, T, cols, 0, False)
    with pytest.raises(TypeError):
        crw_hip.labelmap_ordered_joint_posterior_batch(src, src, G, N, M, rows, cols, order, lab)  # the kind is mandatory
    with pytest.raises(ValueError, match="needs the confidence kind"):
        crw_hip.labelmap_ordered_joint_posterior_batch(src, src, G, N, M, rows, cols, order, lab, confidence=None)
    sig = inspect.signature(crw_hip.labelmap_ordered_posterior_batch).parameters
    assert list(sig)[:9] == ["L", "G", "T", "N", "M", "rows", "cols", "order", "labels"]
    assert [k for k, v in sig.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["flip", "floor", "out", "out_hz", "workspace"]
    sig = inspect.signature(crw_hip.labelmap_ordered_joint_posterior_batch).parameters
    assert list(sig)[:9] == ["a", "b", "G", "N", "M", "rows", "ncols", "order", "labels"]
    assert [k for k, v in sig.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["confidence", "floor", "out", "out_hz", "workspace"]


# ---- 2. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_batch_group_is_registered_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.POSTERIOR_BATCH_ENTRY_POINTS
    assert names == ("crw_labelmap_posterior_workspace_batch", "crw_labelmap_ordered_posterior_batch", "crw_labelmap_ordered_joint_posterior_batch")
    assert set(names) <= set(crw_hip.SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS["posterior_batch"] is names
    assert crw_hip.has_posterior_batch() is True and crw_hip._posterior_batch_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "posterior_batch", False)
    assert crw_hip.has_posterior_batch() is False and crw_hip.has_posterior() is True
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._posterior_batch_lib()
    assert all(name in str(err.value) for name in names)


def test_header_binding_and_status_codes_of_the_batch_calls():
    """Every refusal comes before a launch (no device needed); 16 is a pointer that is never followed."""
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^#define\s+CRW_ABI_VERSION\s+8\s*$", header, re.M)
    assert re.search(r"^size_t\s+crw_labelmap_posterior_workspace_batch\(int G, int rows, int cols, int S\);", header, re.M)
    assert re.search(r"^int\s+crw_labelmap_ordered_posterior_batch\(const float \*L, int G, int T, int N, int M, int rows, int cols, int flip,\s+"
                     r"const int \*order_host, int S, float floor, const void \*labels, int label_dtype, size_t ld,\s+size_t map_stride, "
                     r"float \*post, float \*hz, size_t hz_ld, size_t hz_stride, void \*ws,\s+size_t ws_bytes, crw_stream_t stream\);", header, re.M)
    assert re.search(r"^int\s+crw_labelmap_ordered_joint_posterior_batch\(const float \*La, .*?int flip_b, int G, int N, int M, int rows, int ncols,"
                     r"\s+const int \*order_host, int S, int conf_kind, float floor, const void \*labels,.*?size_t map_stride, float \*post, "
                     r"float \*hz, size_t hz_ld,\s+size_t hz_stride, void \*ws, size_t ws_bytes, crw_stream_t stream\);", header, re.M | re.S)
    assert "(crw_hip.has_posterior_batch())" in header
    assert len(crw_hip.SIGNATURES["crw_labelmap_ordered_posterior_batch"][1]) == 22
    assert len(crw_hip.SIGNATURES["crw_labelmap_ordered_joint_posterior_batch"][1]) == 30
    lib = crw_hip.lib()
    one = lib.crw_labelmap_posterior_workspace(410, 3200, 4)
    assert one == 4 * 410 * 4 * 3200 and lib.crw_labelmap_posterior_workspace_batch(60, 410, 3200, 4) == 60 * one
    assert lib.crw_labelmap_posterior_workspace_batch(1, 8, 8, 4) == lib.crw_labelmap_posterior_workspace(8, 8, 4) == 4 * 8 * 4 * 64
    for bad in ((0, 8, 8, 4), (-1, 8, 8, 4), (3, 0, 8, 4), (3, 8, 0, 4), (3, 8, 8, 1), (3, 8, 8, 17)):
        assert lib.crw_labelmap_posterior_workspace_batch(*bad) == 0, bad
    G = 3
    need = lib.crw_labelmap_posterior_workspace_batch(G, 8, 8, 4)
    ok = dict(La=16, Ta=4, ca=8, oa=0, fa=0, Lb=16, Tb=3, cb=20, ob=12, fb=1, G=G, N=4, M=4, rows=8, ncols=8, order=(0, 1, 2, 3), kind=0,
              floor=1e-4, labels=16, dt=0, ld=8, ms=64, post=16, hz=16, hz_ld=8, hzs=72, ws=16, wsb=need)

    def call(single=True, joint=True, **bad):
        a = dict(ok, **bad)
        order = None if a["order"] is None else (ctypes.c_int * len(a["order"]))(*a["order"])
        S = a.get("S", 0 if a["order"] is None else len(a["order"]))
        tail = (a["floor"], a["labels"], a["dt"], a["ld"], a["ms"], a["post"], a["hz"], a["hz_ld"], a["hzs"], a["ws"], a["wsb"], None)
        codes = set()
        if joint:
            codes.add(lib.crw_labelmap_ordered_joint_posterior_batch(a["La"], a["Ta"], a["ca"], a["oa"], a["fa"], a["Lb"], a["Tb"], a["cb"],
                                                                     a["ob"], a["fb"], a["G"], a["N"], a["M"], a["rows"], a["ncols"], order, S,
                                                                     a["kind"], *tail))
        if single:
            codes.add(lib.crw_labelmap_ordered_posterior_batch(a["La"], a["G"], a["Ta"], a["N"], a["M"], a["rows"], a["ncols"], a["fa"], order,
                                                               S, *tail))
        assert len(codes) == 1, (bad, codes)
        return codes.pop()

    # the batch's own: G, the two strides, slices whose extent overflows a size_t
    for bad in (dict(G=0), dict(G=-3), dict(G=65536), dict(ms=63), dict(ld=9, ms=7 * 9 + 7), dict(hzs=71), dict(hz_ld=9, hzs=80),
                dict(ms=1 << 62), dict(hzs=1 << 62), dict(hz_ld=1 << 62, hzs=1 << 63), dict(ld=1 << 61, ms=(1 << 63) + (1 << 62)),
                # the single calls': the posterior's own, the order's, the window's
                dict(floor=0.0), dict(floor=2.0 ** -21), dict(floor=0.2500001), dict(floor=float("nan")), dict(post=None, hz=None),
                dict(post=18), dict(hz=18), dict(hz_ld=7), dict(ws=None), dict(ws=18), dict(order=(0, 1, 1)), dict(order=(0, 4)),
                dict(order=(2,)), dict(order=None), dict(order=(0, 1), S=1), dict(La=None), dict(La=18), dict(Ta=0), dict(labels=None),
                dict(N=0), dict(M=1), dict(M=17), dict(rows=0), dict(ncols=0), dict(dt=2), dict(ld=7), dict(labels=18)):
        assert call(**bad) == crw_hip.CRW_EINVAL, bad
    for bad in (dict(Lb=None), dict(Tb=0), dict(cb=0), dict(oa=1), dict(ob=13), dict(kind=-1), dict(kind=3)):  # the joint call's
        assert call(single=False, **bad) == crw_hip.CRW_EINVAL, bad
    assert call(wsb=need - 1) == crw_hip.CRW_EWORKSPACE and call(wsb=need // G) == crw_hip.CRW_EWORKSPACE
    assert call(wsb=need - 1, post=None) == call(wsb=need - 1, hz=None, hzs=0) == crw_hip.CRW_EWORKSPACE  # either output may be null
    assert call(G=1, wsb=need // G - 1) == crw_hip.CRW_EWORKSPACE
    assert call(dt=1, labels=17, wsb=0) == crw_hip.CRW_EWORKSPACE  # int8 labels need no alignment


# ---- 3. segment_sweep on the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_last", [False, True], ids=["forward", "use_last_ordered_correction"])
def test_segment_sweep_posterior_equals_segment_per_configuration(monkeypatch, use_last):
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    M, T = 5, 8
    changes = [5, None] if use_last else [None, None]
    sweep = LabelPropSweep(SWEEP_GRID["cxt_size"], SWEEP_GRID["radii"][:1], SWEEP_GRID["temps"], SWEEP_GRID["knns"])
    G = len(sweep.configs)
    kw = dict(correction=use_last, use_last=use_last, dataset_id=3, device="cpu", confidence="margin", upsample="bilinear", decode="ordered",
              order=ORDER, merge="ordered" if use_last else "rule")

    def run_sweep(**extra):
        ds, seg, _, _, _ = synthetic_case(n_rg=2)
        monkeypatch.setattr(crw_inference, "propagate_sweep", forced(oracle_propagate_sweep_soft, changes, T))
        return crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), **kw, **extra), seg

    (plain, _), (out, seg) = run_sweep(), run_sweep(posterior=True, floor=1e-3)
    assert set(out) == set(plain) | {"post", "horizon", "floor"} and out["floor"] == 1e-3 and out["change_idx"] == changes
    for k in plain:  # every other entry bit for bit what it is without the option
        assert torch.equal(out[k], plain[k]) if torch.is_tensor(plain[k]) else True, k
    rows, width = out["pred"].shape[1:]
    assert out["post"].shape == (G, rows, width) and out["horizon"].shape == (G, 3, M - 1, width)
    assert out["post"].dtype == out["horizon"].dtype == torch.float32
    for g, cfg in enumerate(sweep.configs):
        ds, seg, _, _, _ = synthetic_case(n_rg=2)  # a fresh dataset: the correction shortens it for good
        monkeypatch.setattr(crw_inference, "propagate", forced(oracle_propagate_soft, changes, T))
        one = crw_inference.segment(ds, seg, Flatten(), LabelPropVOS_CRW(cfg), M, T, (8, 8), (4, 0), posterior=True, floor=1e-3, **kw)
        assert one["change_idx"] == changes and torch.equal(out["pred"][g], one["pred"].to(torch.int8))
        assert torch.equal(out["post"][g], one["post"]), cfg
        assert torch.equal(out["horizon"][g], one["horizon"]), cfg
    assert len({m.numpy().tobytes() for m in out["post"]}) >= 2
    assert out["post"].min() >= 0 and out["post"].max() <= 1 and torch.isfinite(out["horizon"]).all()
    cals = crw_inference.calibration_sweep(out["pred"], out["post"], seg, 3, remove_unc=False, nclasses=M)
    assert len(cals) == G and all(c.dropped[2] == 0 for c in cals)


def test_segment_sweep_option_errors_are_segments():
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep
    ds, seg, _, M, T = synthetic_case(n_rg=1)
    sweep = LabelPropSweep(4, [4], [0.1], [5, 3])
    run = lambda **kw: crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), device="cpu", posterior=True, **kw)
    with pytest.raises(ValueError, match="posterior=True needs decode='ordered'"):
        run()
    with pytest.raises(ValueError, match="posterior=True needs decode='ordered'"):
        run(upsample="bilinear", confidence="maxprob")
    for merge in ("rule", "confidence"):
        with pytest.raises(ValueError, match="posterior=True with use_last needs merge='ordered'"):
            run(upsample="bilinear", decode="ordered", order=ORDER, confidence="maxprob", merge=merge, use_last=True, dataset_id=3)
    with pytest.raises(ValueError, match="floor must lie in"):
        run(upsample="bilinear", decode="ordered", order=ORDER, floor=0.5)
    with pytest.raises(TypeError, match="unexpected keyword argument 'posteriors'"):  # the two options are keywords, no catch-all
        crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), device="cpu", posteriors=True)


# ---- 4. horizon_bars_sweep --------------------------------------------------------------------------------------------------------------
def test_horizon_bars_sweep_equals_horizon_bars_per_configuration(monkeypatch):
    import inference as crw_inference
    order = (2, 0, 1, 4)
    gen = torch.Generator().manual_seed(8)
    rows, width, G = 30, 50, 4
    seg = torch.randint(0, 5, (rows, width), generator=gen).float().sort(0).values
    horizon = torch.rand(G, 3, 3, width, generator=gen) * rows
    horizon[:, 0] = horizon[:, 0].round()
    horizon[:, 2] /= 8
    calls = []
    real = crw_inference._reference_boundaries
    monkeypatch.setattr(crw_inference, "_reference_boundaries", lambda *a: calls.append(1) or real(*a))
    got = crw_inference.horizon_bars_sweep(horizon, seg, order, z=1.5, slack=0.5)
    assert len(calls) == 1  # the reference's boundaries: once, not G times
    want = [crw_inference.horizon_bars(h, seg, order, z=1.5, slack=0.5) for h in horizon]
    assert len(got) == G
    for a, b in zip(got, want):
        assert np.array_equal(a.n, b.n) and np.array_equal(a.n_inside, b.n_inside) and a.to_dict() == b.to_dict() and str(a) == str(b)
    assert len({str(b) for b in got}) > 1 and got[0].n.sum() > 0
    assert crw_inference.horizon_bars_sweep(horizon[:0], seg, order) == []
    for bad in (horizon[0], horizon[:, :, :2], horizon[..., :-1]):
        with pytest.raises(ValueError, match="horizon must be"):
            crw_inference.horizon_bars_sweep(bad, seg, order)


# ---- 5. the command line ----------------------------------------------------------------------------------------------------------------
BASE = ["--synthetic", "40", "128", "--dataset", "3", "--patch_size", "8", "8", "--overlap", "4", "0", "--seq_length", "8", "-c", "4", "-r", "4",
        "-t", "0.1", "0.01", "-k", "5", "3", "--model", "0"]
ORDERED = ["--upsample", "bilinear", "--decode", "ordered", "--order", "0", "1", "2", "3", "4"]


def stub_propagate_sweep(seq, seg_ref, model, sweep, ncls, do_pos_embed, use_last, confidence=None, soft=False):
    """`propagate_sweep`'s contract (nearest maps) in index arithmetic alone: `test_confidence.stub_propagate`'s labels and
    confidences, rolled down the nodes by the configuration's index -- the same bits on every machine, which a recorded stdout
    needs (the oracle's sums are not that)."""
    import test_confidence as tc
    assert not soft
    one = tc.stub_propagate(seq, seg_ref, model, None, ncls, do_pos_embed, use_last, confidence=confidence)
    G = len(sweep.configs)
    out = (torch.stack([torch.roll(one[0], g, 0) for g in range(G)]),) + one[1:3]
    return out if confidence is None else out + (torch.stack([torch.roll(one[3], g, 0) for g in range(G)]),)


def run_sweep_cli(monkeypatch, capsys, tmp_path, extra, parser=None, cli=None, propagate_sweep=oracle_propagate_sweep_soft):
    import inference as crw_inference
    cli = cli or _cli()
    monkeypatch.setattr(crw_inference, "propagate_sweep", propagate_sweep)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    js = tmp_path / "r.json"
    os.makedirs(tmp_path, exist_ok=True)
    torch.manual_seed(11)
    argv = BASE + ["--output_folder", str(tmp_path / "out"), "--report_json", str(js)] + extra
    cli.main((parser or cli.get_args_parser(posterior="--posterior" in argv)).parse_args(argv))
    text = capsys.readouterr().out.replace(str(tmp_path), "TMP")
    text = re.sub(r"(Time elapsed \([a-z +]+\):) [0-9.e-]+", r"\1 *", text)
    d = json.load(open(js))
    for k in ("elapsed_inference_s", "elapsed_total_s"):
        d.pop(k)
    return text, d


def test_cli_flags():
    cli = _cli()
    base = ["--synthetic", "40", "192"]
    check = lambda extra, **kw: cli.check_confidence_flags(cli.with_defaults(cli.get_args_parser(**kw).parse_args(base + extra)))
    a = check(ORDERED + ["--posterior", "--select", "post_ece"], posterior=True)
    assert a.posterior and a.floor == 1e-4 and a.select == "post_ece"
    assert check(ORDERED + ["--posterior", "--floor", "1e-3", "--select", "post_aurc"], posterior=True).floor == 1e-3
    plain = check([])
    assert (plain.posterior, plain.floor, plain.select) == (False, None, "macro_f1")
    for select in ("post_ece", "post_aurc"):
        with pytest.raises(SystemExit):  # without --posterior on the command line the choice is not offered at all
            cli.get_args_parser().parse_args(base + ["--select", select])
        with pytest.raises(SystemExit, match=f"--select {select} needs --posterior"):
            check(ORDERED + ["--select", select], posterior=True)
    choices = lambda **kw: set(next(x for x in cli.get_args_parser(**kw)._actions if x.dest == "select").choices)
    assert choices(posterior=True) - choices() == {"post_ece", "post_aurc"} and "horizon_mae" not in choices(posterior=True)
    for bad, msg in ((["--posterior"], "--posterior needs --decode ordered"), (["--floor", "1e-3"], "need --posterior"),
                     (ORDERED + ["--posterior", "--floor", "0.5"], "--floor 0.5"),
                     (ORDERED + ["--posterior", "--use_last", "true"], "needs --merge ordered"),
                     (ORDERED + ["--posterior", "--use_last", "true", "--confidence", "margin", "--merge", "confidence"], "needs --merge ordered")):
        with pytest.raises(SystemExit, match=msg):
            check(bad, posterior=True)


class Planted:
    """A `metrics.Calibration` whose ECE is planted; everything else is the real one's."""

    def __init__(self, cal, ece):
        self._cal, self.ece = cal, ece

    def __getattr__(self, name):
        return getattr(self._cal, name)

    def __str__(self):
        return str(self._cal)


def test_cli_select_post_ece_picks_the_first_minimum_and_never_a_nan(monkeypatch, capsys, tmp_path):
    import inference as crw_inference
    real = crw_inference.calibration_sweep
    planted = [float("nan"), 0.3, 0.1, 0.1]
    monkeypatch.setattr(crw_inference, "calibration_sweep", lambda *a, **k: [Planted(c, e) for c, e in zip(real(*a, **k), planted)])
    text, d = run_sweep_cli(monkeypatch, capsys, tmp_path, ORDERED + ["--posterior", "--floor", "1e-3", "--select", "post_ece"])
    assert len(d["configs"]) == 4 and d["select"] == "post_ece" and d["floor"] == 1e-3
    assert d["best"]["index"] == 2 and d["best"]["score"] == 0.1  # the first of the two minima; the NaN never wins
    b = d["configs"][2]
    assert f"Best by post_ece: radius {b['radius']} temp {b['temp']:g} knn {b['knn']} (0.1000)" in text
    assert [c["score"] == c["score"] for c in d["configs"]] == [False, True, True, True]
    # the two columns, and the best configuration's two tables after its other tables
    head = next(line for line in text.splitlines() if line.lstrip().startswith("radius"))
    assert head.endswith(" post ece bar cover") and "posterior=True" in text and "floor=0.001" in text
    assert text.index("Best by post_ece") < text.index("Calibration (posterior of the ordered decode, floor 0.001):") \
        < text.index("Horizon error bars") < text.index("Time elapsed (inference + metrics)")
    for c in d["configs"]:
        p = c["posterior"]
        assert p["calibration"]["total"] == d["pixels"] and len(p["horizon_bars"]["coverage"]) == 4 and p["horizon_bars"]["rows"] == d["map_shape"][0]
    covers = [c["posterior"]["horizon_bars"]["mean_coverage"] for c in d["configs"]]
    rows = [line.split() for line in text.splitlines() if re.match(r"\s+4\s+0\.0?1\s+[35]\s", line)]
    assert len(rows) == 4 and [float(r[-1]) for r in rows] == [round(v, 4) for v in covers]
    assert [r[-2] for r in rows] == ["nan", "0.3000", "0.1000", "0.1000"]


GOLDEN_ARGS = ["--use_last", "true", "--confidence", "maxprob", "--merge", "confidence", "--select", "ece", "--reports"]


def test_cli_without_the_flag_prints_the_recorded_stdout(monkeypatch, capsys, tmp_path):
    """tests/golden/segment_sweep_stdout.txt is this run's stdout as the commit BEFORE the posterior flags printed it (recorded by
    running `run_sweep_cli` of this file, with `stub_propagate_sweep`, against that commit's package; elapsed times and the
    temporary folder blanked): the same bytes now -- the Namespace line, the table, the best configuration's report and
    calibration table --, and a json without the new keys."""
    text, d = run_sweep_cli(monkeypatch, capsys, tmp_path, GOLDEN_ARGS, propagate_sweep=stub_propagate_sweep)
    assert text == open(os.path.join(ROOT, "tests", "golden", "segment_sweep_stdout.txt")).read()
    assert "floor" not in d and all("posterior" not in c for c in d["configs"]) and len(d["configs"]) == 4
    assert len({c["score"] for c in d["configs"]}) > 1  # the stub's configurations differ


def test_cli_without_the_flag_prints_what_the_parser_without_it_prints(monkeypatch, capsys, tmp_path):
    """On the ordered path, for which no stdout was recorded (the stub has no soft labels): without --posterior the bytes on stdout
    and the json are those of a run whose parser does not know the new flags at all (their defaults set on the namespace
    afterwards, so that only their parsing is bypassed).  This compares the script with itself -- it guards the parser and the
    Namespace line, not the table or the json; the recorded stdout above guards those.  `segment_all.py`, which the script builds
    on, still prints its recorded stdout."""
    import test_confidence as tc
    cli = _cli()
    extra = ORDERED + ["--confidence", "maxprob", "--use_last", "true", "--merge", "ordered", "--select", "ece"]
    plain, d = run_sweep_cli(monkeypatch, capsys, tmp_path / "a", extra, cli=cli)
    shown = []

    class Bypassed:
        def parse_args(self, argv):
            p = cli.get_args_parser()
            new = [a for a in p._actions if a.dest in cli.POSTERIOR_FLAGS]
            assert len(new) == len(cli.POSTERIOR_FLAGS) == 2
            old = cli.argparse.ArgumentParser(add_help=True)
            for a in p._actions:
                if a.dest not in cli.POSTERIOR_FLAGS and a.dest != "help":
                    old._add_action(a)
            with pytest.raises(SystemExit):
                old.parse_args(argv + ["--posterior"])  # the bypassed parser does not know the flag
            args = old.parse_args(argv)
            shown.append(str(args))
            for a in new:
                setattr(args, a.dest, a.default)
            return args

    text2, d2 = run_sweep_cli(monkeypatch, capsys, tmp_path / "b", extra, parser=Bypassed(), cli=cli)
    assert len(shown) == 1 and "posterior" not in shown[0] and "floor" not in shown[0]
    assert "posterior" not in plain and "floor" not in plain and "post ece" not in plain
    assert plain == text2 and d == d2 and "floor" not in d and all("posterior" not in c for c in d["configs"])
    text, files, _ = tc.run_cli(monkeypatch, capsys, tmp_path / "all", [])
    assert text == open(os.path.join(ROOT, "tests", "golden", "segment_all_stdout.txt")).read() and files == ["predicted_map.pt"]
