"""The depth-ordered label map on the host: the CPU route of `crw_hip.labelmap_ordered` against the definition in fp64
(ordered_ref.py: feasibility, optimality gap, sanity), the exact dyadic cases and their ties, the confidence that does not depend on
the decode, windows, the batch, the quality claim on synthetic layered items, and the host surface (argument errors, the ABI tables,
`segment(..., decode='ordered')`, `segment_sweep`, the command lines).  The kernel's twins are in test_ordered_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dense_ref as dr
import ordered_ref as od
from conftest import ROOT
from test_confidence import Flatten, synthetic_case
from test_dense import oracle_propagate_soft
from test_sweep_dense import SWEEP_GRID, forced, oracle_propagate_sweep_soft

ORDERS = [(5, 4, 3, 2, 1, 0), (3, 0, 5), (1, 4)]  # on (9, 12, 6, 50, 61)
WIDE = (9, 12, 6, 50, 61)


def unflip(t, flip):
    return torch.flip(t, (1,)) if flip else t


# ---- 1. the CPU route against the definition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.SHAPES + [dr.SLAB], ids=str)
def test_cpu_route_against_the_definition(shape):
    import crw_hip
    T, N, M, rows, cols = shape
    order = tuple(range(M))
    L, ref, _, score = od.reference(shape, order)
    mono = int(((od.positions(ref.labels, order)[1:] >= od.positions(ref.labels, order)[:-1]).all(0)).sum())
    print(f"{shape}: the arg-max map is monotone in {mono} of {cols} columns")
    for dtype, flip in ((torch.float32, False), (torch.int8, True)):
        lab, conf = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip, dtype=dtype)
        assert lab.shape == (rows, cols) and lab.dtype == dtype and conf is None
        od.check(ref.probs, unflip(lab, flip).numpy(), order, score, f"cpu {shape} {dtype} flip={flip}")


@pytest.mark.parametrize("flip", [False, True], ids=["", "flip"])
@pytest.mark.parametrize("order", ORDERS, ids=str)
def test_cpu_route_under_other_orders(order, flip):
    import crw_hip
    T, N, M, rows, cols = WIDE
    L, ref, _, score = od.reference(WIDE, order)
    lab, _ = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip)
    od.check(ref.probs, unflip(lab, flip).numpy(), order, score, f"cpu {WIDE} flip={flip}")
    assert set(np.unique(lab.numpy()).astype(int)) <= set(order)


def test_a_clean_layered_item_keeps_its_arg_max_map():
    """The sanity clause where it bites: without wrong nodes most columns of the arg-max map are monotone and clear already."""
    import crw_hip
    T, N, rows, cols, temp, M, _ = od.QUALITY[1]
    _, L = od.layered_case(T, N, rows, cols, temp, M, 0.0, 0)
    probs = dr.probabilities(L, T, N, M, rows, cols)
    lab, _ = crw_hip.labelmap_ordered(torch.tensor(L), T, N, M, rows, cols, range(M))
    od.check(probs, lab.numpy(), range(M), what="cpu clean layered item")
    dense, _ = crw_hip.labelmap_dense(torch.tensor(L), T, N, M, rows, cols)
    assert int((lab != dense).sum()) <= 0.02 * rows * cols


# ---- 2. exact cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.EXACT, ids=str)
def test_exact_dyadic_case_equals_the_plain_loops(shape):
    import crw_hip
    T, N, M, rows, cols = shape
    L = dr.exact_rows(T, N, M)
    probs = dr.probabilities(L.numpy(), T, N, M, rows, cols)
    for order in (tuple(range(M)), tuple(range(M - 1, -1, -1))):
        want, _ = od.decode(probs, order)
        for flip in (False, True):
            lab, _ = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)
            assert np.array_equal(unflip(lab, flip).numpy().astype(np.int64), want)  # outright, the exact ties included


# ---- 3. the confidence does not depend on the decode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dr.KINDS)
def test_conf_is_labelmap_dense_s(kind):
    import crw_hip
    for shape, order in ((WIDE, (3, 0, 5)), ((4, 3, 16, 9, 130), tuple(range(16)))):
        T, N, M, rows, cols = shape
        L = dr.reference(shape)[0]
        for flip in (False, True):
            lab, conf = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence=kind, flip=flip)
            only, _ = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip)
            _, want = crw_hip.labelmap_dense(L, T, N, M, rows, cols, confidence=kind, flip=flip)
            assert torch.equal(conf, want) and torch.equal(lab, only)


# ---- 4. windows, 5. batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.float32, torch.int8), ids=str)
def test_column_windows_on_the_cpu(dtype):
    import crw_hip
    T, N, M, rows, cols = 9, 12, 6, 50, 29
    L = dr.dirichlet_rows(T, N, M, seed=3)
    order = (0, 2, 1, 5)
    lab, conf = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence="margin", dtype=dtype)
    wide, widec = torch.full((rows, cols + 7), -7, dtype=dtype), torch.full((rows, cols + 7), -7.0)
    out, outc = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence="margin", dtype=dtype, out=wide[:, 3:3 + cols],
                                         out_conf=widec[:, 3:3 + cols])
    assert out.data_ptr() == wide[:, 3:].data_ptr() and torch.equal(wide[:, 3:3 + cols], lab) and torch.equal(widec[:, 3:3 + cols], conf)
    for m in (wide, widec):
        assert (m[:, :3] == -7).all() and (m[:, 3 + cols:] == -7).all()
    with pytest.raises(ValueError, match="contiguous along its columns"):
        crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, out=torch.zeros(rows, 2 * cols)[:, ::2])


@pytest.mark.parametrize("G", [3, 5])
def test_cpu_batch_is_the_loop_of_labelmap_ordered(G):
    import crw_hip
    T, N, M, rows, cols = 5, 7, 3, 37, 61
    L = torch.stack([dr.dirichlet_rows(T, N, M, seed=10 + g) for g in range(G)])
    order = (2, 0, 1)
    lab, conf = crw_hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, confidence="entropy")
    assert lab.shape == (G, rows, cols) and lab.dtype == torch.int8 and conf.shape == (G, rows, cols)
    for g in range(G):
        one, onec = crw_hip.labelmap_ordered(L[g], T, N, M, rows, cols, order, confidence="entropy", dtype=torch.int8)
        assert torch.equal(lab[g], one) and torch.equal(conf[g], onec)
    assert len({m.numpy().tobytes() for m in lab}) == G


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_in_python():
    import crw_hip
    T, N, M, rows, cols = 5, 7, 3, 37, 29
    L = dr.dirichlet_rows(T, N, M)
    for bad in ((0, 0, 1), (0, 3), (-1, 0), (1,), (0, 1, 2, 0), (), 2):
        with pytest.raises(ValueError, match="order"):
            crw_hip.labelmap_ordered(L, T, N, M, rows, cols, bad)
    for bad in (dict(rows=0), dict(cols=0), dict(T=0), dict(M=1), dict(M=17)):
        a = dict(T=T, N=N, M=M, rows=rows, cols=cols)
        a.update(bad)
        with pytest.raises(ValueError):
            crw_hip.labelmap_ordered(L, order=(0, 1), **a)
    with pytest.raises(ValueError):
        crw_hip.labelmap_ordered(L, T, N, M, rows, cols, (0, 1), out_conf=torch.zeros(rows, cols))  # no kind
    sig = inspect.signature(crw_hip.labelmap_ordered).parameters
    assert [k for k, v in sig.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["confidence", "flip", "dtype", "out", "out_conf",
                                                                                     "workspace"]
    assert sig["dtype"].default is torch.float32 and inspect.signature(crw_hip.labelmap_ordered_batch).parameters["dtype"].default is torch.int8


def test_header_binding_and_status_codes_at_abi_8():
    """Every refusal comes before a launch (no device needed); 16 is a pointer that is never followed."""
    import ctypes
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^int\s+crw_labelmap_ordered\(const float \*L, int T, int N, int M, int rows, int cols, int flip, const int \*order_host, "
                     r"int S,\s+int conf_kind, void \*labels, int label_dtype, float \*conf, size_t ld, void \*ws, size_t ws_bytes,\s+"
                     r"crw_stream_t stream\);", header, re.M)
    assert re.search(r"^int\s+crw_labelmap_ordered_batch\(const float \*L, int G, ", header, re.M)
    assert re.search(r"^size_t\s+crw_labelmap_ordered_workspace\(int G, int rows, int cols\);", header, re.M)
    assert "crw_labelmap_ordered_batch (crw_hip.has_ordered())" in header
    assert crw_hip.ORDERED_ENTRY_POINTS == ("crw_labelmap_ordered_workspace", "crw_labelmap_ordered", "crw_labelmap_ordered_batch")
    assert len(crw_hip.SIGNATURES["crw_labelmap_ordered"][1]) == 17 and len(crw_hip.SIGNATURES["crw_labelmap_ordered_batch"][1]) == 19
    lib = crw_hip.lib()
    assert lib.crw_abi_version() == crw_hip.ABI_VERSION == 8 and crw_hip.has_ordered()
    need = lib.crw_labelmap_ordered_workspace(1, 8, 8)
    assert need >= 8 * 8 * 2 and lib.crw_labelmap_ordered_workspace(3, 8, 8) == 3 * need
    assert crw_hip.labelmap_ordered_workspace(1, 8, 8) == need
    ok = dict(L=16, T=4, N=4, M=4, rows=8, cols=8, flip=0, order=(0, 1, 2, 3), kind=-1, labels=16, dt=0, conf=None, ld=8, ws=16, wsb=need)

    def call(**bad):
        a = dict(ok, **bad)
        order = None if a["order"] is None else (ctypes.c_int * len(a["order"]))(*a["order"])
        S = a.get("S", 0 if a["order"] is None else len(a["order"]))
        one = lib.crw_labelmap_ordered(a["L"], a["T"], a["N"], a["M"], a["rows"], a["cols"], a["flip"], order, S, a["kind"], a["labels"],
                                       a["dt"], a["conf"], a["ld"], a["ws"], a["wsb"], None)
        many = lib.crw_labelmap_ordered_batch(a["L"], 1, a["T"], a["N"], a["M"], a["rows"], a["cols"], a["flip"], order, S, a["kind"],
                                              a["labels"], a["dt"], a["conf"], a["ld"], a["rows"] * a["ld"], a["ws"], a["wsb"], None)
        assert one == many, bad
        return one

    for bad in (dict(order=(0, 1, 1)), dict(order=(0, 4)), dict(order=(-1, 0)), dict(order=(2,)), dict(order=(0, 1, 2, 3, 0)),
                dict(order=(0, 1, 2), M=2), dict(order=None), dict(order=(0, 1), S=1), dict(ws=None), dict(ws=17),
                # dense_launch's checks
                dict(L=None), dict(labels=None), dict(T=0), dict(N=0), dict(M=1), dict(M=17), dict(rows=0), dict(cols=0),
                dict(rows=(1 << 22) + 1), dict(cols=(1 << 22) + 1), dict(kind=3), dict(kind=-2), dict(kind=0), dict(conf=16),
                dict(dt=2), dict(ld=7), dict(labels=18)):
        assert call(**bad) == crw_hip.CRW_EINVAL, bad
    assert call(wsb=need - 1) == crw_hip.CRW_EWORKSPACE and call(wsb=0) == crw_hip.CRW_EWORKSPACE
    assert lib.crw_labelmap_ordered_batch(16, 0, 4, 4, 4, 8, 8, 0, (ctypes.c_int * 2)(0, 1), 2, -1, 16, 0, None, 8, 64, 16, need, None) \
        == crw_hip.CRW_EINVAL  # G = 0


def test_a_library_without_the_ordered_entry_points_is_named_stale(monkeypatch):
    import crw_hip
    crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "ordered", False)
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*crw_labelmap_ordered.*rebuild"):
        crw_hip._ordered_lib()


# ---- 7. the quality claim ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", od.SEEDS)
@pytest.mark.parametrize("case", od.QUALITY, ids=str)
def test_ordered_map_on_layered_items_with_wrong_nodes(case, seed):
    import crw_hip
    T, N, rows, cols, temp, M, share = case
    gt, L = od.layered_case(*case, seed)
    L = torch.tensor(L)
    dense, _ = crw_hip.labelmap_dense(L, T, N, M, rows, cols)
    lab, _ = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, range(M))
    od.check_quality(gt, dense.numpy(), lab.numpy(), M, f"cpu {case} seed {seed}")


# ---- 8. segment / segment_sweep / the command lines ---------------------------------------------------------------------------------------
def test_segment_argument_errors():
    import inference as crw_inference
    ds, seg, lp, M, T = synthetic_case(n_rg=1)
    run = lambda **kw: crw_inference.segment(ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0), device="cpu", **kw)
    with pytest.raises(ValueError, match=r"decode must be 'argmax' or 'ordered' \(got 'viterbi'\)"):
        run(decode="viterbi")
    with pytest.raises(ValueError, match="decode='ordered' needs upsample='bilinear'"):
        run(decode="ordered", order=(0, 1, 2, 3, 4))
    with pytest.raises(ValueError, match="decode='ordered' needs upsample='bilinear'"):
        run(decode="ordered", order=(0, 1, 2, 3, 4), upsample="nearest")
    with pytest.raises(ValueError, match="decode='ordered' needs an order"):
        run(decode="ordered", upsample="bilinear")
    with pytest.raises(ValueError, match="order needs decode='ordered'"):
        run(order=(0, 1), upsample="bilinear")
    with pytest.raises(ValueError, match="distinct classes"):
        run(decode="ordered", upsample="bilinear", order=(0, 0, 1))
    with pytest.raises(ValueError, match="distinct classes"):
        run(decode="ordered", upsample="bilinear", order=(0, 5))
    for fn in (crw_inference.segment, crw_inference.segment_sweep):
        sig = inspect.signature(fn).parameters
        assert (sig["decode"].default, sig["order"].default) == ("argmax", None)


@pytest.mark.parametrize("merge", ["rule", "confidence"])
def test_segment_ordered_on_the_oracle(monkeypatch, merge):
    """`segment(upsample='bilinear', decode='ordered')` on the CPU: every pass's window is `labelmap_ordered` of that pass's soft
    labels -- the correction's tail spliced, the reverse pass mirrored; passes, merges and confidence as without the decode."""
    import crw_hip
    import inference as crw_inference
    M, T = 5, 8
    rg_len = T * 8
    changes = [5, None]
    order = (0, 1, 2, 3, 4)

    def segment(**kw):
        ds, seg, lp, _, _ = synthetic_case(n_rg=2)
        monkeypatch.setattr(crw_inference, "propagate", forced(oracle_propagate_soft, changes, T))
        return crw_inference.segment(ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0), correction=True, use_last=True, dataset_id=3,
                                     device="cpu", confidence="maxprob", merge=merge, upsample="bilinear", **kw)

    plain, out = segment(), segment(decode="ordered", order=order)
    assert set(out) == set(plain) | {"decode", "order"} and out["decode"] == "ordered" and out["order"] == list(order)
    assert "decode" not in plain and out["change_idx"] == plain["change_idx"] == changes
    assert torch.equal(out["forward_conf"], plain["forward_conf"])  # the confidence does not depend on the decode
    # by hand
    ds, seg, lp, _, _ = synthetic_case(n_rg=2)
    rows, N = seg.shape[0], ds[0].shape[1]
    ordered = lambda L, frames, cols: crw_hip.labelmap_ordered(L, frames, N, M, rows, cols, order, confidence="maxprob")
    run = lambda seq, ref, last: oracle_propagate_soft(seq, ref, Flatten(), lp, M, False, last, soft=True)[-1]
    fl, fc = zip(*[ordered(run(ds[t * T], seg[:N * 4 + 4, rg_len * t:rg_len * t + 8], False), T, rg_len) for t in range(2)])
    fl, fc = [m.clone() for m in fl], [m.clone() for m in fc]
    px = (T - 5) * 8
    tail = ordered(run(ds.get_smaller_item(0, T - 5), seg[:, rg_len - px:rg_len - px + 8], False), T - 5, px)
    fl[0][:, rg_len - px:], fc[0][:, rg_len - px:] = tail
    fwd, fconf = torch.cat(fl, 1), torch.cat(fc, 1)
    assert torch.equal(out["forward"], fwd) and torch.equal(out["forward_conf"], fconf)
    assert (fwd[1:] >= fwd[:-1]).all()  # the guarantee: forward is monotone in order down every column
    rl, rc = [], []
    for t in range(2):  # the reverse pass runs on the items the correction shortened
        seq = ds[t * T]
        lab, conf = ordered(run(seq, torch.flip(seg[:, rg_len * t:rg_len * (t + 1)], (-1,))[:, :8], True), seq.shape[0], rg_len)
        rl.append(torch.flip(lab, (-1,)))
        rc.append(torch.flip(conf, (-1,)))
    rev, rconf = torch.cat(rl, 1), torch.cat(rc, 1)
    take = rconf > fconf if merge == "confidence" else crw_inference._reverse_rule_mask(fwd, rev, 3).view_as(fwd)
    assert torch.equal(out["pred"], torch.where(take, rev, fwd)) and torch.equal(out["conf"], torch.where(take, rconf, fconf))


def test_segment_sweep_ordered_equals_segment_per_configuration(monkeypatch):
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    M, T = 5, 8
    changes = [5, None]
    sweep = LabelPropSweep(SWEEP_GRID["cxt_size"], SWEEP_GRID["radii"][:1], SWEEP_GRID["temps"], SWEEP_GRID["knns"])
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cpu", confidence="margin", merge="confidence", upsample="bilinear",
              decode="ordered", order=(0, 1, 2, 4))
    ds, seg, _, _, _ = synthetic_case(n_rg=2)
    monkeypatch.setattr(crw_inference, "propagate_sweep", forced(oracle_propagate_sweep_soft, changes, T))
    out = crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), **kw)
    assert out["decode"] == "ordered" and out["order"] == [0, 1, 2, 4] and out["forward"].dtype == torch.int8
    assert not (out["forward"] == 3).any()  # a class outside the order is never written
    for g, cfg in enumerate(sweep.configs):
        ds, seg, _, _, _ = synthetic_case(n_rg=2)
        monkeypatch.setattr(crw_inference, "propagate", forced(oracle_propagate_soft, changes, T))
        one = crw_inference.segment(ds, seg, Flatten(), LabelPropVOS_CRW(cfg), M, T, (8, 8), (4, 0), **kw)
        for k in ("pred", "forward"):
            assert torch.equal(out[k][g], one[k].to(torch.int8)), (cfg, k)
        for k in ("conf", "forward_conf"):
            assert torch.equal(out[k][g], one[k]), (cfg, k)


def test_cli_decode_flags():
    from test_sweep_dense_gpu import _cli
    for name in ("segment_all", "segment_sweep"):
        cli = _cli(name)
        p = cli.get_args_parser()
        base = ["--synthetic", "40", "192"]
        check = lambda extra: cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + extra)))
        a = check([])
        assert (a.decode, a.order) == ("argmax", None)
        a = check(["--upsample", "bilinear", "--decode", "ordered", "--order", "0", "1", "2", "3"])
        assert (a.decode, a.order) == ("ordered", [0, 1, 2, 3])
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--decode", "viterbi"])
        for bad in (["--decode", "ordered", "--order", "0", "1"], ["--upsample", "bilinear", "--decode", "ordered"],
                    ["--upsample", "bilinear", "--order", "0", "1"]):
            with pytest.raises(SystemExit, match="--order|--decode"):
                check(bad)


def test_cli_ordered_run_and_report(monkeypatch, capsys, tmp_path):
    """`segment_all.main` on the CPU with the oracle: the json gains decode / order, and the horizon table at --min_run 1 finds
    every layer at most once per column (the map is monotone)."""
    import json
    import inference as crw_inference
    from test_sweep_dense_gpu import _cli
    cli = _cli("segment_all")
    monkeypatch.setattr(crw_inference, "propagate", oracle_propagate_soft)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    js = tmp_path / "r.json"
    args = ["--synthetic", "40", "128", "--dataset", "3", "--patch_size", "8", "8", "--overlap", "4", "0", "--seq_length", "8", "-c", "4",
            "-r", "4", "-k", "5", "--model", "0", "--output_folder", str(tmp_path / "out"), "--report_json", str(js), "--upsample", "bilinear",
            "--decode", "ordered", "--order", "0", "1", "2", "3", "4", "--horizons", "--min_run", "1"]
    cli.main(cli.get_args_parser().parse_args(args))
    text = capsys.readouterr().out
    d = json.load(open(js))
    assert d["decode"] == "ordered" and d["order"] == [0, 1, 2, 3, 4] and d["upsample"] == "bilinear" and "horizons" in d
    assert "decode='ordered'" in text and "order=[0, 1, 2, 3, 4]" in text
    saved = torch.load(tmp_path / "out" / "predicted_map.pt").long()
    assert (saved[1:] >= saved[:-1]).all()
