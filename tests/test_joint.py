"""The order-preserving merge of the reverse pass on the host: the CPU route of `crw_hip.labelmap_ordered_joint` against its
definition (joint_ref.py) -- the same source twice is `labelmap_ordered`, conf is the confidence merge's bit for bit, the labels
teacher-forced on `took` against the fp64 decode of the selected rows --, the quality claim on the nine paired layered items, and
the host surface: argument and option errors, the `joint` entry-point group, the pinned signatures, the header,
`segment(..., merge='ordered')`, `segment_sweep` and the command lines.  The kernel's twins are in test_joint_gpu.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dense_ref as dr
import joint_ref as jr
import ordered_ref as od
from conftest import ROOT
from test_confidence import Flatten, synthetic_case
from test_dense import oracle_propagate_soft
from test_sweep_dense import SWEEP_GRID, forced, oracle_propagate_sweep_soft

CASE_IDS = [jr.case_id(c) for c in jr.CASES]


# ---- 1. the same source twice is labelmap_ordered -------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(jr.CASES)), ids=CASE_IDS)
def test_the_same_source_twice_is_labelmap_ordered(index):
    """Both sources of the case, each against itself: a tie keeps a, so the map is columns [col0, col0 + ncols) of the
    full-width `labelmap_ordered` map of that source, labels and conf bit for bit (cases 2, 3, 4, 5, 6 and 7 have col0 > 0)."""
    import crw_hip
    c = jr.case(index)
    N, M, rows, ncols, order = c.shared
    for k in (0, 1):
        src = c.source(k)
        L, T, cols, col0, flip = src
        for kind in dr.KINDS:
            lab, conf = crw_hip.labelmap_ordered_joint(src, src, N, M, rows, ncols, order, confidence=kind, dtype=torch.int8)
            want, wantc = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence=kind, flip=flip, dtype=torch.int8)
            assert lab.shape == (rows, ncols) and lab.dtype == torch.int8 and conf.dtype == torch.float32
            assert torch.equal(lab, want[:, col0:col0 + ncols]) and torch.equal(conf, wantc[:, col0:col0 + ncols])


# ---- 2. conf bit for bit, 3. the labels teacher-forced on took ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dr.KINDS)
@pytest.mark.parametrize("index", range(len(jr.CASES)), ids=CASE_IDS)
def test_cpu_route_against_the_definition(index, kind):
    import crw_hip
    c = jr.case(index)
    lab, conf = crw_hip.labelmap_ordered_joint(c.source(0), c.source(1), *c.shared, confidence=kind)
    assert lab.dtype == torch.float32 and lab.shape == conf.shape == (c.rows, c.ncols)
    jr.check_against_the_definition(crw_hip, c, lab, conf, kind, what=f"cpu {CASE_IDS[index]} {kind}")


def test_windows_and_batch_on_the_cpu():
    import crw_hip
    c = jr.case(2)
    N, M, rows, ncols, order = c.shared
    lab, conf = crw_hip.labelmap_ordered_joint(c.source(0), c.source(1), *c.shared, confidence="margin", dtype=torch.int8)
    wide, widec = torch.full((rows, ncols + 7), -7, dtype=torch.int8), torch.full((rows, ncols + 7), -7.0)
    out, outc = crw_hip.labelmap_ordered_joint(c.source(0), c.source(1), *c.shared, confidence="margin", dtype=torch.int8,
                                               out=wide[:, 3:3 + ncols], out_conf=widec[:, 3:3 + ncols])
    assert out.data_ptr() == wide[:, 3:].data_ptr() and torch.equal(wide[:, 3:3 + ncols], lab) and torch.equal(widec[:, 3:3 + ncols], conf)
    for m in (wide, widec):
        assert (m[:, :3] == -7).all() and (m[:, 3 + ncols:] == -7).all()
    G = 3
    Ls = [torch.stack([dr.dirichlet_rows(T, N, M, seed=70 + 5 * g + k) for g in range(G)]) for k, (T, _, _, _) in enumerate(c.geo)]
    labs, confs = crw_hip.labelmap_ordered_joint_batch(c.source(0, Ls[0]), c.source(1, Ls[1]), G, *c.shared, confidence="entropy")
    assert labs.shape == (G, rows, ncols) and labs.dtype == torch.int8 and confs.shape == (G, rows, ncols)
    for g in range(G):
        one, onec = crw_hip.labelmap_ordered_joint(c.source(0, Ls[0][g]), c.source(1, Ls[1][g]), *c.shared, confidence="entropy",
                                                   dtype=torch.int8)
        assert torch.equal(labs[g], one) and torch.equal(confs[g], onec)
    assert len({m.numpy().tobytes() for m in labs}) == G


# ---- 4. the quality claim -----------------------------------------------------------------------------------------------------------
def test_joint_map_on_the_nine_paired_layered_items():
    """The counts of the CPU route (README "Evaluation" quotes them): per case the joint map never steps back, has at most
    1.05 x the wrong pixels of the confidence merge of the two ordered maps and at most M - 1 changes in a column; over the nine
    cases the merge steps back somewhere and the joint map has at most 0.9 x its wrong pixels."""
    import crw_hip
    counts = [jr.quality_counts(crw_hip, i) for i in range(len(jr.PAIRS))]
    for c in counts:
        jr.check_quality(c)
    merge, back, joint = (sum(c[i] for c in counts) for i in (0, 1, 2))
    print(f"total: merge {merge} wrong pixels, {back} columns step back; joint {joint} wrong pixels, ratio {joint / merge:.3f}")
    assert back >= 1
    assert joint <= 0.9 * merge


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_in_python():
    import crw_hip
    c = jr.case(2)
    N, M, rows, ncols, order = c.shared
    a, b = c.source(0), c.source(1)
    run = lambda a=a, b=b, **kw: crw_hip.labelmap_ordered_joint(a, b, N, M, rows, ncols, order, **{"confidence": "maxprob", **kw})
    with pytest.raises(ValueError, match="col0"):
        run(b=(b[0], 12, 84, 65, True))  # col0 + ncols > cols
    with pytest.raises(ValueError, match="col0"):
        run(a=(a[0], 3, 20, -1, False))
    with pytest.raises(ValueError, match="needs a confidence kind"):
        run(confidence=None)
    with pytest.raises(TypeError):
        crw_hip.labelmap_ordered_joint(a, b, N, M, rows, ncols, order)  # the kind is mandatory: a keyword without a default
    with pytest.raises(ValueError, match="confidence kind must be one of"):
        run(confidence="vote")
    with pytest.raises(ValueError, match="L must be float32"):
        run(a=(a[0][:-1], 3, 20, 0, False))
    with pytest.raises(ValueError, match="L must be float32"):
        run(b=(b[0], 11, 84, 64, True))
    with pytest.raises(ValueError, match="share one pitch"):
        run(out=torch.zeros(rows, ncols + 1)[:, :ncols], out_conf=torch.zeros(rows, ncols + 2)[:, :ncols])
    with pytest.raises(ValueError, match="contiguous along its columns"):
        run(out=torch.zeros(rows, 2 * ncols)[:, ::2])
    with pytest.raises(ValueError, match="order"):
        run_order = lambda order: crw_hip.labelmap_ordered_joint(a, b, N, M, rows, ncols, order, confidence="maxprob")
        run_order((0, 0, 1))
    for bad in (dict(rows=0), dict(ncols=0), dict(N=0), dict(M=1), dict(M=17)):
        args = dict(N=N, M=M, rows=rows, ncols=ncols)
        args.update(bad)
        with pytest.raises(ValueError):
            crw_hip.labelmap_ordered_joint(a, b, order=(0, 1), confidence="maxprob", **args)
    with pytest.raises(ValueError, match="G must be"):
        crw_hip.labelmap_ordered_joint_batch(a, b, 0, N, M, rows, ncols, order, confidence="maxprob")
    sig = inspect.signature(crw_hip.labelmap_ordered_joint).parameters
    assert list(sig)[:7] == ["a", "b", "N", "M", "rows", "ncols", "order"]
    assert [k for k, v in sig.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["confidence", "dtype", "out", "out_conf", "workspace"]
    assert sig["dtype"].default is torch.float32
    assert inspect.signature(crw_hip.labelmap_ordered_joint_batch).parameters["dtype"].default is torch.int8


# ---- 6. the group, the signatures, the header -----------------------------------------------------------------------------------------
def test_the_joint_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    """test_host.py's stale-library test for the group `joint`."""
    import crw_hip
    group = "joint"
    names = getattr(crw_hip, f"{group.upper()}_ENTRY_POINTS")
    has, checked_lib = getattr(crw_hip, f"has_{group}"), getattr(crw_hip, f"_{group}_lib")
    assert names and set(names) <= set(crw_hip.SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS[group] is names
    assert has() is True and checked_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, group, False)
    assert has() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        checked_lib()
    assert all(name in str(err.value) for name in names)
    c = jr.case(2)  # the CPU route needs no library
    crw_hip.labelmap_ordered_joint(c.source(0), c.source(1), *c.shared, confidence="maxprob")


def test_header_binding_and_status_codes_at_abi_8():
    """Every refusal comes before a launch (no device needed); 16 is a pointer that is never followed."""
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^#define\s+CRW_ABI_VERSION\s+8\s*$", header, re.M)
    assert re.search(r"^int\s+crw_labelmap_ordered_joint\(const float \*La, int Ta, int cols_a, int col0_a, int flip_a, const float \*Lb, "
                     r"int Tb, int cols_b,\s+int col0_b, int flip_b, int N, int M, int rows, int ncols, const int \*order_host, int S,\s+"
                     r"int conf_kind, void \*labels, int label_dtype, float \*conf, size_t ld, void \*ws, size_t ws_bytes,\s+"
                     r"crw_stream_t stream\);", header, re.M)
    assert re.search(r"^int\s+crw_labelmap_ordered_joint_batch\(const float \*La, .*?int flip_b, int G, int N, ", header, re.M | re.S)
    assert "crw_labelmap_ordered_joint, crw_labelmap_ordered_joint_batch (crw_hip.has_joint())" in header
    assert crw_hip.JOINT_ENTRY_POINTS == ("crw_labelmap_ordered_joint", "crw_labelmap_ordered_joint_batch")
    assert crw_hip.ORDERED_ENTRY_POINTS == ("crw_labelmap_ordered_workspace", "crw_labelmap_ordered", "crw_labelmap_ordered_batch")
    assert len(crw_hip.SIGNATURES["crw_labelmap_ordered_joint"][1]) == 24
    assert len(crw_hip.SIGNATURES["crw_labelmap_ordered_joint_batch"][1]) == 26
    lib = crw_hip.lib()
    assert lib.crw_abi_version() == crw_hip.ABI_VERSION == 8 and crw_hip.has_joint()
    need = lib.crw_labelmap_ordered_workspace(1, 8, 8)
    ok = dict(La=16, Ta=4, ca=8, oa=0, fa=0, Lb=16, Tb=3, cb=20, ob=12, fb=1, N=4, M=4, rows=8, ncols=8, order=(0, 1, 2, 3), kind=0,
              labels=16, dt=0, conf=16, ld=8, ws=16, wsb=need)

    def call(**bad):
        a = dict(ok, **bad)
        order = None if a["order"] is None else (ctypes.c_int * len(a["order"]))(*a["order"])
        S = a.get("S", 0 if a["order"] is None else len(a["order"]))
        sources = (a["La"], a["Ta"], a["ca"], a["oa"], a["fa"], a["Lb"], a["Tb"], a["cb"], a["ob"], a["fb"])
        one = lib.crw_labelmap_ordered_joint(*sources, a["N"], a["M"], a["rows"], a["ncols"], order, S, a["kind"], a["labels"], a["dt"],
                                             a["conf"], a["ld"], a["ws"], a["wsb"], None)
        many = lib.crw_labelmap_ordered_joint_batch(*sources, 1, a["N"], a["M"], a["rows"], a["ncols"], order, S, a["kind"], a["labels"],
                                                    a["dt"], a["conf"], a["ld"], a["rows"] * a["ld"], a["ws"], a["wsb"], None)
        assert one == many, bad
        return one

    for bad in (dict(La=None), dict(Lb=None), dict(La=18), dict(Lb=18), dict(Ta=0), dict(Tb=0), dict(ca=0), dict(cb=0),
                dict(ca=(1 << 22) + 1, oa=0), dict(cb=(1 << 22) + 1), dict(oa=-1), dict(ob=-1), dict(oa=1), dict(ob=13),
                dict(ncols=9, ld=9), dict(kind=-1), dict(kind=-1, conf=None), dict(kind=3), dict(kind=3, conf=None), dict(kind=-2),
                # the order's and the workspace's
                dict(order=(0, 1, 1)), dict(order=(0, 4)), dict(order=(-1, 0)), dict(order=(2,)), dict(order=(0, 1, 2, 3, 0)),
                dict(order=(0, 1, 2), M=2), dict(order=None), dict(order=(0, 1), S=1), dict(ws=None), dict(ws=17),
                # the shared window's
                dict(labels=None), dict(N=0), dict(M=1), dict(M=17), dict(rows=0), dict(ncols=0), dict(rows=(1 << 22) + 1),
                dict(dt=2), dict(ld=7), dict(labels=18), dict(conf=18)):
        assert call(**bad) == crw_hip.CRW_EINVAL, bad
    assert call(wsb=need - 1) == crw_hip.CRW_EWORKSPACE and call(wsb=0) == crw_hip.CRW_EWORKSPACE
    assert call(wsb=need - 1, conf=None) == crw_hip.CRW_EWORKSPACE  # conf may be null: the labels alone
    order = (ctypes.c_int * 2)(0, 1)
    assert lib.crw_labelmap_ordered_joint_batch(16, 4, 8, 0, 0, 16, 4, 8, 0, 1, 0, 4, 4, 8, 8, order, 2, 0, 16, 0, None, 8, 64, 16, need,
                                                None) == crw_hip.CRW_EINVAL  # G = 0


# ---- 7. segment / segment_sweep / the command lines -----------------------------------------------------------------------------------
def test_segment_option_errors():
    import inference as crw_inference
    ds, seg, lp, M, T = synthetic_case(n_rg=1)
    order = (0, 1, 2, 3, 4)
    for fn, extra in ((crw_inference.segment, (lp,)), (crw_inference.segment_sweep, (None,))):
        run = lambda **kw: fn(ds, seg, Flatten(), *extra, M, T, (8, 8), (4, 0), device="cpu", **kw)
        with pytest.raises(ValueError, match=r"merge must be 'rule' or 'confidence' \(got 'vote'\).*'ordered'"):
            run(merge="vote")
        with pytest.raises(ValueError, match="merge='ordered' needs decode='ordered'"):
            run(merge="ordered", confidence="maxprob", upsample="bilinear")
        with pytest.raises(ValueError, match="merge='ordered' needs decode='ordered'"):
            run(merge="ordered", confidence="maxprob", upsample="bilinear", decode="argmax")
        with pytest.raises(ValueError, match="merge='ordered' needs a confidence kind"):
            run(merge="ordered", upsample="bilinear", decode="ordered", order=order)
        with pytest.raises(ValueError, match="decode='ordered' needs upsample='bilinear'"):
            run(merge="ordered", confidence="maxprob", decode="ordered", order=order)
        with pytest.raises(ValueError, match="decode='ordered' needs an order"):
            run(merge="ordered", confidence="maxprob", upsample="bilinear", decode="ordered")
        with pytest.raises(ValueError, match="confidence must be None or one of"):
            run(merge="ordered", confidence="vote", upsample="bilinear", decode="ordered", order=order)


def monotone(labels, order):
    return jr.steps_back(labels.cpu().numpy(), order) == 0


@pytest.mark.parametrize("correction", [False, True], ids=["", "correction"])
def test_segment_merge_ordered_on_the_oracle(monkeypatch, correction):
    """`segment(..., merge='ordered')` on the CPU against merge='confidence' under the same options, and against the joint calls
    assembled by hand: one per radargram, head and tail where the correction succeeded; any dataset id."""
    import crw_hip
    import inference as crw_inference
    M, T = 5, 8
    rg_len = T * 8
    changes = [5, None]
    order = (0, 1, 2, 3, 4)

    def segment(**kw):
        ds, seg, lp, _, _ = synthetic_case(n_rg=2)
        monkeypatch.setattr(crw_inference, "propagate", forced(oracle_propagate_soft, changes, T))
        return crw_inference.segment(ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0), correction=correction, use_last=True, dataset_id=2,
                                     device="cpu", confidence="maxprob", upsample="bilinear", decode="ordered", order=order, **kw)

    plain, out = segment(merge="confidence"), segment(merge="ordered")
    assert set(out) == set(plain)
    for k in ("conf", "forward", "forward_conf"):
        assert torch.equal(out[k], plain[k]), k
    assert monotone(out["pred"], order) and monotone(out["forward"], order)
    assert out["pred"].dtype == torch.float32 and not torch.equal(out["pred"], out["forward"])
    # by hand
    ds, seg, lp, _, _ = synthetic_case(n_rg=2)
    rows, N = seg.shape[0], ds[0].shape[1]
    run = lambda seq, ref, last: oracle_propagate_soft(seq, ref, Flatten(), lp, M, False, last, soft=True)[-1]
    fwd = [run(ds[t * T], seg[:N * 4 + 4, rg_len * t:rg_len * t + 8], False) for t in range(2)]
    px = (T - 5) * 8 if correction else 0
    if correction:
        tail = run(ds.get_smaller_item(0, T - 5), seg[:, rg_len - px:rg_len - px + 8], False)
    joint = lambda a, b, ncols: crw_hip.labelmap_ordered_joint(a, b, N, M, rows, ncols, order, confidence="maxprob")
    for t in range(2):  # the reverse pass runs on the items the correction shortened
        seq = ds[t * T]
        rev = (run(seq, torch.flip(seg[:, rg_len * t:rg_len * (t + 1)], (-1,))[:, :8], True), seq.shape[0], rg_len)
        cut = px if t == 0 else 0
        lab, conf = joint((fwd[t], T, rg_len, 0, False), (*rev, 0, True), rg_len - cut)
        if cut:
            tl, tc = joint((tail, T - 5, px, 0, False), (*rev, rg_len - px, True), px)
            lab, conf = torch.cat([lab, tl], 1), torch.cat([conf, tc], 1)
        assert torch.equal(out["pred"][:, rg_len * t:rg_len * (t + 1)], lab)
        assert torch.equal(out["conf"][:, rg_len * t:rg_len * (t + 1)], conf)


def test_segment_sweep_merge_ordered_equals_segment_per_configuration(monkeypatch):
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    M, T = 5, 8
    changes = [5, None]
    order = (0, 1, 2, 4)
    sweep = LabelPropSweep(SWEEP_GRID["cxt_size"], SWEEP_GRID["radii"][:1], SWEEP_GRID["temps"], SWEEP_GRID["knns"])
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cpu", confidence="margin", merge="ordered", upsample="bilinear",
              decode="ordered", order=order)
    ds, seg, _, _, _ = synthetic_case(n_rg=2)
    monkeypatch.setattr(crw_inference, "propagate_sweep", forced(oracle_propagate_sweep_soft, changes, T))
    out = crw_inference.segment_sweep(ds, seg, Flatten(), sweep, M, T, (8, 8), (4, 0), **kw)
    assert out["pred"].dtype == torch.int8 and not (out["pred"] == 3).any()
    for g, cfg in enumerate(sweep.configs):
        ds, seg, _, _, _ = synthetic_case(n_rg=2)
        monkeypatch.setattr(crw_inference, "propagate", forced(oracle_propagate_soft, changes, T))
        one = crw_inference.segment(ds, seg, Flatten(), LabelPropVOS_CRW(cfg), M, T, (8, 8), (4, 0), **kw)
        assert monotone(out["pred"][g], order)
        for k in ("pred", "forward"):
            assert torch.equal(out[k][g], one[k].to(torch.int8)), (cfg, k)
        for k in ("conf", "forward_conf"):
            assert torch.equal(out[k][g], one[k]), (cfg, k)


def test_cli_merge_flags():
    from test_sweep_dense_gpu import _cli
    for name in ("segment_all", "segment_sweep"):
        cli = _cli(name)
        p = cli.get_args_parser()
        base = ["--synthetic", "40", "192"]
        check = lambda extra: cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + extra)))
        assert check([]).merge == "rule"
        ordered = ["--upsample", "bilinear", "--decode", "ordered", "--order", "0", "1", "2", "3"]
        a = check(ordered + ["--confidence", "margin", "--merge", "ordered"])
        assert (a.merge, a.decode, a.confidence) == ("ordered", "ordered", "margin")
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--merge", "vote"])
        for bad in (["--merge", "ordered", "--confidence", "margin", "--upsample", "bilinear"],  # no --decode ordered
                    ordered + ["--merge", "ordered"]):                                           # no --confidence
            with pytest.raises(SystemExit, match="--merge ordered needs --decode ordered and --confidence"):
                check(bad)
        with pytest.raises(SystemExit, match="--decode ordered needs --upsample bilinear"):
            check(["--merge", "ordered", "--confidence", "margin", "--decode", "ordered", "--order", "0", "1"])


def test_cli_merge_ordered_run_and_report(monkeypatch, capsys, tmp_path):
    """`segment_all.main` on the CPU with the oracle: --merge ordered writes the keys --merge confidence writes, and the
    calibration's merge entry names it."""
    import json
    import inference as crw_inference
    from test_sweep_dense_gpu import _cli
    cli = _cli("segment_all")
    monkeypatch.setattr(crw_inference, "propagate", oracle_propagate_soft)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    reports = {}
    for merge in ("confidence", "ordered"):
        js = tmp_path / f"{merge}.json"
        args = ["--synthetic", "40", "128", "--dataset", "3", "--patch_size", "8", "8", "--overlap", "4", "0", "--seq_length", "8", "-c",
                "4", "-r", "4", "-k", "5", "--model", "0", "--output_folder", str(tmp_path / merge), "--report_json", str(js), "--upsample",
                "bilinear", "--decode", "ordered", "--order", "0", "1", "2", "3", "4", "--use_last", "true", "--confidence", "maxprob",
                "--merge", merge]
        cli.main(cli.get_args_parser().parse_args(args))
        capsys.readouterr()
        reports[merge] = json.load(open(js))
    assert set(reports["ordered"]) == set(reports["confidence"])
    assert reports["ordered"]["calibration"]["merge"] == "ordered" and reports["ordered"]["decode"] == "ordered"
