"""The dense label map on the host: the fp64 helper (dense_ref.py) against torch's bilinear interpolation, the CPU route of
`crw_hip.labelmap_dense` against the helper under the bound B, the exact dyadic cases and their ties, the convexity property, the
quality claim on synthetic boundaries, and the host surface (`propagate(soft=True)`, `segment(upsample=...)`, the ABI tables, the
command line).  The kernel's twins are in test_dense_gpu.py."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import dense_ref as dr
from conftest import PKG, ROOT
from test_confidence import Flatten, oracle_soft_labels, synthetic_case
from oracle import crw_oracle as orc


# ---- 1. the helper is torch's bilinear interpolation ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.SHAPES, ids=str)
def test_helper_is_torch_bilinear_in_fp64(shape):
    T, N, M, rows, cols = shape
    L, ref = dr.reference(shape)
    L64 = L.double().view(T, N, M)
    want = TF.interpolate(L64.permute(2, 1, 0)[None], (rows, cols), mode="bilinear", align_corners=False)[0]
    err = float((torch.tensor(ref.probs) - want).abs().max())
    print(f"{shape}: helper against F.interpolate in fp64: {err:.3e}")
    assert err <= 1e-12
    assert np.array_equal(ref.labels, want.numpy().argmax(0)) or ref.gap.min() < 1e-12


# ---- 2. the CPU route under the bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True], ids=["", "flip"])
@pytest.mark.parametrize("shape", dr.SHAPES + [dr.SLAB], ids=str)
def test_cpu_route_against_the_helper(shape, flip):
    import crw_hip
    T, N, M, rows, cols = shape
    L, ref = dr.reference(shape)
    for kind in (None,) + dr.KINDS:
        for dtype in (torch.float32, torch.int8):
            lab, conf = crw_hip.labelmap_dense(L, T, N, M, rows, cols, confidence=kind, flip=flip, dtype=dtype)
            assert lab.shape == (rows, cols) and lab.dtype == dtype and (conf is None) == (kind is None)
            if flip:
                lab, conf = torch.flip(lab, (1,)), (torch.flip(conf, (1,)) if conf is not None else None)
            dr.check_outputs(ref, lab.numpy(), None if conf is None else conf.numpy(), kind, f"cpu {shape} {kind} {dtype}")
            if shape == dr.SLAB and dtype == torch.int8:
                break


def test_cpu_knots_are_the_integer_formula():
    import crw_hip
    for n_in, n_out in ((1, 1), (1, 7), (7, 1), (3, 16), (12, 50), (48, 410), (8, 5), (256, 8192), (5, 1 << 22)):
        i0, i1, w = crw_hip.dense_knots(n_in, n_out)
        r0, r1, rw = dr.knots(n_in, n_out)
        assert np.array_equal(i0.numpy(), r0) and np.array_equal(i1.numpy(), r1) and w.dtype == torch.float32
        assert np.array_equal(w.numpy(), rw.astype(np.float32))  # the correctly rounded quotient
        f0, f1, fw = crw_hip.dense_knots(n_in, n_out, flip=True)
        assert torch.equal(f0, i0.flip(0)) and torch.equal(f1, i1.flip(0)) and torch.equal(fw, w.flip(0))


# ---- 3. exact cases: dyadic weights on one-hot rows, ties to the lowest class -----------------------------------------------------
@pytest.mark.parametrize("shape", dr.EXACT, ids=str)
def test_exact_dyadic_case_and_ties(shape):
    import crw_hip
    T, N, M, rows, cols = shape
    L = dr.exact_rows(T, N, M)
    ref = dr.Ref(L.numpy(), T, N, M, rows, cols)
    ties = ref.gap == 0
    assert ties.any() and (ref.labels[ties] == M - 2).all()  # exact ties exist: the lower of the two tied classes
    lab, conf = crw_hip.labelmap_dense(L, T, N, M, rows, cols, confidence="maxprob")
    assert np.array_equal(lab.numpy().astype(np.int64), ref.labels)
    assert np.array_equal(conf.numpy().astype(np.float64), ref.conf["maxprob"])  # every value is a dyadic rational: exact in fp32


# ---- 4. convexity: where the four surrounding nodes agree, the dense label is theirs ------------------------------------------------
def test_where_the_neighbourhood_agrees_the_dense_label_is_the_nearest_label():
    import crw_hip
    T, N, M, rows, cols = 9, 12, 5, 50, 61
    g = torch.Generator().manual_seed(4)
    cls = ((torch.arange(N)[None, :] * 3 // N + torch.arange(T)[:, None] // 4) % M)  # patches of one class
    p = torch.rand(T, N, M, generator=g) * 0.15
    p.scatter_(2, cls[..., None], 0.6 + 0.2 * torch.rand(T, N, 1, generator=g))
    L = (p / p.sum(-1, keepdim=True)).reshape(T * N, M)
    s = L.sort(-1).values
    assert float((s[:, -1] - s[:, -2]).min()) >= 0.05
    node = L.view(T, N, M).argmax(-1)
    i0, i1, _ = crw_hip.dense_knots(N, rows)
    j0, j1, _ = crw_hip.dense_knots(T, cols)
    four = torch.stack([node[j[None, :], i[:, None]] for i in (i0, i1) for j in (j0, j1)])  # [4, rows, cols]
    agree = (four == four[0]).all(0)
    assert agree.any() and not agree.all()
    lab, _ = crw_hip.labelmap_dense(L, T, N, M, rows, cols)
    nearest = TF.interpolate(node.t()[None, None].float(), size=(rows, cols), mode="nearest")[0, 0]
    assert torch.equal(lab[agree], nearest[agree]) and torch.equal(lab[agree], four[0][agree].float())


# ---- 5. the quality claim ---------------------------------------------------------------------------------------------------------
def boundary_case(T, N, rows, cols, temp):
    """Two synthetic boundaries (one curved, one sloped) -> (gt [rows, cols], L float32 [T*N, 3]): node (n, t) sits at the centre
    of its cell, its soft labels a sigmoid of its distance to each boundary in units of temp node rows."""
    b1 = lambda c: 0.3 * rows + 0.1 * rows * np.sin(5 * c / cols)
    b2 = lambda c: 0.65 * rows + 0.15 * rows * c / cols
    r, c = np.arange(rows, dtype=np.float64)[:, None], np.arange(cols, dtype=np.float64)[None, :]
    gt = (r > b1(c)).astype(np.int64) + (r > b2(c)).astype(np.int64)
    nr = ((np.arange(N) + 0.5) * rows / N - 0.5)[None, :]
    nc = ((np.arange(T) + 0.5) * cols / T - 0.5)[:, None]
    sig = lambda x: 1 / (1 + np.exp(-x))
    s1, s2 = (sig((nr - b(nc)) / (temp * rows / N)) for b in (b1, b2))
    L = np.stack([1 - s1, s1 * (1 - s2), s1 * s2], -1)  # [T, N, 3]
    L = L / L.sum(-1, keepdims=True)
    return gt, torch.tensor(L.reshape(T * N, 3).astype(np.float32))


QUALITY = [(12, 10, 83, 84, 0.5), (24, 48, 410, 768, 0.5), (8, 6, 50, 64, 1.0)]


@pytest.mark.parametrize("case", QUALITY, ids=str)
def test_dense_map_halves_the_wrong_pixels_of_the_nearest_map(case):
    import crw_hip
    T, N, rows, cols, temp = case
    gt, L = boundary_case(*case)
    node = L.view(T, N, 3).argmax(-1).t()  # [N, T]
    nearest = TF.interpolate(node[None, None].float(), size=(rows, cols), mode="nearest")[0, 0].numpy()
    dense, _ = crw_hip.labelmap_dense(L, T, N, 3, rows, cols)
    wrong_nearest, wrong_dense = int((nearest != gt).sum()), int((dense.numpy() != gt).sum())
    print(f"{case}: wrong pixels nearest {wrong_nearest}, bilinear {wrong_dense}, of {gt.size}")
    assert 2 * wrong_dense <= wrong_nearest


# ---- 6. host surface --------------------------------------------------------------------------------------------------------------
def test_windows_strides_and_argument_errors_on_the_cpu():
    import crw_hip
    shape = (5, 7, 3, 37, 29)
    T, N, M, rows, cols = shape
    L, _ = dr.reference(shape)
    lab, conf = crw_hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin")
    wide, widec = torch.full((rows, cols + 7), -7.0), torch.full((rows, cols + 7), -7.0)
    out, outc = crw_hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin", out=wide[:, 3:3 + cols], out_conf=widec[:, 3:3 + cols])
    assert out.data_ptr() == wide[:, 3:].data_ptr() and torch.equal(wide[:, 3:3 + cols], lab) and torch.equal(widec[:, 3:3 + cols], conf)
    assert (wide[:, :3] == -7).all() and (wide[:, 3 + cols:] == -7).all() and (widec[:, :3] == -7).all() and (widec[:, 3 + cols:] == -7).all()
    flipped, _ = crw_hip.labelmap_dense(L, T, N, M, rows, cols, flip=True)
    assert torch.equal(flipped, torch.flip(lab, (1,)))
    with pytest.raises(ValueError, match="contiguous along its columns"):
        crw_hip.labelmap_dense(L, T, N, M, rows, cols, out=torch.zeros(rows, 2 * cols)[:, ::2])  # strided
    with pytest.raises(ValueError):
        crw_hip.labelmap_dense(L, T, N, M, rows, cols, out=torch.zeros(cols, rows).t())  # transposed
    with pytest.raises(ValueError, match="one pitch"):
        crw_hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin", out=wide[:, :cols], out_conf=torch.zeros(rows, cols))
    for bad in (dict(rows=0), dict(cols=0), dict(rows=(1 << 22) + 1), dict(T=0), dict(M=1), dict(M=17)):
        a = dict(T=T, N=N, M=M, rows=rows, cols=cols)
        a.update(bad)
        with pytest.raises(ValueError):
            crw_hip.labelmap_dense(L, **a)
    with pytest.raises(ValueError):
        crw_hip.labelmap_dense(L, T, N, M, rows, cols, confidence="softmax")
    with pytest.raises(ValueError):
        crw_hip.labelmap_dense(L, T, N, M, rows, cols, dtype=torch.int32)
    with pytest.raises(ValueError):
        crw_hip.labelmap_dense(L, T, N, M, rows, cols, out_conf=torch.zeros(rows, cols))  # no kind
    with pytest.raises(ValueError):
        crw_hip.labelmap_dense(L.double(), T, N, M, rows, cols)


def test_header_and_binding_declare_the_dense_entry_point_at_abi_8():
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^int\s+crw_labelmap_dense\(const float \*L, int T, int N, int M, int rows, int cols, int flip, int conf_kind, "
                     r"void \*labels,\s+int label_dtype, float \*conf, size_t ld, crw_stream_t stream\);", header, re.M)
    assert int(re.search(r"^#define\s+CRW_ABI_VERSION\s+(\d+)", header, re.M).group(1)) == crw_hip.ABI_VERSION == 8
    assert crw_hip.DENSE_ENTRY_POINTS == ("crw_labelmap_dense",) and len(crw_hip.SIGNATURES["crw_labelmap_dense"][1]) == 13
    assert "crw_labelmap_dense (crw_hip.has_dense())" in header and "imported/crw.py:124-127" in header
    lib = crw_hip.lib()
    assert lib.crw_abi_version() == 8 and crw_hip.has_dense()
    # argument errors are refused before anything is launched (no device needed); 16 is a pointer that is never followed
    ok = dict(L=16, T=4, N=4, M=4, rows=8, cols=8, flip=0, kind=-1, labels=16, dt=0, conf=None, ld=8)
    for bad in (dict(L=None), dict(labels=None), dict(T=0), dict(N=0), dict(M=1), dict(M=17), dict(rows=0), dict(cols=0),
                dict(rows=(1 << 22) + 1), dict(cols=(1 << 22) + 1), dict(kind=3), dict(kind=-2), dict(kind=0), dict(conf=16),
                dict(dt=2), dict(ld=7), dict(labels=18)):
        a = dict(ok, **bad)
        assert lib.crw_labelmap_dense(a["L"], a["T"], a["N"], a["M"], a["rows"], a["cols"], a["flip"], a["kind"], a["labels"], a["dt"],
                                      a["conf"], a["ld"], None) == crw_hip.CRW_EINVAL, bad


def test_a_library_without_the_dense_entry_point_is_named_stale(monkeypatch):
    import crw_hip
    crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "dense", False)
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*crw_labelmap_dense.*rebuild"):
        crw_hip._dense_lib()


def test_propagate_soft_on_the_branches_the_cpu_reaches(monkeypatch):
    import utils as crw_utils
    sig = inspect.signature(crw_utils.propagate)
    assert sig.parameters["soft"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["soft"].default is False
    N, M = 6, 4
    seed = torch.tensor([0., 0., 1., 3., 3., 2.])
    monkeypatch.setattr(crw_utils, "_features_and_seed", lambda seq, *a: (torch.zeros(seq.shape[0], N, 8), seed))
    seq = torch.zeros(1, N, 4, 4)  # a one-frame item: nothing is propagated
    assert len(crw_utils.propagate(seq, None, None, None, M, False, False)) == 3
    *_, L = out = crw_utils.propagate(seq, None, None, None, M, False, False, soft=True)
    assert len(out) == 4 and L.shape == (N, M) and L.dtype == torch.float32
    assert torch.equal(L, torch.nn.functional.one_hot(seed.long(), M).float())
    out = crw_utils.propagate(seq, None, None, None, M, False, False, confidence="margin", soft=True)
    assert len(out) == 5 and out[3].shape == (N, 1) and torch.equal(out[4], L)


def oracle_propagate_soft(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, confidence=None, soft=False):
    """`utils.propagate`'s contract on the CPU with the fp32 oracle standing in for the kernels, soft labels included."""
    import crw_hip
    T, N = seq.shape[:2]
    emb = model(seq.reshape(T * N, 1, *seq.shape[2:])).reshape(T, N, -1).numpy()
    if use_last:
        emb = emb[::-1].copy()
    L = torch.tensor(oracle_soft_labels(emb, orc.seed_labels(seg_ref.numpy(), N), ncls, lp))
    out = (L.view(T, N, ncls).argmax(-1).t().float(), torch.tensor(orc.xent_metric(emb)) if T > 1 else torch.zeros(N, 0), None)
    if confidence is not None:
        out += (crw_hip.labelprop_confidence(L, T, N, ncls, confidence),)
    return out + (L,) if soft else out


@pytest.mark.parametrize("merge", ["rule", "confidence"])
def test_segment_bilinear_on_the_oracle(monkeypatch, merge):
    """`segment(upsample='bilinear')` on the CPU: every pass's window is `labelmap_dense` of that pass's soft labels -- the
    correction's tail spliced, the reverse pass mirrored --, and 'nearest' is the call without the argument."""
    import crw_hip
    import inference as crw_inference
    M, T = 5, 8
    rg_len = T * 8
    forced = [5, None]

    def segment(**kw):
        ds, seg, lp, _, _ = synthetic_case(n_rg=2)
        it = iter(forced)

        def propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, **k):
            out = oracle_propagate_soft(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, **k)
            return out[:2] + ((next(it, None) if (seq.shape[0] == T and not use_last) else None),) + out[3:]

        monkeypatch.setattr(crw_inference, "propagate", propagate)
        return crw_inference.segment(ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0), correction=True, use_last=True, dataset_id=3,
                                     device="cpu", confidence="maxprob", merge=merge, **kw)

    plain, near, out = segment(), segment(upsample="nearest"), segment(upsample="bilinear")
    for k in ("pred", "forward", "conf", "forward_conf"):
        assert torch.equal(plain[k], near[k])
    assert out["change_idx"] == plain["change_idx"] == forced and set(out) == set(plain)
    # by hand
    ds, seg, lp, _, _ = synthetic_case(n_rg=2)
    rows, N = seg.shape[0], ds[0].shape[1]
    dense = lambda L, frames, cols: crw_hip.labelmap_dense(L, frames, N, M, rows, cols, confidence="maxprob")
    run = lambda seq, ref, last: oracle_propagate_soft(seq, ref, Flatten(), lp, M, False, last, soft=True)[-1]
    fl, fc = zip(*[dense(run(ds[t * T], seg[:N * 4 + 4, rg_len * t:rg_len * t + 8], False), T, rg_len) for t in range(2)])
    fl, fc = [m.clone() for m in fl], [m.clone() for m in fc]
    px = (T - 5) * 8
    tail = dense(run(ds.get_smaller_item(0, T - 5), seg[:, rg_len - px:rg_len - px + 8], False), T - 5, px)
    fl[0][:, rg_len - px:], fc[0][:, rg_len - px:] = tail
    fwd, fconf = torch.cat(fl, 1), torch.cat(fc, 1)
    assert torch.equal(out["forward"], fwd) and torch.equal(out["forward_conf"], fconf)
    assert not torch.equal(out["forward"], plain["forward"])  # the boundaries left the node grid
    rl, rc = [], []
    for t in range(2):  # the reverse pass runs on the items the correction shortened
        seq = ds[t * T]
        lab, conf = dense(run(seq, torch.flip(seg[:, rg_len * t:rg_len * (t + 1)], (-1,))[:, :8], True), seq.shape[0], rg_len)
        rl.append(torch.flip(lab, (-1,)))
        rc.append(torch.flip(conf, (-1,)))
    rev, rconf = torch.cat(rl, 1), torch.cat(rc, 1)
    take = rconf > fconf if merge == "confidence" else crw_inference._reverse_rule_mask(fwd, rev, 3).view_as(fwd)
    assert torch.equal(out["pred"], torch.where(take, rev, fwd)) and torch.equal(out["conf"], torch.where(take, rconf, fconf))


def test_segment_refuses_an_unknown_upsample():
    import inference as crw_inference
    ds, seg, lp, M, T = synthetic_case(n_rg=1)
    with pytest.raises(ValueError, match="upsample must be 'nearest' or 'bilinear'"):
        crw_inference.segment(ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0), device="cpu", upsample="bogus")
    assert inspect.signature(crw_inference.segment).parameters["upsample"].default == "nearest"


def test_cli_upsample_flag():
    spec = importlib.util.spec_from_file_location("segment_all", os.path.join(PKG, "scripts", "segment_all.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    p = cli.get_args_parser()
    base = ["--synthetic", "40", "192"]
    assert p.parse_args(base).upsample == "nearest"
    assert p.parse_args(base + ["--upsample", "bilinear"]).upsample == "bilinear"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--upsample", "bicubic"])
    with pytest.raises(SystemExit, match="--single"):
        cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + ["--single", "--upsample", "bilinear"])))
