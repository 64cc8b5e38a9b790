"""GPU side of the confidence maps: the kernels of csrc/confidence.hip -- `crw_labelprop_confidence` against torch formulas and,
through `LabelPropVOS_CRW.propagate_all`, against the soft labels the reference's own `predict` returned (fixtures
confidence_*.npz, tests/golden/make_golden_confidence.py); `crw_merge_confidence` bitwise against torch.where; `crw_calibration`
against the binding's CPU route over sizes, dtypes, alignments and masks; `segment(..., confidence=...)` end to end on random-init
encoders.  Invalid labels and confidences are data the kernels count -- nothing here provokes a fault."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, load_golden
from oracle import crw_oracle as orc
from test_confidence import KINDS, formula, random_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_confidence()
    return crw_hip


# ---- crw_labelprop_confidence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", list(range(2, 17)))
def test_confidence_kernel_against_torch(hip, M):
    """maxprob and margin bitwise; entropy against the formula in fp64 within 4 x what the same formula in fp32 torch misses it by
    on the same rows (the kernel differs from that in logf and in summation order only)."""
    T, N = 37, 53
    gen = torch.Generator().manual_seed(100 + M)
    rows = random_rows(T * N, M, gen)
    assert rows.max() <= 1 and ((rows == 0).sum(-1) == M - 1).any()  # probability rows, one-hot rows among them
    L = rows.cuda()
    p = rows.view(T, N, M)
    bar = 4 * float((formula(p, "entropy", torch.float32).double() - formula(p, "entropy", torch.float64)).abs().max())
    for first_frame in (1, 5):
        cols = slice(0 if first_frame == 1 else first_frame, T)
        conf = {k: hip.labelprop_confidence(L, T, N, M, k, first_frame=first_frame).cpu() for k in KINDS}
        assert all(c.shape == (N, T) and c.dtype == torch.float32 for c in conf.values())
        assert torch.equal(conf["maxprob"][:, cols], p.max(-1).values.t()[:, cols])
        top = torch.topk(p, 2, dim=-1).values
        assert torch.equal(conf["margin"][:, cols], (top[..., 0] - top[..., 1]).t()[:, cols])
        err = float((conf["entropy"].double() - formula(p, "entropy", torch.float64).t())[:, cols].abs().max())
        print(f"M={M} first_frame={first_frame}: entropy misses fp64 by {err:.3e}, fp32 torch bar (4x) {bar:.3e}")
        assert err <= bar
        hot = ((p == 1).any(-1) & ((p == 0).sum(-1) == M - 1)).t()  # one-hot rows
        for c in conf.values():
            assert (c[:, cols][hot[:, cols]] == 1).all() and c.min() >= 0 and c.max() <= 1
            assert first_frame == 1 or not c[:, :first_frame].any()  # not written: the binding hands out zeros there
    # rows that do not start on a 16-byte boundary (a view one float into a buffer) take the scalar loads
    buf = torch.zeros(T * N * M + 1, device="cuda")
    buf[1:] = L.view(-1)
    for k in KINDS:
        assert torch.equal(hip.labelprop_confidence(buf[1:].view(T * N, M), T, N, M, k).cpu(), conf_of(hip, L, T, N, M, k))
    # a duplicated maximum: margin 0; a row an ulp above 1: 1
    dup = torch.zeros(2 * N, M, device="cuda")
    dup[:, 0] = dup[:, M - 1] = 0.5
    dup[0] = 0
    dup[0, M - 1] = 1 + 2 ** -23
    m = hip.labelprop_confidence(dup, 2, N, M, "margin").cpu()
    assert m[0, 0] == 1 and not m[1:, 0].any() and not m[:, 1].any()
    assert hip.labelprop_confidence(dup, 2, N, M, "maxprob").cpu()[0, 0] == 1


def conf_of(hip, L, T, N, M, kind):
    return hip.labelprop_confidence(L, T, N, M, kind).cpu()


def test_confidence_kernel_argument_errors(hip):
    L = torch.full((12, 3), 1 / 3, device="cuda")
    for bad in (dict(kind="softmax"), dict(first_frame=0), dict(first_frame=5)):
        with pytest.raises(ValueError):
            hip.labelprop_confidence(L, 4, 3, 3, **bad)
    lib = hip.lib()
    out = torch.zeros(3, 4, device="cuda")
    for M, kind, ff in ((1, 0, 1), (17, 0, 1), (3, 3, 1), (3, -1, 1), (3, 0, 0), (3, 0, 5)):
        assert lib.crw_labelprop_confidence(L.data_ptr(), 4, 3, M, kind, ff, out.data_ptr(), None) == hip.CRW_EINVAL
    assert not out.any()


# ---- pinned to the reference -----------------------------------------------------------------------------------------------------
LP_CASES = ["trunc_T14N10", "full_T40N48", "last_T20N24", "mc1_T100N12"]


def soft_labels_fp64(emb, seed, M, cxt_size, radius, temp, knn):
    """The propagation restated in float64: the chain of oracle.labelprop_weights, lists of the truncated keys on the untruncated
    labels (as oracle.labelprop) -> L [T*N, M]."""
    T, N, C = emb.shape
    ehat = orc.l2_normalize(emb.astype(np.float64), np.float64)
    L = np.zeros((T * N, M), np.float64)
    L[:N] = seed[:, None] == np.arange(M)[None, :]
    for n in range(1, T):
        W, I = orc.labelprop_weights(ehat, n, cxt_size, radius, temp, knn, dtype=np.float64)
        L[n * N:(n + 1) * N] = (L[I] * W[..., None]).sum(0)
    return L


@pytest.mark.parametrize("name", LP_CASES)
def test_soft_labels_and_confidences_against_the_reference(hip, name):
    """`propagate_all` on the inputs of labelprop_<name>.npz: pred exact; the device's L and the three confidences of EVERY node of
    every frame against the fp64 restatement, within 8 x the largest deviation of the reference's own recorded fp32 masks
    (confidence_<name>.npz) from that restatement -- the device sums the same k terms in another order after a differently ordered
    score product: the reference's kind of rounding."""
    from imported.labelprop import LabelPropVOS_CRW
    g, ref = load_golden("labelprop_" + name), load_golden("confidence_" + name)["L"]
    emb = g["emb"][::-1].copy() if bool(g["use_last"]) else g["emb"]
    T, N, C = emb.shape
    M = int(g["nclasses"])
    cfg = dict(CXT_SIZE=int(g["cxt_size"]), RADIUS=int(g["radius"]), TEMP=float(g["temp"]), KNN=int(g["knn"]))
    seed = orc.seed_labels(g["seg_ref"], N)
    L64 = soft_labels_fp64(emb, seed, M, cfg["CXT_SIZE"], cfg["RADIUS"], cfg["TEMP"], cfg["KNN"])
    assert ref.shape == (T, N, M) and np.array_equal(ref.argmax(-1).T, g["pred"]) and np.array_equal(L64.reshape(T, N, M).argmax(-1).T, g["pred"])
    ref_dev = float(np.abs(ref.reshape(T * N, M) - L64).max())
    tol = 8 * ref_dev
    feats = hip.normalize(torch.tensor(emb).cuda())
    pred, L = LabelPropVOS_CRW(cfg).propagate_all(feats, torch.tensor(seed).cuda(), M)
    assert np.array_equal(pred.cpu().numpy(), g["pred"]), f"{(pred.cpu().numpy() != g['pred']).sum()} labels differ"
    dev = float(np.abs(L.cpu().numpy().astype(np.float64) - L64).max())
    print(f"{name}: reference's masks deviate from fp64 by {ref_dev:.3e} (tolerance {tol:.3e}); device L by {dev:.3e}")
    assert L.shape == (T * N, M) and dev <= tol
    p64 = torch.tensor(L64).view(T, N, M)
    for kind in KINDS:
        conf = hip.labelprop_confidence(L, T, N, M, kind).cpu()
        want = formula(p64, kind, torch.float64).t()
        err = float((conf.double() - want).abs().max())
        print(f"{name}: {kind} deviates from fp64 by {err:.3e}")
        assert conf.shape == (N, T) and err <= tol and (conf[:, 0] == 1).all()


# ---- crw_merge_confidence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.int8], ids=["fp32", "int8"])
@pytest.mark.parametrize("P,offset", [(1, 0), (15, 0), (16, 0), (4099, 0), (410 * 640, 0), (100003, 1), (100003, 5), (100003, 16)])
def test_merge_kernel_is_torch_where(hip, dtype, P, offset):
    """Bitwise the torch.where statement of the rule -- ties and NaNs keep the forward pass -- on whole tensors and on views that
    start `offset` elements into a wider buffer (no 16-byte boundary in common between the label and the confidence maps when
    the labels are int8), with and without `took`, out of place and in place."""
    gen = torch.Generator().manual_seed(P + offset)
    wide = lambda t: torch.cat([t.new_zeros(offset), t, t.new_zeros(3)]).cuda()[offset:offset + P]
    fl = wide(torch.randint(0, 6, (P,), generator=gen).to(dtype))
    rl = wide(torch.randint(0, 6, (P,), generator=gen).to(dtype))
    fc, rc = torch.rand(P, generator=gen), torch.rand(P, generator=gen)
    rc[::5] = fc[::5]
    fc[1::11] = float("nan")
    rc[2::13] = float("nan")
    if dtype == torch.float32:
        fl[3::17] = float("nan")  # labels are copied, never decoded
    fc, rc = wide(fc), wide(rc)
    take = rc > fc
    want_lab, want_conf = torch.where(take, rl, fl), torch.where(take, rc, fc)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    lab, conf, took = hip.merge_confidence(fl, fc, rl, rc, want_took=True)
    assert torch.equal(bits(lab), bits(want_lab)) and torch.equal(bits(conf), bits(want_conf)) and torch.equal(took.bool(), take)
    lab2, conf2, none = hip.merge_confidence(fl, fc, rl, rc)
    assert none is None and torch.equal(bits(lab2), bits(want_lab)) and torch.equal(bits(conf2), bits(want_conf))
    f2, c2 = fl.clone(), fc.clone()
    hip.merge_confidence(f2, c2, rl, rc, out_lab=f2, out_conf=c2)  # in place
    assert torch.equal(bits(f2), bits(want_lab)) and torch.equal(bits(c2), bits(want_conf))
    if P > 20:
        assert take.any() and not take[::5].any() and not take[1::11].any() and not take[2::13].any()
    # output views into a wider buffer: nothing outside them is written
    ob, oc = torch.full((P + 9,), 7, dtype=dtype, device="cuda"), torch.full((P + 9,), 7.0, device="cuda")
    hip.merge_confidence(fl, fc, rl, rc, out_lab=ob[5:5 + P], out_conf=oc[5:5 + P])
    assert torch.equal(bits(ob[5:5 + P]), bits(want_lab)) and (ob[:5] == 7).all() and (ob[5 + P:] == 7).all()
    assert torch.equal(bits(oc[5:5 + P]), bits(want_conf)) and (oc[:5] == 7).all() and (oc[5 + P:] == 7).all()


# ---- crw_calibration -------------------------------------------------------------------------------------------------------------
def calibration_inputs(P, K, seed, label_dtype, aux_dtype):
    """Layered maps (runs, as label maps have) with noise; masked, invalid-label and invalid-confidence pixels mixed in."""
    gen = torch.Generator().manual_seed(seed)
    cols = 1024
    r = torch.arange((P + cols - 1) // cols).float()[:, None]
    c = torch.arange(cols).float()[None, :]
    band = lambda shift: torch.clamp(torch.floor((r + shift + 6 * torch.sin(c / 97.0)) * K / max(len(r), 1)), 0, K - 1).flatten()[:P]
    gt, pred = band(0.0), band(2.0)
    noisy = torch.rand(P, generator=gen) < 0.05
    pred = torch.where(noisy, torch.randint(0, K, (P,), generator=gen).float(), pred)
    conf = torch.where(noisy, torch.rand(P, generator=gen), 0.5 + 0.5 * torch.rand(P, generator=gen) ** 0.3)
    conf[::997], conf[1::1499], conf[2::1999], conf[3::2503] = float("nan"), -0.1, 1.5, 1.0
    aux = torch.where(torch.rand(P, generator=gen) < 0.03, 4.0, gt)
    if label_dtype == torch.float32:
        gt[5::1009], pred[7::2003] = 2.5, float("nan")
    else:
        gt[5::1009], pred[7::2003] = K, -3  # integers outside [0, K)
    return gt.to(label_dtype), pred.to(label_dtype), conf, aux.to(aux_dtype)


def check_calibration(hip, gt, pred, conf, K, bins, **kw):
    """Device against the binding's CPU route: integers exact; conf_sum per bin within P * 2^-53 relative of a float64 torch sum
    (the worst case of a double accumulation of P fp32 values); a second run bit-identical."""
    P = gt.numel()
    cpu = lambda t: None if t is None else t.cpu()
    wc, ws, wd = hip.calibration(cpu(gt), cpu(pred), cpu(conf), K, bins=bins, **{k: cpu(v) if torch.is_tensor(v) else v for k, v in kw.items()})
    counts, sums, dropped = hip.calibration(gt, pred, conf, K, bins=bins, **kw)
    assert counts.is_cuda and counts.dtype == torch.int64 and sums.dtype == torch.float64 and dropped.shape == (3,)
    assert torch.equal(counts.cpu(), wc) and torch.equal(dropped.cpu(), wd)
    assert int(counts[:, 0].sum()) + int(dropped.sum()) == P
    c32 = conf.reshape(-1).float().cpu()
    ok = (c32 >= 0) & (c32 <= 1)
    b = torch.clamp(torch.floor(torch.where(ok, c32, torch.zeros(())) * bins), max=bins - 1).long()
    binned = torch.zeros(P, dtype=torch.bool)
    # which pixels were binned: the CPU route's masks restated through its counts is circular -- recompute from the rules
    g, p = cpu(gt).reshape(-1).double(), cpu(pred).reshape(-1).double()
    masked = torch.zeros(P, dtype=torch.bool)
    if kw.get("ignore_gt", -1) >= 0:
        masked |= g == kw["ignore_gt"]
    if kw.get("ignore_pred", -1) >= 0:
        masked |= p == kw["ignore_pred"]
    if kw.get("ignore_aux", -1) >= 0:
        masked |= cpu(kw["aux"]).reshape(-1).double() == kw["ignore_aux"]
    valid = (g == g.floor()) & (g >= 0) & (g < K) & (p == p.floor()) & (p >= 0) & (p < K)
    binned = ~masked & valid & ok
    for k in range(bins):
        want = float(c32[binned & (b == k)].double().sum())
        assert abs(float(sums[k]) - want) <= P * 2.0 ** -53 * abs(want), (k, float(sums[k]), want)
        assert int(counts[k, 0]) == int((binned & (b == k)).sum())
    _, d2 = hip.confusion(gt, pred, K, **kw)
    assert torch.equal(dropped[:2], d2)
    again = hip.calibration(gt, pred, conf, K, bins=bins, **kw)
    assert torch.equal(again[0], counts) and torch.equal(again[1].view(torch.int64), sums.view(torch.int64)) and torch.equal(again[2], dropped)
    return counts, sums, dropped


@pytest.mark.parametrize("label_dtype,aux_dtype", [(torch.float32, torch.float32), (torch.int8, torch.int8), (torch.float32, torch.int8),
                                                   (torch.int8, torch.float32)], ids=["fp32", "int8", "fp32+aux8", "int8+aux32"])
@pytest.mark.parametrize("bins", [1, 10, 64])
def test_calibration_kernel_against_the_cpu_route(hip, label_dtype, aux_dtype, bins):
    P, K = 1000 * 1024 + 77, 5
    gt, pred, conf, aux = (t.cuda() for t in calibration_inputs(P, K, bins, label_dtype, aux_dtype))
    c, s, d = check_calibration(hip, gt, pred, conf, K, bins)
    assert d[0] == 0 and d[1] > 0 and d[2] > 0 and c[-1, 0] > 0
    check_calibration(hip, gt, pred, conf, K, bins, ignore_gt=1, ignore_pred=3)
    c, s, d = check_calibration(hip, gt, pred, conf, K, bins, aux=aux, ignore_aux=4)
    assert d[0] > 0
    check_calibration(hip, gt, pred, conf, K, bins, aux=aux, ignore_aux=4, ignore_gt=0)


@pytest.mark.parametrize("offsets", [(0, 0, 0, 0), (1, 1, 1, 1), (3, 3, 3, 3), (1, 2, 3, 5), (0, 0, 7, 0), (16, 16, 16, 16)])
def test_calibration_on_views_at_odd_offsets(hip, offsets):
    """Maps that start inside a wider one: a scalar head up to the first pixel where every operand is 16-byte aligned, or -- offsets
    that share no such pixel -- the scalar route throughout.  Mixed dtypes, so that one element offset is 1 byte here, 4 there."""
    P, K = 300 * 1024 + 5, 4
    gt, pred, conf, aux = calibration_inputs(P, K, 7, torch.int8, torch.float32)
    wide = lambda t, o: torch.cat([t.new_zeros(o), t, t.new_zeros(5)]).cuda()[o:o + P]
    og, op, oc, oa = offsets
    check_calibration(hip, wide(gt, og), wide(pred.float(), op), wide(conf, oc), K, 10, aux=wide(aux, oa), ignore_aux=4)
    check_calibration(hip, wide(gt, og), wide(pred, op), wide(conf, oc), K, 10)


@pytest.mark.parametrize("P", [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4097])
def test_calibration_small_and_empty_maps(hip, P):
    gt, pred, conf, aux = (t.cuda() for t in calibration_inputs(max(P, 1), 3, P, torch.float32, torch.float32))
    gt, pred, conf, aux = gt[:P], pred[:P], conf[:P], aux[:P]
    c, s, d = check_calibration(hip, gt, pred, conf, 3, 10, aux=aux, ignore_aux=4)
    if P == 0:
        assert not c.any() and not s.any() and d.tolist() == [0, 0, 0]


def test_calibration_random_bins_and_argument_errors(hip):
    """No runs at all (every lane of a wave in another bin), every bin of 64 filled; refused arguments."""
    gen = torch.Generator().manual_seed(1)
    P = 500 * 1024
    gt = torch.randint(0, 16, (P,), generator=gen).to(torch.int8).cuda()
    pred = torch.randint(0, 16, (P,), generator=gen).to(torch.int8).cuda()
    conf = torch.rand(P, generator=gen).cuda()
    c, s, d = check_calibration(hip, gt, pred, conf, 16, 64)
    assert (c[:, 0] > 0).all() and d.tolist() == [0, 0, 0]
    for bad in (dict(K=1), dict(K=17), dict(bins=0), dict(bins=65), dict(ignore_aux=1)):
        with pytest.raises(ValueError):
            hip.calibration(gt, pred, conf, **dict(dict(K=16), **bad))
    with pytest.raises(ValueError):
        hip.calibration(gt, pred, conf.cpu(), 16)
    lib = hip.lib()
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    ws = torch.zeros(16, dtype=torch.uint8, device="cuda")
    o = out.data_ptr()
    assert lib.crw_calibration(gt.data_ptr(), 1, pred.data_ptr(), 1, conf.data_ptr(), None, 1, P, 16, 10, -1, -1, -1, o, o + 160, o + 240,
                               ws.data_ptr(), 16, None) == hip.CRW_EWORKSPACE
    assert not out.any()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
T_E2E, PATCH, OVERLAP, M_E2E = 10, (16, 16), (8, 0), 5


def e2e_case(model_id, n_rg=3, H=200):
    import dataset as crw_dataset
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    torch.manual_seed(17 + model_id)
    enc = crw_utils.create_model(model_id, False).cuda()
    rg = crw_dataset.synthetic_radargram(H, n_rg * T_E2E * 16)
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T_E2E, PATCH, OVERLAP)  # `get_smaller_item` shortens a dataset for good
    N = fresh()[0].shape[1]
    rows = N * 8 + 8
    r = torch.arange(rows).float()[:, None]
    c = torch.arange(rg.shape[1]).float()[None, :]
    seg = torch.clamp(torch.floor((r + 5 * torch.sin(c / 41.0)) * M_E2E / rows), 0, M_E2E - 1)
    return enc, fresh, seg, LabelPropVOS_CRW(dict(CXT_SIZE=6, RADIUS=6, TEMP=0.1, KNN=8)), N


def forced_propagate(forced):
    """`utils.propagate` with the change points of the whole-length items forced (PELT finds none on this synthetic medium)."""
    import utils as crw_utils
    it = iter(forced)

    def propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, **kw):
        out = crw_utils.propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, **kw)
        change = next(it, None) if (seq.shape[0] == T_E2E and not use_last) else None
        return out[:2] + (change,) + out[3:]
    return propagate


def compose(ds, seg, enc, lp, N, kind, forced, correction, use_last):
    """`segment`'s confidence maps composed by hand from `propagate(..., confidence=kind)`: upsample, splice the correction
    window, flip the reverse pass back -> (forward labels, forward conf, reverse labels | None, reverse conf | None)."""
    import inference as crw_inference
    import utils as crw_utils
    T, W = T_E2E, PATCH[1]
    rg_len, rows, rg_h = T * W, seg.shape[0], N * 8 + 8
    seg = seg.cuda()
    up = crw_inference._upsample
    run = lambda seq, ref, last: crw_utils.propagate(seq.cuda(), ref, enc, lp, M_E2E, False, last, confidence=kind)
    n_rg = seg.shape[1] // rg_len
    labs, confs = [], []
    for t in range(n_rg):
        pred, _, _, conf = run(ds[t * T], seg[:rg_h, rg_len * t:rg_len * t + W], False)
        assert pred.shape == conf.shape == (N, T)
        labs.append(up(pred, rows, rg_len))
        confs.append(up(conf, rows, rg_len))
    if correction:
        for t, change in enumerate(forced):
            if change is None:
                continue
            small = T - change
            px = small * W
            pred, _, _, conf = run(ds.get_smaller_item(t * T, small), seg[:, rg_len * t + rg_len - px:rg_len * t + rg_len - px + W], False)
            labs[t][:, rg_len - px:] = up(pred, rows, px)
            confs[t][:, rg_len - px:] = up(conf, rows, px)
    fwd, fconf = torch.cat(labs, 1), torch.cat(confs, 1)
    if not use_last:
        return fwd, fconf, None, None
    rl, rc = [], []
    for t in range(n_rg):
        ref = torch.flip(seg[:, rg_len * t:rg_len * (t + 1)], (-1,))[:, :W]
        pred, _, _, conf = run(ds[t * T], ref, True)  # after a correction: the shortened items, stretched to rg_len
        rl.append(torch.flip(up(pred, rows, rg_len), (-1,)))
        rc.append(torch.flip(up(conf, rows, rg_len), (-1,)))
    return fwd, fconf, torch.cat(rl, 1), torch.cat(rc, 1)


@pytest.mark.parametrize("use_last", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("correction", [False, True], ids=["plain", "correction"])
@pytest.mark.parametrize("model_id", [0, 1], ids=["CNN", "Resnet"])
def test_segment_with_confidence_end_to_end(hip, monkeypatch, model_id, correction, use_last):
    import inference as crw_inference
    enc, fresh, seg, lp, N = e2e_case(model_id)
    forced = [6, None, 3]
    kind = KINDS[(model_id + 2 * correction + use_last) % 3]
    args = (seg, enc, lp, M_E2E, T_E2E, PATCH, OVERLAP)
    kw = dict(correction=correction, use_last=use_last, dataset_id=3)

    def segment(**more):
        monkeypatch.setattr(crw_inference, "propagate", forced_propagate(forced))
        return crw_inference.segment(fresh(), *args, **kw, **more)

    plain = segment()
    out = segment(confidence=kind)
    assert set(plain) == {"pred", "forward", "xent", "change_idx"} and set(out) == set(plain) | {"conf", "forward_conf"}
    assert torch.equal(out["pred"], plain["pred"]) and torch.equal(out["forward"], plain["forward"])  # the labels do not move
    assert out["change_idx"] == plain["change_idx"] == forced
    conf, fconf = out["conf"], out["forward_conf"]
    assert conf.is_cuda and conf.dtype == torch.float32 and conf.shape == out["pred"].shape == fconf.shape
    lo = 1 / M_E2E - 1e-6 if kind == "maxprob" else 0.0
    for c in (conf, fconf):
        assert float(c.min()) >= lo and float(c.max()) <= 1
    rg_len = T_E2E * 16
    for t in range(3):
        assert (fconf[:, t * rg_len:t * rg_len + 16] == 1).all()  # the forward pass's seed column
    fwd, hand_fconf, rev, rconf = compose(fresh(), seg, enc, lp, N, kind, forced, correction, use_last)
    assert torch.equal(fwd, out["forward"]) and torch.equal(hand_fconf, fconf)
    if correction:
        for t, change in enumerate(forced):
            if change is not None:
                start = t * rg_len + change * 16
                assert (fconf[:, start:start + 16] == 1).all()  # re-seeded there
    if not use_last:
        assert torch.equal(conf, fconf)
    else:
        wrote = crw_inference._reverse_rule_mask(fwd, rev, 3).view_as(fwd)
        assert torch.equal(conf, torch.where(wrote, rconf, fconf)) and torch.equal(out["pred"], torch.where(wrote, rev, fwd))
        assert (rconf[:, rg_len - 16:rg_len] == 1).all()  # the reverse pass's seed column
    # merge='confidence' on a dataset id the class rule refuses
    if use_last:
        with pytest.raises(ValueError):
            crw_inference.segment(fresh(), *args, correction=False, use_last=True, dataset_id=7, confidence=kind)
    kw["dataset_id"] = 7
    mc = segment(confidence=kind, merge="confidence")
    assert torch.equal(mc["forward"], fwd) and torch.equal(mc["forward_conf"], fconf)
    if use_last:
        take = rconf > fconf
        assert take.any() and not take.all()
        assert torch.equal(mc["pred"], torch.where(take, rev, fwd)) and torch.equal(mc["conf"], torch.where(take, rconf, fconf))
    else:
        assert torch.equal(mc["pred"], fwd) and torch.equal(mc["conf"], fconf)
    # the calibration of that map bins the pixels `evaluate` counts
    cal = crw_inference.calibration(mc["pred"], mc["conf"], seg, 3, bins=10)
    rep = crw_inference.evaluate(mc["pred"], seg, 3)
    assert cal.total == rep.total == seg.numel() and int(cal.correct.sum()) == int(np.trace(rep.counts)) and cal.dropped == (0, 0, 0)
    assert 0 <= cal.ece <= 1 and 0 <= cal.aurc <= 1 and (np.diff(cal.risk_coverage()["coverage"]) <= 0).all()
    with pytest.raises(ValueError, match="needs a confidence kind"):
        crw_inference.segment(fresh(), *args, merge="confidence")


def test_propagate_confidence_one_frame_and_foreign_lp(hip):
    """A one-frame item gives ones; an `lp` that only offers the reference's `predict` gets its confidence from the masks `predict`
    returns -- the same numbers as `propagate_all`'s, since both run the same kernels on the same lists."""
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    from test_hip_parity import _Flatten
    g = load_golden("labelprop_trunc_T14N10")
    T, N, C = g["emb"].shape
    M = int(g["nclasses"])
    cfg = dict(CXT_SIZE=int(g["cxt_size"]), RADIUS=int(g["radius"]), TEMP=float(g["temp"]), KNN=int(g["knn"]))
    seq, seg_ref = torch.tensor(g["emb"]).cuda().reshape(T, N, C // 4, 4), torch.tensor(g["seg_ref"]).cuda()

    class PredictOnly:
        def __init__(self, inner):
            self.inner = inner

        def predict(self, feats, masks, curr_feat):
            return self.inner.predict(feats, masks, curr_feat)

    for kind in KINDS:
        three = crw_utils.propagate(seq, seg_ref, _Flatten(), LabelPropVOS_CRW(cfg), M, False, False)
        four = crw_utils.propagate(seq, seg_ref, _Flatten(), LabelPropVOS_CRW(cfg), M, False, False, confidence=kind)
        assert len(three) == 3 and len(four) == 4 and torch.equal(three[0], four[0]) and four[3].shape == (N, T) and four[3].is_cuda
        foreign = crw_utils.propagate(seq, seg_ref, _Flatten(), PredictOnly(LabelPropVOS_CRW(cfg)), M, False, False, confidence=kind)
        assert torch.equal(foreign[0], four[0]) and torch.equal(foreign[3], four[3])
        one = crw_utils.propagate(seq[:1], seg_ref, _Flatten(), LabelPropVOS_CRW(cfg), M, False, False, confidence=kind)
        assert len(one) == 4 and one[3].shape == (N, 1) and (one[3] == 1).all() and one[3].is_cuda


def test_cli_with_confidence_in_a_child_process(hip, tmp_path):
    H, W, T = 200, 3 * 16 * 20, 20
    js = tmp_path / "report.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_all.py"), "--synthetic", str(H), str(W), "--dataset", "0",
                        "--model", "0", "--seq_length", str(T), "-c", "10", "--use_last", "true", "--output_folder",
                        str(tmp_path / "out") + "/", "--report_json", str(js), "--confidence", "maxprob", "--merge", "confidence",
                        "--bins", "8", "--save_conf"], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(js.read_text())
    conf = torch.load(tmp_path / "out" / "confidence_map.pt", map_location="cpu")
    assert conf.dtype == torch.float32 and list(conf.shape) == d["map_shape"] and 0.25 - 1e-6 <= float(conf.min()) and float(conf.max()) <= 1
    cal = d["calibration"]
    assert cal["bins"] == 8 and cal["kind"] == "maxprob" and cal["merge"] == "confidence"
    assert cal["total"] == sum(sum(row) for row in d["matrix"]) and cal["dropped"]["masked"] == d["dropped"]["masked"] > 0
    assert "Calibration (maxprob, merge: confidence):" in r.stdout and "ECE" in r.stdout
