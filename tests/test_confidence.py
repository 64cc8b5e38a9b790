"""Confidence maps, the confidence-ruled merge and the calibration report on the host: the CPU routes of `crw_hip.labelprop_confidence`
/ `merge_confidence` / `calibration` against plain torch formulas, `metrics.Calibration`'s arithmetic on hand-made counts, bin
edges, agreement of the dropped pixels with `crw_hip.confusion` under the three dataset rules, `utils.propagate` / `inference.segment`
with the fp32 oracle standing in for the kernels, the ABI tables and the command line.  The kernels' twins are in
test_confidence_gpu.py."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT, load_golden
from oracle import crw_oracle as orc

KINDS = ("maxprob", "margin", "entropy")


def random_rows(rows, M, gen, one_hot_every=7):
    """Probability rows [rows, M] with exact zeros and one-hot rows mixed in."""
    p = torch.rand(rows, M, generator=gen) ** 3
    p[torch.rand(rows, M, generator=gen) < 0.2] = 0
    p[:, 0] += 1e-3
    p = p / p.sum(-1, keepdim=True)
    hot = torch.arange(0, rows, one_hot_every)
    p[hot] = torch.nn.functional.one_hot(hot % M, M).float()
    return p.float()


def formula(p, kind, dtype=torch.float32):
    """The three confidences of probability rows [..., M], written out."""
    p = p.to(dtype)
    if kind == "maxprob":
        return p.max(-1).values
    if kind == "margin":
        top = torch.topk(p, 2, dim=-1).values
        return top[..., 0] - top[..., 1]
    plogp = torch.where(p > 0, p * torch.log(p), torch.zeros_like(p))
    return (1 + plogp.sum(-1) / np.log(p.shape[-1])).clamp(0, 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [2, 3, 5, 16])
def test_cpu_confidence_is_the_formula(kind, M):
    import crw_hip
    T, N = 6, 9
    L = random_rows(T * N, M, torch.Generator().manual_seed(M))
    conf = crw_hip.labelprop_confidence(L, T, N, M, kind)
    assert conf.shape == (N, T) and conf.dtype == torch.float32
    want = formula(L.view(T, N, M), kind, torch.float64).t()
    torch.testing.assert_close(conf.double(), want, rtol=0, atol=2e-6)
    assert conf.min() >= 0 and conf.max() <= 1
    if kind == "maxprob":
        assert torch.equal(conf, L.view(T, N, M).max(-1).values.t()) and conf.min() >= 1 / M - 1e-6
    hot = ((L == 1).any(-1) & ((L == 0).sum(-1) == M - 1)).view(T, N).t()  # one-hot rows
    assert hot.any() and (conf[hot] == 1).all()  # a one-hot row: 1 for every kind
    over = L.clone()
    over[0] = 0
    over[0, 1] = 1 + 2 ** -23  # a propagated row can sum to an ulp more than 1: the confidence reads 1
    assert crw_hip.labelprop_confidence(over, T, N, M, kind)[0, 0] == 1
    part = crw_hip.labelprop_confidence(L, T, N, M, kind, first_frame=3)
    assert torch.equal(part[:, 3:], conf[:, 3:]) and not part[:, :3].any()


def test_confidence_argument_errors():
    import crw_hip
    L = torch.full((12, 3), 1 / 3)
    for bad in (dict(kind="softmax"), dict(first_frame=0), dict(first_frame=5)):
        with pytest.raises(ValueError):
            crw_hip.labelprop_confidence(L, 4, 3, 3, **bad)
    with pytest.raises(ValueError):
        crw_hip.labelprop_confidence(L, 4, 3, 4)  # shape
    with pytest.raises(ValueError):
        crw_hip.labelprop_confidence(torch.zeros(4, 1), 2, 2, 1)
    with pytest.raises(ValueError):
        crw_hip.labelprop_confidence(torch.zeros(4, 17), 2, 2, 17)
    with pytest.raises(ValueError):
        crw_hip.labelprop_confidence(L.double(), 4, 3, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int8])
def test_cpu_merge_is_torch_where(dtype):
    import crw_hip
    gen = torch.Generator().manual_seed(3)
    P = 1000
    fl, rl = torch.randint(0, 5, (P,), generator=gen).to(dtype), torch.randint(0, 5, (P,), generator=gen).to(dtype)
    fc, rc = torch.rand(P, generator=gen), torch.rand(P, generator=gen)
    rc[::5] = fc[::5]               # ties keep the forward label
    fc[1::11] = float("nan")        # so does a NaN on either side
    rc[2::13] = float("nan")
    take = rc > fc
    lab, conf, took = crw_hip.merge_confidence(fl.view(10, 100), fc.view(10, 100), rl.view(10, 100), rc.view(10, 100), want_took=True)
    assert lab.shape == (10, 100) and lab.dtype == dtype and took.dtype == torch.uint8
    assert torch.equal(lab.view(-1), torch.where(take, rl, fl)) and torch.equal(took.view(-1).bool(), take)
    assert torch.equal(conf.view(-1).view(torch.int32), torch.where(take, rc, fc).view(torch.int32))  # bitwise, NaNs included
    assert not take[::5].any() and not take[1::11].any() and not take[2::13].any() and take.any()
    f2, c2 = fl.clone(), fc.clone()  # in place
    out = crw_hip.merge_confidence(f2, c2, rl, rc, out_lab=f2, out_conf=c2)
    assert out[0] is f2 and out[2] is None and torch.equal(f2, lab.view(-1)) and torch.equal(c2.view(torch.int32), conf.view(-1).view(torch.int32))
    with pytest.raises(ValueError):
        crw_hip.merge_confidence(fl, fc, rl[:-1], rc[:-1])
    with pytest.raises(ValueError):
        crw_hip.merge_confidence(fl, fc, rl.to(torch.int64), rc)
    with pytest.raises(ValueError):
        crw_hip.merge_confidence(fl, fc.double(), rl, rc)


def plain_calibration(gt, pred, conf, K, bins, keep):
    """Pixel by pixel in Python: (counts, conf_sum, invalid-label count, invalid-confidence count) over the pixels `keep` marks."""
    counts, sums, bad_lab, bad_conf = np.zeros((bins, 2), np.int64), np.zeros(bins), 0, 0
    for g, p, c, k in zip(gt.flatten().tolist(), pred.flatten().tolist(), conf.flatten().float().tolist(), keep.flatten().tolist()):
        if not k:
            continue
        if not (g in range(K) and p in range(K)):  # an integer in [0, K); NaN and 2.5 are in no range
            bad_lab += 1
        elif not 0 <= c <= 1:
            bad_conf += 1
        else:
            b = min(bins - 1, int(np.floor(np.float32(c) * np.float32(bins))))
            counts[b] += (1, g == p)
            sums[b] += c
    return counts, sums, bad_lab, bad_conf


def test_cpu_calibration_counts_and_masks():
    import crw_hip
    gen = torch.Generator().manual_seed(5)
    P, K, bins = 4000, 5, 10
    gt = torch.randint(0, K, (P,), generator=gen).float()
    pred = torch.where(torch.rand(P, generator=gen) < 0.7, gt, torch.randint(0, K, (P,), generator=gen).float())
    conf = torch.rand(P, generator=gen)
    aux = torch.randint(0, 5, (P,), generator=gen).float()
    gt[5::97], pred[7::89] = 2.5, float("nan")                  # invalid labels
    conf[3::101], conf[4::103], conf[9::107] = float("nan"), -0.1, 1.5  # invalid confidences
    for kw, keep in ((dict(), torch.ones(P, dtype=torch.bool)), (dict(ignore_gt=1, ignore_pred=3), (gt != 1) & (pred != 3)),
                     (dict(aux=aux, ignore_aux=4), aux != 4)):
        counts, sums, dropped = crw_hip.calibration(gt, pred, conf, K, bins=bins, **kw)
        assert counts.dtype == torch.int64 and counts.shape == (bins, 2) and sums.dtype == torch.float64 and dropped.shape == (3,)
        wc, ws, bad_lab, bad_conf = plain_calibration(gt, pred, conf, K, bins, keep)
        assert np.array_equal(counts.numpy(), wc) and dropped.tolist() == [P - int(keep.sum()), bad_lab, bad_conf]
        np.testing.assert_allclose(sums.numpy(), ws, rtol=1e-12)
        assert bad_lab > 0 and bad_conf > 0 and int(counts[:, 0].sum()) + sum(dropped.tolist()) == P
        _, d2 = crw_hip.confusion(gt, pred, K, **kw)
        assert dropped[:2].tolist() == d2.tolist()
    # int8 labels and a float64 confidence map are taken as well
    c8, s8, d8 = crw_hip.calibration(gt.nan_to_num(0).floor().to(torch.int8), pred.nan_to_num(0).to(torch.int8), conf.double(), K)
    assert int(c8[:, 0].sum()) + int(d8.sum()) == P
    for bad in (dict(K=1), dict(K=17), dict(bins=0), dict(bins=65), dict(ignore_gt=-2), dict(ignore_aux=2)):
        with pytest.raises(ValueError):
            crw_hip.calibration(gt, pred, conf, **dict(dict(K=K), **bad))
    with pytest.raises(ValueError):
        crw_hip.calibration(gt, pred, conf[:-1], K)
    with pytest.raises(ValueError):
        crw_hip.calibration(gt, pred, conf.long(), K)
    c0, s0, d0 = crw_hip.calibration(torch.zeros(0), torch.zeros(0), torch.zeros(0), K, bins=4)
    assert c0.shape == (4, 2) and not c0.any() and not s0.any() and d0.tolist() == [0, 0, 0]


@pytest.mark.parametrize("bins", [1, 4, 10, 64])
def test_bin_edges(bins):
    """conf = 0, k / bins, 1, just below 1, and the three invalid values: bin = min(bins - 1, floor(fl32(conf * bins)))."""
    import crw_hip
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    edges = [k / bins for k in range(bins + 1)]
    vals = [0.0, 1.0, below_one, float("nan"), -0.1, 1.5, -0.0] + edges
    conf = torch.tensor(vals, dtype=torch.float32)
    z = torch.zeros(len(vals))
    counts, sums, dropped = crw_hip.calibration(z, z, conf, 2, bins=bins)
    want = np.zeros(bins, np.int64)
    for v in conf[[0, 1, 2, 6] + list(range(7, len(vals)))].tolist():
        want[min(bins - 1, int(np.floor(np.float32(v) * np.float32(bins))))] += 1
    assert counts[:, 0].tolist() == want.tolist() == counts[:, 1].tolist() and dropped.tolist() == [0, 0, 3]
    assert want[-1] >= 3 and (bins == 1 or want[0] >= 3)  # 1, just below 1 and the last edge; 0, -0 and the first edge
    for k in range(bins):  # an edge belongs to the bin it opens (the fp32 product decides, as in the kernel)
        c, _, _ = crw_hip.calibration(z[:1], z[:1], torch.tensor([edges[k]], dtype=torch.float32), 2, bins=bins)
        assert c[min(bins - 1, int(np.floor(np.float32(edges[k]) * np.float32(bins)))), 0] == 1


def test_calibration_arithmetic_on_hand_made_counts():
    import metrics as crw_metrics
    #                 bin:   0        1         2        3 (empty)   4
    counts = np.array([[10, 2], [20, 10], [30, 24], [0, 0], [40, 38]])
    sums = np.array([1.0, 6.0, 15.0, 0.0, 36.0])
    cal = crw_metrics.Calibration(counts, sums, dropped=(3, 0, 1))
    assert cal.bins == 5 and cal.total == 100 and cal.dropped == (3, 0, 1)
    np.testing.assert_allclose(cal.accuracy[[0, 1, 2, 4]], [0.2, 0.5, 0.8, 0.95])
    np.testing.assert_allclose(cal.mean_confidence[[0, 1, 2, 4]], [0.1, 0.3, 0.5, 0.9])
    assert np.isnan(cal.accuracy[3]) and np.isnan(cal.mean_confidence[3])
    np.testing.assert_allclose(cal.ece, (10 * 0.1 + 20 * 0.2 + 30 * 0.3 + 40 * 0.05) / 100)
    np.testing.assert_allclose(cal.mce, 0.3)
    np.testing.assert_allclose(cal.overall_accuracy, 0.74)
    rc = cal.risk_coverage()
    np.testing.assert_allclose(rc["threshold"], [0, 0.2, 0.4, 0.6, 0.8])
    np.testing.assert_allclose(rc["coverage"], [1.0, 0.9, 0.7, 0.4, 0.4])
    np.testing.assert_allclose(rc["accuracy"], [0.74, 72 / 90, 62 / 70, 0.95, 0.95])
    assert (np.diff(rc["coverage"]) <= 0).all()
    # trapezoid over coverage 0.4 -> 0.7 -> 0.9 -> 1.0 (the doubled 0.4 adds nothing), continued to 0 at the first risk
    risk = 1 - np.array([0.95, 62 / 70, 72 / 90, 0.74])
    want = 0.4 * risk[0] + 0.3 * (risk[0] + risk[1]) / 2 + 0.2 * (risk[1] + risk[2]) / 2 + 0.1 * (risk[2] + risk[3]) / 2
    np.testing.assert_allclose(cal.aurc, want)
    assert cal.coverage_at(0.9) == 0.4 and cal.coverage_at(0.85) == 0.7 and cal.coverage_at(0.5) == 1.0 and cal.coverage_at(0.99) == 0.0
    d = cal.to_dict()
    assert d["count"] == [10, 20, 30, 0, 40] and d["dropped"] == dict(masked=3, invalid=0, invalid_confidence=1)
    assert d["ece"] == cal.ece and d["risk_coverage"]["coverage"] == list(rc["coverage"]) and np.isnan(d["accuracy"][3])
    json.dumps(d)
    text = str(cal)
    lines = text.split("\n")
    assert lines[0].split() == ["confidence", "pixels", "accuracy", "mean", "conf", "coverage", "kept", "acc"]
    assert lines[2] == "[0.000,0.200)           10     0.2000     0.1000     1.0000     0.7400"
    assert lines[5] == "[0.600,0.800)            0          -          -     0.4000     0.9500"
    assert lines[6].startswith("[0.800,1.000]") and "ECE" in lines[8] and lines[8].endswith("0.1600")
    assert text == str(crw_metrics.Calibration(torch.tensor(counts), torch.tensor(sums), (3, 0, 1)))  # fixed format, tensors too
    # degenerate inputs
    empty = crw_metrics.Calibration(np.zeros((3, 2), np.int64), np.zeros(3))
    assert empty.total == 0 and np.isnan(empty.ece) and np.isnan(empty.mce) and np.isnan(empty.aurc) and empty.coverage_at(0.5) == 0.0
    assert empty.dropped is None and "dropped" not in empty.to_dict() and "-" in str(empty)
    one = crw_metrics.Calibration([[0, 0], [8, 6]], [0.0, 7.0])
    np.testing.assert_allclose([one.ece, one.mce, one.aurc], [0.125, 0.125, 0.25])
    for bad in (np.zeros((3, 3)), np.zeros((0, 2)), [[1, 2]]):
        with pytest.raises(ValueError):
            crw_metrics.Calibration(bad, np.zeros(len(bad)))
    with pytest.raises(ValueError):
        crw_metrics.Calibration(np.zeros((3, 2)), np.zeros(2))


GT = torch.tensor([[0., 0., 1., 1.], [2., 2., 3., 3.], [0., 1., 2., 3.]])
PR = torch.tensor([[0., 1., 1., 1.], [2., 3., 3., 0.], [0., 1., 2., 2.]])
CF = torch.tensor([[.95, .15, .85, .75], [.65, .25, .55, .35], [1., 0., .45, float("nan")]])


def test_inference_calibration_follows_evaluates_rules():
    """dropped[0:2] of `calibration` = `confusion`'s on the same masked inputs, for the three dataset rules; the binned pixels are
    `evaluate`'s total, the correct ones its trace."""
    import crw_hip
    import inference as crw_inference
    aux = torch.tensor([[4., 0., 0., 0.], [0., 4., 4., 0.], [1., 2., 3., 0.]])
    gt5, pr5 = GT.clone(), PR.clone()
    gt5[0, 0], pr5[2, 2], pr5[0, 1] = 5, 5, 4
    cases = ((0, PR, GT, dict(unc_seg=aux), dict(aux=aux, ignore_aux=4)), (1, pr5, gt5, {}, dict(ignore_gt=5, ignore_pred=5)),
             (3, PR, GT, {}, {}), (0, PR, GT, dict(remove_unc=False), {}))
    for ds, pr, gt, kw, mask in cases:
        cal = crw_inference.calibration(pr, CF, gt, ds, bins=10, **kw)
        rep = crw_inference.evaluate(pr, gt, ds, **kw)
        _, d = crw_hip.confusion(gt, pr, crw_inference.NCLASSES[ds], **mask)
        assert list(cal.dropped[:2]) == d.tolist() == list(rep.dropped) and cal.dropped[2] == 1  # the NaN at [2, 3]
        assert cal.total + 1 == rep.total and int(cal.correct.sum()) == int(np.trace(rep.counts))  # that pixel is a wrong one
    cal = crw_inference.calibration(PR, CF, GT, 3, bins=10)
    assert cal.count.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2] and cal.correct.tolist() == [1, 0, 0, 0, 1, 1, 1, 1, 1, 2]
    np.testing.assert_allclose(cal.mean_confidence, [0, .15, .25, .35, .45, .55, .65, .75, .85, .975], atol=1e-7)
    assert crw_inference.calibration(PR, CF, GT, 3, bins=4).bins == 4
    with pytest.raises(ValueError):
        crw_inference.calibration(PR, CF, GT, 0)  # remove_unc on dataset 0 needs the uncertain map
    with pytest.raises(ValueError):
        crw_inference.calibration(PR, CF, GT, 2, remove_unc=False)
    with pytest.raises(ValueError):
        crw_inference.calibration(PR, CF[:, :3], GT, 3)
    bad = GT.clone()
    bad[1, 1] = 2.5
    with pytest.raises(crw_hip.LabelError):
        crw_inference.calibration(PR, CF, bad, 3)


def test_header_and_binding_declare_the_confidence_entry_points():
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^int\s+crw_labelprop_confidence\(const float \*L, int T, int N, int M, int kind, int first_frame, float \*conf,",
                     header, re.M)
    assert re.search(r"^int\s+crw_merge_confidence\(const void \*fwd_lab, const float \*fwd_conf, const void \*rev_lab, "
                     r"const float \*rev_conf, int lab_dtype,", header, re.M)
    assert re.search(r"^size_t\s+crw_calibration_ws_bytes\(size_t P, int K, int bins\);", header, re.M)
    assert re.search(r"^int\s+crw_calibration\(const void \*gt, int gt_dtype, const void \*pred, int pred_dtype, const float \*conf,",
                     header, re.M)
    assert int(re.search(r"^#define\s+CRW_ABI_VERSION\s+(\d+)", header, re.M).group(1)) == crw_hip.ABI_VERSION == 8
    for name, n in (("crw_labelprop_confidence", 8), ("crw_merge_confidence", 10), ("crw_calibration_ws_bytes", 3), ("crw_calibration", 19)):
        assert len(crw_hip.SIGNATURES[name][1]) == n and name in crw_hip.CONFIDENCE_ENTRY_POINTS
    assert crw_hip.CONF_KINDS == {k: int(re.search(rf"^#define\s+CRW_CONF_{k.upper()}\s+(\d+)", header, re.M).group(1)) for k in KINDS}
    lib = crw_hip.lib()
    assert lib.crw_abi_version() == 8 and crw_hip.has_confidence()
    # host-side query: the grid of crw_confusion, 2 * bins + 3 32-bit rows (16-byte padded) and `bins` 64-bit rows of partials
    assert lib.crw_calibration_ws_bytes(1, 5, 10) == 96 + 80 == lib.crw_calibration_ws_bytes(0, 5, 10)
    assert lib.crw_calibration_ws_bytes(410 * 8192 * 3, 5, 10) == 2048 * (23 * 4 + 10 * 8)
    assert lib.crw_calibration_ws_bytes(1 << 44, 16, 64) == (1 << 13) * (131 * 4 + 64 * 8)
    for K, bins in ((1, 10), (17, 10), (5, 0), (5, 65)):
        assert lib.crw_calibration_ws_bytes(100, K, bins) == 0
    # argument errors are refused before anything is launched (no device needed)
    assert lib.crw_labelprop_confidence(None, 4, 4, 4, 0, 1, None, None) == crw_hip.CRW_EINVAL
    assert lib.crw_merge_confidence(None, None, None, None, 0, 10, None, None, None, None) == crw_hip.CRW_EINVAL
    assert lib.crw_merge_confidence(None, None, None, None, 7, 0, None, None, None, None) == crw_hip.CRW_EINVAL
    assert lib.crw_calibration(None, 0, None, 0, None, None, 0, 10, 5, 10, -1, -1, -1, None, None, None, None, 0, None) == crw_hip.CRW_EINVAL


def test_a_library_without_the_confidence_entry_points_is_named_stale(monkeypatch):
    import crw_hip
    crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "confidence", False)
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*crw_labelprop_confidence.*rebuild"):
        crw_hip._confidence_lib()


# ---- propagate / segment on the CPU: the fp32 oracle stands in for the kernels ---------------------------------------------------
class Flatten(torch.nn.Module):
    def forward(self, x):
        return x.flatten(1)


def oracle_soft_labels(emb, seed, M, lp):
    T, N, C = emb.shape
    ehat = orc.l2_normalize(emb, np.float32).astype(np.float32)
    L = np.zeros((T * N, M), np.float32)
    L[:N] = seed[:, None] == np.arange(M)[None, :]
    for n in range(1, T):
        W, I = orc.labelprop_weights(ehat, n, lp.cxt_size, lp.radius, lp.temperature, lp.topk)
        L[n * N:(n + 1) * N] = (L[I] * W[..., None]).sum(0)
    return L


def oracle_propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, confidence=None):
    """`utils.propagate`'s contract on the CPU, confidence included (through the binding's CPU route)."""
    import crw_hip
    T, N = seq.shape[:2]
    emb = model(seq.reshape(T * N, 1, *seq.shape[2:])).reshape(T, N, -1).numpy()
    if use_last:
        emb = emb[::-1].copy()
    L = torch.tensor(oracle_soft_labels(emb, orc.seed_labels(seg_ref.numpy(), N), ncls, lp))
    out = (L.view(T, N, ncls).argmax(-1).t().float(), torch.tensor(orc.xent_metric(emb)) if T > 1 else torch.zeros(N, 0), None)
    return out if confidence is None else out + (crw_hip.labelprop_confidence(L, T, N, ncls, confidence),)


def synthetic_case(n_rg=3, T=8, H_rg=40, M=5):
    import dataset as crw_dataset
    from imported.labelprop import LabelPropVOS_CRW
    rg = crw_dataset.synthetic_radargram(H_rg, n_rg * T * 8)
    ds = crw_dataset.RGDataset.from_tensor(rg, T, (8, 8), (4, 0))
    N = ds[0].shape[1]
    r = torch.arange(N * 8).float()[:, None]
    c = torch.arange(rg.shape[1]).float()[None, :]
    seg = torch.clamp(torch.floor((r + 3 * torch.sin(c / 23.0)) * M / (N * 8)), 0, M - 1)
    return ds, seg, LabelPropVOS_CRW(dict(CXT_SIZE=4, RADIUS=4, TEMP=0.1, KNN=5)), M, T


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("use_last", [False, True])
def test_segment_with_confidence_on_the_oracle(monkeypatch, kind, use_last):
    import inference as crw_inference
    monkeypatch.setattr(crw_inference, "propagate", oracle_propagate)
    ds, seg, lp, M, T = synthetic_case()
    args = (seg, Flatten(), lp, M, T, (8, 8), (4, 0))
    kw = dict(use_last=use_last, dataset_id=3, device="cpu")
    plain = crw_inference.segment(ds, *args, **kw)
    out = crw_inference.segment(ds, *args, confidence=kind, **kw)
    assert set(plain) == {"pred", "forward", "xent", "change_idx"} and set(out) == set(plain) | {"conf", "forward_conf"}
    assert torch.equal(out["pred"], plain["pred"]) and torch.equal(out["forward"], plain["forward"])
    conf, fconf = out["conf"], out["forward_conf"]
    assert conf.shape == out["pred"].shape == fconf.shape and conf.dtype == torch.float32
    assert conf.min() >= 0 and conf.max() <= 1 and (kind != "maxprob" or conf.min() >= 1 / M - 1e-6)
    rg_len = T * 8
    for t in range(3):
        assert (fconf[:, t * rg_len:t * rg_len + 8] == 1).all()  # the forward pass's seed column
    assert use_last or (torch.equal(conf, fconf) and torch.equal(out["pred"], out["forward"]))
    # merge='confidence': any dataset id, the torch.where composition of the two passes
    with pytest.raises(ValueError):
        crw_inference.segment(ds, *args, use_last=True, dataset_id=7, device="cpu", confidence=kind)  # the class rule has no rule
    mc = crw_inference.segment(ds, *args, use_last=use_last, dataset_id=7, device="cpu", confidence=kind, merge="confidence")
    assert torch.equal(mc["forward"], plain["forward"]) and torch.equal(mc["forward_conf"], fconf)
    if not use_last:
        assert torch.equal(mc["pred"], mc["forward"]) and torch.equal(mc["conf"], fconf)
    else:
        rev, rconf = reverse_pass(ds, seg, lp, M, T, kind)
        take = rconf > fconf
        assert take.any() and not take.all()
        assert torch.equal(mc["pred"], torch.where(take, rev, plain["forward"])) and torch.equal(mc["conf"], torch.where(take, rconf, fconf))
        assert (mc["conf"][:, rg_len - 8:rg_len] == 1).all()  # the reverse pass's seed column wins its ties with nothing: it is 1
        # merge='rule': conf is the reverse pass's exactly where the rule wrote the reverse label
        wrote = crw_inference._reverse_rule_mask(plain["forward"], rev, 3).view_as(rev)
        assert torch.equal(conf, torch.where(wrote, rconf, fconf)) and torch.equal(out["pred"], torch.where(wrote, rev, plain["forward"]))


def reverse_pass(ds, seg, lp, M, T, kind, propagate=oracle_propagate, model=None, rows=None):
    """The reverse maps (labels, confidence) composed by hand: propagate from the last column, upsample, flip back."""
    import inference as crw_inference
    rg_len, rows = T * 8, seg.shape[0] if rows is None else rows
    labs, confs = [], []
    for t in range(seg.shape[1] // rg_len):
        seq = ds[t * T].to(seg.device)
        seg_ref = torch.flip(seg[:, t * rg_len:(t + 1) * rg_len], (-1,))[:, :8]
        pred, _, _, conf = propagate(seq, seg_ref, model or Flatten(), lp, M, False, True, confidence=kind)
        labs.append(torch.flip(crw_inference._upsample(pred, rows, rg_len), (-1,)))
        confs.append(torch.flip(crw_inference._upsample(conf, rows, rg_len), (-1,)))
    return torch.cat(labs, 1), torch.cat(confs, 1)


def test_segment_argument_errors_and_defaults(monkeypatch):
    import inference as crw_inference
    monkeypatch.setattr(crw_inference, "propagate", oracle_propagate)
    ds, seg, lp, M, T = synthetic_case(n_rg=1)
    args = (ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0))
    with pytest.raises(ValueError, match="needs a confidence kind"):
        crw_inference.segment(*args, device="cpu", merge="confidence")
    with pytest.raises(ValueError):
        crw_inference.segment(*args, device="cpu", merge="vote")
    with pytest.raises(ValueError):
        crw_inference.segment(*args, device="cpu", confidence="softmax")


def test_correction_splices_the_confidence_with_the_labels(monkeypatch):
    """The correction window: spliced where the labels are, left alone where the correction is skipped on a data error."""
    import inference as crw_inference
    ds, seg, lp, M, T = synthetic_case(n_rg=2)
    forced = iter([5, 6])  # change points of the two forward passes; the correction's own calls report none

    def propagate(seq, *a, **k):
        out = oracle_propagate(seq, *a, **k)
        return out[:2] + ((next(forced) if seq.shape[0] == T else None),) + out[3:]

    monkeypatch.setattr(crw_inference, "propagate", propagate)
    args = (seg, Flatten(), lp, M, T, (8, 8), (4, 0))
    out = crw_inference.segment(ds, *args, correction=True, dataset_id=3, device="cpu", confidence="maxprob")
    assert out["change_idx"] == [5, 6]
    rg_len = T * 8
    for t, px in ((0, 24), (1, 16)):
        start = t * rg_len + rg_len - px
        assert (out["conf"][:, start:start + 8] == 1).all()        # re-seeded there: the shortened item's seed column
        assert (out["conf"][:, start - 8:start] < 1).any()         # the forward pass's confidence before it
    # a correction that fails on its data is skipped for both maps
    ds2, _, _, _, _ = synthetic_case(n_rg=2)
    forced = iter([5, 6])
    monkeypatch.setattr(ds2, "get_smaller_item", lambda *a: (_ for _ in ()).throw(IndexError("no such item")), raising=False)
    skipped = crw_inference.segment(ds2, *args, correction=True, dataset_id=3, device="cpu", confidence="maxprob")
    ds3, _, _, _, _ = synthetic_case(n_rg=2)
    monkeypatch.setattr(crw_inference, "propagate", oracle_propagate)
    uncorrected = crw_inference.segment(ds3, *args, dataset_id=3, device="cpu", confidence="maxprob")
    assert torch.equal(skipped["conf"], uncorrected["conf"]) and torch.equal(skipped["pred"], uncorrected["pred"])
    assert not torch.equal(out["conf"], uncorrected["conf"])


def test_propagate_keeps_its_three_outputs_without_a_kind():
    import inspect
    import utils as crw_utils
    sig = inspect.signature(crw_utils.propagate)
    assert sig.parameters["confidence"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["confidence"].default is None
    assert list(sig.parameters)[:7] == ["seq", "seg_ref", "model", "lp", "nclasses", "do_pos_embed", "use_last"]
    with pytest.raises(ValueError):
        crw_utils.propagate(torch.zeros(2, 2, 4, 4), torch.zeros(8, 4), Flatten(), None, 3, False, False, confidence="softmax")


# ---- command line ---------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("segment_all", os.path.join(PKG, "scripts", "segment_all.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_accepts_the_confidence_flags():
    cli = _cli()
    p = cli.get_args_parser()
    a = cli.check_confidence_flags(cli.with_defaults(p.parse_args(["--model_path", "x.pt"])))
    assert (a.confidence, a.merge, a.bins, a.save_conf) == (None, "rule", 10, False)
    a = cli.check_confidence_flags(cli.with_defaults(p.parse_args(["--model_path", "x.pt", "--confidence", "margin", "--merge", "confidence",
                                                                  "--bins", "20", "--save_conf"])))
    assert (a.confidence, a.merge, a.bins, a.save_conf) == ("margin", "confidence", 20, True)
    for bad in (["--merge", "confidence"], ["--save_conf"], ["--confidence", "entropy", "--bins", "0"],
                ["--confidence", "entropy", "--bins", "65"], ["--confidence", "maxprob", "--single"]):
        with pytest.raises(SystemExit):
            cli.check_confidence_flags(cli.with_defaults(p.parse_args(["--model_path", "x.pt"] + bad)))
    for bad in (["--confidence", "softmax"], ["--merge", "vote"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--model_path", "x.pt"] + bad)


CLI_ARGS = ["--synthetic", "40", "384", "--dataset", "1", "--patch_size", "8", "8", "--overlap", "4", "0", "--seq_length", "8", "-c", "4",
            "-r", "4", "-k", "5", "--use_last", "true", "--model", "0", "--iou"]


def stub_propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last, confidence=None):
    """`propagate`'s contract in index arithmetic alone -- labels that drift down the column of seed labels, a confidence that is a
    fixed pattern of tenths: the same bits on every machine, which a recorded stdout needs (the oracle's sums are not that)."""
    T, N = seq.shape[:2]
    seed = torch.tensor(orc.seed_labels(seg_ref.numpy(), N))
    n, t = torch.arange(N)[:, None], torch.arange(T)[None, :]
    pred = seed[(n + (t + 1) // 3 * (2 if use_last else 1)) % N].float()
    out = (pred, torch.zeros(N, max(T - 1, 0)), None)
    if confidence is None:
        return out
    conf = ((n * 7 + t * 3 + (5 if use_last else 0)) % 10).float() / 10 + 0.05
    conf[:, 0] = 1
    return out + (conf,)


def run_cli(monkeypatch, capsys, tmp_path, extra):
    """`segment_all.main` on a synthetic radargram with `stub_propagate` for `propagate` -> (stdout without the two elapsed times
    and with the output folder's name blanked, files written, report json)."""
    import inference as crw_inference
    cli = _cli()
    monkeypatch.setattr(crw_inference, "propagate", stub_propagate)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    out_dir, js = tmp_path / "out", tmp_path / "r.json"
    torch.manual_seed(11)
    cli.main(cli.get_args_parser().parse_args(CLI_ARGS + ["--output_folder", str(out_dir), "--report_json", str(js)] + extra))
    text = capsys.readouterr().out.replace(str(tmp_path), "TMP")
    text = re.sub(r"(Time elapsed \([a-z +]+\):) [0-9.e-]+", r"\1 *", text)
    return text, sorted(os.listdir(out_dir)), json.load(open(js))


def test_cli_without_the_flags_prints_what_it_printed(monkeypatch, capsys, tmp_path):
    """tests/golden/segment_all_stdout.txt is this run's stdout as the commit BEFORE the confidence flags printed it (recorded by
    running `run_cli` of this file, with `stub_propagate`, against that commit's package; elapsed times and the temporary folder blanked): same bytes
    now, the same files, the same json keys."""
    text, files, d = run_cli(monkeypatch, capsys, tmp_path, [])
    assert text == open(os.path.join(GOLDEN, "segment_all_stdout.txt")).read()
    assert files == ["predicted_map.pt"] and "calibration" not in d and "Calibration" not in text
    assert sorted(d) == sorted(["0.0", "1.0", "2.0", "3.0", "4.0", "accuracy", "macro avg", "weighted avg", "mean_iou", "labels", "matrix",
                                "dropped", "pixels", "map_shape", "elapsed_inference_s", "elapsed_total_s", "dataset", "remove_unc",
                                "single"])


@pytest.mark.parametrize("merge", ["rule", "confidence"])
def test_cli_with_the_flags(monkeypatch, capsys, tmp_path, merge):
    plain, _, d0 = run_cli(monkeypatch, capsys, tmp_path / "a", [])
    text, files, d = run_cli(monkeypatch, capsys, tmp_path / "b", ["--confidence", "entropy", "--merge", merge, "--bins", "5", "--save_conf"])
    assert files == ["confidence_map.pt", "predicted_map.pt"]
    conf = torch.load(tmp_path / "b" / "out" / "confidence_map.pt")
    assert conf.dtype == torch.float32 and tuple(conf.shape) == (40, 384) == tuple(d["map_shape"]) and 0 <= conf.min() and conf.max() <= 1
    cal = d["calibration"]
    assert cal["kind"] == "entropy" and cal["merge"] == merge and cal["bins"] == 5 and len(cal["count"]) == 5
    assert cal["total"] == int(np.sum(d["matrix"])) and sum(cal["correct"]) == int(np.trace(np.array(d["matrix"])))
    assert cal["dropped"] == dict(masked=d["dropped"]["masked"], invalid=0, invalid_confidence=0)
    # the table comes after the confusion matrix and before the IoU table; the rest of the text is the plain run's
    i_mat, i_cal, i_iou = text.index("]]\n"), text.index(f"Calibration (entropy, merge: {merge}):"), text.index("iou\n")
    assert i_mat < i_cal < i_iou and "ECE" in text and "[0.800,1.000]" in text
    if merge == "rule":  # nothing else changes: without the calibration block the text is the plain run's, but for the line of arguments
        end = text.index("\n", text.index("accuracy", text.index("AURC"))) + 2
        rest = lambda s: s[s.index("\n"):]
        assert d["matrix"] == d0["matrix"] and rest(text[:i_cal - 1] + text[end:]) == rest(plain)
