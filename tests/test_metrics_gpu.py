"""GPU side of the segmentation reports: the HIP kernel `crw_confusion` (csrc/metrics.hip) against the reference's recorded
reports (fixtures report_*.npz) and against torch.bincount on the device over sizes, alignments, class counts, masks and label
statistics; stream independence; `segment` -> `evaluate` end to end; the command line.  Invalid labels are data the kernel
counts -- nothing here provokes a fault."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, load_golden
from test_metrics import REPORT_CASES, check_report, expected_counts, fixture_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    return crw_hip


@pytest.mark.parametrize("dtype", [torch.float32, torch.int8], ids=["fp32", "int8"])
@pytest.mark.parametrize("case", REPORT_CASES)
def test_fixtures_through_the_kernel(hip, case, dtype):
    """`counts` and `dropped` exact, and the whole report (numbers to 1e-12, both texts) as the reference printed it."""
    import inference as crw_inference
    g = load_golden(case)
    pred, seg, kw = fixture_maps(g, "cuda", dtype)
    rep = crw_inference.evaluate(pred, seg, **kw)
    assert np.array_equal(rep.counts, expected_counts(g, int(g["nclasses"])))
    check_report(rep, g)


def bincount_reference(gt, pred, K, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1):
    """The same counts from PyTorch ops on the device (valid labels only): boolean-index masking, then bincount."""
    keep = torch.ones(gt.shape, dtype=torch.bool, device=gt.device)
    if ignore_gt >= 0:
        keep &= gt != ignore_gt
    if ignore_pred >= 0:
        keep &= pred != ignore_pred
    if ignore_aux >= 0:
        keep &= aux != ignore_aux
    idx = gt[keep].long() * K + pred[keep].long()
    return torch.bincount(idx, minlength=K * K).view(K, K), int((~keep).sum())


def layered(rows, cols, K, seed, device="cuda"):
    """Label maps like a radargram's: K sub-horizontal bands whose interfaces undulate (cf. `_real_radargram`), and a prediction
    whose interfaces are displaced -- long runs of one (gt, pred) bin along every row."""
    r = torch.arange(rows, device=device).float()[:, None]
    c = torch.arange(cols, device=device).float()[None, :]
    gt = torch.clamp(torch.floor((r + 6 * torch.sin(2 * np.pi * c / 700.0)) * K / rows), 0, K - 1)
    pr = torch.clamp(torch.floor((r + 9 * torch.sin(2 * np.pi * c / 500.0 + seed) + 4) * K / rows), 0, K - 1)
    return gt.flatten(), pr.flatten()


def make_labels(kind, P, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "random":  # uniformly random: no runs, the worst case for the in-lane aggregation
        return (torch.randint(0, K, (P,), generator=g, device="cuda").float(),
                torch.randint(0, K, (P,), generator=g, device="cuda").float())
    if kind == "one_class":  # every lane of every wave in one bin
        return torch.full((P,), float(K - 1), device="cuda"), torch.full((P,), 1.0, device="cuda")
    cols = 8192 if P >= 8192 else max(P, 1)
    rows = -(-P // cols)
    gt, pr = layered(rows, cols, K, seed)
    return gt[:P].contiguous(), pr[:P].contiguous()


BIG = 410 * 8192 * 3 + 5
MASKS = [dict(), dict(ignore_gt=1), dict(ignore_pred=0), dict(ignore_aux=4), dict(ignore_gt=1, ignore_pred=0, ignore_aux=4)]


def check_against_bincount(hip, gt, pr, K, aux, mask, dtype, offset):
    """gt / pr / aux: fp32 device vectors; the kernel gets them as `dtype`, starting `offset` elements into a wider buffer."""
    P = gt.numel()

    def view(t):
        wide = torch.empty(P + 8, dtype=dtype, device="cuda")
        wide[offset:offset + P] = t.to(dtype)
        v = wide[offset:offset + P]
        assert v.is_contiguous() and v.data_ptr() == wide.data_ptr() + offset * wide.element_size()
        return v

    use_aux = "ignore_aux" in mask
    counts, dropped = hip.confusion(view(gt), view(pr), K, aux=view(aux) if use_aux else None, **mask)
    want, masked = bincount_reference(gt, pr, K, aux, **mask)
    assert counts.dtype == torch.int64 and dropped.dtype == torch.int64 and counts.is_cuda
    assert torch.equal(counts, want), (P, K, mask, dtype, offset, (counts - want).abs().sum().item())
    assert dropped.tolist() == [masked, 0]
    assert int(counts.sum()) + masked == P


@pytest.mark.parametrize("K", [2, 5, 6, 16])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 4097, BIG])
def test_kernel_against_bincount(hip, P, K):
    """Every size x class count, each with fp32 and int8 operands, pointers offset by 0 / 1 (fp32) and 0 ... 3 (int8) elements, all
    five mask settings, on layered maps; the big size also on uniformly random and one-class maps."""
    kinds = ["layered", "random", "one_class"] if P == BIG else ["layered", "random"]
    for kind in kinds:
        gt, pr = make_labels(kind, P, K, seed=P % 97 + K)
        g = torch.Generator(device="cuda").manual_seed(K)
        aux = torch.where(torch.rand(P, generator=g, device="cuda") < 0.2, 4.0, 0.0)
        for dtype, offsets in ((torch.float32, (0, 1)), (torch.int8, (0, 1, 2, 3))):
            for offset in offsets:
                masks = MASKS if (offset in (0, 1) or P != BIG) else MASKS[-1:]
                for mask in masks:
                    check_against_bincount(hip, gt, pr, K, aux, mask, dtype, offset)


def test_operands_of_mixed_dtype_and_alignment(hip):
    """fp32 ground truth against an int8 prediction (a saved map), and operands whose offsets differ (no common 16-byte phase:
    the scalar route) -- same counts."""
    P, K = 50_000, 5
    gt, pr = make_labels("layered", P, K, 3)
    want, _ = bincount_reference(gt, pr, K)
    c, d = hip.confusion(gt, pr.to(torch.int8), K)
    assert torch.equal(c, want) and d.tolist() == [0, 0]
    c, d = hip.confusion(gt.to(torch.int8), pr, K)
    assert torch.equal(c, want)
    wide_g, wide_p = torch.zeros(P + 8, device="cuda"), torch.zeros(P + 8, device="cuda")
    wide_g[1:P + 1], wide_p[3:P + 3] = gt, pr
    c, d = hip.confusion(wide_g[1:P + 1], wide_p[3:P + 3], K)
    assert torch.equal(c, want) and d.tolist() == [0, 0]
    w8g, w8p = torch.zeros(P + 8, dtype=torch.int8, device="cuda"), torch.zeros(P + 8, dtype=torch.int8, device="cuda")
    w8g[2:P + 2], w8p[5:P + 5] = gt.to(torch.int8), pr.to(torch.int8)
    c, d = hip.confusion(w8g[2:P + 2], w8p[5:P + 5], K, aux=gt, ignore_aux=2)
    want2, masked = bincount_reference(gt, pr, K, gt, ignore_aux=2)
    assert torch.equal(c, want2) and d.tolist() == [masked, 0]
    # a column range of a wider map: made contiguous by the binding
    gm, pm = gt[:49_152].view(6, 8192), pr[:49_152].view(6, 8192)
    c, _ = hip.confusion(gm[:, 100:4001], pm[:, 100:4001], K)
    want3, _ = bincount_reference(gm[:, 100:4001].flatten(), pm[:, 100:4001].flatten(), K)
    assert torch.equal(c, want3)


def test_everything_masked_and_empty(hip):
    P, K = 100_003, 5
    gt, pr = make_labels("layered", P, K, 1)
    c, d = hip.confusion(gt, pr, K, aux=torch.full((P,), 4.0, device="cuda"), ignore_aux=4)
    assert not c.any() and d.tolist() == [P, 0]
    c, d = hip.confusion(torch.full((P,), 3, dtype=torch.int8, device="cuda"), pr, K, ignore_gt=3)
    assert not c.any() and d.tolist() == [P, 0]
    c, d = hip.confusion(torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda"), K)
    assert c.shape == (K, K) and c.is_cuda and not c.any() and d.tolist() == [0, 0]


def test_invalid_labels_are_counted_not_binned(hip):
    """-1, 2.5, NaN, K, +-inf, 1e30 in either map (fp32), -128 / 127 / K (int8): counted in dropped[1], in no bin, and a masked
    pixel is never invalid; the same answer as the CPU route.  `evaluate` turns the count into LabelError."""
    import inference as crw_inference
    P, K = 70_001, 5
    gt, pr = make_labels("layered", P, K, 2)
    gt, pr = gt.clone(), pr.clone()
    bad = [-1.0, 2.5, float("nan"), float(K), float("inf"), float("-inf"), 1e30, -0.5, 16777217.0]
    pos = torch.arange(len(bad), device="cuda") * 7001 + 3
    gt[pos] = torch.tensor(bad, device="cuda")
    pr[pos + 11] = torch.tensor(bad, device="cuda")
    pr[pos] = 0.0
    pr[pos[0]] = 3.0  # masked below: not invalid
    c, d = hip.confusion(gt, pr, K, ignore_pred=3)
    c_cpu, d_cpu = hip.confusion(gt.cpu(), pr.cpu(), K, ignore_pred=3)
    assert torch.equal(c.cpu(), c_cpu) and d.tolist() == d_cpu.tolist()
    assert d[1].item() == 2 * len(bad) - 1 and int(c.sum()) + int(d.sum()) == P
    g8, p8 = torch.zeros(1000, dtype=torch.int8, device="cuda"), torch.ones(1000, dtype=torch.int8, device="cuda")
    g8[[5, 500, 999]] = torch.tensor([-128, 127, K], dtype=torch.int8, device="cuda")
    c, d = hip.confusion(g8, p8, K)
    assert d.tolist() == [0, 3] and c[0, 1].item() == 997 and int(c.sum()) == 997
    with pytest.raises(hip.LabelError) as e:
        crw_inference.evaluate(pr, gt, 3, remove_unc=False)
    assert isinstance(e.value, ValueError) and e.value.invalid == 2 * len(bad)


def test_output_is_int64_and_partials_cannot_overflow(hip):
    """Counts above 2^31 are out of reach at test sizes (2^31 labels = 8 GB per fp32 map).  What is checked instead: the outputs
    are int64, and the 32-bit per-workgroup partials cannot overflow BY CONSTRUCTION -- a workgroup's pixels are bounded by
    ceil(P / grid), and the grid (2 048 workgroups up to P = 2^42) grows with P so that this never exceeds 2^31; every lane's run
    counter, every LDS counter and every partial is a sum over a subset of one workgroup's pixels, hence < 2^32.  The grid is read
    back from the workspace query: bytes / ((K*K+2) * 4)."""
    lib = hip.lib()
    for P in (1, 4096, BIG, 1 << 33, 1 << 42, (1 << 42) + 1, 1 << 50, (1 << 62) - 1):
        grid = lib.crw_confusion_ws_bytes(P, 16) // (258 * 4)
        assert grid >= 1 and -(-P // grid) <= 1 << 31, (P, grid)
    assert lib.crw_confusion_ws_bytes(BIG, 16) // (258 * 4) == 2048  # sized to the chip (256 CUs x 8), not to P
    gt, pr = make_labels("one_class", BIG, 5, 0)  # the largest single bin the suite produces
    c, d = hip.confusion(gt, pr, 5)
    assert c.dtype == torch.int64 and d.dtype == torch.int64 and c[4, 1].item() == BIG and int(c.sum()) == BIG
    # a workspace that is too small is refused, not overrun
    out = torch.zeros(27, dtype=torch.int64, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lib.crw_confusion(p(gt), 0, p(pr), 0, None, 0, BIG, 5, -1, -1, -1, p(out), ctypes.c_void_p(out.data_ptr() + 200), p(ws), 64,
                           None)
    assert st == hip.CRW_EWORKSPACE
    assert lib.crw_confusion(p(gt), 0, p(pr), 0, None, 0, BIG, 17, -1, -1, -1, p(out), p(out), p(ws), 64, None) == hip.CRW_EINVAL
    assert lib.crw_confusion(p(gt), 2, p(pr), 0, None, 0, BIG, 5, -1, -1, -1, p(out), p(out), p(ws), 64, None) == hip.CRW_EINVAL
    torch.cuda.synchronize()
    assert not out.any()


def test_two_streams_keep_their_own_results(hip):
    """Two calls on two streams with different inputs, repeated: every result is its own (no state shared between calls; each
    call has its own workspace and outputs)."""
    K = 6
    a = make_labels("layered", 3_000_017, K, 5)
    b = make_labels("random", 2_000_003, K, 6)
    want_a, _ = bincount_reference(*a, K)
    want_b, _ = bincount_reference(*b, K)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    for _ in range(4):
        with torch.cuda.stream(s1):
            got.append(("a", hip.confusion(*a, K)))
        with torch.cuda.stream(s2):
            got.append(("b", hip.confusion(*b, K, ignore_gt=-1)))
    torch.cuda.synchronize()
    for name, (c, d) in got:
        assert torch.equal(c, want_a if name == "a" else want_b) and d.tolist() == [0, 0]


@pytest.mark.parametrize("case", ["segment_ds1_reverse", "segment_ds3_correction_reverse"])
def test_segment_then_evaluate_end_to_end(hip, case):
    """`segment` on a segment_* fixture through the HIP path, then `evaluate` on the device map, equals `evaluate` of the
    fixture's recorded final map (the reference's own run)."""
    import inference as crw_inference
    import utils as crw_utils
    from test_host import run_segment_golden
    g = load_golden(case)
    out = run_segment_golden(g, crw_utils.propagate, "cuda")
    seg = torch.tensor(g["seg"])[:out["pred"].shape[0]]
    assert out["pred"].is_cuda
    ds_id = int(g["dataset_id"])
    got = crw_inference.evaluate(out["pred"], seg, ds_id)
    want = crw_inference.evaluate(torch.tensor(g["final_map"]), seg, ds_id)
    assert np.array_equal(got.counts, want.counts) and got.dropped == want.dropped
    assert str(got) == str(want) and got.matrix_str() == want.matrix_str() and got.total > 0


def test_cli_synthetic_run_in_a_child_process(hip, tmp_path):
    """scripts/segment_all.py --synthetic ... --report_json: exit status 0, the JSON's matrix sums to the unmasked pixel count,
    predicted_map.pt is int8 of the map's shape."""
    H, W, T = 200, 3 * 16 * 20, 20
    js = tmp_path / "report.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_all.py"), "--synthetic", str(H), str(W), "--dataset", "0",
                        "--model", "0", "--seq_length", str(T), "-c", "10", "--use_last", "true", "--output_folder",
                        str(tmp_path / "out") + "/", "--report_json", str(js)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(js.read_text())
    m = torch.load(tmp_path / "out" / "predicted_map.pt", map_location="cpu")
    N = (H - 8) // 8
    assert m.dtype == torch.int8 and tuple(m.shape) == (min(H, N * 16), W) == tuple(d["map_shape"])
    total = sum(sum(row) for row in d["matrix"])
    assert d["dropped"]["masked"] > 0 and d["dropped"]["invalid"] == 0
    assert total == d["pixels"] - d["dropped"]["masked"] == d["macro avg"]["support"]
    assert "precision    recall  f1-score   support" in r.stdout and "Time elapsed (inference + metrics):" in r.stdout
    assert 0.0 <= d["accuracy"] <= 1.0 and len(d["labels"]) == len(d["matrix"])
