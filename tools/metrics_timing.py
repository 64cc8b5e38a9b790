"""Time of the evaluation report's counting pass on three cfg5 label maps (410 x 24 576 pixels, 5 classes), layered and uniformly
random labels, fp32 and int8, without and with the auxiliary (uncertain-map) mask:
  (a) crw_confusion (csrc/metrics.hip) through crw_hip.confusion;
  (b) the same counts from PyTorch-ROCm ops on the device: (gt * K + pred).long() -> torch.bincount, plus the boolean-index
      masking of scripts/test/test_all.py:161-180;
  (c) the CPU route of crw_hip.confusion (torch.bincount on the host), wall clock.
(a) and (b): HIP events around each call, REPS calls after WARM warm-up calls, in the same process, alternating blocks; the
median per-call time, the minimum, and the back-to-back mean (one event pair around all REPS calls, which also holds the host's
per-call cost).  (a) is also given as bytes / time against the 8 TB/s HBM peak; its bytes are the maps read once.  Results must
agree exactly before anything is timed.
usage: python tools/metrics_timing.py [--reps 200] [--no-cpu]        (needs an MI355X; prints one JSON line per case)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd")]
import numpy as np
import torch

import crw_hip

ROWS, COLS, K = 410, 3 * 8192, 5
HBM_PEAK = 8e12
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 200
WARM = 10


def maps(kind):
    if kind == "random":
        g = torch.Generator(device="cuda").manual_seed(1)
        gt = torch.randint(0, K, (ROWS, COLS), generator=g, device="cuda").float()
        pr = torch.randint(0, K, (ROWS, COLS), generator=g, device="cuda").float()
    else:
        r = torch.arange(ROWS, device="cuda").float()[:, None]
        c = torch.arange(COLS, device="cuda").float()[None, :]
        gt = torch.clamp(torch.floor((r + 6 * torch.sin(2 * np.pi * c / 700.0)) * K / ROWS), 0, K - 1)
        pr = torch.clamp(torch.floor((r + 9 * torch.sin(2 * np.pi * c / 500.0 + 1) + 4) * K / ROWS), 0, K - 1)
    unc = gt.clone()
    unc[(torch.arange(ROWS, device="cuda").float()[:, None] - ROWS / 2).abs().expand(ROWS, COLS) < 0.03 * ROWS] = 4.0
    return gt, pr, unc


def torch_ops(gt, pr, unc):
    gt, pr = gt.flatten(), pr.flatten()
    if unc is not None:
        keep = (unc != 4).flatten()
        gt, pr = gt[keep], pr[keep]
    return torch.bincount((gt * K + pr).long(), minlength=K * K).view(K, K)


def per_call(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], back_to_back_ms=a.elapsed_time(b) / REPS)


def main():
    assert torch.cuda.is_available(), "needs an MI355X: a CPU run cannot give these times"
    crw_hip.lib()
    print(f"# {ROWS} x {COLS} = {ROWS * COLS} pixels, K = {K}, {REPS} calls after {WARM} warm-up, {torch.cuda.get_device_name(0)}")
    for kind in ("layered", "random"):
        gt32, pr32, unc32 = maps(kind)
        for dtype in (torch.float32, torch.int8):
            gt, pr, unc = gt32.to(dtype), pr32.to(dtype), unc32.to(dtype)
            for masked in (False, True):
                aux = unc if masked else None
                hip_fn = lambda: crw_hip.confusion(gt, pr, K, aux=aux, ignore_aux=4 if masked else -1)
                ops_fn = lambda: torch_ops(gt, pr, aux)
                assert torch.equal(hip_fn()[0], ops_fn())
                ta, tb = per_call(hip_fn), per_call(ops_fn)
                ta2, tb2 = per_call(hip_fn), per_call(ops_fn)  # second block of each, alternating: the spread
                nbytes = ROWS * COLS * gt.element_size() * (3 if masked else 2)
                res = dict(labels=kind, dtype=str(dtype).split(".")[-1], aux_mask=masked, bytes=nbytes,
                           crw_confusion=ta, crw_confusion_repeat=ta2, torch_ops=tb, torch_ops_repeat=tb2,
                           crw_confusion_TBps=nbytes / (ta["median_ms"] * 1e-3) / 1e12,
                           crw_confusion_share_of_hbm_peak=nbytes / (ta["median_ms"] * 1e-3) / HBM_PEAK,
                           speedup_over_torch_ops=tb["median_ms"] / ta["median_ms"],
                           not_slower_than_torch_ops=bool(max(ta["median_ms"], ta2["median_ms"]) <= min(tb["median_ms"], tb2["median_ms"])))
                print(json.dumps(res), flush=True)
        if "--no-cpu" not in sys.argv:
            g, p, u = gt32.cpu(), pr32.cpu(), unc32.cpu()
            crw_hip.confusion(g, p, K)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                crw_hip.confusion(g, p, K, aux=u, ignore_aux=4)
                ts.append(time.perf_counter() - t0)
            print(json.dumps(dict(labels=kind, dtype="float32", route="cpu (torch.bincount on the host)", aux_mask=True,
                                  threads=torch.get_num_threads(), seconds=sorted(ts)[1], seconds_all=ts)), flush=True)
    print("# scikit-learn on the host (classification_report + confusion_matrix on three 410 x 8192 maps, 5 classes): 7.4 s, measured "
          "on the CPU-only build machine (16 threads), not on this box")


if __name__ == "__main__":
    main()
