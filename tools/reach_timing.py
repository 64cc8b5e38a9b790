"""Times of the grouped confusion matrix (csrc/reach.hip) at the cfg5 map size, 410 x 24 576 pixels, K = 5, 12 column groups (the
default edges around the seed frames of 16-column items' frames), layered maps with 2 % speckle, for the operand dtypes fp32 / fp32
(as `segment` leaves its maps) and fp32 / int8 (as `segment_sweep` does), each without and with a confidence map:

  grouped    crw_confusion_grouped               (the C entry point through ctypes: outputs and workspace allocated once)
  confusion  crw_confusion on the same operands  (what it generalises: one matrix, no groups, no confidence -- the yardstick)
  bincount   the same counts from PyTorch-ROCm ops on the device: one torch.bincount of group * K * K + gt * K + pred under the
             mask (with a confidence map: a second, weighted bincount of the groups for the sums)

EXPECTATION, written before the first run: crw_confusion_grouped reads the maps the way crw_horizons does -- one lane per column, 256
contiguous bytes per wave and load instruction where crw_confusion reads 1 KiB, 8 rows in flight -- and crw_horizons landed at
2.0 - 2.4 x crw_confusion.  It does less work per pixel than crw_horizons (no run bookkeeping beyond one open bin, no join), so
the guess is 1.5 - 2.5 x crw_confusion without a confidence map and, with one (a third more bytes and one fp64 add per pixel),
2 - 3 x; and several times faster than the bincount arm, which materialises an int64 index per pixel.  A guess, not a bound: the log
says how it came out.

Arms alternate (A B C A B C ...) after a warm-up of each, device events around REPS calls that end in a synchronise; every round's
time and the spread of each arm are on the line.  Before timing, the kernel's counts are checked against the bincount arm's.

usage: python tools/reach_timing.py [--out FILE] [--rounds N]
One JSON line per result, appended to FILE (default profiles/reach_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from confidence_timing import emit, med, spread, timed
from horizons_timing import maps

ROWS, COLS, K, REPS, STEP, T = 410, 24576, 5, 20, 16, 96


def bincount(gt, pr, conf, group, groups):
    """valid labels, no mask: the index of every pixel, one bincount (and, with confidences, their sums per group)"""
    g = group.to(torch.int64)[None, :]
    idx = ((g * K + gt.to(torch.int64)) * K + pr.to(torch.int64)).reshape(-1)
    counts = torch.bincount(idx, minlength=groups * K * K)
    if conf is None:
        return counts, None
    return counts, torch.bincount(g.expand(ROWS, COLS).reshape(-1), weights=conf.reshape(-1).double(), minlength=groups)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    a = p.parse_args()
    L = crw_hip.lib()
    assert crw_hip.has_reach()
    gt, pr32 = maps(5)
    conf32 = torch.rand(ROWS, COLS, generator=torch.Generator().manual_seed(6)).cuda()
    rg_len = T * STEP                                                   # items of 96 frames of 16 columns, seeded at both ends
    labelled = [c for t in range(COLS // rg_len) for c in list(range(rg_len * t, rg_len * t + STEP)) + list(range(rg_len * (t + 1) - STEP, rg_len * (t + 1)))]
    group = crw_hip.column_groups(COLS, labelled, STEP, segments=list(range(0, COLS + 1, rg_len)))[0].cuda()
    groups = len(crw_hip.REACH_EDGES) + 2
    stream, ptr = crw_hip._stream(), crw_hip._ptr
    n = groups * K * K
    for name, pr in (("fp32/fp32", pr32), ("fp32/int8", pr32.to(torch.int8))):
        code = crw_hip.DT_F32 if pr.dtype == torch.float32 else crw_hip.DT_I8
        gout = torch.empty(n + groups + 4, dtype=torch.int64, device="cuda")
        gws = torch.empty(L.crw_confusion_grouped_ws_bytes(ROWS, COLS, K, groups), dtype=torch.uint8, device="cuda")
        cout = torch.empty(K * K + 2, dtype=torch.int64, device="cuda")
        cws = torch.empty(L.crw_confusion_ws_bytes(ROWS * COLS, K), dtype=torch.uint8, device="cuda")
        at = lambda o: ctypes.c_void_p(gout.data_ptr() + 8 * o)

        def confusion():
            st = L.crw_confusion(ptr(gt), crw_hip.DT_F32, ptr(pr), code, None, crw_hip.DT_I8, ROWS * COLS, K, -1, -1, -1, ptr(cout),
                                 ctypes.c_void_p(cout.data_ptr() + 8 * K * K), ptr(cws), cws.numel(), stream)
            assert st == 0, st

        for conf in (None, conf32):
            def grouped():
                st = L.crw_confusion_grouped(ptr(gt), crw_hip.DT_F32, ptr(pr), code, None, crw_hip.DT_I8, ptr(conf) if conf is not None else None,
                                             ROWS, COLS, COLS, ptr(group), groups, K, -1, -1, -1, at(0), at(n) if conf is not None else None,
                                             at(n + groups), ptr(gws), gws.numel(), stream)
                assert st == 0, st

            grouped()
            want, wsum = bincount(gt, pr, conf, group, groups)
            assert torch.equal(gout[:n], want) and not gout[n + groups:].any()
            if conf is not None:
                assert torch.allclose(gout[n:n + groups].view(torch.float64), wsum, rtol=1e-9, atol=0)
            arms = dict(grouped=lambda: [grouped() for _ in range(REPS)], confusion=lambda: [confusion() for _ in range(REPS)],
                        bincount=lambda: [bincount(gt, pr, conf, group, groups) for _ in range(REPS)])
            for fn in arms.values():
                fn()
            times = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    times[k].append(timed(fn))
            read = ROWS * COLS * (4 + (4 if pr.dtype == torch.float32 else 1) + (4 if conf is not None else 0))
            emit(a.out, what="reach", shape=[ROWS, COLS], K=K, groups=groups, dtypes=name, conf=conf is not None, calls_per_round=REPS,
                 **{k + "_ms": t for k, t in times.items()}, **{k + "_us_per_call": 1e3 * med(t) / REPS for k, t in times.items()},
                 grouped_over_confusion=med(times["grouped"]) / med(times["confusion"]),
                 bincount_over_grouped=med(times["bincount"]) / med(times["grouped"]),
                 grouped_read_GBps=read * REPS / med(times["grouped"]) / 1e6,
                 **{"spread_" + k: spread(t) for k, t in times.items()})


if __name__ == "__main__":
    main()
