"""Times of the layer horizons (csrc/horizons.hip) at the cfg5 map size, 410 x 24 576 pixels, K = 5, layered maps with 2 % speckle,
for min_run 1 and 3 and the operand dtypes fp32 / fp32 (as `segment` leaves its maps) and fp32 / int8 (as `segment_sweep` does):

  horizons        crw_horizons with picks            (the C entry point through ctypes: outputs and workspace allocated once)
  horizons_stats  crw_horizons without picks
  confusion       crw_confusion on the same operands -- the parent commit's kernel over the same bytes: the yardstick
  composite       min_run 1 only: the PyTorch-ROCm composite on the device -- per class (map == k) -> first index, last index and
                  sum down the columns, for both maps, and the differences' sums

Arms alternate (A B C D A B C D ...) after a warm-up of each, device events around REPS calls that end in a synchronise; every
round's time and the spread of each arm are on the line.  Before timing, the kernel's statistics are checked against the
composite's (min_run 1) and against the binding's CPU route (min_run 3).

usage: python tools/horizons_timing.py [--out FILE] [--rounds N] [--row_slabs S]
One JSON line per result, appended to FILE (default profiles/horizons_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from confidence_timing import emit, med, spread, timed

ROWS, COLS, K, REPS, TOL = 410, 24576, 5, 20, 2


def maps(seed):
    g = torch.Generator().manual_seed(seed)
    r, c = torch.arange(ROWS).float()[:, None], torch.arange(COLS).float()[None, :]
    gt = torch.clamp(torch.floor((r + 8 * torch.sin(2 * torch.pi * c / 900.0)) * K / ROWS), 0, K - 1)
    pr = torch.clamp(torch.floor((r + 11 * torch.sin(2 * torch.pi * c / 700.0) + 3) * K / ROWS), 0, K - 1)
    hit = torch.rand(pr.shape, generator=g) < 0.02
    pr = torch.where(hit, torch.randint(0, K, pr.shape, generator=g).float(), pr)
    return gt.cuda(), pr.cuda()


def composite(gt, pr):
    """min_run = 1 with valid labels: first / last row and pixel count per class from comparisons and reductions."""
    rows = torch.arange(ROWS, device=gt.device)[:, None]
    picks = []
    for m in (gt, pr):
        per = []
        for k in range(K):
            hot = m == k
            n = hot.sum(0)
            top = torch.where(hot, rows, ROWS).amin(0)
            bottom = torch.where(hot, rows, -1).amax(0)
            per.append(torch.stack([torch.where(n > 0, top, -1), bottom, n]))
        picks.append(torch.stack(per, 1))
    picks = torch.stack(picks)  # [2, 3, K, cols]
    both = (picks[0, 2] > 0) & (picks[1, 2] > 0)
    d = torch.where(both, picks[1] - picks[0], 0)
    stats = torch.stack([both.sum(1), ((picks[0, 2] > 0) & ~both).sum(1), ((picks[1, 2] > 0) & ~both).sum(1)]
                        + [v for q in range(3) for v in (d[q].abs().sum(1), (d[q] * d[q]).sum(1), d[q].abs().amax(1),
                                                         (both & (d[q].abs() <= TOL)).sum(1), d[q].sum(1))], 1)
    return stats, picks


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "horizons_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--row_slabs", type=int, default=0, help="crw_horizons' row_slabs (0: the library chooses)")
    a = p.parse_args()
    L = crw_hip.lib()
    assert crw_hip.has_horizons()
    gt, pr32 = maps(5)
    stream, ptr = crw_hip._stream(), crw_hip._ptr
    for name, pr in (("fp32/fp32", pr32), ("fp32/int8", pr32.to(torch.int8))):
        code = crw_hip.DT_F32 if pr.dtype == torch.float32 else crw_hip.DT_I8
        hout = torch.empty(K * 18 + 2, dtype=torch.int64, device="cuda")
        picks = torch.empty(2, 3, K, COLS, dtype=torch.int32, device="cuda")
        hws = torch.empty(L.crw_horizons_ws_bytes(ROWS, COLS, K), dtype=torch.uint8, device="cuda")
        cout = torch.empty(K * K + 2, dtype=torch.int64, device="cuda")
        cws = torch.empty(L.crw_confusion_ws_bytes(ROWS * COLS, K), dtype=torch.uint8, device="cuda")

        def horizons(min_run, want_picks):
            st = L.crw_horizons(ptr(gt), crw_hip.DT_F32, ptr(pr), code, None, crw_hip.DT_I8, ROWS, COLS, COLS, K, -1, -1, -1, min_run, TOL, a.row_slabs,
                                ptr(picks) if want_picks else None, ptr(hout), ctypes.c_void_p(hout.data_ptr() + 8 * K * 18), ptr(hws),
                                hws.numel(), stream)
            assert st == 0, st

        def confusion():
            st = L.crw_confusion(ptr(gt), crw_hip.DT_F32, ptr(pr), code, None, crw_hip.DT_I8, ROWS * COLS, K, -1, -1, -1, ptr(cout),
                                 ctypes.c_void_p(cout.data_ptr() + 8 * K * K), ptr(cws), cws.numel(), stream)
            assert st == 0, st

        for min_run in (1, 3):
            horizons(min_run, True)
            got = hout[:K * 18].view(K, 18).clone()
            if min_run == 1:
                want, wpicks = composite(gt, pr)
                assert torch.equal(got, want) and torch.equal(picks, wpicks.to(torch.int32))
            else:
                want = crw_hip.horizons(gt.cpu(), pr.cpu(), K, min_run=min_run, tol=TOL)[0]
                assert torch.equal(got.cpu(), want)
            arms = dict(horizons=lambda: [horizons(min_run, True) for _ in range(REPS)],
                        horizons_stats=lambda: [horizons(min_run, False) for _ in range(REPS)],
                        confusion=lambda: [confusion() for _ in range(REPS)])
            if min_run == 1:
                arms["composite"] = lambda: [composite(gt, pr) for _ in range(REPS)]
            for fn in arms.values():
                fn()
            times = {n: [] for n in arms}
            for _ in range(a.rounds):
                for n, fn in arms.items():
                    times[n].append(timed(fn))
            read = ROWS * COLS * (4 + (4 if pr.dtype == torch.float32 else 1))
            emit(a.out, what="horizons", shape=[ROWS, COLS], K=K, min_run=min_run, tol=TOL, dtypes=name, row_slabs=a.row_slabs, calls_per_round=REPS,
                 **{n + "_ms": t for n, t in times.items()}, **{n + "_us_per_call": 1e3 * med(t) / REPS for n, t in times.items()},
                 horizons_over_confusion=med(times["horizons"]) / med(times["confusion"]),
                 horizons_stats_over_confusion=med(times["horizons_stats"]) / med(times["confusion"]),
                 horizons_read_GBps=read * REPS / med(times["horizons"]) / 1e6, confusion_read_GBps=read * REPS / med(times["confusion"]) / 1e6,
                 **{"spread_" + n: spread(t) for n, t in times.items()})


if __name__ == "__main__":
    main()
