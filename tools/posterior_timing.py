"""Times of the ordered maps' posterior (csrc/labelmap_dense.hip, crw_labelmap_ordered_posterior / _joint_posterior): what do the
confidence and the error bars cost next to the decode they belong to?

Four arms at T = 256, N = 48, M = 4 and 6 (order = all classes), 410 x 8192 pixels, int8 labels, through the C entry points,
outputs and workspaces allocated once:
  posterior        crw_labelmap_ordered_posterior on the map crw_labelmap_ordered wrote (post and hz)
  joint_posterior  crw_labelmap_ordered_joint_posterior ('maxprob') on the map crw_labelmap_ordered_joint wrote: a forward source
                   and a mirrored reverse source of the same geometry
  ordered          crw_labelmap_ordered (no confidence map) on the same operands
  joint            crw_labelmap_ordered_joint ('maxprob', with its confidence map) on the same operands
The two decodes are the yardsticks: the posterior runs two scans of `rows` steps in series where the decode runs one and a
back-track.

Arms alternate (A B C D A B C D ...) after a warm-up of each, device events around REPS calls that end in a synchronise; every
round's time and the spread of each arm are on the line.

usage: python tools/posterior_timing.py [--out FILE] [--rounds N]
One JSON line per M, appended to FILE (default profiles/posterior_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from confidence_timing import emit, med, spread, timed

T, N, ROWS, COLS, REPS, FLOOR = 256, 48, 410, 8192, 20, 1e-4


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    a = p.parse_args()
    torch.manual_seed(5)
    lib = crw_hip.lib()
    assert crw_hip.has_posterior() and crw_hip.has_joint()
    stream, ptr = crw_hip._stream(), crw_hip._ptr
    kind = crw_hip._conf_kind("maxprob")
    for M in (4, 6):
        La, Lb = (torch.distributions.Dirichlet(torch.ones(M)).sample((T * N,)).float().cuda() for _ in range(2))
        corder = (ctypes.c_int * M)(*range(M))
        dws = torch.empty(lib.crw_labelmap_ordered_workspace(1, ROWS, COLS), dtype=torch.uint8, device="cuda")
        pws = torch.empty(lib.crw_labelmap_posterior_workspace(ROWS, COLS, M), dtype=torch.uint8, device="cuda")
        lab, jlab = (torch.empty(ROWS, COLS, dtype=torch.int8, device="cuda") for _ in range(2))
        jconf = torch.empty(ROWS, COLS, device="cuda")
        post, jpost = torch.empty(ROWS, COLS, device="cuda"), torch.empty(ROWS, COLS, device="cuda")
        hz, jhz = torch.empty(3, M - 1, COLS, device="cuda"), torch.empty(3, M - 1, COLS, device="cuda")
        both = (ptr(La), T, COLS, 0, 0, ptr(Lb), T, COLS, 0, 1)

        def ordered():
            for _ in range(REPS):
                st = lib.crw_labelmap_ordered(ptr(La), T, N, M, ROWS, COLS, 0, corder, M, -1, ptr(lab), crw_hip.DT_I8, None, COLS, ptr(dws),
                                              dws.numel(), stream)
                assert st == 0, st

        def joint():
            for _ in range(REPS):
                st = lib.crw_labelmap_ordered_joint(*both, N, M, ROWS, COLS, corder, M, kind, ptr(jlab), crw_hip.DT_I8, ptr(jconf), COLS, ptr(dws),
                                                    dws.numel(), stream)
                assert st == 0, st

        def posterior():
            for _ in range(REPS):
                st = lib.crw_labelmap_ordered_posterior(ptr(La), T, N, M, ROWS, COLS, 0, corder, M, FLOOR, ptr(lab), crw_hip.DT_I8, COLS, ptr(post),
                                                        ptr(hz), COLS, ptr(pws), pws.numel(), stream)
                assert st == 0, st

        def joint_posterior():
            for _ in range(REPS):
                st = lib.crw_labelmap_ordered_joint_posterior(*both, N, M, ROWS, COLS, corder, M, kind, FLOOR, ptr(jlab), crw_hip.DT_I8, COLS,
                                                              ptr(jpost), ptr(jhz), COLS, ptr(pws), pws.numel(), stream)
                assert st == 0, st

        arms = dict(ordered=ordered, joint=joint, posterior=posterior, joint_posterior=joint_posterior)
        for fn in arms.values():  # the decodes first: the posteriors read their maps
            fn()
        torch.cuda.synchronize()
        for m in (post, jpost):
            assert torch.isfinite(m).all() and m.min() >= 0 and m.max() <= 1
        assert torch.isfinite(hz).all() and torch.isfinite(jhz).all()
        times = {n: [] for n in arms}
        for _ in range(a.rounds):
            for n, fn in arms.items():
                times[n].append(timed(fn))
        per_call = {n: 1e3 * med(t) / REPS for n, t in times.items()}
        emit(a.out, what="kernel", T=T, N=N, M=M, S=M, shape=[ROWS, COLS], labels="int8", floor=FLOOR, confidence="maxprob",
             calls_per_round=REPS, workspace_bytes=pws.numel(), mean_post=float(post.mean()), mean_joint_post=float(jpost.mean()),
             mean_bar_rows=float(hz[2].mean()), **{n + "_ms": t for n, t in times.items()},
             **{n + "_us_per_call": v for n, v in per_call.items()},
             posterior_over_ordered=per_call["posterior"] / per_call["ordered"],
             joint_posterior_over_joint=per_call["joint_posterior"] / per_call["joint"],
             posterior_us_per_row=per_call["posterior"] / ROWS, waves=(COLS + 63) // 64,
             **{"spread_" + n: spread(t) for n, t in times.items()})


if __name__ == "__main__":
    main()
