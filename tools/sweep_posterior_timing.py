"""Times of the sweep's posterior (csrc/labelmap_dense.hip, crw_labelmap_ordered_posterior_batch / _joint_posterior_batch): what
does one launch for the G configurations of a sweep's window cost next to the loop of G one-map calls?

kernels  G = 60, T = 100, N = 48, a 410 x 3200 window, int8 labels, M = 4 and 6 (order = all classes), through the C entry points,
         labels, outputs and workspace allocated once, for the single and the joint ('maxprob') posterior:
           batch  ONE crw_labelmap_ordered[_joint]_posterior_batch launch for the G maps
           loop   G crw_labelmap_ordered[_joint]_posterior calls, one after the other, on the same operands' slices -- the kernel
                  the batch replaces, and the thing to compare against
         Both write the same bits (asserted once before the rounds).
driver   `inference.segment_sweep` with and without posterior=True on the `--synthetic 410 3200` input of scripts/segment_sweep.py
         (16 x 16 patches, overlap (8, 0), T = 100, two radargrams, the 60-configuration grid of launch_test_batch.sh, a
         random-init Resnet), decode='ordered', use_last with merge='ordered'.  A radargram is T * 16 = 1600 columns, so the
         driver's windows are 410 x 1600 (the `chunks` field is the binding's split for that window), not the kernels arm's 3200.

Arms alternate (A B A B ...) after a warm-up of each, device events around REPS calls (kernels) or one call (driver) that end in a
synchronise; every round's time and the spread of each arm are on the line.  No ratio is asserted.

usage: python tools/sweep_posterior_timing.py {kernels,driver} [--out FILE] [--rounds N]
One JSON line per case, appended to FILE (default profiles/sweep_posterior_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from confidence_timing import emit, med, spread, timed

RADII, TEMPS, KNNS = (45, 50, 55, 60, 65), (0.1, 0.01, 0.001), (15, 20, 25, 30)
G, T, N, ROWS, COLS, REPS, FLOOR = 60, 100, 48, 410, 3200, 20, 1e-4
PATCH, OVERLAP, CXT, K = (16, 16), (8, 0), 100, 5


def kernels(a):
    lib = crw_hip.lib()
    assert crw_hip.has_posterior() and crw_hip.has_posterior_batch() and crw_hip.has_joint()
    stream, ptr = crw_hip._stream(), crw_hip._ptr
    kind = crw_hip._conf_kind("maxprob")
    I8 = crw_hip.DT_I8
    for M in (4, 6):
        gen = torch.Generator().manual_seed(M)
        La, Lb = (torch.softmax(2 * torch.randn(G, T * N, M, generator=gen), -1).cuda() for _ in range(2))
        order = tuple(range(M))
        corder = (ctypes.c_int * M)(*order)
        one = lib.crw_labelmap_posterior_workspace(ROWS, COLS, M)
        ws = torch.empty(lib.crw_labelmap_posterior_workspace_batch(G, ROWS, COLS, M), dtype=torch.uint8, device="cuda")
        a_src, b_src = (La, T, COLS, 0, False), (Lb, T, COLS, 0, True)
        lab = crw_hip.labelmap_ordered_batch(La, G, T, N, M, ROWS, COLS, order, dtype=torch.int8)[0]
        jlab = crw_hip.labelmap_ordered_joint_batch(a_src, b_src, G, N, M, ROWS, COLS, order, confidence="maxprob", dtype=torch.int8)[0]
        post, ref = torch.empty(G, ROWS, COLS, device="cuda"), torch.empty(G, ROWS, COLS, device="cuda")
        hz, ref_hz = torch.empty(G, 3, M - 1, COLS, device="cuda"), torch.empty(G, 3, M - 1, COLS, device="cuda")
        ms, hzs, ls = ROWS * COLS, 3 * (M - 1) * COLS, T * N * M

        def single_batch(post=post, hz=hz):
            st = lib.crw_labelmap_ordered_posterior_batch(ptr(La), G, T, N, M, ROWS, COLS, 0, corder, M, FLOOR, ptr(lab), I8, COLS, ms, ptr(post),
                                                          ptr(hz), COLS, hzs, ptr(ws), ws.numel(), stream)
            assert st == 0, st

        def single_loop(post=post, hz=hz):
            for g in range(G):
                st = lib.crw_labelmap_ordered_posterior(ptr(La[g]), T, N, M, ROWS, COLS, 0, corder, M, FLOOR, ptr(lab[g]), I8, COLS, ptr(post[g]),
                                                        ptr(hz[g]), COLS, ptr(ws), one, stream)
                assert st == 0, st

        def joint_batch(post=post, hz=hz):
            st = lib.crw_labelmap_ordered_joint_posterior_batch(ptr(La), T, COLS, 0, 0, ptr(Lb), T, COLS, 0, 1, G, N, M, ROWS, COLS, corder, M, kind,
                                                                FLOOR, ptr(jlab), I8, COLS, ms, ptr(post), ptr(hz), COLS, hzs, ptr(ws), ws.numel(),
                                                                stream)
            assert st == 0, st

        def joint_loop(post=post, hz=hz):
            for g in range(G):
                st = lib.crw_labelmap_ordered_joint_posterior(ptr(La[g]), T, COLS, 0, 0, ptr(Lb[g]), T, COLS, 0, 1, N, M, ROWS, COLS, corder, M, kind,
                                                              FLOOR, ptr(jlab[g]), I8, COLS, ptr(post[g]), ptr(hz[g]), COLS, ptr(ws), one, stream)
                assert st == 0, st

        for name, batch, loop in (("single", single_batch, single_loop), ("joint", joint_batch, joint_loop)):
            batch(), loop(ref, ref_hz)  # the warm-up of each arm, and the claim: the same bits
            torch.cuda.synchronize()
            assert torch.equal(post.view(torch.int32), ref.view(torch.int32)) and torch.equal(hz.view(torch.int32), ref_hz.view(torch.int32))
            assert torch.isfinite(post).all() and post.min() >= 0 and post.max() <= 1 and torch.isfinite(hz).all()
            arms = dict(batch=lambda: [batch() for _ in range(REPS)], loop=lambda: [loop() for _ in range(REPS)])
            times = {n: [] for n in arms}
            for _ in range(a.rounds):
                for n, fn in arms.items():
                    times[n].append(timed(fn))
            emit(a.out, what="kernels", posterior=name, G=G, T=T, N=N, M=M, S=M, shape=[ROWS, COLS], labels="int8", floor=FLOOR,
                 confidence="maxprob" if name == "joint" else None, calls_per_round=REPS, workspace_bytes=ws.numel(),
                 waves_per_launch={"batch": G * ((COLS + 63) // 64), "loop": (COLS + 63) // 64}, mean_post=float(post.mean()),
                 **{n + "_ms": t for n, t in times.items()}, **{n + "_ms_per_call": med(t) / REPS for n, t in times.items()},
                 **{"spread_" + n: spread(t) for n, t in times.items()}, loop_over_batch=med(times["loop"]) / med(times["batch"]),
                 every_batch_round_beat_every_loop_round=max(times["batch"]) < min(times["loop"]),
                 slowest_batch_over_fastest_loop=max(times["batch"]) / min(times["loop"]))


def driver(a):
    import dataset as crw_dataset
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropSweep
    torch.manual_seed(11)
    enc = crw_utils.create_model(1, False).cuda()
    enc.train(True)
    rg = crw_dataset.synthetic_radargram(ROWS, COLS)
    seg = (torch.arange(ROWS)[:, None] * K // ROWS).float().repeat(1, COLS)
    sweep = LabelPropSweep(CXT, RADII, TEMPS, KNNS)
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, PATCH, OVERLAP)
    kw = dict(use_last=True, dataset_id=3, device="cuda", upsample="bilinear", confidence="maxprob", decode="ordered", order=tuple(range(K)),
              merge="ordered")
    run = dict(posterior=lambda: crw_inference.segment_sweep(fresh(), seg, enc, sweep, K, T, PATCH, OVERLAP, posterior=True, **kw),
               plain=lambda: crw_inference.segment_sweep(fresh(), seg, enc, sweep, K, T, PATCH, OVERLAP, **kw))
    out = {k: f() for k, f in run.items()}  # the warm-up of each arm
    torch.cuda.synchronize()
    assert torch.equal(out["posterior"]["pred"], out["plain"]["pred"])
    shape = list(out["posterior"]["post"].shape)
    del out
    res = {k: [] for k in run}
    for _ in range(a.rounds):
        for k, f in run.items():
            res[k].append(timed(f))
    emit(a.out, what="driver", configs=len(sweep.configs), post_shape=shape, T=T, patch=PATCH, overlap=OVERLAP, decode="ordered", merge="ordered",
         chunks=crw_hip.posterior_batch_chunks(len(sweep.configs), shape[1], T * PATCH[1], K),
         **{k + "_ms": v for k, v in res.items()}, **{"spread_" + k: spread(v) for k, v in res.items()},
         posterior_minus_plain_ms=med(res["posterior"]) - med(res["plain"]), posterior_over_plain=med(res["posterior"]) / med(res["plain"]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("kernels", "driver"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_posterior_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    a = p.parse_args()
    kernels(a) if a.mode == "kernels" else driver(a)


if __name__ == "__main__":
    main()
