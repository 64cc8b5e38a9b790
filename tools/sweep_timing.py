"""Times of the (radius, temp, knn) sweep over the grid of the reference's scripts/launch/launch_test_batch.sh (5 x 3 x 4 = 60
configurations) at the mc1-like and mc3-like geometries ([T, N] = [100, 48] and [100, 190]; 410-row radargram, 32 x 32 patches,
random-init Resnet in train mode), forward + reverse pass of one radargram, plus the report of every configuration:

  A  the loop over configurations: 60 x (inference.segment + inference.evaluate)
  B  inference.segment_sweep + evaluate_sweep with CRW_SWEEP_PER_CONFIG=1 (encoder once, label propagation per configuration)
  C  inference.segment_sweep + evaluate_sweep (one selection per (radius, temp), all configurations' chains side by side)

All arms in one process, alternating (A C B A C B ...), each warmed up, device events around work that ends in a synchronise.

usage: python tools/sweep_timing.py arms|kernels|trace [--out FILE] [--rounds N] [--geom mc1 mc3] [--arms ABC]
  arms     the three arms at both geometries (every round's time, so that the A/A and C/C spread is on the line); --arms A: that
           arm alone (with CRW_HIP_LIB=<another build of the library>: the per-configuration loop on that build)
  kernels  the three entry points alone against their per-configuration counterparts
  trace    arm C once per geometry after one warm-up, for `rocprofv3 --kernel-trace --stats -- python tools/sweep_timing.py trace`
One JSON line per result, appended to FILE (default profiles/sweep_timing.log) and printed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd")]
import torch

import crw_hip
import dataset as crw_dataset
import inference as crw_inference
import utils as crw_utils
from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW

RADII, TEMPS, KNNS = (45, 50, 55, 60, 65), (0.1, 0.01, 0.001), (15, 20, 25, 30)
GEOM = {"mc1": dict(overlap=(24, 0), cxt=80, N=48), "mc3": dict(overlap=(30, 0), cxt=100, N=190)}
ROWS, COLS, T, PATCH, K = 410, 3200, 100, (32, 32), 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def ev_time(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    return timed(lambda: [fn() for _ in range(reps)]) / reps


def emit(out, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def arms(geom, enc, seg, rg):
    g = GEOM[geom]
    sweep = LabelPropSweep(g["cxt"], RADII, TEMPS, KNNS)
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, PATCH, g["overlap"])
    kw = dict(use_last=True, dataset_id=3, device="cuda")

    def arm_a():
        for cfg in sweep.configs:
            out = crw_inference.segment(fresh(), seg, enc, LabelPropVOS_CRW(cfg), K, T, PATCH, g["overlap"], **kw)
            crw_inference.evaluate(out["pred"], seg, 3, nclasses=K)

    def arm_sweep(per_config):
        def run():
            os.environ["CRW_SWEEP_PER_CONFIG"] = "1" if per_config else "0"
            try:
                out = crw_inference.segment_sweep(fresh(), seg, enc, sweep, K, T, PATCH, g["overlap"], **kw)
                return crw_inference.evaluate_sweep(out["pred"], seg, 3, nclasses=K)
            finally:
                os.environ.pop("CRW_SWEEP_PER_CONFIG", None)
        return run
    return arm_a, arm_sweep(True), arm_sweep(False)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("arms", "kernels", "trace"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_timing.log"))
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--geom", nargs="+", default=list(GEOM))
    p.add_argument("--arms", default="ABC", help="arms to time, e.g. A alone (with CRW_HIP_LIB=<another build>: arm A on that build)")
    a = p.parse_args()
    if a.mode == "kernels":
        for geom in a.geom:
            g = GEOM[geom]
            N, cxt, M = g["N"], g["cxt"], K
            gen = torch.Generator().manual_seed(1)
            feats = crw_hip.normalize((torch.randn(1, N, 128, generator=gen) + 0.5 * torch.randn(T, N, 128, generator=gen)).float().cuda())
            seed = (torch.arange(N) * M // N).float().cuda()
            r, temp = 60, 0.01
            t_per = ev_time(lambda: [crw_hip.labelprop_topk(feats, cxt, r, temp, k) for k in KNNS])
            t_one = ev_time(lambda: crw_hip.labelprop_sweep_weights(crw_hip.labelprop_topk_scores(feats, cxt, r, temp, max(KNNS))[0], KNNS))
            emit(a.out, what="topk", geom=geom, per_config_4x_topk_ms=t_per, scores_plus_weights_ms=t_one, ratio=t_per / t_one)
            V, I = crw_hip.labelprop_topk_scores(feats, cxt, r, temp, max(KNNS))
            W4 = crw_hip.labelprop_sweep_weights(V, KNNS)
            lists = [crw_hip.labelprop_topk(feats, cxt, r, temp, k) for k in KNNS]
            for G in (12, 60):
                W = W4.repeat(G // 4, 1, 1, 1).contiguous()
                t_batch = ev_time(lambda: crw_hip.labelprop_propagate_batch(seed, W, I, T, N, M, cxt_size=cxt))
                t_loop = ev_time(lambda: [crw_hip.labelprop_gather(seed, *lists[i % 4], T, N, M, cxt_size=cxt) for i in range(G)], reps=3, warm=1)
                emit(a.out, what="propagate", geom=geom, G=G, per_config_ms=t_loop, batch_ms=t_batch, ratio=t_loop / t_batch)
        return
    torch.manual_seed(11)
    enc = crw_utils.create_model(1, False).cuda()
    enc.train(True)
    rg = crw_dataset.synthetic_radargram(ROWS, COLS)
    seg = (torch.arange(ROWS)[:, None] * K // ROWS).float().repeat(1, COLS)
    for geom in a.geom:
        arm_a, arm_b, arm_c = arms(geom, enc, seg, rg)
        if a.mode == "trace":
            arm_c()
            torch.cuda.synchronize()
            arm_c()
            torch.cuda.synchronize()
            continue
        med = lambda v: sorted(v)[len(v) // 2]
        spread = lambda v: (max(v) - min(v)) / med(v)
        if a.arms != "ABC":
            run = dict(A=arm_a, B=arm_b, C=arm_c)
            res = {}
            for k in a.arms:
                run[k]()
            for _ in range(a.rounds):
                for k in a.arms:
                    res.setdefault(k + "_ms", []).append(timed(run[k]))
            emit(a.out, what="arms", geom=geom, lib=os.path.basename(crw_hip.LIB_PATH), has_sweep=crw_hip.has_sweep(), **res)
            continue
        for f in (arm_a, arm_b, arm_c):
            f()
        ta, tb, tc = [], [], []
        for _ in range(a.rounds):
            ta.append(timed(arm_a))
            tc.append(timed(arm_c))
            tb.append(timed(arm_b))
        emit(a.out, what="arms", geom=geom, configs=len(RADII) * len(TEMPS) * len(KNNS), A_ms=ta, B_ms=tb, C_ms=tc,
             A_over_B=med(ta) / med(tb), B_over_C=med(tb) / med(tc), A_over_C=med(ta) / med(tc),
             spread_AA=spread(ta), spread_BB=spread(tb), spread_CC=spread(tc))


if __name__ == "__main__":
    main()
