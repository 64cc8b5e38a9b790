"""Times of the sweep's dense label maps: the G maps of a pass in one launch against the loop of one-map launches, and
`inference.segment_sweep` with bilinear maps, confidence and the merge by confidence against the plain sweep and against the
per-configuration loop.  The method of tools/sweep_timing.py: all arms in one process, alternating, each warmed up, device events
around work that ends in a synchronise, every round's time on the log line.

  kernels  crw_hip.labelmap_dense_batch (one launch) against the loop of G crw_hip.labelmap_dense calls -- the parent's kernel, the
           thing to beat -- at G = 60, T = 100, N = 48, M = 4 and 6, 410 x 3200, int8, with and without 'maxprob'.  The batch
           kernel runs in each of its shapes: CRW_DENSE_BATCH_CHUNK = 1 (one configuration per blockIdx.z) and the chunked ones
           (a workgroup stages its knots once and walks `chunk` configurations).
  arms     on the `--synthetic 410 3200` input of scripts/segment_sweep.py (16 x 16 patches, overlap (8, 0), T = 100, two
           radargrams, random-init Resnet in train mode, reverse pass), the 5 x 3 x 4 grid:
             X  segment_sweep(upsample='bilinear', confidence='maxprob', merge='confidence')
             Y  segment_sweep()                                  (nearest maps, class rule: what the sweep did before)
             Z  G x segment(same options as X)                   (what X replaces)

usage: python tools/sweep_dense_timing.py kernels|arms [--out FILE] [--rounds N] [--chunks 1 4 8] [--arms XYZ]
One JSON line per result, appended to FILE (default profiles/sweep_dense_timing.log) and printed."""
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
G, T, N, ROWS, COLS = 60, 100, 48, 410, 3200
PATCH, OVERLAP, CXT, K = (16, 16), (8, 0), 100, 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def emit(out, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: (max(v) - min(v)) / med(v)


def with_chunk(chunk, fn):
    def run():
        os.environ["CRW_DENSE_BATCH_CHUNK"] = str(chunk)
        try:
            return fn()
        finally:
            os.environ.pop("CRW_DENSE_BATCH_CHUNK", None)
    return run


def kernels(a):
    for M in (4, 6):
        gen = torch.Generator().manual_seed(M)
        L = torch.softmax(2 * torch.randn(G, T * N, M, generator=gen), -1).cuda()
        for kind in (None, "maxprob"):
            lab = torch.empty(G, ROWS, COLS, dtype=torch.int8, device="cuda")
            conf = torch.empty(G, ROWS, COLS, device="cuda") if kind else None
            loop = lambda: [crw_hip.labelmap_dense(L[g], T, N, M, ROWS, COLS, confidence=kind, dtype=torch.int8, out=lab[g],
                                                   out_conf=None if conf is None else conf[g]) for g in range(G)]
            batch = lambda: crw_hip.labelmap_dense_batch(L, G, T, N, M, ROWS, COLS, confidence=kind, dtype=torch.int8, out=lab, out_conf=conf)
            run = {"loop": loop, **{f"batch_chunk{c}": with_chunk(c, batch) for c in a.chunks}}
            res = {k: [] for k in run}
            for f in run.values():
                f()
            for _ in range(a.rounds):
                for k, f in run.items():
                    res[k].append(timed(f))
            nbytes = G * ROWS * COLS * (5 if kind else 1)
            emit(a.out, what="kernels", G=G, T=T, N=N, M=M, rows=ROWS, cols=COLS, dtype="int8", confidence=kind, bytes_written=nbytes,
                 **{k + "_ms": v for k, v in res.items()}, **{k + "_spread": spread(v) for k, v in res.items()},
                 **{f"loop_over_{k}": med(res["loop"]) / med(v) for k, v in res.items() if k != "loop"})


def arms(a):
    torch.manual_seed(11)
    enc = crw_utils.create_model(1, False).cuda()
    enc.train(True)
    rg = crw_dataset.synthetic_radargram(ROWS, COLS)
    seg = (torch.arange(ROWS)[:, None] * K // ROWS).float().repeat(1, COLS)
    sweep = LabelPropSweep(CXT, RADII, TEMPS, KNNS)
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, PATCH, OVERLAP)
    kw = dict(use_last=True, dataset_id=3, device="cuda")
    on = dict(upsample="bilinear", confidence="maxprob", merge="confidence")
    run = dict(X=lambda: crw_inference.segment_sweep(fresh(), seg, enc, sweep, K, T, PATCH, OVERLAP, **kw, **on),
               Y=lambda: crw_inference.segment_sweep(fresh(), seg, enc, sweep, K, T, PATCH, OVERLAP, **kw),
               Z=lambda: [crw_inference.segment(fresh(), seg, enc, LabelPropVOS_CRW(cfg), K, T, PATCH, OVERLAP, **kw, **on) for cfg in sweep.configs])
    res = {k: [] for k in a.arms}
    for k in a.arms:
        run[k]()
    for _ in range(a.rounds):
        for k in a.arms:
            res[k].append(timed(run[k]))
    emit(a.out, what="arms", configs=len(sweep.configs), rows=ROWS, cols=COLS, T=T, patch=PATCH, overlap=OVERLAP,
         **{k + "_ms": v for k, v in res.items()}, **{k + "_spread": spread(v) for k, v in res.items()},
         **({"Z_over_X": med(res["Z"]) / med(res["X"])} if "X" in res and "Z" in res else {}),
         **({"X_over_Y": med(res["X"]) / med(res["Y"])} if "X" in res and "Y" in res else {}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("kernels", "arms"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_dense_timing.log"))
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 8])
    p.add_argument("--arms", default="XYZ")
    a = p.parse_args()
    kernels(a) if a.mode == "kernels" else arms(a)


if __name__ == "__main__":
    main()
