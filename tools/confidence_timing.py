"""Times of the confidence path (csrc/confidence.hip):

  calibration  crw_hip.calibration on three cfg5-sized maps side by side (410 x 24 576 pixels, 5 classes, 10 bins; layered int8
               labels as the drivers save them, fp32 confidence) against the same counts and sums from PyTorch-ROCm ops on the
               device (mask, floor, three torch.bincount calls -- what the binding's CPU route does, on the GPU), for a layered
               confidence map (an upsampled node map) and for uniformly random confidences (no runs: the kernel's worst case)
  segment      inference.segment(..., confidence='maxprob') against the same call without it -- what the parent commit does --
               on one 410 x 3 200 radargram (32 x 32 patches, [T, N] = [100, 48], random-init Resnet in train mode), forward +
               reverse pass
  merge        crw_hip.merge_confidence against two torch.where calls on one cfg5-sized fp32 map

Arms alternate (A B A B ...) after a warm-up of each, device events around work that ends in a synchronise; every round's time
and the spread of each arm are on the line.

usage: python tools/confidence_timing.py [calibration segment merge] [--out FILE] [--rounds N]
One JSON line per result, appended to FILE (default profiles/confidence_timing.log) and printed."""
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
from imported.labelprop import LabelPropVOS_CRW

ROWS, COLS, K, BINS = 410, 24576, 5, 10


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


def alternate(arm_a, arm_b, rounds):
    arm_a()
    arm_b()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(arm_a))
        tb.append(timed(arm_b))
    return ta, tb


def torch_calibration(gt, pred, conf, K, bins):
    """The binding's CPU route on the device: the same integers, the sums in float64."""
    g, p = gt.reshape(-1).long(), pred.reshape(-1).long()
    c = conf.reshape(-1)
    valid = (g >= 0) & (g < K) & (p >= 0) & (p < K)
    cvalid = (c >= 0) & (c <= 1)
    binned = valid & cvalid
    b = torch.clamp(torch.floor(torch.where(binned, c, torch.zeros_like(c)) * bins), max=bins - 1).long()
    row = torch.where(~valid, bins + 1, torch.where(~cvalid, bins + 2, b))
    n = torch.bincount(row, minlength=bins + 3)
    ok = torch.bincount(row, weights=(binned & (g == p)).double(), minlength=bins + 3).long()
    s = torch.bincount(row, weights=torch.where(binned, c.double(), torch.zeros((), dtype=torch.float64, device=c.device)), minlength=bins + 3)
    return torch.stack([n[:bins], ok[:bins]], 1), s[:bins], n[bins:]


def layered_maps(gen):
    r = torch.arange(ROWS).float()[:, None]
    c = torch.arange(COLS).float()[None, :]
    gt = torch.clamp(torch.floor((r + 12 * torch.sin(c / 700.0)) * K / ROWS), 0, K - 1)
    pred = torch.clamp(torch.floor((r + 5 + 12 * torch.sin(c / 650.0)) * K / ROWS), 0, K - 1)
    nodes = 0.4 + 0.6 * torch.rand(ROWS // 8 + 1, COLS // 32, generator=gen)  # one confidence per 8 x 32 block, as `segment` upsamples
    conf = nodes.repeat_interleave(8, 0)[:ROWS].repeat_interleave(32, 1)
    return gt.to(torch.int8).cuda(), pred.to(torch.int8).cuda(), conf.contiguous().cuda()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", nargs="*", default=["calibration", "merge", "segment"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidence_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    a = p.parse_args()
    gen = torch.Generator().manual_seed(3)
    if "calibration" in a.what:
        maps = [layered_maps(gen) for _ in range(3)]
        for stats in ("layered", "random"):
            if stats == "random":
                maps = [(g, q, torch.rand(ROWS, COLS, generator=gen).cuda()) for g, q, _ in maps]
            kernel = lambda: [crw_hip.calibration(g, q, c, K, bins=BINS) for g, q, c in maps]
            ops = lambda: [torch_calibration(g, q, c, K, BINS) for g, q, c in maps]
            for (kc, ks, kd), (tc, ts, td) in zip(kernel(), ops()):  # the two arms count the same thing
                assert torch.equal(kc, tc) and torch.equal(kd, td) and torch.allclose(ks, ts, rtol=1e-9, atol=0)
            tk, tt = alternate(kernel, ops, a.rounds)
            emit(a.out, what="calibration", confidence=stats, maps=3, pixels=ROWS * COLS, K=K, bins=BINS, kernel_ms=tk, torch_ops_ms=tt,
                 kernel_median_ms=med(tk), torch_ops_median_ms=med(tt), torch_over_kernel=med(tt) / med(tk),
                 kernel_GBps=3 * ROWS * COLS * 6 / med(tk) / 1e6, spread_kernel=spread(tk), spread_torch=spread(tt))
    if "merge" in a.what:
        fl, rl = (torch.randint(0, K, (ROWS, COLS), generator=gen).float().cuda() for _ in range(2))
        fc, rc = (torch.rand(ROWS, COLS, generator=gen).cuda() for _ in range(2))
        kernel = lambda: crw_hip.merge_confidence(fl, fc, rl, rc)
        ops = lambda: (torch.where(rc > fc, rl, fl), torch.where(rc > fc, rc, fc))
        assert torch.equal(kernel()[0], ops()[0]) and torch.equal(kernel()[1], ops()[1])
        tk, tt = alternate(kernel, ops, a.rounds)
        emit(a.out, what="merge", pixels=ROWS * COLS, kernel_ms=tk, torch_where_ms=tt, kernel_median_ms=med(tk), torch_where_median_ms=med(tt),
             torch_over_kernel=med(tt) / med(tk), kernel_GBps=ROWS * COLS * 24 / med(tk) / 1e6, spread_kernel=spread(tk), spread_torch=spread(tt))
    if "segment" in a.what:
        T, patch, overlap, cols = 100, (32, 32), (24, 0), 3200
        torch.manual_seed(11)
        enc = crw_utils.create_model(1, False).cuda()
        enc.train(True)
        rg = crw_dataset.synthetic_radargram(ROWS, cols)
        seg = (torch.arange(ROWS)[:, None] * K // ROWS).float().repeat(1, cols)
        lp = LabelPropVOS_CRW(dict(CXT_SIZE=80, RADIUS=30, TEMP=0.1, KNN=20))
        fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap)
        run = lambda **kw: crw_inference.segment(fresh(), seg, enc, lp, K, T, patch, overlap, use_last=True, dataset_id=3, device="cuda", **kw)
        plain, conf = (lambda: run()), (lambda: run(confidence="maxprob"))
        assert torch.equal(plain()["pred"], conf()["pred"])
        tp, tc = alternate(plain, conf, a.rounds)
        emit(a.out, what="segment", shape=[ROWS, cols], T=T, N=48, plain_ms=tp, confidence_ms=tc, plain_median_ms=med(tp),
             confidence_median_ms=med(tc), confidence_over_plain=med(tc) / med(tp), spread_plain=spread(tp), spread_confidence=spread(tc))


if __name__ == "__main__":
    main()
