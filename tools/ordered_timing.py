"""Times of the depth-ordered label map (csrc/labelmap_dense.hip, crw_labelmap_ordered): what does the order cost?

  kernel   three arms at T = 256, N = 48, M = 4 and 6 (order = all classes), 410 x 8192 pixels, int8 labels, with and without the
           'maxprob' confidence, through the C entry points, outputs and workspace allocated once:
             ordered    crw_labelmap_ordered
             ordered_back1  the same with CRW_ORDERED_BACK=1: the backward scan with one back-pointer word in flight, not 8 (the
                        A/B of the kernel's one tuning constant; the maps are the same)
             dense      crw_labelmap_dense on the same operands -- the per-pixel arg-max map, the yardstick for the price of the order
             composite  the same DP from PyTorch-ROCm ops on the device: F.interpolate(bilinear), then a loop over the rows with
                        tensors over [S, cols] (cummax, compare, add), then the backtrack loop (COMPOSITE_REPS calls per round)
  segment  inference.segment(..., upsample='bilinear', decode='ordered') against decode='argmax' on one 410 x 8192 synthetic
           radargram (tools/dense_timing.py's case: [T, N] = [256, 48], random-init Resnet in train mode, forward + reverse pass,
           confidence='maxprob')

Arms alternate (A B C A B C ...) after a warm-up of each, device events around REPS calls that end in a synchronise; every round's
time and the spread of each arm are on the line.

usage: python tools/ordered_timing.py [kernel segment] [--out FILE] [--rounds N]
One JSON line per result, appended to FILE (default profiles/ordered_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch
import torch.nn.functional as TF

import crw_hip
import dataset as crw_dataset
import inference as crw_inference
import utils as crw_utils
from confidence_timing import alternate, emit, med, spread, timed
from imported.labelprop import LabelPropVOS_CRW

T, N, ROWS, COLS, REPS, COMPOSITE_REPS = 256, 48, 410, 8192, 20, 2


def composite(L, M, order, want_conf):
    """The definition's recurrence, tie rules and backtrack from torch ops on the device -> (labels int8, conf | None)."""
    p = TF.interpolate(L.view(T, N, M).permute(2, 1, 0)[None], size=(ROWS, COLS), mode="bilinear", align_corners=False)[0]
    conf = p.max(0).values if want_conf else None
    S = len(order)
    e = p[torch.tensor(order, device=L.device)]  # [S, rows, cols]
    D = e[:, 0].clone()
    new = torch.ones(ROWS, S, COLS, dtype=torch.bool, device=L.device)
    for r in range(1, ROWS):
        best = torch.cummax(D, 0).values
        new[r, 1:] = D[1:] > best[:-1]
        D = e[:, r] + best
    idx = torch.arange(S, device=L.device)[:, None]
    state = torch.where(D == D.max(0).values, idx, S).min(0).values
    states = torch.empty(ROWS, COLS, dtype=torch.int64, device=L.device)
    for r in range(ROWS - 1, 0, -1):
        states[r] = state
        state = torch.where(new[r] & (idx <= state[None]), idx, 0).max(0).values
    states[0] = state
    return torch.tensor(order, device=L.device)[states].to(torch.int8), conf


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", nargs="*", default=["kernel", "segment"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordered_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    a = p.parse_args()
    torch.manual_seed(5)
    lib = crw_hip.lib()
    assert crw_hip.has_ordered()
    stream, ptr = crw_hip._stream(), crw_hip._ptr
    if "kernel" in a.what:
        for M in (4, 6):
            L = torch.distributions.Dirichlet(torch.ones(M)).sample((T * N,)).float().cuda()
            order = list(range(M))
            corder = (ctypes.c_int * M)(*order)
            ws = torch.empty(lib.crw_labelmap_ordered_workspace(1, ROWS, COLS), dtype=torch.uint8, device="cuda")
            for want_conf in (False, True):
                kind = crw_hip._conf_kind("maxprob") if want_conf else -1
                lab = torch.empty(ROWS, COLS, dtype=torch.int8, device="cuda")
                dlab = torch.empty(ROWS, COLS, dtype=torch.int8, device="cuda")
                conf = torch.empty(ROWS, COLS, device="cuda") if want_conf else None
                dconf = torch.empty(ROWS, COLS, device="cuda") if want_conf else None
                cp = lambda t: ptr(t) if t is not None else None

                def ordered(back=None, out=None):
                    if back:
                        os.environ["CRW_ORDERED_BACK"] = back
                    else:
                        os.environ.pop("CRW_ORDERED_BACK", None)
                    for _ in range(REPS):
                        st = lib.crw_labelmap_ordered(ptr(L), T, N, M, ROWS, COLS, 0, corder, M, kind, ptr(lab if out is None else out), crw_hip.DT_I8, cp(conf), COLS,
                                                      ptr(ws), ws.numel(), stream)
                        assert st == 0, st

                def dense():
                    for _ in range(REPS):
                        st = lib.crw_labelmap_dense(ptr(L), T, N, M, ROWS, COLS, 0, kind, ptr(dlab), crw_hip.DT_I8, cp(dconf), COLS, stream)
                        assert st == 0, st

                ops = lambda: [composite(L, M, order, want_conf) for _ in range(COMPOSITE_REPS)]
                lab1 = torch.empty_like(lab)
                ordered("1", lab1), ordered(), dense()
                assert torch.equal(lab, lab1)
                tlab, tconf = ops()[0]
                differ = float((lab != tlab).float().mean())  # the composite interpolates in its own float arithmetic
                assert differ <= 2e-2 and (lab[1:] >= lab[:-1]).all() and (conf is None or torch.equal(conf, dconf)), differ
                arms = dict(ordered=ordered, ordered_back1=lambda: ordered("1"), dense=dense, composite=ops)
                times = {n: [] for n in arms}
                for _ in range(a.rounds):
                    for n, fn in arms.items():
                        times[n].append(timed(fn))
                per_call = {n: 1e3 * med(t) / (COMPOSITE_REPS if n == "composite" else REPS) for n, t in times.items()}
                emit(a.out, what="kernel", T=T, N=N, M=M, S=M, shape=[ROWS, COLS], labels="int8", confidence="maxprob" if want_conf else None,
                     calls_per_round=dict(ordered=REPS, ordered_back1=REPS, dense=REPS, composite=COMPOSITE_REPS),
                     labels_differ_share_ordered_vs_composite=differ, argmax_differs_share=float((lab != dlab).float().mean()),
                     **{n + "_ms": t for n, t in times.items()}, **{n + "_us_per_call": v for n, v in per_call.items()},
                     ordered_over_dense=per_call["ordered"] / per_call["dense"], back1_over_ordered=per_call["ordered_back1"] / per_call["ordered"], composite_over_ordered=per_call["composite"] / per_call["ordered"],
                     ordered_us_per_row=per_call["ordered"] / ROWS, waves=(COLS + 63) // 64,
                     **{"spread_" + n: spread(t) for n, t in times.items()})
    if "segment" in a.what:
        K, patch, overlap = 5, (32, 32), (24, 0)
        torch.manual_seed(11)
        enc = crw_utils.create_model(1, False).cuda()
        enc.train(True)
        rg = crw_dataset.synthetic_radargram(ROWS, COLS)
        seg = (torch.arange(ROWS)[:, None] * K // ROWS).float().repeat(1, COLS)
        lp = LabelPropVOS_CRW(dict(CXT_SIZE=80, RADIUS=30, TEMP=0.1, KNN=20))
        fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap)
        run = lambda **kw: crw_inference.segment(fresh(), seg, enc, lp, K, T, patch, overlap, use_last=True, dataset_id=3, device="cuda",
                                                 confidence="maxprob", upsample="bilinear", **kw)
        argmax, ordered = (lambda: run()), (lambda: run(decode="ordered", order=list(range(K))))
        assert argmax()["pred"].shape == ordered()["pred"].shape == (ROWS, COLS)
        ta, to = alternate(argmax, ordered, a.rounds)
        emit(a.out, what="segment", shape=[ROWS, COLS], T=T, N=N, argmax_ms=ta, ordered_ms=to, argmax_median_ms=med(ta),
             ordered_median_ms=med(to), ordered_over_argmax=med(to) / med(ta), spread_argmax=spread(ta), spread_ordered=spread(to))


if __name__ == "__main__":
    main()
