"""Times of the joint ordered label map (csrc/labelmap_dense.hip, crw_labelmap_ordered_joint): what does the order-preserving
merge of the reverse pass cost against the merge it replaces?

  kernel   three arms at T = 256, N = 48, M = 4 and 6 (order = all classes), 410 x 8192 pixels, int8 labels, 'maxprob', through
           the C entry points, outputs and workspace allocated once (the forward map and its confidence, which both routes need
           anyway, are written before the clock starts):
             joint      one crw_labelmap_ordered_joint over the forward and the mirrored reverse soft labels
             replaced   what it replaces: crw_labelmap_ordered with confidence on the reverse soft labels (the reverse map), then
                        crw_merge_confidence of the forward and the reverse maps
             ordered    crw_labelmap_ordered with confidence alone, for scale
  segment  inference.segment(..., decode='ordered', merge='ordered') against merge='confidence' on one 410 x 8192 synthetic
           radargram (tools/ordered_timing.py's case: [T, N] = [256, 48], random-init Resnet in train mode, forward + reverse pass,
           confidence='maxprob')

tools/ordered_timing.py's protocol: arms alternate (A B C A B C ...) after a warm-up of each, device events around REPS calls that
end in a synchronise; every round's time and the spread of each arm are on the line.

usage: python tools/joint_timing.py [kernel segment] [--out FILE] [--rounds N]
One JSON line per result, appended to FILE (default profiles/joint_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
import dataset as crw_dataset
import inference as crw_inference
import utils as crw_utils
from confidence_timing import alternate, emit, med, spread, timed
from imported.labelprop import LabelPropVOS_CRW

T, N, ROWS, COLS, REPS = 256, 48, 410, 8192, 20


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", nargs="*", default=["kernel", "segment"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    a = p.parse_args()
    torch.manual_seed(5)
    lib = crw_hip.lib()
    assert crw_hip.has_joint()
    stream, ptr = crw_hip._stream(), crw_hip._ptr
    if "kernel" in a.what:
        kind = crw_hip._conf_kind("maxprob")
        for M in (4, 6):
            Lf, Lr = (torch.distributions.Dirichlet(torch.ones(M)).sample((T * N,)).float().cuda() for _ in range(2))
            corder = (ctypes.c_int * M)(*range(M))
            ws = torch.empty(lib.crw_labelmap_ordered_workspace(1, ROWS, COLS), dtype=torch.uint8, device="cuda")
            new = lambda dt: torch.empty(ROWS, COLS, dtype=dt, device="cuda")
            flab, fconf, rlab, rconf, mlab, mconf, jlab, jconf = (new(dt) for dt in (torch.int8, torch.float32) * 4)

            def ordered(L=Lr, flip=1, lab=rlab, conf=rconf, reps=REPS):
                for _ in range(reps):
                    st = lib.crw_labelmap_ordered(ptr(L), T, N, M, ROWS, COLS, flip, corder, M, kind, ptr(lab), crw_hip.DT_I8, ptr(conf), COLS,
                                                  ptr(ws), ws.numel(), stream)
                    assert st == 0, st

            def replaced():
                for _ in range(REPS):
                    st = lib.crw_labelmap_ordered(ptr(Lr), T, N, M, ROWS, COLS, 1, corder, M, kind, ptr(rlab), crw_hip.DT_I8, ptr(rconf), COLS,
                                                  ptr(ws), ws.numel(), stream)
                    assert st == 0, st
                    st = lib.crw_merge_confidence(ptr(flab), ptr(fconf), ptr(rlab), ptr(rconf), crw_hip.DT_I8, ROWS * COLS, ptr(mlab),
                                                  ptr(mconf), None, stream)
                    assert st == 0, st

            def joint():
                for _ in range(REPS):
                    st = lib.crw_labelmap_ordered_joint(ptr(Lf), T, COLS, 0, 0, ptr(Lr), T, COLS, 0, 1, N, M, ROWS, COLS, corder, M, kind,
                                                        ptr(jlab), crw_hip.DT_I8, ptr(jconf), COLS, ptr(ws), ws.numel(), stream)
                    assert st == 0, st

            ordered(Lf, 0, flab, fconf, 1)  # the forward map: both routes have it before the merge
            replaced(), joint(), ordered()
            torch.cuda.synchronize()
            assert torch.equal(jconf, mconf) and (jlab[1:] >= jlab[:-1]).all()
            back = int((mlab[1:] < mlab[:-1]).any(0).sum())
            arms = dict(joint=joint, replaced=replaced, ordered=ordered)
            times = {n: [] for n in arms}
            for _ in range(a.rounds):
                for n, fn in arms.items():
                    times[n].append(timed(fn))
            per_call = {n: 1e3 * med(t) / REPS for n, t in times.items()}
            emit(a.out, what="kernel", T=T, N=N, M=M, S=M, shape=[ROWS, COLS], labels="int8", confidence="maxprob", calls_per_round=REPS,
                 merged_columns_that_step_back=back, joint_differs_share=float((jlab != mlab).float().mean()),
                 **{n + "_ms": t for n, t in times.items()}, **{n + "_us_per_call": v for n, v in per_call.items()},
                 joint_over_replaced=per_call["joint"] / per_call["replaced"], joint_over_ordered=per_call["joint"] / per_call["ordered"],
                 joint_us_per_row=per_call["joint"] / ROWS, waves=(COLS + 63) // 64, **{"spread_" + n: spread(t) for n, t in times.items()})
    if "segment" in a.what:
        K, patch, overlap = 5, (32, 32), (24, 0)
        torch.manual_seed(11)
        enc = crw_utils.create_model(1, False).cuda()
        enc.train(True)
        rg = crw_dataset.synthetic_radargram(ROWS, COLS)
        seg = (torch.arange(ROWS)[:, None] * K // ROWS).float().repeat(1, COLS)
        lp = LabelPropVOS_CRW(dict(CXT_SIZE=80, RADIUS=30, TEMP=0.1, KNN=20))
        fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap)
        run = lambda merge: crw_inference.segment(fresh(), seg, enc, lp, K, T, patch, overlap, use_last=True, dataset_id=3, device="cuda",
                                                  confidence="maxprob", upsample="bilinear", decode="ordered", order=list(range(K)),
                                                  merge=merge)
        by_conf, by_order = (lambda: run("confidence")), (lambda: run("ordered"))
        assert by_conf()["pred"].shape == by_order()["pred"].shape == (ROWS, COLS)
        tc, to = alternate(by_conf, by_order, a.rounds)
        emit(a.out, what="segment", shape=[ROWS, COLS], T=T, N=N, merge_confidence_ms=tc, merge_ordered_ms=to,
             merge_confidence_median_ms=med(tc), merge_ordered_median_ms=med(to), ordered_over_confidence=med(to) / med(tc),
             spread_merge_confidence=spread(tc), spread_merge_ordered=spread(to))


if __name__ == "__main__":
    main()
