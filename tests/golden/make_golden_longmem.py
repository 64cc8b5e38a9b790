#!/usr/bin/env python3
"""Fixtures of the sliding rule with K long-term frames (include/crw_hip_longmem.h) -> ``longmem_<name>.npz``.

The reference's own ``LabelPropVOS_CRW.predict`` computes that rule when it is handed the lists the rule names: for frame n,
``feats[:K] + feats[max(K, n - cxt):n]`` and the masks likewise, by an object whose CXT_SIZE is K - 1 + cxt -- the lists then never
hold more than CXT_SIZE + 1 frames, its truncation branch (src/imported/maskedatt.py:165-166) never triggers, and the indices it
returns address the list they were scored on.  It is driven frame by frame as in make_golden_sliding.py (the item flipped for
``use_last``, ``normalize(emb, dim=-1)``, features as [1, C, N, 1]); the frames before first_frame carry the one-hot rows of their
true classes.  Recorded:
  emb (as propagated: flipped already), cls_front [first_frame, N], M, cxt, K, radius, temp, knn, first_frame ... the inputs
  pred [N, F] .......... arg-max of the masks (the frames in front: their classes)
  L [F * N, M] ......... the frames in front one-hot, frame n the mask ``predict`` returned for it
  deviation ............ largest |L - L64|, L64 the fp64 restatement (tests/longmem_ref.labelprop_long, dtype=np.float64)
The generator asserts that the fp64 restatement's arg-max equals the recorded pred; an item's seed is the first for which the
smallest top-two margin of the fp64 soft labels and the smallest gap between the knn-th selected score and the best one left out
(fp64 logits) both exceed 1e-4, so that exact label equality is a fair demand of an fp32 implementation.

Plumbing as in make_golden_sliding.py (make_golden's helpers are imported, nothing of the reference is edited or stored): runs only
where the reference is (CRW_REFERENCE, as make_golden.py reads it).

Usage:  python tests/golden/make_golden_longmem.py        (rewrites longmem_*.npz)
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch
import torch.nn.functional as TF

import make_golden as mg
import longmem_ref as lm
import sliding_ref as sr
from oracle import crw_oracle as orc

# name: (T, N, C, M, cxt, radius, temp, knn, amp, use_last, K, first_frame); the items are tests/sliding_ref.drifting_item
CASES = {
    "T14N10K2": (14, 10, 8, 3, 4, 3, 0.1, 4, 3, False, 2, 2),
    "T30N13K3": (30, 13, 8, 3, 4, 3, 0.1, 4, 5, False, 3, 3),    # the ring wraps twice
    "T20N24K4": (20, 24, 16, 3, 6, 4, 0.05, 5, 6, True, 4, 4),
    "T12N10K5": (12, 10, 8, 3, 1, 3, 0.1, 3, 3, False, 5, 5),    # more long-term frames than the window has
    "T14N10K3F2": (14, 10, 8, 3, 4, 3, 0.1, 4, 3, False, 3, 2),  # the last long-term frame is predicted: no seed of its own
}
MARGIN = 1e-4


def boundary_gap(emb, cxt, K, radius, temp, knn, first_frame):
    """Smallest (knn-th selected logit - best logit left out) over every frame and query, fp64, on the rule's key list."""
    T, N, _ = emb.shape
    ehat = orc.l2_normalize(emb.astype(np.float64), np.float64)
    gap = np.inf
    for n in range(first_frame, T):
        S = np.concatenate([ehat[f] @ ehat[n].T + orc.band_bias(N, radius, np.float64) for f in lm.key_frames(n, K, cxt)], 0) / temp
        S = -np.sort(-S, axis=0)
        if S.shape[0] > knn:
            real = S[knn - 1] > orc.MASK_NEG / 2 / temp
            gap = min(gap, float((S[knn - 1] - S[knn])[real].min()) if real.any() else np.inf)
    return gap


def run_case(ref_lp, name, T, N, C, M, cxt, radius, temp, knn, amp, use_last, K, first, seed):
    emb_np, cls = sr.drifting_item(seed, T, N, C, M, amp)
    if use_last:
        emb_np, cls = emb_np[::-1].copy(), cls[::-1].copy()
    ehat = TF.normalize(torch.tensor(emb_np), dim=-1)
    lp = ref_lp.LabelPropVOS_CRW(dict(CXT_SIZE=K - 1 + cxt, RADIUS=radius, TEMP=temp, KNN=knn))
    as_feat = lambda n: ehat[n].t().reshape(1, C, N, 1)
    onehot = lambda c: (torch.tensor(c)[None, :] == torch.arange(M)[:, None]).float().reshape(1, M, N, 1)
    feats, masks = [as_feat(f) for f in range(first)], [onehot(cls[f]) for f in range(first)]
    with mg.cuda_is_cpu():
        for n in range(first, T):
            lo = max(K, n - cxt)
            mask = lp.predict(feats=feats[:K] + feats[lo:n], masks=masks[:K] + masks[lo:n], curr_feat=as_feat(n))
            feats.append(as_feat(n))
            masks.append(mask)
    L = torch.cat(masks, 0)[..., 0].permute(0, 2, 1).contiguous().float().numpy()  # [T, N, M]
    pred = L.argmax(-1).T.astype(np.float32)
    p64, L64, _, _ = lm.labelprop_long(emb_np, cls[:first], M, cxt, K, radius, temp, knn, first, np.float64)
    L64 = L64.reshape(T, N, M)
    if not np.array_equal(p64, pred):
        return None
    top = np.sort(L64[first:], -1)
    margin, gap = float((top[..., -1] - top[..., -2]).min()), boundary_gap(emb_np, cxt, K, radius, temp, knn, first)
    if not (margin > MARGIN and gap > MARGIN):
        return None
    dev = float(np.abs(L - L64).max())
    np.savez(os.path.join(HERE, f"longmem_{name}.npz"), emb=emb_np, cls_front=cls[:first].astype(np.int32), M=np.int32(M), cxt=np.int32(cxt),
             K=np.int32(K), radius=np.int32(radius), temp=np.float32(temp), knn=np.int32(knn), first_frame=np.int32(first),
             use_last=np.bool_(use_last), pred=pred, L=L.reshape(T * N, M), deviation=np.float32(dev))
    print(f"longmem_{name}: seed {seed}, L{L.shape}, deviation from the fp64 restatement {dev:.2e}, smallest top-two margin {margin:.2e}, "
          f"smallest top-k boundary gap {gap:.2e}")
    return dev


def main():
    _, _, _, _, ref_lp = mg.import_reference()
    for name, case in CASES.items():
        for seed in range(64):
            if run_case(ref_lp, name, *case, seed) is not None:
                break
        else:
            raise SystemExit(f"longmem_{name}: no seed in 0 .. 63 gives margins above {MARGIN}")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
