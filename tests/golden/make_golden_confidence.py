#!/usr/bin/env python3
"""Fixtures of the soft labels: what the reference's ``LabelPropVOS_CRW.predict`` returns before ``src/utils.py:160`` arg-maxes
it away -> ``confidence_<name>.npz`` for each of the four ``labelprop_<name>.npz`` fixtures.

For every source fixture its inputs are read back (``emb``, ``seg_ref``, the CXT_SIZE / RADIUS / TEMP / KNN it was made with,
``use_last``) and the reference's own ``predict`` is driven frame by frame the way ``src/utils.py:107-160`` drives it: the item
flipped for ``use_last``, ``normalize(emb, dim=-1)``, the seed labels a NEAREST resize of ``seg_ref`` to (N, 1), features as
[1, C, N, 1], the one-hot seed mask first.  The encoder of the source fixtures is the identity on the patch pixels
(make_golden.PatchFlatten), so ``emb`` IS the encoder output.  Recorded:
  L ....... [T, N, M] float32: frame 0 the one-hot seed, frame n the mask ``predict`` returned for it
The generator asserts that the arg-max of what it records is the source fixture's ``pred``, label for label, and prints the
largest deviation of the recorded masks from their fp64 restatement (the chain of oracle.labelprop_weights with
dtype=np.float64 -- the yardstick tests/test_confidence_gpu.py scales its tolerance by).

Plumbing as in make_golden.py (its helpers are imported, nothing of the reference is edited or stored): runs only where the
reference is (CRW_REFERENCE, as make_golden.py reads it).

Usage:  python tests/golden/make_golden_confidence.py        (rewrites confidence_*.npz)
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch
import torch.nn.functional as TF

import make_golden as mg

CASES = ["labelprop_trunc_T14N10", "labelprop_full_T40N48", "labelprop_last_T20N24", "labelprop_mc1_T100N12"]


def soft_labels_fp64(emb, seed, M, cxt_size, radius, temp, knn):
    """oracle.labelprop's loop in float64 -> L [T, N, M] (same index quirk: lists of the truncated keys on the untruncated labels)."""
    from oracle import crw_oracle as orc
    T, N, C = emb.shape
    ehat = orc.l2_normalize(emb.astype(np.float64), np.float64)
    L = np.zeros((T * N, M), np.float64)
    L[:N] = seed[:, None] == np.arange(M)[None, :]
    for n in range(1, T):
        W, I = orc.labelprop_weights(ehat, n, cxt_size, radius, temp, knn, dtype=np.float64)
        L[n * N:(n + 1) * N] = (L[I] * W[..., None]).sum(0)
    return L.reshape(T, N, M)


def run_case(ref_lp, name):
    g = dict(np.load(os.path.join(HERE, name + ".npz")))
    emb = torch.tensor(g["emb"])
    T, N, C = emb.shape
    M = int(g["nclasses"])
    cfg = dict(CXT_SIZE=int(g["cxt_size"]), RADIUS=int(g["radius"]), TEMP=float(g["temp"]), KNN=int(g["knn"]))
    if bool(g["use_last"]):
        emb = torch.flip(emb, (0,))
    ehat = TF.normalize(emb, dim=-1)
    label = TF.interpolate(torch.tensor(g["seg_ref"])[None, None].float(), size=(N, 1), mode="nearest")[0, 0, :, 0]
    lp = ref_lp.LabelPropVOS_CRW(cfg)
    as_feat = lambda n: ehat[n].t().reshape(1, C, N, 1)
    mask = (label[None, :] == torch.arange(M)[:, None]).float().reshape(1, M, N, 1)
    feats, masks = [as_feat(0)], [mask]
    with mg.cuda_is_cpu():
        for n in range(1, T):
            mask = lp.predict(feats=feats, masks=masks, curr_feat=as_feat(n))
            feats.append(as_feat(n))
            masks.append(mask)
    L = torch.cat(masks, 0)[..., 0].permute(0, 2, 1).contiguous().float().numpy()  # [T, N, M]
    pred = L.argmax(-1).T.astype(np.float32)
    assert np.array_equal(pred, g["pred"]), f"{name}: the recorded masks' arg-max differs from the fixture's pred"
    L64 = soft_labels_fp64(emb.numpy(), label.numpy(), M, cfg["CXT_SIZE"], cfg["RADIUS"], cfg["TEMP"], cfg["KNN"])
    assert np.array_equal(L64.argmax(-1).T, g["pred"]), f"{name}: the fp64 restatement's arg-max differs from the fixture's pred"
    top = np.sort(L64, -1)
    out = "confidence_" + name[len("labelprop_"):]
    np.savez(os.path.join(HERE, out + ".npz"), L=L)
    print(f"{out}: L{L.shape} row sums within {np.abs(L.sum(-1) - 1).max():.1e}, deviation from the fp64 restatement "
          f"{np.abs(L - L64).max():.2e}, smallest top-two margin {float((top[..., -1] - top[..., -2]).min()):.2e}")


def main():
    _, _, _, _, ref_lp = mg.import_reference()
    for name in CASES:
        run_case(ref_lp, name)


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
