"""Times of the dense label map (csrc/labelmap_dense.hip):

  kernel   crw_hip.labelmap_dense against the PyTorch-ROCm composite on the device (permute -> F.interpolate(bilinear) -> argmax,
           plus max for the confidence; it materialises the interpolated probabilities [M, rows, cols]) at T = 256, N = 48,
           M = 4 and 6, 410 x 8192 pixels, int8 and fp32 labels, with and without the 'maxprob' confidence; a round is REPS calls
  segment  inference.segment(..., upsample='bilinear') against upsample='nearest' -- what the parent commit does -- on one
           410 x 8192 synthetic radargram (32 x 32 patches, overlap (24, 0): [T, N] = [256, 48], random-init Resnet in train
           mode), forward + reverse pass, confidence='maxprob'

Arms alternate (A B A B ...) after a warm-up of each, device events around work that ends in a synchronise; every round's time
and the spread of each arm are on the line, and `kernel_slowest_under_composite_fastest` is the sweep table's condition.

usage: python tools/dense_timing.py [kernel segment] [--out FILE] [--rounds N]
One JSON line per result, appended to FILE (default profiles/dense_timing.log) and printed."""
import argparse
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
from confidence_timing import alternate, emit, med, spread
from imported.labelprop import LabelPropVOS_CRW

T, N, ROWS, COLS, REPS = 256, 48, 410, 8192, 20


def composite(L, M, dtype, want_conf):
    p = TF.interpolate(L.view(T, N, M).permute(2, 1, 0)[None], size=(ROWS, COLS), mode="bilinear", align_corners=False)[0]
    return p.argmax(0).to(dtype), (p.max(0).values if want_conf else None)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", nargs="*", default=["kernel", "segment"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_timing.log"))
    p.add_argument("--rounds", type=int, default=7)
    a = p.parse_args()
    torch.manual_seed(5)
    if "kernel" in a.what:
        for M in (4, 6):
            L = torch.distributions.Dirichlet(torch.ones(M)).sample((T * N,)).float().cuda()
            for dtype in (torch.int8, torch.float32):
                for want_conf in (False, True):
                    kind = "maxprob" if want_conf else None
                    out = torch.empty(ROWS, COLS, dtype=dtype, device="cuda")
                    outc = torch.empty(ROWS, COLS, device="cuda") if want_conf else None
                    kernel = lambda: [crw_hip.labelmap_dense(L, T, N, M, ROWS, COLS, confidence=kind, dtype=dtype, out=out, out_conf=outc)
                                      for _ in range(REPS)]
                    ops = lambda: [composite(L, M, dtype, want_conf) for _ in range(REPS)]
                    (kl, kc), (tl, tc) = kernel()[0], ops()[0]  # the two arms draw the same map, up to the composite's float scale
                    differ = float((kl != tl).float().mean())
                    assert differ <= 1e-3 and (kc is None or float((kc - tc).abs().max()) <= 1e-5), differ
                    tk, tt = alternate(kernel, ops, a.rounds)
                    written = ROWS * COLS * ((1 if dtype == torch.int8 else 4) + (4 if want_conf else 0))
                    emit(a.out, what="kernel", T=T, N=N, M=M, shape=[ROWS, COLS], labels=str(dtype).replace("torch.", ""),
                         confidence=kind, calls_per_round=REPS, labels_differ_share=differ, kernel_ms=tk, composite_ms=tt,
                         kernel_us_per_call=1e3 * med(tk) / REPS, composite_us_per_call=1e3 * med(tt) / REPS,
                         composite_over_kernel=med(tt) / med(tk), kernel_store_GBps=written * REPS / med(tk) / 1e6,
                         kernel_slowest_under_composite_fastest=max(tk) < min(tt), spread_kernel=spread(tk), spread_composite=spread(tt))
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
                                                 confidence="maxprob", **kw)
        near, dense = (lambda: run(upsample="nearest")), (lambda: run(upsample="bilinear"))
        assert near()["pred"].shape == dense()["pred"].shape == (ROWS, COLS)
        tn, td = alternate(near, dense, a.rounds)
        emit(a.out, what="segment", shape=[ROWS, COLS], T=T, N=N, nearest_ms=tn, bilinear_ms=td, nearest_median_ms=med(tn),
             bilinear_median_ms=med(td), bilinear_over_nearest=med(td) / med(tn), spread_nearest=spread(tn), spread_bilinear=spread(td))


if __name__ == "__main__":
    main()
