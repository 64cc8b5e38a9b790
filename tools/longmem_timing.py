"""What a bank of long-term frames costs: the entry points of include/crw_hip_longmem.h against the sliding entry points they
extend, and those on this build against a build of the parent commit -- at tools/sliding_timing.py's geometries (cfg5 [T, N, M] =
[256, 48, 4] and an mc1-like item [100, 48, 4], CXT_SIZE 80, KNN 20, RADIUS 10, C 128) and by its protocol.  Top-k (t*),
propagation (p*):

  tc / pc       crw_labelprop_topk_grid / crw_labelprop_propagate_sliding (seeded), this build
  tc0 / pc0     the same calls on the library given by --parent_lib (built from the parent commit, or a copy of this build: the
                tool's own noise), loaded by path beside this build's.  Left out when no such library is given
  tk1 / pk1     crw_labelprop_topk_long / crw_labelprop_propagate_long at n_long = 1, first_frame = 1 (frame 0's rows are in L)
  tk5 / pk5     at n_long = 5, first_frame = 5: the item's first five frames are the bank, four fewer frames are computed
  tk9 / pk9     at n_long = 9, first_frame = 9

c, c0 and k1 write the same bits (lists, L and pred of the frames >= 1), asserted before the rounds.  Buffers allocated once, 20
calls per round between two device events, seven rounds alternating the arms after a warm-up of each; every round is on the log
line.  --segment: `inference.segment()` against `segment(memory=4 traces)` on --synthetic 410 8192 with the CNN, alternating, wall
clock around a synchronised call, seven rounds.

usage: python tools/longmem_timing.py [--parent_lib FILE] [--segment] [--out FILE]
One JSON line per geometry, appended to FILE (default profiles/longmem_timing.log) and printed."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from restart_timing import parent_entries
from sliding_timing import C, GEOM, RADIUS, ROUNDS, TEMP, alternate, checked, emit, stats

BANKS = (1, 5, 9)


def run(out, parent_lib):
    lib = crw_hip.lib()
    parent = parent_entries(parent_lib) if parent_lib else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    for name, g in GEOM.items():
        T, N, M, cxt, knn = g["T"], g["N"], g["M"], g["cxt"], g["knn"]
        gen = torch.Generator().manual_seed(1)
        feats = crw_hip.normalize((torch.randn(1, N, C, generator=gen) + 0.5 * torch.randn(T, N, C, generator=gen)).float().cuda())
        seed = (torch.arange(N) * M // N).float().cuda()
        lists = lambda ff=1: (torch.empty(T - ff, knn, N, device="cuda"), torch.empty(T - ff, knn, N, device="cuda", dtype=torch.int32))
        labels = lambda: (torch.empty(T * N, M, device="cuda"), torch.empty(N, T, device="cuda"))
        (Wc, Ic), (Wc0, Ic0), (Lc, qc), (Lc0, qc0) = lists(), lists(), labels(), labels()
        topk = lambda fn, W, I: checked(fn(p(feats), T, N, C, cxt, RADIUS, TEMP, knn, 1, 1, p(W), p(I), None), "topk_grid")
        slide = lambda fn, W, I, L, q: checked(fn(p(seed), p(W), p(I), T, N, M, knn, 1, cxt, p(L), p(q), None), "sliding")
        arms = dict(tc=lambda: topk(lib.crw_labelprop_topk_grid, Wc, Ic), pc=lambda: slide(lib.crw_labelprop_propagate_sliding, Wc, Ic, Lc, qc))
        arms["tc"](), arms["pc"]()
        torch.cuda.synchronize()
        if parent is not None:
            arms["tc0"] = lambda: topk(parent[0], Wc0, Ic0)
            arms["pc0"] = lambda: slide(parent[1], Wc, Ic, Lc0, qc0)
            arms["tc0"](), arms["pc0"]()
            torch.cuda.synchronize()
            assert bits(Wc, Wc0) and torch.equal(Ic, Ic0) and bits(Lc, Lc0) and torch.equal(qc, qc0), "c and c0 differ"
        routes = {}
        for K in BANKS:
            (W, I), (L, q) = lists(K), labels()
            L[:K * N], q[:, :K] = Lc[:K * N], qc[:, :K]  # the frames in front: (c)'s own labels, so that K = 1 is (c)'s call

            def arm_t(K=K, W=W, I=I):
                checked(lib.crw_labelprop_topk_long(p(feats), T, N, C, cxt, K, RADIUS, TEMP, knn, K, p(W), p(I), 0, 0, None), "topk_long")

            def arm_p(K=K, W=W, I=I, L=L, q=q):
                checked(lib.crw_labelprop_propagate_long(p(W), p(I), T, N, M, knn, K, cxt, K, p(L), p(q), 0, None), "propagate_long")

            with crw_hip.routes() as hit:
                arm_t(), arm_p()
            torch.cuda.synchronize()
            routes[f"k{K}"] = sorted(hit)
            if K == 1:
                assert bits(W, Wc) and torch.equal(I, Ic) and bits(L, Lc) and torch.equal(q, qc), "k1 and c differ"
            arms[f"tk{K}"], arms[f"pk{K}"] = arm_t, arm_p
        res = alternate(arms)
        med = lambda k: stats(res[k])["median"]
        extra = {}
        for k in ("tc", "pc"):
            s = stats(res[k])
            extra[f"{k[0]}k1_median_within_{k}_rounds"] = bool(s["min"] <= med(k[0] + "k1") <= s["max"])
            extra[f"{k[0]}k1_over_{k}"] = med(k[0] + "k1") / s["median"]
            if parent is not None:
                s0 = stats(res[k + "0"])
                extra[k + "_median_within_parent_rounds"] = bool(s0["min"] <= med(k) <= s0["max"])
                extra[k + "_over_parent"] = med(k) / s0["median"]
        for K in BANKS[1:]:
            extra[f"tk{K}_over_tc"], extra[f"pk{K}_over_pc"] = med(f"tk{K}") / med("tc"), med(f"pk{K}") / med("pc")
            extra[f"pk{K}_us_per_frame"], extra["pc_us_per_frame"] = med(f"pk{K}") / (T - K), med("pc") / (T - 1)
        emit(out, what="long memory", geom=name, unit="us per call", **g, radius=RADIUS, C=C, parent_lib=bool(parent), routes=routes, rounds=res,
             **{k + "_stats": stats(v) for k, v in res.items()}, c_k1_bitwise_equal=True, **extra)


def segment(out):
    """`segment()` against `segment(memory=4 traces)` on --synthetic 410 8192 (segment_all.py's defaults, the CNN, CONTEXT sliding)"""
    import inference
    import utils
    from dataset import RGDataset
    from imported.labelprop import LabelPropVOS_CRW
    sys.path.insert(0, os.path.join(ROOT, "radar-sounder-crw_amd", "scripts"))
    import segment_all
    args = segment_all.with_defaults(segment_all.get_args_parser().parse_args(["--synthetic", "410", "8192", "--context", "sliding"]))
    torch.manual_seed(11)
    enc = utils.create_model(args.model, args.pos_embed).cuda()
    dataset, nclasses, seg, _ = segment_all.load_data(args)
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=args.cxt_size, RADIUS=args.radius, TEMP=args.temp, KNN=args.knn, CONTEXT="sliding"))
    T, (W, ow) = args.seq_length, (args.patch_size[1], args.overlap[1])
    rg_len = T * (W - ow) + ow
    bank = utils.bank_from_columns(dataset, seg.cpu(), [0, rg_len // 3, 2 * rg_len // 3, rg_len - W])
    call = lambda **kw: inference.segment(dataset, seg, enc, lp, nclasses, T, args.patch_size, args.overlap, dataset_id=args.dataset, **kw)
    arms = dict(plain=lambda: call(), memory=lambda: call(memory=bank))
    res = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[k].append(round((time.perf_counter() - t0) * 1e3, 2))
    emit(out, what="segment with a bank of 4 traces", synthetic=[410, 8192], unit="ms per call", seq_length=T, patch_size=list(args.patch_size),
         cxt=args.cxt_size, knn=args.knn, radius=args.radius, radargrams=seg.shape[-1] // rg_len, rounds=res,
         **{k + "_stats": stats(v) for k, v in res.items()}, memory_over_plain=stats(res["memory"])["median"] / stats(res["plain"])["median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longmem_timing.log"))
    ap.add_argument("--parent_lib", default=None, help="a libcrw_hip.so built from the parent commit (arms tc0, pc0)")
    ap.add_argument("--segment", action="store_true", help="also time segment() against segment(memory=4 traces)")
    a = ap.parse_args()
    run(a.out, a.parent_lib)
    if a.segment:
        segment(a.out)


if __name__ == "__main__":
    main()
