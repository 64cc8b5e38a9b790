"""What the memory bank costs in the parameter sweep: crw_labelprop_propagate_long_batch (include/crw_hip_sweepmem.h) against the
loop of one-configuration calls it replaces, at tools/sliding_timing.py's geometries (cfg5 [T, N, M] = [256, 48, 4] and an mc1-like
item [100, 48, 4], CXT_SIZE 80, KNN 20, RADIUS 10, C 128), G = 60 configurations, n_long = 5 (first_frame 5), by
tools/longmem_timing.py's protocol:

  a         ONE crw_labelprop_propagate_long_batch launch over the G configurations
  b         the loop of G crw_labelprop_propagate_long calls (route 0) on the same lists, slice by slice: the thing to beat
  c / c0    crw_labelprop_propagate_sliding_batch (seeded, G configurations) on this build / on the library given by --parent_lib
            (built from the parent commit, loaded by path beside this build's).  Left out when no such library is given

a and b write the same bits, asserted before the rounds (c and c0 likewise).  The G configurations are one selection's lists under G
different temperatures of the softmax, so no two slices are equal.  Buffers allocated once, 20 calls per round between two device
events, seven rounds alternating the arms after a warm-up of each; every round is on the log line.
--segment: `inference.segment_sweep(bank=4 traces)` on --synthetic 410 3200 with the CNN and a 60-point grid of two biases against
the same configurations as a loop of `segment(memory=, memory_bias=)`, alternating, wall clock around a synchronised call.

usage: python tools/sweep_longmem_timing.py [--parent_lib FILE] [--segment] [--out FILE]
One JSON line per geometry, appended to FILE (default profiles/sweep_longmem_timing.log) and printed."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from sliding_timing import C, GEOM, RADIUS, ROUNDS, alternate, checked, emit, stats

G, K = 60, 5


def run(out, parent_lib):
    lib = crw_hip.lib()
    parent = None
    if parent_lib:
        handle = ctypes.CDLL(parent_lib)
        handle.crw_abi_version.restype = ctypes.c_int
        assert handle.crw_abi_version() == crw_hip.ABI_VERSION
        parent = handle.crw_labelprop_propagate_sliding_batch
        parent.restype, parent.argtypes = crw_hip.SIGNATURES["crw_labelprop_propagate_sliding_batch"]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    for name, g in GEOM.items():
        T, N, M, cxt, knn = g["T"], g["N"], g["M"], g["cxt"], g["knn"]
        gen = torch.Generator().manual_seed(1)
        feats = crw_hip.normalize((torch.randn(1, N, C, generator=gen) + 0.5 * torch.randn(T, N, C, generator=gen)).float().cuda())
        seed = (torch.arange(N) * M // N).float().cuda()
        front = (torch.arange(K * N, device="cuda") % N * M // N)
        # G configurations: one selection at n_long = K, the softmax at G temperatures
        V, I = crw_hip.labelprop_topk_scores(feats, cxt, RADIUS, 1.0, knn, first_frame=K, n_long=K, route="auto")
        W = torch.stack([torch.softmax(V * (10.0 + i), 1) for i in range(G)]).contiguous()
        F = T - K
        labels = lambda: (torch.empty(G, T * N, M, device="cuda"), torch.empty(G, N, T, device="cuda"))
        (La, qa), (Lb, qb) = labels(), labels()
        for L, q in ((La, qa), (Lb, qb)):
            L[:, :K * N] = (front[:, None] == torch.arange(M, device="cuda")).float()
            q[:, :, :K] = front.view(K, N).t().float()

        def arm_a():
            checked(lib.crw_labelprop_propagate_long_batch(p(W), p(I), 0, G, T, N, M, knn, K, cxt, K, p(La), p(qa), None), "long_batch")

        def arm_b():
            for i in range(G):
                checked(lib.crw_labelprop_propagate_long(p(W[i]), p(I), T, N, M, knn, K, cxt, K, p(Lb[i]), p(qb[i]), 0, None), "propagate_long")

        routes = {}
        for k, fn in (("a", arm_a), ("b", arm_b)):
            with crw_hip.routes() as hit:
                fn()
            routes[k] = sorted(hit)
        torch.cuda.synchronize()
        assert bits(La, Lb) and torch.equal(qa, qb), "a and b differ"
        arms = dict(a=arm_a, b=arm_b)
        # the sliding batch, this build against the parent's: the lists of the plain rule at the same G temperatures
        V1, I1 = crw_hip.labelprop_topk_scores(feats, cxt, RADIUS, 1.0, knn)
        W1 = torch.stack([torch.softmax(V1 * (10.0 + i), 1) for i in range(G)]).contiguous()
        (Lc, qc), (Lc0, qc0) = labels(), labels()
        slide = lambda fn, L, q: checked(fn(p(seed), p(W1), p(I1), 0, G, T, N, M, knn, 1, cxt, p(L), p(q), None), "sliding_batch")
        arms["c"] = lambda: slide(lib.crw_labelprop_propagate_sliding_batch, Lc, qc)
        arms["c"]()
        if parent is not None:
            arms["c0"] = lambda: slide(parent, Lc0, qc0)
            arms["c0"]()
            torch.cuda.synchronize()
            assert bits(Lc, Lc0) and torch.equal(qc, qc0), "c and c0 differ"
        res = alternate(arms)
        med = lambda k: stats(res[k])["median"]
        extra = dict(b_over_a=med("b") / med("a"), a_over_c=med("a") / med("c"), any_a_round_slower_than_any_b_round=bool(max(res["a"]) > min(res["b"])),
                     a_us_per_frame=med("a") / F, c_us_per_frame=med("c") / (T - 1))
        if parent is not None:
            s0 = stats(res["c0"])
            extra.update(c_median_within_parent_rounds=bool(s0["min"] <= med("c") <= s0["max"]), c_over_parent=med("c") / s0["median"])
        emit(out, what="long memory in the sweep", geom=name, unit="us per call", **g, G=G, n_long=K, radius=RADIUS, C=C, parent_lib=bool(parent),
             routes=routes, rounds=res, **{k + "_stats": stats(v) for k, v in res.items()}, a_b_bitwise_equal=True, **extra)


def segment(out, rounds=3):
    """`segment_sweep(bank=4 traces)` against the loop of `segment(memory=, memory_bias=)` on --synthetic 410 3200 (segment_all.py's
    defaults, the CNN, CONTEXT sliding): 5 radii x 3 temps x 2 biases x 2 knns = 60 configurations"""
    import inference
    import utils
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    sys.path.insert(0, os.path.join(ROOT, "radar-sounder-crw_amd", "scripts"))
    import segment_all
    args = segment_all.with_defaults(segment_all.get_args_parser().parse_args(["--synthetic", "410", "3200", "--context", "sliding"]))
    torch.manual_seed(11)
    enc = utils.create_model(args.model, args.pos_embed).cuda()
    dataset, nclasses, seg, _ = segment_all.load_data(args)
    sweep = LabelPropSweep(args.cxt_size, [6, 8, 10, 12, 14], [0.1, 0.05, 0.01], [10, 20], context="sliding", biases=[0.0, 0.1])
    assert len(sweep) == 60
    T, (W, ow) = args.seq_length, (args.patch_size[1], args.overlap[1])
    rg_len = T * (W - ow) + ow
    bank = utils.bank_from_columns(dataset, seg.cpu(), [0, rg_len // 3, 2 * rg_len // 3, rg_len - W])
    kw = dict(dataset_id=args.dataset)

    def one_pass():
        return inference.segment_sweep(dataset, seg, enc, sweep, nclasses, T, args.patch_size, args.overlap, bank=bank, **kw)

    def loop():
        return [inference.segment(dataset, seg, enc, LabelPropVOS_CRW(cfg), nclasses, T, args.patch_size, args.overlap, memory=bank,
                                  memory_bias=cfg["MEMORY_BIAS"], **kw) for cfg in sweep.configs]
    arms = dict(sweep=one_pass, loop=loop)
    a, b = one_pass(), loop()
    assert all(torch.equal(a["pred"][i].to(b[i]["pred"].dtype), b[i]["pred"]) for i in range(60)), "the sweep and the loop differ"
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[k].append(round((time.perf_counter() - t0) * 1e3, 2))
    emit(out, what="segment_sweep with a bank of 4 traces against the loop of segment", synthetic=[410, 3200], unit="ms per call", G=60,
         seq_length=T, patch_size=list(args.patch_size), cxt=args.cxt_size, radargrams=seg.shape[-1] // rg_len, rounds=res, maps_equal=True,
         **{k + "_stats": stats(v) for k, v in res.items()}, loop_over_sweep=stats(res["loop"])["median"] / stats(res["sweep"])["median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_longmem_timing.log"))
    ap.add_argument("--parent_lib", default=None, help="a libcrw_hip.so built from the parent commit (arm c0)")
    ap.add_argument("--segment", action="store_true", help="also time segment_sweep(bank=) against the loop of segment(memory=)")
    a = ap.parse_args()
    run(a.out, a.parent_lib)
    if a.segment:
        segment(a.out)


if __name__ == "__main__":
    main()
