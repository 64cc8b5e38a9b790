"""Times of label propagation under the 'sliding' context rule (crw_labelprop_propagate_sliding) against the existing kernels doing
the same job, at cfg5 ([T, N, M] = [256, 48, 4], CXT_SIZE 80, KNN 20) and an mc1-like item ([100, 48, 4], CXT_SIZE 80):

  a   crw_labelprop_propagate_sliding, default route (the one-workgroup ring kernel where it fits)
  g   the same entry point with CRW_LABELPROP_SLIDING_GENERAL=1 (the general kernels translating in the kernel)
  b   crw_labelprop_gather on lists translated beforehand (`crw_hip.sliding_rows`) -- the existing kernel, the thing to beat
  c   crw_labelprop_propagate on the same lists: the reference rule, a chain of CXT_SIZE frames and a parallel tail -- another,
      shorter problem, for context only

C entry points through ctypes, buffers allocated once, 20 calls per round between two device events, seven rounds alternating
a b c g after a warm-up of each arm; every round is on the log line.  `batch`: crw_labelprop_propagate_sliding_batch at G = 60
against 60 single calls.  `segment`: inference.segment on a synthetic 410 x 8192 radargram (32 x 32 patches, overlap (24, 0), one
item of T = 256, CXT_SIZE 80, reverse pass) with and without CONTEXT 'sliding'.

usage: python tools/sliding_timing.py kernels|batch|segment|all [--out FILE]
One JSON line per result, appended to FILE (default profiles/sliding_timing.log) and printed."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd")]
import torch

import crw_hip

GEOM = {"cfg5": dict(T=256, N=48, M=4, cxt=80, knn=20), "mc1": dict(T=100, N=48, M=4, cxt=80, knn=20)}
RADIUS, TEMP, C = 10, 0.05, 128
CALLS, ROUNDS = 20, 7


def emit(out, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def timed(fn, calls=CALLS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # us per call


def alternate(arms, rounds=ROUNDS, calls=CALLS):
    for fn in arms.values():
        timed(fn, 3)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(round(timed(fn, calls), 2))
    return res


def stats(v):
    s = sorted(v)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def lists(g, G=1):
    T, N = g["T"], g["N"]
    gen = torch.Generator().manual_seed(1)
    feats = crw_hip.normalize((torch.randn(1, N, C, generator=gen) + 0.5 * torch.randn(T, N, C, generator=gen)).float().cuda())
    W, I = crw_hip.labelprop_topk(feats, g["cxt"], RADIUS, TEMP, g["knn"])
    return W, I, crw_hip.sliding_rows(I, N, g["cxt"]), (torch.arange(N) * g["M"] // N).float().cuda()


def checked(rc, what):
    if rc != crw_hip.CRW_OK:
        raise RuntimeError(f"{what}: status {rc}")


def kernels(out):
    lib = crw_hip.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for name, g in GEOM.items():
        T, N, M, cxt, knn = g["T"], g["N"], g["M"], g["cxt"], g["knn"]
        W, I, R, seed = lists(g)
        L, pred = torch.empty(T * N, M, device="cuda"), torch.empty(N, T, device="cuda")

        def arm_a():
            checked(lib.crw_labelprop_propagate_sliding(p(seed), p(W), p(I), T, N, M, knn, 1, cxt, p(L), p(pred), None), "sliding")

        def arm_g():
            os.environ["CRW_LABELPROP_SLIDING_GENERAL"] = "1"
            try:
                arm_a()
            finally:
                del os.environ["CRW_LABELPROP_SLIDING_GENERAL"]

        def arm_b():
            checked(lib.crw_labelprop_gather(p(seed), p(W), p(R), T, N, M, knn, 1, p(L), p(pred), None), "gather")

        def arm_c():
            checked(lib.crw_labelprop_propagate(p(seed), p(W), p(I), T, N, M, knn, 1, cxt, p(L), p(pred), None), "propagate")

        res = alternate(dict(a=arm_a, b=arm_b, c=arm_c, g=arm_g))
        emit(out, what="kernels", geom=name, unit="us per call", **g, rounds=res, **{k + "_stats": stats(v) for k, v in res.items()},
             every_a_beats_every_b=max(res["a"]) < min(res["b"]), a_us_per_frame=stats(res["a"])["median"] / (T - 1))


def batch(out, G=60):
    lib = crw_hip.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for name, g in GEOM.items():
        T, N, M, cxt, knn = g["T"], g["N"], g["M"], g["cxt"], g["knn"]
        W, I, _, seed = lists(g)
        Wg = W[None].repeat(G, 1, 1, 1).contiguous()
        Lg, pg = torch.empty(G, T * N, M, device="cuda"), torch.empty(G, N, T, device="cuda")

        def arm_batch():
            checked(lib.crw_labelprop_propagate_sliding_batch(p(seed), p(Wg), p(I), 0, G, T, N, M, knn, 1, cxt, p(Lg), p(pg), None), "batch")

        def arm_loop():
            for i in range(G):
                checked(lib.crw_labelprop_propagate_sliding(p(seed), p(Wg[i]), p(I), T, N, M, knn, 1, cxt, p(Lg[i]), p(pg[i]), None), "sliding")

        res = alternate(dict(batch=arm_batch, singles=arm_loop), calls=5)
        emit(out, what="batch", geom=name, G=G, unit="us per call (all G configurations)", rounds=res,
             **{k + "_stats": stats(v) for k, v in res.items()})


def segment(out):
    import dataset as crw_dataset
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    rows, cols, T, patch, overlap, K = 410, 8192, 256, (32, 32), (24, 0), 5
    torch.manual_seed(11)
    enc = crw_utils.create_model(1, False).cuda()
    enc.train(True)
    rg = crw_dataset.synthetic_radargram(rows, cols)
    seg = (torch.arange(rows)[:, None] * K // rows).float().repeat(1, cols)
    cfg = dict(CXT_SIZE=80, RADIUS=RADIUS, TEMP=TEMP, KNN=20)

    def arm(context):
        lp = LabelPropVOS_CRW(dict(cfg, CONTEXT=context))
        return lambda: crw_inference.segment(crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap), seg, enc, lp, K, T, patch, overlap,
                                             use_last=True, dataset_id=3, device="cuda")

    res = alternate(dict(reference=arm("reference"), sliding=arm("sliding")), calls=3)
    emit(out, what="segment", rows=rows, cols=cols, T=T, unit="us per segment call", rounds=res, **{k + "_stats": stats(v) for k, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "batch", "segment", "all"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliding_timing.log"))
    a = ap.parse_args()
    for mode, fn in (("kernels", kernels), ("batch", batch), ("segment", segment)):
        if a.mode in (mode, "all"):
            fn(a.out)


if __name__ == "__main__":
    main()
