"""What the context novelty costs: `crw_labelprop_novelty` (include/crw_hip_novelty.h) against what one would do without it, at
tools/restart_timing.py's geometries (cfg5 [T, N] = [256, 48] and an mc1-like item [100, 48], C = 128 the Resnet encoder's feature
width, CXT_SIZE 80, RADIUS 10) and by its protocol, without origins and with an origin every 8 frames:

  am / av   (a) ONE crw_labelprop_novelty call: the matrix route / the vector route
  b         (b) without the entry point: crw_labelprop_topk_scores at kcap = 1 (the parent's kernel; with origins
            crw_labelprop_topk_origin, raw), then 1 - temp V and torch.topk(top).values.mean on it
  bk        the top-k call of (b) alone
  c         (c) crw_labelprop_topk_grid at knn 20 -- what the propagation itself spends on its lists, for scale

am and b give the same novelties within the rounding bounds of tests/novelty_ref.py, asserted before the rounds.  Buffers allocated
once, 20 calls per round between two device events, seven rounds alternating the arms after a warm-up of each; every round is on
the log line.  Then `inference.segment(..., suggest=1)` against suggest=0 on --synthetic 410 8192 (tools/sliding_timing.py's
segment arm), alternating, 3 calls per round.

usage: python tools/novelty_timing.py [--out FILE] [--skip_segment]
One JSON line per (geometry, origins) and one for segment, appended to FILE (default profiles/novelty_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from sliding_timing import C, GEOM, RADIUS, TEMP, alternate, checked, emit, stats

EVERY = (0, 8)  # 0: no origins


def kernels(out):
    lib = crw_hip.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for name, g in GEOM.items():
        T, N, cxt, knn = g["T"], g["N"], g["cxt"], g["knn"]
        top = crw_hip.novelty_top(N)
        gen = torch.Generator().manual_seed(1)
        feats = crw_hip.normalize((torch.randn(1, N, C, generator=gen) + 0.5 * torch.randn(T, N, C, generator=gen)).float().cuda())
        for every in EVERY:
            origin = torch.zeros(T, dtype=torch.int32)
            for n in range(1, T):
                origin[n] = n - 1 if every and (n - 1) and (n - 1) % every == 0 else origin[n - 1]
            od = origin.cuda() if every else None
            novm, scm, novv, scv = (torch.empty(T - 1, N, device="cuda"), torch.empty(T - 1, device="cuda"),
                                    torch.empty(T - 1, N, device="cuda"), torch.empty(T - 1, device="cuda"))
            V1, I1 = torch.empty(T - 1, 1, N, device="cuda"), torch.empty(T - 1, 1, N, device="cuda", dtype=torch.int32)
            Wk, Ik = torch.empty(T - 1, knn, N, device="cuda"), torch.empty(T - 1, knn, N, device="cuda", dtype=torch.int32)
            held = {}

            def arm_am():
                checked(lib.crw_labelprop_novelty(p(feats), T, N, C, cxt, RADIUS, 1, top, p(od), p(novm), p(scm), 2, None), "novelty matrix")

            def arm_av():
                checked(lib.crw_labelprop_novelty(p(feats), T, N, C, cxt, RADIUS, 1, top, p(od), p(novv), p(scv), 1, None), "novelty vector")

            def arm_bk():
                if od is None:
                    checked(lib.crw_labelprop_topk_scores(p(feats), T, N, C, cxt, RADIUS, TEMP, 1, 1, 1, p(V1), p(I1), None), "topk_scores")
                else:
                    checked(lib.crw_labelprop_topk_origin(p(feats), T, N, C, cxt, RADIUS, TEMP, 1, 1, 1, p(od), p(V1), p(I1), 1, None), "topk_origin")

            def arm_b():
                arm_bk()
                nov = 1 - TEMP * V1[:, 0, :]
                held["b"] = (nov, torch.topk(nov, top, dim=1).values.mean(1))

            def arm_c():
                if od is None:
                    checked(lib.crw_labelprop_topk_grid(p(feats), T, N, C, cxt, RADIUS, TEMP, knn, 1, 1, p(Wk), p(Ik), None), "topk_grid")
                else:
                    checked(lib.crw_labelprop_topk_origin(p(feats), T, N, C, cxt, RADIUS, TEMP, knn, 1, 1, p(od), p(Wk), p(Ik), 0, None), "topk_origin")

            for t in (novm, scm, novv, scv):
                t.fill_(float("nan"))
            arm_am(), arm_av(), arm_b()
            torch.cuda.synchronize()
            u = 2.0 ** -24
            dn, ds = (novm - held["b"][0]).abs().max().item(), (scm - held["b"][1]).abs().max().item()
            dv = (novm - novv).abs().max().item()
            assert dn <= 2 * (C + 2) * u + 2 * u and ds <= 2 * (C + 2 + 2 * (top + 1)) * u and dv <= 2 * (C + 2) * u, (dn, ds, dv)
            res = alternate(dict(am=arm_am, av=arm_av, b=arm_b, bk=arm_bk, c=arm_c))
            med = lambda k: stats(res[k])["median"]
            emit(out, what="novelty", geom=name, T=T, N=N, C=C, cxt=cxt, radius=RADIUS, top=top, origin_every=every, knn_of_c=knn,
                 unit="us per call", rounds=res, **{k + "_stats": stats(v) for k, v in res.items()},
                 max_abs_diff=dict(nov_am_b=dn, score_am_b=ds, nov_am_av=dv),
                 every_am_round_faster_than_every_b_round=bool(max(res["am"]) < min(res["b"])),
                 every_am_round_faster_than_every_bk_round=bool(max(res["am"]) < min(res["bk"])),
                 b_over_am=med("b") / med("am"), bk_over_am=med("bk") / med("am"), av_over_am=med("av") / med("am"),
                 c_over_am=med("c") / med("am"))


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
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=80, RADIUS=RADIUS, TEMP=TEMP, KNN=20, CONTEXT="sliding"))

    def arm(suggest):
        return lambda: crw_inference.segment(crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap), seg, enc, lp, K, T, patch, overlap,
                                             use_last=True, dataset_id=3, device="cuda", suggest=suggest)

    res = alternate(dict(suggest0=arm(0), suggest1=arm(1)), calls=3)
    med = lambda k: stats(res[k])["median"]
    emit(out, what="segment", rows=rows, cols=cols, T=T, unit="us per segment call", rounds=res, **{k + "_stats": stats(v) for k, v in res.items()},
         suggest1_over_suggest0=med("suggest1") / med("suggest0"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "novelty_timing.log"))
    ap.add_argument("--skip_segment", action="store_true")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    kernels(a.out)
    if not a.skip_segment:
        segment(a.out)


if __name__ == "__main__":
    main()
