"""What anchor_context='restart' costs: the entry points of include/crw_hip_restart.h against the segmented construction they
replace, against clamp mode, and the un-anchored entry points on this build against a build of the parent commit -- at
tools/anchor_lists_timing.py's geometries (cfg5 [T, N, M] = [256, 48, 4] and an mc1-like item [100, 48, 4], CXT_SIZE 80, KNN 20;
every node of every 8th and of every 32nd frame anchored, so each of those frames is an origin) and by its protocol.  Top-k (t*),
propagation (p*) and both together are timed separately:

  tr / pr / r   ONE crw_labelprop_topk_origin call / ONE crw_labelprop_propagate_origin call on its marked lists / both
  ts / ps / s   the segmented construction from the entry points without origins: one crw_labelprop_topk_grid call, one
                crw_labelprop_propagate_sliding call per stretch between origins, on sub-items, and the pred copies between them
  to / po / o   clamp mode in one launch each (crw_labelprop_topk_grid on the whole item, crw_labelprop_propagate_sliding on marked
                lists).  It computes ANOTHER result and is here for context
  tc / pc       the un-anchored entry points (crw_labelprop_topk_grid, crw_labelprop_propagate_sliding on unmarked lists), this build
  tc0 / pc0     the same calls on the library given by --parent_lib (built from the parent commit, loaded by path beside this
                build's).  Left out when no such library is given
  gb / gl       crw_labelprop_propagate_origin_batch at G = 60 / 60 crw_labelprop_propagate_origin calls (a second set of rounds)

r and s write the same bits (lists, L and pred), c and c0 likewise, asserted before the rounds.  Buffers allocated once, 20 calls per
round between two device events, seven rounds alternating the arms after a warm-up of each; every round is on the log line.

usage: python tools/restart_timing.py [--parent_lib FILE] [--out FILE]
One JSON line per (geometry, spacing), appended to FILE (default profiles/restart_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from sliding_timing import C, GEOM, RADIUS, TEMP, alternate, checked, emit, stats

EVERY = (8, 32)
G_SWEEP = 60


def parent_entries(path):
    """crw_labelprop_topk_grid and crw_labelprop_propagate_sliding of another build of the library, loaded by path"""
    handle = ctypes.CDLL(path)
    handle.crw_abi_version.restype = ctypes.c_int
    assert handle.crw_abi_version() == crw_hip.ABI_VERSION
    out = []
    for name in ("crw_labelprop_topk_grid", "crw_labelprop_propagate_sliding"):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = crw_hip.SIGNATURES[name]
        out.append(fn)
    return out


def run(out, parent_lib):
    lib = crw_hip.lib()
    parent = parent_entries(parent_lib) if parent_lib else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for name, g in GEOM.items():
        T, N, M, cxt, knn = g["T"], g["N"], g["M"], g["cxt"], g["knn"]
        gen = torch.Generator().manual_seed(1)
        feats = crw_hip.normalize((torch.randn(1, N, C, generator=gen) + 0.5 * torch.randn(T, N, C, generator=gen)).float().cuda())
        seed = (torch.arange(N) * M // N).float().cuda()
        gen = torch.Generator().manual_seed(2)
        for every in EVERY:
            frames = list(range(every, T, every))
            classes = torch.randint(0, M, (T, N), generator=gen)
            anchor = torch.full((T, N), -1, dtype=torch.int8)
            anchor[frames] = classes[frames].to(torch.int8)
            origin = crw_hip.anchor_origins(anchor, M, T)
            stretches = crw_hip.origin_stretches(origin.tolist(), T)
            od, anchor = origin.cuda(), anchor.cuda()
            lists = lambda: (torch.empty(T - 1, knn, N, device="cuda"), torch.empty(T - 1, knn, N, device="cuda", dtype=torch.int32))
            labels = lambda: (torch.empty(T * N, M, device="cuda"), torch.empty(N, T, device="cuda"))
            (Wr, Ir), (Ws, Is), (Wo, Io), (Wc, Ic), (Wc0, Ic0) = lists(), lists(), lists(), lists(), lists()
            (Lr, qr), (Ls, qs), (Lo, qo), (Lc, qc), (Lc0, qc0) = labels(), labels(), labels(), labels(), labels()
            parts = [qs.new_empty(N, e + 1 - a) for a, e in stretches]
            topk = lambda fn, e, n, ff, W, I: checked(fn(p(e), n, N, C, cxt, RADIUS, TEMP, knn, ff, 1, p(W), p(I), None), "topk_grid")
            slide = lambda fn, s, W, I, n, ff, L, q: checked(fn(p(s), p(W), p(I), n, N, M, knn, ff, cxt, p(L), p(q), None), "sliding")

            def arm_tr():
                checked(lib.crw_labelprop_topk_origin(p(feats), T, N, C, cxt, RADIUS, TEMP, knn, 1, 1, p(od), p(Wr), p(Ir), 0, None), "topk_origin")

            def arm_ts():
                for a, e in stretches:
                    topk(lib.crw_labelprop_topk_grid, feats[a:], e + 1 - a, 1, Ws[a:], Is[a:])

            def arm_pr():
                checked(lib.crw_labelprop_propagate_origin(p(seed), p(Wrm), p(Irm), T, N, M, knn, 1, cxt, p(od), p(Lr), p(qr), None), "origin")

            def arm_ps():
                for (a, e), part in zip(stretches, parts):
                    slide(lib.crw_labelprop_propagate_sliding, seed if a == 0 else None, Wrm[a:], Irm[a:], e + 1 - a, 1, Ls[a * N:], part)
                    qs[:, a + 1:e + 1] = part[:, 1:]
                qs[:, 0] = parts[0][:, 0]

            arm_to = lambda: topk(lib.crw_labelprop_topk_grid, feats, T, 1, Wo, Io)
            arm_po = lambda: slide(lib.crw_labelprop_propagate_sliding, seed, Wom, Iom, T, 1, Lo, qo)
            arm_tc = lambda: topk(lib.crw_labelprop_topk_grid, feats, T, 1, Wc, Ic)
            arm_pc = lambda: slide(lib.crw_labelprop_propagate_sliding, seed, Wc, Ic, T, 1, Lc, qc)
            arm_r = lambda: (arm_tr(), arm_pr())
            arm_s = lambda: (arm_ts(), arm_ps())
            arm_o = lambda: (arm_to(), arm_po())

            for t in (Wr, Ws, Lr, Ls, qr, qs, *parts):
                t.fill_(float("nan"))
            arm_tr(), arm_ts(), arm_to(), arm_tc()
            Wrm, Irm = crw_hip.mark_anchors(Wr.clone(), Ir.clone(), anchor, M, 1)       # the lists of (r) and (s), marked beforehand
            Wom, Iom = crw_hip.mark_anchors(Wo.clone(), Io.clone(), anchor, M, 1)
            arm_pr(), arm_ps(), arm_po(), arm_pc()
            torch.cuda.synchronize()
            bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert bits(Wr, Ws) and torch.equal(Ir, Is), "the lists of r and s differ"
            assert bits(Lr, Ls) and torch.equal(qr, qs), "L / pred of r and s differ"
            arms = dict(tr=arm_tr, ts=arm_ts, to=arm_to, tc=arm_tc, pr=arm_pr, ps=arm_ps, po=arm_po, pc=arm_pc, r=arm_r, s=arm_s, o=arm_o)
            if parent is not None:
                arms["tc0"] = lambda: topk(parent[0], feats, T, 1, Wc0, Ic0)
                arms["pc0"] = lambda: slide(parent[1], seed, Wc, Ic, T, 1, Lc0, qc0)
                arms["tc0"](), arms["pc0"]()
                torch.cuda.synchronize()
                assert bits(Wc, Wc0) and torch.equal(Ic, Ic0) and bits(Lc, Lc0) and torch.equal(qc, qc0), "c and c0 differ"
            res = alternate(arms)

            Wg = Wrm[None].repeat(G_SWEEP, 1, 1, 1).contiguous()
            Lg, qg = torch.empty(G_SWEEP, T * N, M, device="cuda"), torch.empty(G_SWEEP, N, T, device="cuda")

            def arm_gb():
                checked(lib.crw_labelprop_propagate_origin_batch(p(seed), p(Wg), p(Irm), 0, G_SWEEP, T, N, M, knn, 1, cxt, p(od), p(Lg), p(qg),
                                                                 None), "origin_batch")

            def arm_gl():
                for i in range(G_SWEEP):
                    checked(lib.crw_labelprop_propagate_origin(p(seed), p(Wg[i]), p(Irm), T, N, M, knn, 1, cxt, p(od), p(Lg[i]), p(qg[i]), None),
                            "origin")

            arm_gb()
            torch.cuda.synchronize()
            assert bits(Lg[0], Lr) and torch.equal(qg[-1], qr), "the batch and r differ"
            res.update(alternate(dict(gb=arm_gb, gl=arm_gl)))
            med = lambda k: stats(res[k])["median"]
            extra = {}
            if parent is not None:
                for k in ("tc", "pc"):
                    s0 = stats(res[k + "0"])
                    extra[k + "_median_within_parent_rounds"] = bool(s0["min"] <= med(k) <= s0["max"])
                    extra[k + "_over_parent"] = med(k) / s0["median"]
            emit(out, what="anchor restart", geom=name, every=every, origins=len(frames), stretches=len(stretches), unit="us per call", **g,
                 G_sweep=G_SWEEP, parent_lib=bool(parent), rounds=res, **{k + "_stats": stats(v) for k, v in res.items()},
                 r_s_bitwise_equal=True, **{f"every_{a}_round_faster_than_every_{b}_round": bool(max(res[a]) < min(res[b]))
                                            for a, b in (("r", "s"), ("tr", "ts"), ("pr", "ps"), ("gb", "gl"))},
                 s_over_r=med("s") / med("r"), tr_over_to=med("tr") / med("to"), pr_over_po=med("pr") / med("po"),
                 gl_over_gb=med("gl") / med("gb"), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restart_timing.log"))
    ap.add_argument("--parent_lib", default=None, help="a libcrw_hip.so built from the parent commit (arms tc0, pc0)")
    a = ap.parse_args()
    run(a.out, a.parent_lib)


if __name__ == "__main__":
    main()
