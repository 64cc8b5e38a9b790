"""What the anchor marks cost: anchored label propagation as ONE crw_labelprop_propagate_sliding call on marked lists against the
segments it replaces, and against the un-anchored call on this build and on a build of the commit before the marks -- at
tools/anchored_timing.py's four geometries (cfg5 [T, N, M] = [256, 48, 4] and an mc1-like item [100, 48, 4], CXT_SIZE 80, KNN 20;
every node of every 8th and of every 32nd frame anchored) and by its protocol:

  o    one launch on marked lists (`crw_hip.mark_anchors`, made beforehand) through the C entry point
  b    the segments through the C entry point, buffers and one-hot rows made beforehand: K + 1 launches for K anchored frames and
       the copies between them (tools/anchored_timing.py's arm b, the route before the marks)
  c    crw_labelprop_propagate_sliding on the same lists without anchors, this build
  c0   the same call on the library given by --parent_lib (a libcrw_hip.so built from the commit before the marks, loaded by path
       beside this build's): what an un-anchored caller paid before.  Left out when no such library is given
  c_NAME   the same call on every library given as --also NAME=FILE, e.g. this source built with
       `make EXTRA=-DCRW_LABELPROP_RING_NO_ANCHORS OUT=...`: the ring kernel without the anchors' select, which says what the select
       itself costs an un-anchored caller
  po   the binding, `crw_hip.labelprop_gather(anchors=)`, on its default route: a copy of the lists, two selects, one launch
  p    the binding under CRW_ANCHORS_SEGMENTED=1 (the route before the marks)
  so / s   crw_labelprop_propagate_sliding_batch at G = 60 on marked / on unmarked lists (a second set of rounds per geometry)

o, b, po and p write the same bits, asserted before the rounds; so's slice 0 equals o's.  Buffers allocated once, 20 calls per round
between two device events, seven rounds alternating the arms after a warm-up of each; every round is on the log line.

usage: python tools/anchor_lists_timing.py [--parent_lib FILE] [--also NAME=FILE ...] [--out FILE]
One JSON line per (geometry, spacing), appended to FILE (default profiles/anchor_lists_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from sliding_timing import GEOM, alternate, checked, emit, lists, stats

EVERY = (8, 32)
G_SWEEP = 60


def parent_entry(path):
    """crw_labelprop_propagate_sliding of another build of the library, loaded by path"""
    handle = ctypes.CDLL(path)
    fn = handle.crw_labelprop_propagate_sliding
    fn.restype, fn.argtypes = crw_hip.SIGNATURES["crw_labelprop_propagate_sliding"]
    handle.crw_abi_version.restype = ctypes.c_int
    assert handle.crw_abi_version() == crw_hip.ABI_VERSION
    return fn


def run(out, parent_lib, also=()):
    lib = crw_hip.lib()
    parent = parent_entry(parent_lib) if parent_lib else None
    others = {"c_" + spec.split("=", 1)[0]: parent_entry(spec.split("=", 1)[1]) for spec in also}
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for name, g in GEOM.items():
        T, N, M, cxt, knn = g["T"], g["N"], g["M"], g["cxt"], g["knn"]
        W, I, _, seed = lists(g)
        gen = torch.Generator().manual_seed(2)
        for every in EVERY:
            frames = list(range(every, T, every))
            classes = torch.randint(0, M, (T, N), generator=gen)
            anchor = torch.full((T, N), -1, dtype=torch.int8)
            anchor[frames] = classes[frames].to(torch.int8)
            anchor = anchor.cuda()
            Wm, Im = crw_hip.mark_anchors(W.clone(), I.clone(), anchor, M, 1)
            rows = {f: torch.nn.functional.one_hot(classes[f], M).float().cuda() for f in frames}
            cols = {f: classes[f].float().cuda() for f in frames}
            new = lambda: (torch.empty(T * N, M, device="cuda"), torch.empty(N, T, device="cuda"))
            (Lo, po_), (Lb, pb), (Lc, pc), (Lc0, pc0), (Lp, pp) = new(), new(), new(), new(), new()
            ends = frames + ([T - 1] if frames[-1] != T - 1 else [])
            parts = [pb.new_empty(N, e + 1) for e in ends]

            def arm_o():
                checked(lib.crw_labelprop_propagate_sliding(p(seed), p(Wm), p(Im), T, N, M, knn, 1, cxt, p(Lo), p(po_), None), "sliding")

            def arm_b():
                start = 1
                for e, part in zip(ends, parts):
                    checked(lib.crw_labelprop_propagate_sliding(p(seed) if start == 1 else None, p(W[start - 1:]), p(I[start - 1:]), e + 1, N, M,
                                                                knn, start, cxt, p(Lb), p(part), None), "sliding")
                    if e in rows:
                        Lb[e * N:(e + 1) * N].copy_(rows[e])
                        part[:, e].copy_(cols[e])
                    pb[:, start:e + 1] = part[:, start:e + 1]
                    start = e + 1
                pb[:, 0] = parts[0][:, 0]

            def arm_c():
                checked(lib.crw_labelprop_propagate_sliding(p(seed), p(W), p(I), T, N, M, knn, 1, cxt, p(Lc), p(pc), None), "sliding")

            def arm_c0():
                checked(parent(p(seed), p(W), p(I), T, N, M, knn, 1, cxt, p(Lc0), p(pc0), None), "sliding (parent build)")

            def arm_po():
                os.environ.pop("CRW_ANCHORS_SEGMENTED", None)
                crw_hip.labelprop_gather(seed, W, I, T, N, M, L=Lp, pred=pp, cxt_size=cxt, context="sliding", anchors=anchor)

            def arm_p():
                os.environ["CRW_ANCHORS_SEGMENTED"] = "1"
                crw_hip.labelprop_gather(seed, W, I, T, N, M, L=Lp, pred=pp, cxt_size=cxt, context="sliding", anchors=anchor)
                del os.environ["CRW_ANCHORS_SEGMENTED"]

            assert crw_hip.has_anchor_lists()
            for t in (Lb, pb, Lo, po_, *parts):
                t.fill_(float("nan"))
            arm_b()
            arm_o()
            torch.cuda.synchronize()
            same = lambda L, q: torch.equal(L.view(torch.int32), Lb.view(torch.int32)) and torch.equal(q, pb)
            assert same(Lo, po_), "o and b differ"
            for arm in (arm_po, arm_p):
                Lp.fill_(float("nan"))
                pp.fill_(float("nan"))
                arm()
                torch.cuda.synchronize()
                assert same(Lp, pp), "b and the binding differ"
            arms = dict(o=arm_o, b=arm_b, c=arm_c, po=arm_po, p=arm_p)
            if parent is not None:
                arm_c()
                arm_c0()
                torch.cuda.synchronize()
                assert torch.equal(Lc.view(torch.int32), Lc0.view(torch.int32)) and torch.equal(pc, pc0), "c and c0 differ"
                arms = dict(o=arm_o, b=arm_b, c=arm_c, c0=arm_c0, po=arm_po, p=arm_p)
            for k, fn in others.items():
                arms[k] = lambda fn=fn: checked(fn(p(seed), p(W), p(I), T, N, M, knn, 1, cxt, p(Lc0), p(pc0), None), "sliding (" + k + ")")
            res = alternate(arms)

            Wg, Wgm = W[None].repeat(G_SWEEP, 1, 1, 1).contiguous(), Wm[None].repeat(G_SWEEP, 1, 1, 1).contiguous()
            Lg, pg = torch.empty(G_SWEEP, T * N, M, device="cuda"), torch.empty(G_SWEEP, N, T, device="cuda")

            def arm_so():
                checked(lib.crw_labelprop_propagate_sliding_batch(p(seed), p(Wgm), p(Im), 0, G_SWEEP, T, N, M, knn, 1, cxt, p(Lg), p(pg), None), "batch")

            def arm_s():
                checked(lib.crw_labelprop_propagate_sliding_batch(p(seed), p(Wg), p(I), 0, G_SWEEP, T, N, M, knn, 1, cxt, p(Lg), p(pg), None), "batch")

            arm_so()
            torch.cuda.synchronize()
            assert same(Lg[0], pg[0]) and same(Lg[-1], pg[-1]), "the batch on marked lists and b differ"
            res.update(alternate(dict(so=arm_so, s=arm_s)))
            med = lambda k: stats(res[k])["median"]
            extra = {}
            if parent is not None:
                s0 = stats(res["c0"])
                extra = dict(c_median_within_c0_rounds=bool(med("c") <= s0["max"]), c_over_c0=med("c") / s0["median"])
            emit(out, what="anchor lists", geom=name, every=every, anchored_frames=len(frames), launches_b=len(ends), unit="us per call", **g,
                 G_sweep=G_SWEEP, parent_lib=bool(parent), rounds=res, **{k + "_stats": stats(v) for k, v in res.items()},
                 o_b_po_p_bitwise_equal=True, every_o_round_faster_than_every_b_round=bool(max(res["o"]) < min(res["b"])),
                 o_over_c=med("o") / med("c"), b_over_o=med("b") / med("o"), so_over_s=med("so") / med("s"), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_lists_timing.log"))
    ap.add_argument("--parent_lib", default=None, help="a libcrw_hip.so built from the commit before the marks (arm c0)")
    ap.add_argument("--also", default=[], action="append", metavar="NAME=FILE", help="another build of the library: arm c_NAME")
    a = ap.parse_args()
    run(a.out, a.parent_lib, a.also)


if __name__ == "__main__":
    main()
