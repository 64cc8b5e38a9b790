#!/usr/bin/env python3
"""A/B of two builds of the library on the CNN front end (encoder_front.hip): are all outputs the same bits, and how long does
each backward entry point take?

usage: python tools/front_bwd_ab.py LIB_A LIB_B [--timeout SECONDS] [--keep DIR]

Each library runs in a fresh child process of its own (CRW_HIP_LIB selects the build, each child under its own time limit;
the tool stops at the first child that fails).  A child runs, on fixed-seed inputs, for split in {1, 3} and cin in {1, 2}:
enc_front_fwd(save=True), enc_front_bwd with and without the saved record at P = 257 (two patches per workgroup, empty
workgroups), and enc_front_fwd_map / enc_front_bwd_map at 43 patches of 20x27 and 29 patches of 32x32 (two units per workgroup,
partial tiles) -- the shapes of tests/test_hip_parity.py's two-per-workgroup cases -- and saves every output tensor.  It then
times each backward entry point with HIP events (3 warm-up + 20 timed launches, median), at those shapes and at the training
sizes of bench.py (16128 patches of 16x16; 1792 patches of 32x32 = 16128 units).  This process compares A with B tensor by
tensor (one line each), prints the medians side by side and exits non-zero if any tensor differs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS, CINS = (1, 3), (1, 2)
P16 = 257
MAPS = (((20, 27), 43), ((32, 32), 29))
BIG16, BIGMAP = 16128, ((32, 32), 1792)
WARMUP, TIMED = 3, 20


def child(out_path):
    sys.path.insert(0, os.path.join(ROOT, "radar-sounder-crw_amd"))
    import torch
    import crw_hip as hip
    hip.lib()
    outs, times = {}, {}

    def weights(g, cin, split):
        w1 = (torch.randn(8, cin, 5, 5, generator=g) * 0.2).cuda()
        b1 = (torch.randn(8, generator=g) * 0.1).cuda()
        w2 = (torch.randn(32, 8, 5, 5, generator=g) * 0.07).cuda()
        b2 = (torch.randn(32, generator=g) * 0.1).cuda()
        return w1, b1, hip.enc_front_pack(w2, split), b2

    def keep(key, names, tensors):
        for n, t in zip(names, tensors):
            if t is not None:
                outs[f"{key}/{n}"] = t.cpu()

    def median_ms(fn):
        ms = []
        for i in range(WARMUP + TIMED):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= WARMUP:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    grads = ("dw1", "db1", "dw2", "db2")
    for split in SPLITS:
        for cin in CINS:
            for P in (P16, BIG16):
                g = torch.Generator().manual_seed(1000 + 10 * cin + split)
                w1, b1, w2p, b2 = weights(g, cin, split)
                x = torch.randn(P, cin, 16, 16, generator=g).cuda()
                dy = torch.randn(P, 100, 32, generator=g).cuda()
                key = f"s{split}c{cin} 16x16 P{P}"
                yh, yl, saved = hip.enc_front_fwd(split, x, w1, b1, w2p[:2], b2, save=True)
                saved_bwd = lambda: hip.enc_front_bwd(split, x, w1, b1, w2p[:2], b2, w2p[2:], dy, saved=saved)
                recompute_bwd = lambda: hip.enc_front_bwd(split, x, w1, b1, w2p[:2], b2, w2p[2:], dy)
                if P == P16:
                    keep(key + " fwd", ("yh", "yl", "saved"), (yh, yl, saved))
                    keep(key + " bwd saved", grads, saved_bwd())
                    keep(key + " bwd recompute", grads, recompute_bwd())
                times[key + " bwd saved"] = median_ms(saved_bwd)
                times[key + " bwd recompute"] = median_ms(recompute_bwd)
            for (h, w), P in MAPS + (BIGMAP,):
                g = torch.Generator().manual_seed(2000 + 100 * cin + h + split)
                w1, b1, w2p, b2 = weights(g, cin, split)
                x = torch.randn(P, cin, h, w, generator=g).cuda()
                dy = torch.randn(P, (h - 6) * (w - 6), 32, generator=g).cuda()
                key = f"s{split}c{cin} {h}x{w} P{P}"
                tile_bwd = lambda: hip.enc_front_bwd_map(split, x, w1, b1, w2p[:2], b2, w2p[2:], dy)
                if ((h, w), P) in MAPS:
                    keep(key + " fwd_map", ("yh", "yl"), hip.enc_front_fwd_map(split, x, w1, b1, w2p[:2], b2))
                    keep(key + " bwd_map", grads, tile_bwd())
                times[key + " bwd_map"] = median_ms(tile_bwd)
    torch.cuda.synchronize()
    torch.save({"outs": outs, "times": times}, out_path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of each child, seconds")
    ap.add_argument("--keep", default=None, help="directory for the children's records (default: a temporary one)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import torch
    work = a.keep or tempfile.mkdtemp(prefix="front_bwd_ab_")
    os.makedirs(work, exist_ok=True)
    recs = []
    for tag, lib in (("A", a.lib_a), ("B", a.lib_b)):
        path = os.path.join(work, f"{tag}.pt")
        env = dict(os.environ, CRW_HIP_LIB=os.path.abspath(lib))
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), lib, lib, "--child", path], env=env,
                                timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"child {tag} ({lib}) exited with {rc}: stopping", flush=True)
            return 1
        recs.append(torch.load(path))
    (oa, ta), (ob, tb) = [(r["outs"], r["times"]) for r in recs]
    assert oa.keys() == ob.keys() and ta.keys() == tb.keys()
    ndiff = 0
    for k in oa:
        same = oa[k].shape == ob[k].shape and torch.equal(oa[k], ob[k])
        ndiff += not same
        print(f"{'equal ' if same else 'DIFFER'} {k} {tuple(oa[k].shape)}")
    print(f"{len(oa) - ndiff} of {len(oa)} tensors equal")
    print(f"{'median ms of %d launches' % TIMED:44s} {'A':>9s} {'B':>9s} {'B/A':>7s}")
    for k in ta:
        print(f"{k:44s} {ta[k]:9.4f} {tb[k]:9.4f} {tb[k] / ta[k]:7.3f}")
    print(json.dumps({"tensors": len(oa), "differ": ndiff, "median_ms": {"A": ta, "B": tb}}))
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
