"""What guarding the Adam step costs: crw_adam_step_guarded (include/crw_hip_guard.h) against crw_adam_step at the two encoders'
parameter counts, n = 263 088 (CNN) and n = 4 971 468 (Resnet), by tools/longmem_timing.py's protocol: the C entry points, buffers
allocated once, 20 calls per round between two device events, seven rounds alternating the arms after a warm-up of each; every
round is on the log line.

  as            crw_adam_step, this build
  as0           crw_adam_step of the library given by --parent_lib (built from the parent commit), loaded by path beside this
                build's.  Left out when no such library is given.  Known artefact of this way of measuring: the library loaded
                second tends to run about 1 % faster
  gd            crw_adam_step_guarded, finite gradient, no bound (max_norm 0): the bits of `as` (asserted before the timing)
  gc            crw_adam_step_guarded, finite gradient under a bound a tenth of its norm: every step scaled
  gs            crw_adam_step_guarded on a gradient with one NaN: every step refused (the update launch returns at once)

THE EXPECTATION, written down before the run.  The update reads p, g, m, v and writes p, m, v: 7 x 4 = 28 bytes per element.  The
guard reads g once more for the norm: 32 bytes against 28, 8 / 7 = 1.14 x on traffic alone -- at most, since at these sizes g
(1 MB / 20 MB) stays in the caches between the norm pass and the update.  On top come two more launches (the partials, the
one-workgroup decision), a few microseconds each when nothing overlaps them: at the CNN's size, where crw_adam_step itself is about
5 us, they should dominate (expected 2 - 3 x); at the Resnet's size the traffic ratio should show (expected 1.1 - 1.3 x).  A
refused step reads g once: expected well under `as`.  The log line carries these under "expected"; what was found stands beside it.

WHAT WAS FOUND (profiles/guard_timing.log, one MI355X, medians of seven rounds, us per call).  CNN: as 4.65, gd 10.63, gc 10.55,
gs 10.63 -- gd / as = 2.29, inside the expected band, and all three guarded arms cost the same: at this size the call IS its three
dependent launches, about 3.5 us each.  That also makes the expectation for a refused step wrong here: it is not under `as` but
2.29 x it.  Resnet: as 20.78, gd 30.02, gc 30.42, gs 10.51 -- gd / as = 1.44, ABOVE the expected 1.1 - 1.3: the traffic ratio
(8 / 7 of 20.8 = 23.8 us) explains 3 us of the 9.2 us, the rest is the same launch chain, which at 20 us per update is not yet
small; a refused step costs 0.51 x `as`, the chain again (10.5 us at either size).  Scaling the gradient costs 0.4 us at the
Resnet's size and nothing measurable at the CNN's.  `as` against the parent build's `as0`: 1.018 and 0.988, the two orders of the
known load-order artefact -- the kernel is the same.  Against a training step of 6.4 ms (CNN) the guard adds about 6 us, 0.1 %.

usage: python tools/guard_timing.py [--parent_lib FILE] [--out FILE]
One JSON line per size, appended to FILE (default profiles/guard_timing.log) and printed."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radar-sounder-crw_amd"), os.path.join(ROOT, "tools")]
import torch

import crw_hip
from sliding_timing import alternate, checked, emit, stats

SIZES = dict(cnn=263088, resnet=4971468)
HP = (1e-3, 0.9, 0.999, 1e-8)          # lr, beta1, beta2, eps
EXPECTED = dict(bytes_per_element=dict(plain=28, guarded=32), traffic_ratio=32 / 28, extra_launches=2,
                gd_over_as=dict(cnn="2 - 3 (launch bound)", resnet="1.1 - 1.3 (traffic bound)"), gs_over_as="below 1: g is read once")


def parent_adam(path):
    handle = ctypes.CDLL(path)
    handle.crw_abi_version.restype = ctypes.c_int
    assert handle.crw_abi_version() == crw_hip.ABI_VERSION
    fn = handle.crw_adam_step
    fn.restype, fn.argtypes = crw_hip.SIGNATURES["crw_adam_step"]
    return fn


def run(out, parent_lib):
    lib = crw_hip.lib()
    parent = parent_adam(parent_lib) if parent_lib else None
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    for name, n in SIZES.items():
        gen = torch.Generator().manual_seed(1)
        g = (torch.randn(n, generator=gen) * 1e-2).cuda()
        g_nan = g.clone()
        g_nan[n // 2] = float("nan")
        p0 = torch.randn(n, generator=gen).cuda()
        bound = 0.1 * float(g.double().norm())
        nws = lib.crw_adam_guard_ws_bytes(n)

        def state():
            return dict(p=p0.clone(), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"), step=[0],
                        ctl=torch.zeros(crw_hip.GUARD_CTL_BYTES, dtype=torch.uint8, device="cuda"), ws=torch.empty(nws, dtype=torch.uint8, device="cuda"))

        def plain(fn, s):
            def call():
                s["step"][0] += 1
                checked(fn(p(s["p"]), p(g), p(s["m"]), p(s["v"]), n, *HP, s["step"][0], None), "crw_adam_step")
            return call

        def guarded(s, grad, max_norm):
            def call():
                s["step"][0] += 1
                checked(lib.crw_adam_step_guarded(p(s["p"]), p(grad), p(s["m"]), p(s["v"]), n, *HP, s["step"][0], max_norm, p(s["ctl"]), p(s["ws"]),
                                                  nws, None), "crw_adam_step_guarded")
            return call

        s_as, s_gd = state(), state()                                   # the bits first: three steps of each on equal states
        a, b = plain(lib.crw_adam_step, s_as), guarded(s_gd, g, 0.0)
        for _ in range(3):
            a(), b()
        torch.cuda.synchronize()
        assert all(bits(s_as[k], s_gd[k]) for k in "pmv"), "gd and as differ"
        states = {k: state() for k in ("as", "as0", "gd", "gc", "gs")}
        arms = dict({"as": plain(lib.crw_adam_step, states["as"])})
        if parent is not None:
            arms["as0"] = plain(parent, states["as0"])
        arms.update(gd=guarded(states["gd"], g, 0.0), gc=guarded(states["gc"], g, bound), gs=guarded(states["gs"], g_nan, 0.0))
        res = alternate(arms)
        torch.cuda.synchronize()
        ctl = {k: crw_hip.guard_ctl_unpack(states[k]["ctl"]) for k in ("gd", "gc", "gs")}
        assert ctl["gd"]["skipped"] == 0 and ctl["gs"]["applied"] == 0 and abs(ctl["gc"]["scale"] - 0.1) < 1e-4, ctl
        assert bits(states["gs"]["p"], p0), "a refused step moved p"
        med = lambda k: stats(res[k])["median"]
        extra = {k + "_over_as": med(k) / med("as") for k in ("gd", "gc", "gs")}
        if parent is not None:
            s0 = stats(res["as0"])
            extra.update(as_over_parent=med("as") / s0["median"], as_median_within_parent_rounds=bool(s0["min"] <= med("as") <= s0["max"]),
                         gd_over_parent_as=med("gd") / s0["median"])
        gbps = lambda k, nbytes: nbytes * n / med(k) / 1e3              # GB/s from the bytes the algorithm moves
        emit(out, what="guard", encoder=name, n=n, unit="us per call", parent_lib=bool(parent), expected=EXPECTED, rounds=res,
             **{k + "_stats": stats(v) for k, v in res.items()}, gd_as_bitwise_equal=True, as_GBps_at_28B=gbps("as", 28), gd_GBps_at_32B=gbps("gd", 32),
             gs_GBps_at_4B=gbps("gs", 4), counters={k: (v["applied"], v["skipped"]) for k, v in ctl.items()}, **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guard_timing.log"))
    ap.add_argument("--parent_lib", default=None, help="a libcrw_hip.so built from the parent commit (arm as0)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guard_timing.py measures on the GPU; there is none here")
    run(a.out, a.parent_lib)


if __name__ == "__main__":
    main()
