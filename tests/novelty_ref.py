"""Context novelty and anchor picks as plain loops -- the definition `crw_labelprop_novelty` (include/crw_hip_novelty.h),
`crw_hip.labelprop_novelty` and `crw_hip.suggest_frames` are held to.

ehat [T, N, C] normalised features, cxt, radius, origin [T] (`restart_ref.origins`; all zero when absent).  Frame n >= 1 has the keys
`restart_ref.key_frames(n, origin[n], cxt)` -- what the top-k scores under either context rule -- and of each the in-band nodes p,
|p - q| < radius (an N x 1 grid).
  nov[n, q] = 1 - max over key frames f and in-band p of <ehat[n, q], ehat[f, p]>                       (`novelty`)
  s[n]      = mean of the `top` largest nov[n, .], top = max(1, N // 4) by default                      (`frame_scores`)
  z[n]      = s[n] - numpy.median{ s[m] : m != n, max(first, n - cxt) <= m <= min(T - 1, n + cxt) }     (`excess`; no neighbour: s[n])
  picks     = budget rounds of "largest z, lowest frame on ties, then remove the frames within min_gap of it", the fully anchored
              frames and their +- min_gap neighbours removed before the first round -> [(frame, z, s)]  (`picks`)
Arrays of per-frame values start at frame `first_frame`: index i is frame first_frame + i.

Also here: the items with two onsets (`two_onsets_item`), the planted defects (`DEFECTS`) and the ONE checker of the CPU and the GPU
tests (`violations`)."""
import numpy as np

import oracle.crw_oracle as oracle
import restart_ref as rr

U = 2.0 ** -24
DEFECTS = ("window_before_origin",   # the window reaches before the origin
           "band_le",                # the band is |p - q| <= radius
           "mean",                   # the excess is over the mean of the neighbours, not their median
           "top_smallest")           # the frame score averages the `top` SMALLEST


def default_top(N):
    return max(1, N // 4)


def normalized(emb):
    return oracle.l2_normalize(emb, np.float32).astype(np.float32)


def novelty(ehat, cxt, radius, origin=None, first_frame=1, dtype=np.float64, defect=None):
    """-> nov [T - first_frame, N] in `dtype` (float32: the products and their sum in fp32, in channel order)"""
    assert defect is None or defect in DEFECTS
    T, N, C = ehat.shape
    e = np.asarray(ehat).astype(dtype)
    out = np.empty((T - first_frame, N), dtype)
    for n in range(first_frame, T):
        a = 0 if origin is None else int(origin[n])
        keys = rr.key_frames(n, a, cxt)
        if defect == "window_before_origin" and a > 0:
            keys = [a] + [f for f in range(max(1, n - cxt), n) if f != a]
        for q in range(N):
            best = -np.inf
            for f in keys:
                for p in range(N):
                    if abs(p - q) < radius or (defect == "band_le" and abs(p - q) == radius):
                        d = dtype(0)
                        for c in range(C):
                            d = dtype(d + e[n, q, c] * e[f, p, c])
                        best = max(best, d)
            out[n - first_frame, q] = dtype(1) - best
    return out


def novelty_fast(ehat, cxt, radius, origin=None, first_frame=1, dtype=np.float64):
    """`novelty` with the dot products as one matrix product per key frame (another summation order: equal within the bound in
    fp32, and to a few fp64 roundings in fp64) -- what the tests that need many items call"""
    T, N, C = ehat.shape
    e = np.asarray(ehat).astype(dtype)
    band = np.abs(np.arange(N)[:, None] - np.arange(N)[None]) < radius
    out = np.empty((T - first_frame, N), dtype)
    for n in range(first_frame, T):
        best = np.full(N, -np.inf, dtype)
        for f in rr.key_frames(n, 0 if origin is None else int(origin[n]), cxt):
            best = np.maximum(best, np.where(band, e[n] @ e[f].T, -np.inf).max(1))
        out[n - first_frame] = 1 - best
    return out


def frame_scores(nov, top=None, dtype=np.float64, defect=None):
    """s [F]: float64 -- the mean; float32 -- the `top` largest added in descending order in fp32, then one division"""
    F, N = nov.shape
    top = default_top(N) if top is None else top
    assert 1 <= top <= N
    out = np.empty(F, dtype)
    for i in range(F):
        v = np.sort(np.asarray(nov[i]).astype(dtype))[::-1]
        if defect == "top_smallest":
            v = v[::-1]
        s = dtype(0)
        for j in range(top):
            s = dtype(s + v[j])
        out[i] = dtype(s / dtype(top))
    return out


def excess(s, cxt, defect=None):
    """z [F] float64 from s [F] (index 0 = the first scored frame)"""
    s = np.asarray(s, np.float64)
    z = np.empty_like(s)
    for i in range(len(s)):
        nb = [s[m] for m in range(max(0, i - cxt), min(len(s) - 1, i + cxt) + 1) if m != i]
        z[i] = s[i] - ((np.mean(nb) if defect == "mean" else np.median(nb)) if nb else 0.0)
    return z


def picks(s, cxt, budget, min_gap=2, first_frame=1, anchored=(), defect=None):
    """[(frame, z, s)] in pick order.  anchored: the frames that are already fully anchored"""
    s = np.asarray(s, np.float64)
    z = excess(s, cxt, defect)
    left = set(range(first_frame, first_frame + len(s)))
    for f in anchored:
        left -= set(range(int(f) - min_gap, int(f) + min_gap + 1))
    out = []
    for _ in range(budget):
        if not left:
            break
        best = max(sorted(left), key=lambda f: z[f - first_frame])          # max keeps the FIRST maximum: the lowest frame
        out.append((best, float(z[best - first_frame]), float(s[best - first_frame])))
        left -= set(range(best - min_gap, best + min_gap + 1))
    return out


def suggest(emb, cxt, radius, budget, top=None, min_gap=2, origin=None, anchored=(), dtype=np.float64, defect=None, fast=True):
    """features -> picks, the whole definition (first_frame 1)"""
    ehat = normalized(emb)
    if fast and defect not in ("window_before_origin", "band_le"):
        nov = novelty_fast(ehat, cxt, radius, origin, 1, dtype)
    else:
        nov = novelty(ehat, cxt, radius, origin, 1, dtype, defect)
    return picks(frame_scores(nov, top, dtype, defect), cxt, budget, min_gap, 1, anchored, defect)


def two_onsets_item(seed, T, N, C, M, amp):
    """`anchored_ref.emerging_item` (the same generator call order: prototypes, walk, then per-node noise in (t, i) order; the same
    class formula) with TWO layers entering: class M - 1 folded into M - 2 for t < fb = (5 T) // 8, then class M - 2 folded into
    M - 3 for t < fa = T // 4.  Called with the shape's M + 1.  -> (emb [T, N, C], cls [T, N], (fa, fb))"""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((M, C))
    walk = rng.standard_normal((T, C)).cumsum(0) * 0.15
    fa, fb = T // 4, (5 * T) // 8
    emb = np.empty((T, N, C))
    cls = np.empty((T, N), np.int64)
    for t in range(T):
        for i in range(N):
            k = int(np.clip(np.floor((i + amp * t / (T - 1)) * M / N), 0, M - 1))
            if t < fb and k == M - 1:
                k = M - 2
            if t < fa and k == M - 2:
                k = M - 3
            cls[t, i] = k
            emb[t, i] = proto[k] + walk[t] + 0.35 * rng.standard_normal(C)
    return emb.astype(np.float32), cls, (fa, fb)


def nov_bound(C):
    """|nov - its fp64 value|: `oracle.topk_score_bound(C, 1.0)` -- the dot product of two unit vectors summed in fp32 in any order,
    (C + 2) 2^-24 (the two roundings it grants the division by temp cover the subtraction from 1: |1 - d| <= 2)"""
    return oracle.topk_score_bound(C, 1.0)


def score_bound(C, top):
    """|s - its fp64 value|: the mean of the `top` largest is 1-Lipschitz in the sup norm (nov_bound), plus the roundings of `top`
    additions and one division on values in [0, 2]: each at most 2 u relative to a partial mean <= 2 -> 2 (top + 1) 2^-24"""
    return (C + 2 + 2 * (top + 1)) * U


def violations(ehat, cxt, radius, top, origin, first_frame, nov, score, ref=None):
    """(nov, score) of frames first_frame .. against the fp64 definition -> dict of violation counts (all zero = passes).
      shape ... nov [T - first_frame, N], score [T - first_frame]
      nov ..... entries further than nov_bound(C) from the definition (NaN counts)
      score ... entries further than score_bound(C, top) from the definition's score
    ref: (nov, s) of the fp64 definition when the caller has them already"""
    as_np = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    ehat, nov, score = as_np(ehat), as_np(nov), as_np(score)
    T, N, C = ehat.shape
    top = default_top(N) if top is None else top
    out = dict(shape=0, nov=0, score=0)
    if nov.shape != (T - first_frame, N) or score.shape != (T - first_frame,):
        out["shape"] = 1
        return out
    n64, s64 = ref if ref is not None else reference(ehat, cxt, radius, top, origin, first_frame)
    out["nov"] = int((~(np.abs(nov.astype(np.float64) - n64) <= nov_bound(C))).sum())
    out["score"] = int((~(np.abs(score.astype(np.float64) - s64) <= score_bound(C, top))).sum())
    return out


def reference(ehat, cxt, radius, top, origin, first_frame=1):
    """(nov, s) of the fp64 definition"""
    as_np = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    ehat = as_np(ehat)
    n64 = novelty_fast(ehat, cxt, radius, None if origin is None else as_np(origin), first_frame, np.float64)
    return n64, frame_scores(n64, top, np.float64)
