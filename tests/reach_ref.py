"""Accuracy against the distance from the nearest labelled trace, as plain Python loops over pixels: the rule of
include/crw_hip_reach.h (`confusion_grouped`), `crw_hip.column_groups` (`column_groups`), a builder of layered maps with speckle and
planted invalid labels, ignore labels and bad confidences (`case`), and the drifting items' node maps under the two context rules
(`drift_maps`, computed once per process).  No GPU, no torch."""
import functools
import math

import numpy as np

import oracle.crw_oracle as orc
import sliding_ref as slr

DEFAULT_EDGES = (1, 2, 3, 5, 9, 17, 33, 65, 129, 257)


def column_groups(cols, labelled, step, edges=None, segments=None, direction="both"):
    """-> (group [cols] uint8, frames [cols] int64; -1: no admissible labelled column)"""
    edges = list(DEFAULT_EDGES if edges is None else edges)
    segments = [0, cols] if segments is None else list(segments)
    group, frames = np.zeros(cols, np.uint8), np.zeros(cols, np.int64)
    for c in range(cols):
        s = max(i for i in range(len(segments) - 1) if segments[i] <= c)
        best = None
        for l in labelled:
            if not segments[s] <= l < segments[s + 1]:
                continue
            if (direction == "forward" and l > c) or (direction == "backward" and l < c):
                continue
            best = abs(c - l) if best is None else min(best, abs(c - l))
        if best is None:
            group[c], frames[c] = len(edges) + 1, -1
        else:
            f = -(-best // step)
            group[c], frames[c] = sum(1 for e in edges if e <= f), f
    return group, frames


def _code(v):
    """a label's integer, or None for one that is no integer (NaN, 1.5, 1e30): equals no ignore label, fits no bin"""
    v = float(v)
    if v != v or abs(v) > 16777216.0 or v != math.floor(v):
        return None
    return int(v)


def confusion_grouped(gt, pred, K, col_group, groups, conf=None, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1):
    """-> (counts [groups, K, K] int64, conf_sum [groups] float64 (None without conf), dropped [4] int64)"""
    rows, cols = gt.shape
    counts, dropped = np.zeros((groups, K, K), np.int64), np.zeros(4, np.int64)
    sums = [[] for _ in range(groups)]
    G, P = gt.tolist(), pred.tolist()
    A = None if aux is None else aux.tolist()
    C = None if conf is None else conf.tolist()
    grp = [int(v) for v in col_group]
    for r in range(rows):
        for c in range(cols):
            if grp[c] >= groups:
                dropped[3] += 1
                continue
            g, p = _code(G[r][c]), _code(P[r][c])
            a = None if A is None else _code(A[r][c])
            if (ignore_gt >= 0 and g == ignore_gt) or (ignore_pred >= 0 and p == ignore_pred) or (ignore_aux >= 0 and a == ignore_aux):
                dropped[0] += 1
            elif g is None or p is None or not (0 <= g < K and 0 <= p < K):
                dropped[1] += 1
            elif C is not None and not (0.0 <= C[r][c] <= 1.0):        # NaN fails both
                dropped[2] += 1
            else:
                counts[grp[c], g, p] += 1
                if C is not None:
                    sums[grp[c]].append(C[r][c])
    conf_sum = None if conf is None else np.array([math.fsum(s) for s in sums], np.float64)   # the exact sum, rounded once
    return counts, conf_sum, dropped


F32_INVALID, I8_INVALID, BAD_CONF = (float("nan"), -1.0, None, 1.5), (-1, None), (float("nan"), 1.5, -0.1)   # None: K


def case(rows, cols, K, seed, dg="f32", dp="f32", da=None, conf=False, ignore=False, plant=True):
    """Layered maps with speckle -> dict(gt, pred, aux, conf: numpy [rows, cols] or None; ignore_gt / ignore_pred / ignore_aux).
    gt: K layers whose borders undulate along the columns; pred: the same layers moved by a column-dependent offset, 3 % of the
    pixels a random class.  Planted (`plant`): labels that are invalid in their dtype in both maps -- NaN, -1, K and 1.5 in fp32,
    -1 and K in int8 --; with `ignore`: ignore_gt = K - 1 (a class), ignore_pred = K + 1 planted into pred; with aux: ignore_aux = 4
    planted as a block and as single pixels; with conf: fp32 in [0, 1] with exact 0s and 1s, and NaN, 1.5 and -0.1 planted.  Some of
    what is planted lands on masked pixels on purpose: the order of the rule's tests shows there."""
    rng = np.random.default_rng(seed)
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    layer = lambda shift: np.clip(np.floor((r + shift) * K / max(rows, 1)), 0, K - 1).astype(np.int64)
    gt = layer(0.08 * rows * np.sin(c / 17.0))
    pred = layer(0.08 * rows * np.sin(c / 17.0) + 0.05 * rows * np.cos(c / 5.0))
    speckle = rng.random((rows, cols)) < 0.03
    pred = np.where(speckle, rng.integers(0, K, (rows, cols)), pred)
    P = rows * cols
    spots = lambda n: (rng.integers(0, rows, min(n, P)), rng.integers(0, cols, min(n, P)))

    def typed(m, dt):
        out = m.astype(np.float32 if dt == "f32" else np.int8)
        if plant:
            bad = F32_INVALID if dt == "f32" else I8_INVALID
            rr, cc = spots(2 * len(bad))
            for i in range(len(rr)):
                v = bad[i % len(bad)]
                out[rr[i], cc[i]] = K if v is None else v
        return out

    out = dict(gt=typed(gt, dg), pred=typed(pred, dp), aux=None, conf=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1)
    if ignore:
        out["ignore_gt"], out["ignore_pred"] = K - 1, K + 1
        rr, cc = spots(5)
        out["pred"][rr, cc] = K + 1
    if da is not None:
        aux = rng.integers(0, 4, (rows, cols))
        aux[rows // 3:rows // 3 + max(rows // 8, 1), cols // 4:cols // 4 + max(cols // 3, 1)] = 4
        rr, cc = spots(4)
        aux[rr, cc] = 4
        out["aux"], out["ignore_aux"] = aux.astype(np.float32 if da == "f32" else np.int8), 4
    if conf:
        cf = rng.random((rows, cols)).astype(np.float32)
        rr, cc = spots(6)
        cf[rr, cc] = np.array([0.0, 1.0] * 3, np.float32)[:len(rr)]
        if plant:
            rr, cc = spots(2 * len(BAD_CONF))
            cf[rr, cc] = np.array(BAD_CONF * 2, np.float32)[:len(rr)]
        out["conf"] = cf
    return out


def group_maps(cols, kind, seed=0):
    """(col_group uint8 [cols], groups) of a test: 'one' (a single group), 'default' (`column_groups` with the default edges from
    three labelled columns, frames of 4 pixel columns: 12 groups, the far ones empty at small widths), 'own' (every column its own
    group, cols <= 64), 'holes' (12 groups, three of them never used, and some columns excluded by an entry of 255 or of `groups`)"""
    rng = np.random.default_rng(seed + cols)
    if kind == "one":
        return np.zeros(cols, np.uint8), 1
    if kind == "default":
        labelled = sorted({0, cols // 3, (2 * cols) // 3})
        return column_groups(cols, labelled, 4)[0], len(DEFAULT_EDGES) + 2
    if kind == "own":
        assert cols <= 64
        return rng.permutation(64)[:cols].astype(np.uint8), 64
    assert kind == "holes"
    g = rng.choice(np.array([0, 1, 2, 4, 5, 7, 8, 10, 11], np.uint8), cols)       # 3, 6 and 9 stay empty
    g[rng.random(cols) < 0.15] = 255
    g[rng.random(cols) < 0.05] = 12
    return g, 12


@functools.lru_cache(maxsize=None)
def drift_maps():
    """The nine drifting items of `sliding_ref` -> [(T, N, M, cxt, seed, cls [N, T] int64, reference-rule pred [N, T], sliding-rule
    pred [N, T])], the node maps as `oracle.labelprop` and `sliding_ref.labelprop_sliding` give them (float32)."""
    out = []
    for (T, N, C, M, cxt, radius, temp, knn, amp) in slr.DRIFT_SHAPES:
        for seed in slr.DRIFT_SEEDS:
            emb, cls = slr.drifting_item(seed, T, N, C, M, amp)
            ps = slr.labelprop_sliding(emb, cls[0].astype(np.float32), M, cxt, radius, temp, knn)[0]
            pr = orc.labelprop(emb, cls[0].astype(np.float32), M, cxt, radius, temp, knn)
            out.append((T, N, M, cxt, seed, np.ascontiguousarray(cls.T), np.asarray(pr, np.float32), np.asarray(ps, np.float32)))
    return out
