"""The definition of the depth-ordered label map (include/crw_hip.h, crw_labelmap_ordered) restated over fp64 probabilities
(`dense_ref.probabilities`): plain loops over rows and states, every column at once; it shares no code with
`crw_hip._labelmap_ordered_cpu` or the kernel.  Also here: `check`, the three properties every ordered map must have, the bound it
uses (DESIGN.md section 3 derives it), and the synthetic layered items of the quality tests.  Shared by test_ordered.py and
test_ordered_gpu.py; a reference is computed once per case and never modified."""
import functools

import numpy as np

import dense_ref as dr
import horizons_ref as hr


def bound(rows):
    """E(rows): how far the fp32 score of ANY monotone path (a left fold of rounded adds over computed probabilities) can lie from
    its fp64 score.  rows * B: every interpolated probability is within B of its fp64 value.  The add at row r (1 ... rows - 1)
    rounds a partial sum <= r + 1 + E: at most 2^-24 (r + 1 + E) off, in all 2^-25 (rows^2 + rows - 2) + 2^-24 rows E <=
    2^-25 (rows^2 + 2 rows) while E <= 1/2 (rows <= 4000).  fp32 addition is monotone, so the fp32 DP returns a path whose fp32
    score is the largest of all paths': its fp64 score is within 2 E of the fp64 optimum."""
    E = rows * dr.B + (rows * rows + 2 * rows) * 2.0 ** -25
    assert E <= 0.5
    return E


def decode(probs, order):
    """probs [M, rows, cols] fp64 -> (labels int64 [rows, cols], score fp64 [cols]): the recurrence, the tie rules and the
    backtrack of the definition, state by state, row by row."""
    order = [int(k) for k in order]
    S = len(order)
    _, rows, cols = probs.shape
    e = np.stack([probs[k] for k in order])  # [S, rows, cols]
    D = [e[s, 0].copy() for s in range(S)]
    pred = np.zeros((rows, S, cols), dtype=np.int64)
    for r in range(1, rows):
        best, arg = D[0].copy(), np.zeros(cols, dtype=np.int64)
        new = []
        for s in range(S):
            if s > 0:
                up = D[s] > best  # strict: the lowest s' that attains the prefix maximum
                best, arg = np.where(up, D[s], best), np.where(up, s, arg)
            pred[r, s] = arg
            new.append(e[s, r] + best)
        D = new
    score, state = D[0].copy(), np.zeros(cols, dtype=np.int64)
    for s in range(1, S):
        up = D[s] > score  # strict: the lowest final state
        score, state = np.where(up, D[s], score), np.where(up, s, state)
    labels = np.empty((rows, cols), dtype=np.int64)
    cols_i = np.arange(cols)
    for r in range(rows - 1, 0, -1):
        labels[r] = np.asarray(order)[state]
        state = pred[r, state, cols_i]
    labels[0] = np.asarray(order)[state]
    return labels, score


@functools.lru_cache(maxsize=None)
def reference(shape, order, seed=0):
    """`dense_ref.reference(shape)`'s Dirichlet case under `order` (a tuple) -> (L, Ref, labels, score), computed once."""
    L, ref = dr.reference(shape, seed)
    labels, score = decode(ref.probs, order)
    labels.setflags(write=False), score.setflags(write=False)
    return L, ref, labels, score


def positions(labels, order):
    """labels [rows, cols] of classes 0 ... 15 -> the position of every label in `order` (-1: not in it)."""
    pos = np.full(16, -1, dtype=np.int64)
    pos[np.asarray(order)] = np.arange(len(order))
    return pos[labels]


def changes(labels):
    """Class changes down every column -> [cols]."""
    labels = np.asarray(labels)
    return (labels[1:] != labels[:-1]).sum(0)


def check(ref_probs, labels, order, score=None, what=""):
    """The three properties of an ordered map `labels` [rows, cols] against the fp64 probabilities [M, rows, cols] (unflipped).
    Feasibility: every label is in `order`, its position never decreases down a column.  Optimality gap: the fp64 score of the
    map's path is within 2 E(rows) of the fp64 optimum (`score`, computed here when not given).  Sanity: in a column whose fp64
    arg-max labels are already monotone in `order` and whose every top-two gap exceeds 2 E(rows), the map IS the arg-max map.
    Prints the worst gap next to the bound before it asserts."""
    labels = np.asarray(labels).astype(np.int64)
    M, rows, cols = ref_probs.shape
    order = [int(k) for k in order]
    assert labels.shape == (rows, cols)
    assert np.isin(labels, order).all(), f"{what}: a label outside order {order}"
    pos = positions(labels, order)
    assert (pos[1:] >= pos[:-1]).all(), f"{what}: a column steps back in order {order}"
    if score is None:
        score = decode(ref_probs, order)[1]
    mine = np.take_along_axis(ref_probs, labels[None], 0)[0].sum(0)
    gap, tol = float((score - mine).max()), 2 * bound(rows)
    s = np.sort(ref_probs, axis=0)
    argmax = ref_probs.argmax(0)
    apos = positions(argmax, order)
    clear = (apos >= 0).all(0) & (apos[1:] >= apos[:-1]).all(0) & ((s[-1] - s[-2]) > tol).all(0)
    print(f"{what}: order {order}, worst optimality gap {gap:.3e} (bound {tol:.3e}), smallest {float((score - mine).min()):.3e}; "
          f"{int(clear.sum())} of {cols} columns are monotone and clear in the arg-max map, at most {int(changes(labels).max())} changes")
    assert gap <= tol and float((score - mine).min()) >= -1e-9  # nothing beats the optimum (fp64 summation noise aside)
    assert np.array_equal(labels[:, clear], argmax[:, clear]), f"{what}: a clear monotone column was changed"


def layered_case(T, N, rows, cols, temp, M, share, seed):
    """A synthetic layered item -> (gt [rows, cols], L float32 [T*N, M]): M - 1 curved boundaries, sigmoid soft labels at the
    nodes, and a `share` of the nodes (never of frame 0) with a WRONG row: its own, rotated."""
    g = np.random.default_rng(seed); K = M - 1
    bs = [lambda c, k=k: (k + 1) / (K + 1) * rows + 0.06 * rows * np.sin(3 * c / cols + k) + 0.05 * rows * c / cols for k in range(K)]
    r, c = np.arange(rows, dtype=np.float64)[:, None], np.arange(cols, dtype=np.float64)[None, :]
    gt = sum((r > b(c)).astype(np.int64) for b in bs)
    nr = ((np.arange(N) + 0.5) * rows / N - 0.5)[None, :]; nc = ((np.arange(T) + 0.5) * cols / T - 0.5)[:, None]
    s = [1 / (1 + np.exp(-(nr - b(nc)) / (temp * rows / N))) for b in bs]
    L = np.stack([np.prod([s[j] if j < k else 1 - s[j] for j in range(K)], 0) for k in range(M)], -1)
    L /= L.sum(-1, keepdims=True)
    bad = g.random((T, N)) < share; bad[0] = False; sh = g.integers(1, M, size=(T, N)); out = L.copy()
    for t, n in zip(*np.nonzero(bad)): out[t, n] = np.roll(L[t, n], sh[t, n])   # a wrong node: its row rotated
    return gt, out.reshape(T * N, M).astype(np.float32)


# (T, N, rows, cols, temp, M, share)
QUALITY = [(12, 10, 83, 84, 0.5, 3, 0.06), (8, 12, 50, 64, 1.0, 4, 0.08), (30, 24, 200, 300, 0.5, 4, 0.05)]
SEEDS = (0, 1, 2)


def top_mae(gt, labels, M, min_run):
    """Mean over the classes 1 ... M - 1 of the mean |top pick of `labels` - top pick of gt| (rows) over the columns in which
    both maps have the class (`horizons_ref.picks_of`; the ground truth at min_run 1)."""
    pg, pl = hr.picks_of(np.asarray(gt), M, 1), hr.picks_of(np.asarray(labels).astype(np.int64), M, min_run)
    maes = []
    for k in range(1, M):
        both = (pg[2, k] > 0) & (pl[2, k] > 0)
        if both.any():
            maes.append(float(np.abs(pl[0, k, both].astype(np.int64) - pg[0, k, both]).mean()))
    return float(np.mean(maes))


def check_quality(gt, dense, ordered, M, what=""):
    """Item 7's three assertions for one case's two maps; prints the counts first -> (wrong dense, wrong ordered, MAE dense at
    min_run 3, MAE ordered at min_run 1)."""
    gt, dense, ordered = (np.asarray(a).astype(np.int64) for a in (gt, dense, ordered))
    wd, wo = int((dense != gt).sum()), int((ordered != gt).sum())
    md1, md3, mo = top_mae(gt, dense, M, 1), top_mae(gt, dense, M, 3), top_mae(gt, ordered, M, 1)
    print(f"{what}: wrong pixels arg-max {wd} -> ordered {wo} of {gt.size}; mean top-MAE arg-max min_run=1 {md1:.2f} -> min_run=3 "
          f"{md3:.2f} -> ordered min_run=1 {mo:.2f} rows; changes per column arg-max {changes(dense).mean():.2f}, ordered max "
          f"{int(changes(ordered).max())}")
    assert wo <= 0.75 * wd
    assert mo <= 0.75 * md3
    assert (changes(ordered) <= M - 1).all()
    return wd, wo, md3, mo
