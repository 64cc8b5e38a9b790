"""Anchor marks in the lists of the sliding entry points (include/crw_hip.h) in numpy -- what
`crw_hip.mark_anchors` is held to, and the literal loop "gather over marked lists" that `anchored_ref.gather_anchored` equals.

A mark: the slot-0 weight of node q of frame f is EXACTLY -inf (bits 0xFF800000); the node's class is its slot-0 index clamped into
[0, M - 1]; the other slots of that list are ignored.  `anchored_ref` holds the definition of anchored propagation itself; nothing
of it is restated here.  Also here: the extra shapes and anchor patterns of tests/test_anchor_lists*.py."""
import numpy as np

import anchored_ref as ar
import sliding_ref as sr

ANCHOR_BITS = 0xFF800000

# (T, N, C, M, cxt, radius, knn) beside `anchored_ref.SHAPES` -- the smallest that can break the marks' own code:
#   T = 2: one propagated frame, the ring holds one slot
#   knn = 1: slot 0 is the only slot, every padding register re-reads it; cxt = 2, T = 9 > 2 (cxt + 1) + 1: the ring wraps twice
#   knn = 9: not a multiple of the 8 / 16 / 24 register instances; N * M = 55: the last lane of the one compute wave is clamped
EXTRA_SHAPES = ((2, 7, 8, 3, 4, 3, 3), (9, 5, 8, 3, 2, 3, 1), (16, 11, 8, 5, 3, 4, 9))


def mark(W, I, anchor, M, first_frame=1):
    """-> marked COPIES (W, I) of the lists [F, knn, N] (or [G, F, knn, N]) of frames first_frame ..: slot 0 only, frames before
    first_frame ignored, a value outside [0, M) leaves the node free."""
    W, I = np.array(W, np.float32), np.array(I, np.int32)
    F = W.shape[-3]
    a = np.asarray(anchor).astype(np.int64)[first_frame:first_frame + F]
    v = ar.clamped(a, M)
    for f, q in zip(*np.nonzero(v)):
        W[..., f, 0, q] = -np.inf
        I[..., f, 0, q] = a[f, q]
    return W, I


def is_mark(W):
    """[..., knn, N] weights -> [..., N] bool: the slot-0 weight has exactly the mark's bits"""
    return np.ascontiguousarray(np.asarray(W, np.float32)[..., 0, :]).view(np.uint32) == ANCHOR_BITS


def gather_marked(seed, W, I, M, cxt, first_frame=1, L_init=None, pred_init=None, dtype=np.float32):
    """The literal loop over MARKED lists (I untranslated, as the entry point takes it): a marked node's row is the one-hot of its
    clamped slot-0 index, every other row the sliding rule's sum in neighbour order from 0 -> (L [T*N, M], pred [N, T])."""
    F, knn, N = W.shape
    T = first_frame + F
    R = sr.rows(I, N, cxt, first_frame).astype(np.int64)
    marks = is_mark(W)
    L = np.zeros((T * N, M), dtype) if L_init is None else np.array(L_init, dtype)
    pred = np.zeros((N, T), np.float32) if pred_init is None else np.array(pred_init, np.float32)
    if seed is not None:
        L[:N] = ar.onehot(seed, M, dtype)
        pred[:, 0] = seed
    for n in range(first_frame, T):
        f = n - first_frame
        for q in range(N):
            if marks[f, q]:
                row = ar.onehot(np.array([min(max(int(I[f, 0, q]), 0), M - 1)]), M, dtype)[0]
            else:
                row = np.zeros(M, dtype)
                for j in range(knn):
                    row = row + L[min(max(int(R[f, j, q]), 0), n * N - 1)] * dtype(W[f, j, q])
            L[n * N + q] = row
            pred[q, n] = row.argmax()
    return L, pred


def extra_patterns(T, N, M, cxt, seed=1):
    """The anchor positions `anchored_ref.patterns` leaves out: name -> (anchor [T, N] int8, first_frame)."""
    rng = np.random.default_rng(seed)
    free = lambda: np.full((T, N), ar.FREE, np.int8)
    out = {}
    if cxt + 1 < T:
        a = free()
        a[cxt + 1] = rng.integers(0, M, N)
        out["frame cxt + 1, the last one before the window slides"] = (a, 1)
    a = free()
    a[1:, 0] = 0
    out["node 0 only, class 0, every frame"] = (a, 1)
    a = free()
    a[1:, N - 1] = M - 1
    out["node N - 1 only, class M - 1, every frame"] = (a, 1)
    a = free()
    a[T - 1, 0], a[T - 1, N - 1] = M - 1, 0
    out["the two end nodes of frame T - 1"] = (a, 1)
    return out


def all_patterns(T, N, M, cxt):
    """`anchored_ref.patterns` (its frames need T >= 8) and `extra_patterns`"""
    out = dict(ar.patterns(T, N, M, cxt)) if T >= 8 else {"none": (np.full((T, N), ar.FREE, np.int8), 1)}
    out.update(extra_patterns(T, N, M, cxt))
    return out
