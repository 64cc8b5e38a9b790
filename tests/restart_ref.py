"""anchor_context='restart' as plain loops -- the definition `crw_hip.labelprop_topk(origin=)` / `labelprop_gather(origin=)` and the
entry points of include/crw_hip_restart.h are held to.

A frame is an ORIGIN when it is frame 0, or when all N of its nodes are clamped by the anchors (frames before first_frame are never
clamped).  For frame n let a = origin[n] be the latest origin < n and n' = n - a: frame n is propagated as frame n' of the item that
starts at a.
  lists .. `oracle.labelprop_weights` of frame n' on the sub-item ehat[a:]: the keys are frame a followed by frames
           max(a + 1, n - cxt) .. n - 1;
  rows ... index i addresses label row a N + i if i < N or n' <= cxt + 1, else a N + i + (n' - cxt - 1) N;
  sum .... `anchored_ref.gather_anchored` on those absolute rows (products rounded, added in neighbour order from 0, the first
           maximum wins, anchored rows one-hot before the next frame reads them).
Also here: the construction by cutting the item at every origin (`cut`), the anchor patterns every test runs (`patterns`), the
planted defects (`DEFECTS`, through `propagate(defect=)`) and the ONE checker of the CPU and the GPU tests (`violations`)."""
import numpy as np

import anchored_ref as ar
import oracle.crw_oracle as oracle
import sliding_ref as sr

DEFECTS = ("memory_frame0",          # the long-term frame stays frame 0
           "window_before_origin",   # the window reaches before the origin
           "late",                   # the restart comes one frame late
           "partial_restarts",       # a partially anchored frame restarts
           "rows_n")                 # rows are translated with n instead of n'


def origins(anchor, M, first_frame=1, partial=False):
    """origin [T] int32: origin[n] the latest origin < n, origin[0] = 0.  partial: the planted defect 'partial_restarts'."""
    c = ar.clamped(anchor, M)
    full = c.any(1) if partial else c.all(1)
    full[:max(first_frame, 1)] = False
    full[0] = True
    out = np.zeros(len(full), np.int32)
    for n in range(1, len(full)):
        out[n] = n - 1 if full[n - 1] else out[n - 1]
    return out


def chain_rule_ok(origin):
    o = [int(x) for x in origin]
    return all(0 <= o[n] < n and (n == 1 or o[n] in (o[n - 1], n - 1)) for n in range(1, len(o)))


def stretches(origin, first_frame=1):
    """[(a, e)]: frames a + 1 .. e (those >= first_frame) share the origin a."""
    out = []
    for n in range(max(first_frame, 1), len(origin)):
        if out and out[-1][0] == origin[n]:
            out[-1][1] = n
        else:
            out.append([int(origin[n]), n])
    return [tuple(x) for x in out]


def _frame_lists(ehat, n, key_frames, radius, temp, knn):
    """(W, I, V [knn, N]) of frame n scored against the explicit key frames, I on that key list, in the device's layout (empty slots
    W = 0, I = 0, V = -inf): `oracle.labelprop_lists` on the item [key frames, frame n] with no truncation."""
    sub = np.concatenate([ehat[list(key_frames)], ehat[n:n + 1]])
    W, I, V = oracle.labelprop_lists(sub, len(sub), radius, temp, knn, first_frame=len(key_frames))
    return W[0], I[0], V[0]


def lists_restart(emb, cxt, radius, knn, temp, origin, first_frame=1, defect=None):
    """-> (W, I, R, V), each [T - first_frame, knn, N]: the lists of the rule, I as the device writes it (on the sub-item's truncated
    key list), R the ABSOLUTE label rows, V the selected logits.  Per frame `oracle.labelprop_lists` on the sub-item ehat[a:n + 1]."""
    assert defect is None or defect in DEFECTS
    T, N, _ = emb.shape
    ehat = oracle.l2_normalize(emb, np.float32).astype(np.float32)
    Ws, Is, Rs, Vs = [], [], [], []
    for n in range(first_frame, T):
        a = int(origin[n])
        npr = n - a
        if defect == "window_before_origin" and a > 0:
            keys = [a] + list(range(max(1, n - cxt), n))                     # today's window, whatever lies before the origin
            keys = [keys[0]] + [k for k in keys[1:] if k != a]
            W, I, V = _frame_lists(ehat, n, keys, radius, temp, knn)
            R = np.asarray(keys)[I // N] * N + I % N
        else:
            W, I, V = (x[0] for x in oracle.labelprop_lists(ehat[a:n + 1], cxt, radius, temp, knn, first_frame=npr))
            m = n if defect == "rows_n" else npr
            R = a * N + np.where((I < N) | (m <= cxt + 1), I, I + (m - cxt - 1) * N)
            R = np.minimum(R, n * N - 1)                                     # (a defect must not read a frame that does not exist yet)
            if defect == "memory_frame0":
                R = np.where(I < N, I, R)
        Ws.append(W), Is.append(I), Rs.append(R.astype(np.int32)), Vs.append(V)
    return np.stack(Ws), np.stack(Is).astype(np.int32), np.stack(Rs), np.stack(Vs)


def key_frames(n, a, cxt):
    """the frames frame n scores against, in list order"""
    return [a] + list(range(max(a + 1, n - cxt), n))


def propagate(emb, seed, M, cxt, radius, knn, temp, anchor, first_frame=1, L_init=None, pred_init=None, defect=None):
    """The definition end to end -> (L, pred, W, R, origin).  defect: one of DEFECTS, planted for the checker's own test."""
    origin = origins(anchor, M, first_frame, partial=defect == "partial_restarts")
    if defect == "late":
        origin = np.concatenate([[0, 0], origin[1:-1]]).astype(np.int32)
    W, _, R, _ = lists_restart(emb, cxt, radius, knn, temp, origin, first_frame, defect)
    L, pred = ar.gather_anchored(seed, W, R, M, anchor, first_frame, L_init, pred_init)
    return L, pred, W, R, origin


def cut(emb, seed, M, cxt, radius, knn, temp, anchor, first_frame=1, L_init=None, pred_init=None):
    """The construction the definition equals bit for bit: the item cut at every origin, each piece propagated by the CLAMP-mode
    definition (`anchored_ref.gather_anchored` on `sliding_ref.rows` of the piece's own lists) as an item of its own -- frame a is the
    piece's frame 0 and what the piece before left there (the seed for the first piece when it starts at frame 0)."""
    T, N, _ = emb.shape
    ehat = oracle.l2_normalize(emb, np.float32).astype(np.float32)
    origin = origins(anchor, M, first_frame)
    L = np.zeros((T * N, M), np.float32) if L_init is None else np.array(L_init, np.float32)
    pred = np.zeros((N, T), np.float32) if pred_init is None else np.array(pred_init, np.float32)
    if seed is not None:
        L[:N] = ar.onehot(seed, M)
        pred[:, 0] = seed
    for a, e in stretches(origin, first_frame):
        ff = max(first_frame - a, 1)
        W, I, _ = oracle.labelprop_lists(ehat[a:e + 1], cxt, radius, temp, knn, first_frame=ff)
        Ls, ps = ar.gather_anchored(None, W, sr.rows(I, N, cxt, ff), M, anchor[a:e + 1], ff, L[a * N:(e + 1) * N], pred[:, a:e + 1])
        L[(a + ff) * N:(e + 1) * N], pred[:, a + ff:e + 1] = Ls[ff * N:], ps[:, ff:]
    return L, pred


def patterns(T, N, M, cxt, seed=0):
    """The anchor patterns of one shape: name -> (anchor [T, N] int8, first_frame).  Anchored classes are random, so a clamp shows."""
    rng = np.random.default_rng(seed + 17)
    free = lambda: np.full((T, N), ar.FREE, np.int8)
    full = lambda: rng.integers(0, M, N).astype(np.int8)

    def at(frames, first_frame=1):
        a = free()
        for f in frames:
            a[f] = full()
        return a, first_frame

    def partial(a, frames):
        for f in frames:
            nodes = rng.permutation(N)[:max(1, N // 3)]
            a[f] = ar.FREE
            a[f, nodes] = rng.integers(0, M, nodes.size)
        return a

    out = {"none": (free(), 1), "a full frame at 1": at([1]), "a full frame at T - 1": at([T - 1]),
           "two consecutive full frames": at([T // 2, T // 2 + 1])}
    if cxt + 2 < T - 1:
        out["a full frame at cxt + 2"] = at([cxt + 2])
    if 2 + cxt + 3 < T:
        out["a restart at 2, after which the window slides again"] = at([2])
    out["every frame full"] = at(range(T))
    out["partial rows only"] = (partial(free(), (2, T // 2, T - 2)), 1)
    a, _ = at([3, T - 4])
    out["partial rows between full frames"] = (partial(a, (5, T - 5 if T - 5 > 5 else 6)), 1)
    a, _ = at([3, T - 3])
    a[5] = np.resize(np.array([M, 127, -128, -2, M + 1], np.int8), N)
    a[T - 3, ::2] = np.resize(np.array([-128, M, 127], np.int8), a[T - 3, ::2].size)     # no longer full: clamps, restarts nothing
    out["a frame of out-of-range values"] = (a, 1)
    a, _ = at([1, 2, 4, T - 2])
    out["first_frame 3, no seed: full frames 1 - 2 ignored"] = (a, 3)
    return out


def item(shape):
    """the features of one shape of `anchored_ref.SHAPES`, as tests/test_anchored_gpu.py draws them (numpy)"""
    import torch
    T, N, C = shape[:3]
    g = torch.Generator().manual_seed(sum(shape))
    return (torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).numpy()


def violations(seed, W, R, M, anchor, first_frame, L, pred, L_init=None, pred_init=None, ref=None):
    """(L, pred) against the definition: W, R are the DEFINITION's lists and absolute rows (`lists_restart`, or the device's own
    lists translated by the rule), ref the cut construction.  `anchored_ref.violations`: bit equality with ref, free rows within
    `oracle.gather_bound(knn)` of the fp64 sum teacher-forced on the pair's own earlier rows, clamped rows one-hot, pred the first
    maximum, frame 0 the seed, frames before first_frame untouched -> dict of violation counts (all zero = passes)."""
    return ar.violations(seed, W, R, M, anchor, first_frame, L, pred, L_init, pred_init, ref)


def rows_of(I, origin, N, cxt, first_frame=1):
    """the rule's translation of device lists I [F, knn, N] -> absolute rows (numpy)"""
    I = np.asarray(I).astype(np.int64)
    n = np.arange(first_frame, first_frame + I.shape[0])
    a = np.asarray(origin).astype(np.int64)[n]
    shift = (np.maximum(n - a - cxt - 1, 0) * N)[:, None, None]
    return (a * N)[:, None, None] + np.where(I >= N, I + shift, I)
