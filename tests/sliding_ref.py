"""The 'sliding' context rule of label propagation as plain loops -- the definition the device code is held to.

For frame n the lists (W, I) are those of the reference rule (`oracle.labelprop_weights`: scores against frame 0 and frames
n - cxt .. n - 1 once n > cxt + 1); an index i addresses label row

    row(i, n) = i                          if i < N or n <= cxt + 1
                i + (n - cxt - 1) * N      otherwise

and L[n] = sum_j W[j] * L[row(I[j], n)] in neighbour order from 0, pred the first maximum.  Also here: the drifting-layer items of the
README's table, the periodic item that makes the oldest frame of the window the best match, and the one check that both the CPU and
the GPU tests apply to an (L, pred) pair -- `definition_violations`.
"""
import numpy as np

import oracle.crw_oracle as oracle

# (T, N, C, M, cxt, radius, temp, knn, amp) of the drifting-layer items
DRIFT_SHAPES = ((30, 13, 8, 3, 4, 3, 0.1, 4, 5), (40, 24, 16, 3, 6, 4, 0.05, 5, 8), (64, 48, 32, 4, 10, 5, 0.05, 10, 14))
DRIFT_SEEDS = (0, 1, 2)


def rows(I, N, cxt, first_frame=1):
    """I [F, knn, N] of frames first_frame .. -> the label rows the sliding rule reads (numpy, same dtype)."""
    I = np.asarray(I)
    n = np.arange(first_frame, first_frame + I.shape[0])
    shift = (np.maximum(n - cxt - 1, 0) * N).astype(I.dtype)[:, None, None]
    return np.where(I >= N, I + shift, I)


def gather(seed, W, R, M, first_frame=1, L_init=None, pred_init=None, dtype=np.float32, last_max=False):
    """`crw_labelprop_gather` as loops: W, R [F, knn, N] weights and ABSOLUTE label rows -> (L [T*N, M], pred [N, T]); the sum runs
    in neighbour order from 0 in `dtype` (products rounded, then added: no fused multiply-add).  last_max: a planted defect."""
    F, knn, N = W.shape
    T = first_frame + F
    L = np.zeros((T * N, M), dtype) if L_init is None else np.array(L_init, dtype)
    pred = np.zeros((N, T), np.float32) if pred_init is None else np.array(pred_init, np.float32)
    if seed is not None:
        L[:N] = (np.asarray(seed)[:, None] == np.arange(M)[None]).astype(dtype)
        pred[:, 0] = seed
    for n in range(first_frame, T):
        p = np.zeros((N, M), dtype)
        for j in range(knn):
            p = p + L[R[n - first_frame, j]] * W[n - first_frame, j].astype(dtype)[:, None]
        L[n * N:(n + 1) * N] = p
        pred[:, n] = (M - 1 - p[:, ::-1].argmax(-1)) if last_max else p.argmax(-1)
    return L, pred


def labelprop_sliding(emb, seed, nclasses, cxt, radius, temp, knn, dtype=np.float32, context="sliding"):
    """`oracle.labelprop` with the indices applied to the frames they were scored on -> (pred [N, T], L [T*N, M], W, I) -- W, I the
    reference rule's lists [T-1, knn, N] (I untranslated).  context='reference': `oracle.labelprop` itself, through the same loop."""
    T, N, _ = emb.shape
    ehat = oracle.l2_normalize(emb, dtype).astype(dtype)
    Ws, Is = [], []
    for n in range(1, T):
        W, I = oracle.labelprop_weights(ehat, n, cxt, radius, temp, knn, dtype)
        Ws.append(W)
        Is.append(I)
    W, I = np.stack(Ws), np.stack(Is)
    R = rows(I, N, cxt) if context == "sliding" else I
    L, pred = gather(seed, W, R, nclasses, dtype=dtype)
    return pred, L, W, I


def drifting_item(seed, T, N, C, M, amp):
    """Layered item whose class boundaries drift by `amp` nodes along the item: -> (emb [T, N, C] float32, cls [T, N] int)."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((M, C))
    walk = rng.standard_normal((T, C)).cumsum(0) * 0.15
    emb = np.empty((T, N, C))
    cls = np.empty((T, N), np.int64)
    for t in range(T):
        for i in range(N):
            k = int(np.clip(np.floor((i - amp * t / (T - 1)) * M / N), 0, M - 1))
            cls[t, i] = k
            emb[t, i] = proto[k] + walk[t] + 0.35 * rng.standard_normal(C)
    return emb.astype(np.float32), cls


def late_errors(pred, cls, cxt):
    """(wrong labels, labels) among the frames n >= cxt + 2 -- the only ones the two rules can differ on."""
    late = slice(cxt + 2, None)
    return int((pred.T[late] != cls[late]).sum()), int(cls[late].size)


def periodic_item(seed, T, N, C, period, noise=0.02):
    """Features that repeat along-track with `period` (plus noise): frame n's best match is frame n - period, and with period = cxt
    that is the OLDEST frame of the sliding window -- the one a ring of cxt slots would be overwriting."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((period, N, C))
    return np.stack([base[t % period] + noise * rng.standard_normal((N, C)) for t in range(T)]).astype(np.float32)


def oldest_top_fraction(I, N, cxt, first_frame=1):
    """Share of the late queries (n > cxt + 1) whose TOP neighbour lies in frame n - cxt (list frame 1)."""
    I = np.asarray(I)
    n = np.arange(first_frame, first_frame + I.shape[0])
    late = I[n > cxt + 1, 0]
    return float(((late >= N) & (late < 2 * N)).mean()) if late.size else 0.0


def definition_violations(gather_fn, seed, W, R, M, first_frame, L, pred, L_init=None, pred_init=None):
    """The check of every sliding test, CPU and GPU: (L, pred) against the definition on the translated rows R.
      * bit equality with `gather_fn(seed, W, R, L_init, pred_init) -> (L, pred)` -- the general gather on translated lists;
      * `oracle.gather_audit(W, R, seed, M, first_frame, None, L, pred)`: (knn + 2) * 2^-24 teacher-forced, structure exact.
    -> dict of violation counts (all zero = passes)."""
    Lr, pr = gather_fn(seed, W, R, L_init, pred_init)
    as_np = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    Ln, pn, Lrn, prn = as_np(L), as_np(pred), as_np(Lr), as_np(pr)
    out = dict(bits_L=int((Ln.view(np.uint32) != Lrn.view(np.uint32)).sum()), bits_pred=int((pn != prn).sum()))
    audit = oracle.gather_audit(W, R, seed, M, first_frame, None, L, pred, L_init=L_init, pred_init=pred_init)
    out.update({"audit_" + k: v for k, v in audit["violations"].items()})
    return out
