"""The sliding rule with K long-term frames (include/crw_hip_longmem.h) as plain loops -- the definition the
device code is held to.

A call works on a virtual item of F frames whose first K frames are long-term.  For frame n >= first_frame:

    key frames   0 .. min(n, K) - 1, then max(K, n - cxt) .. n - 1          (nf = min(n, K + cxt) frames)
    row(i, n)    i                        if i < K * N or n <= K + cxt
                 i + (n - cxt - K) * N    otherwise                          (i clamped into [0, nf * N) first)

and L[n] = sum_j W[j] * L[row(I[j], n)] in neighbour order from 0 (`sliding_ref.gather` on the absolute rows).  Also here: the
campaign items of the README's bank tables, the ring layout of the one-workgroup kernel as loops, the planted defects, and the one
checker `violations` that the CPU and the GPU tests apply.
"""
import numpy as np

import oracle.crw_oracle as oracle
import sliding_ref

DEFECTS = ("long_rows_shifted", "window_overlaps_bank", "limit_cxt_plus_1", "bank_frame_in_ring", "bank_translated_as_one")


def key_frames(n, K, cxt, defect=None):
    """the frames frame n scores against, in list order"""
    if defect == "window_overlaps_bank":      # the window starts at n - cxt even where that is inside the bank
        return list(range(n)) if n <= K else list(range(K)) + list(range(max(0, n - cxt), n))
    if defect == "limit_cxt_plus_1":          # the list is cut at cxt + 1 frames, not K + cxt
        nf = min(n, cxt + 1)
        return [p if (n <= cxt + 1 or p < K) else n - cxt + (p - K) for p in range(nf)]
    return list(range(min(n, K))) + list(range(max(K, n - cxt), n))


def rows(I, N, cxt, K, first_frame=1, defect=None):
    """I [F, knn, N] of frames first_frame .. -> the label rows the rule reads (clamped into the frame's list first)."""
    I = np.asarray(I)
    out = np.empty_like(I)
    for f in range(I.shape[0]):
        n = first_frame + f
        i = np.clip(I[f], 0, min(n, K + cxt) * N - 1)
        if defect == "long_rows_shifted":
            out[f] = i + max(n - cxt - K, 0) * N
        elif defect == "bank_translated_as_one":        # (kept below the frame's own rows: the defect reads wrong labels, not none)
            out[f] = np.minimum(np.where((i >= N) & (n > cxt + 1), i + (n - cxt - 1) * N, i), n * N - 1)
        else:
            out[f] = np.where((i >= K * N) & (n > K + cxt), i + (n - cxt - K) * N, i)
    return out


def frame_lists(ehat, n, K, cxt, radius, temp, knn, dtype=np.float32, defect=None, weights_fn=None):
    """(W [knn, N], I [knn, N]) of frame n: the reference's own top-k (`oracle.labelprop_weights`, or `weights_fn` with its
    signature) on the gathered copy [key frames..., frame n], whose context bound is the copy itself -- nothing is truncated, so an
    index is a list position.  Empty slots (fewer in-band keys than knn) as the device leaves them: W = 0, I = 0."""
    keys = key_frames(n, K, cxt, defect)
    sub = np.concatenate([ehat[keys], ehat[n:n + 1]]).astype(dtype)
    W, I, V = (weights_fn or oracle.labelprop_weights)(sub, len(keys), len(keys), radius, temp, knn, dtype, 1, True)
    pad = knn - W.shape[0]
    if pad > 0:
        W, I = np.concatenate([W, np.zeros((pad, W.shape[1]), W.dtype)]), np.concatenate([I, np.zeros((pad, I.shape[1]), I.dtype)])
        V = np.concatenate([V, np.full((pad, V.shape[1]), -np.inf, V.dtype)])
    empty = V < oracle.MASK_NEG / 2 / temp
    return np.where(empty, 0, W).astype(dtype), np.where(empty, 0, I).astype(np.int32)


def lists(ehat, K, cxt, radius, temp, knn, first_frame=1, dtype=np.float32, defect=None):
    """(W, I) [F - first_frame, knn, N] of every frame n >= first_frame"""
    out = [frame_lists(ehat, n, K, cxt, radius, temp, knn, dtype, defect) for n in range(first_frame, ehat.shape[0])]
    return np.stack([w for w, _ in out]), np.stack([i for _, i in out])


def ring_gather(W, I, N, M, cxt, K, first_frame, L_init, pred_init, dtype=np.float32, defect=None):
    """The one-workgroup ring kernel's LDS layout as loops: K long-term slots followed by R = cxt + 1 ring slots, frame f < K at slot
    f and frame f >= K at K + (f - K) % R, a list position read through the running shift ((n - cxt - K) % R) wrapped once.
    defect 'bank_frame_in_ring': a frame f < K that the call computes is stored into the ring instead of its slot."""
    F = W.shape[0]
    T, R, knn = first_frame + F, cxt + 1, W.shape[1]
    L, pred = np.array(L_init, dtype), np.array(pred_init, np.float32)
    lab = np.zeros((K + R, N, M), dtype)
    for f in range(min(K, first_frame)):
        lab[f] = L[f * N:(f + 1) * N]
    for f in range(max(K, first_frame - cxt), first_frame):
        lab[K + (f - K) % R] = L[f * N:(f + 1) * N]
    for n in range(first_frame, T):
        i = np.clip(I[n - first_frame], 0, min(n, K + cxt) * N - 1)
        slot, node = i // N, i % N
        shift = (n - cxt - K) % R if n > K + cxt else 0
        moved = slot + shift
        moved = np.where(moved >= K + R, moved - R, moved)
        slot = np.where(slot >= K, moved, slot)
        p = np.zeros((N, M), dtype)
        for j in range(knn):
            p = p + lab[slot[j], node[j]] * W[n - first_frame, j].astype(dtype)[:, None]
        lab[K + (n - K) % R if (n >= K or defect == "bank_frame_in_ring") else n] = p
        L[n * N:(n + 1) * N] = p
        pred[:, n] = p.argmax(-1)
    return L, pred


def initial_labels(cls, first_frame, N, M, T, dtype=np.float32):
    """(L_init [T*N, M], pred_init [N, T]) with the one-hot rows of cls [>= first_frame, N] in the frames before first_frame"""
    L, pred = np.zeros((T * N, M), dtype), np.zeros((N, T), np.float32)
    for f in range(first_frame):
        L[f * N:(f + 1) * N] = (np.asarray(cls[f])[:, None] == np.arange(M)[None]).astype(dtype)
        pred[:, f] = cls[f]
    return L, pred


def labelprop_long(emb, cls_front, nclasses, cxt, K, radius, temp, knn, first_frame=None, dtype=np.float32, defect=None, ring=False):
    """The rule on the virtual item emb [F, N, C] (raw features) whose frames before first_frame (default K) carry the classes
    cls_front [first_frame, N] -> (pred [N, F], L [F*N, M], W, I).  ring: through `ring_gather` (the kernel's layout)."""
    F, N, _ = emb.shape
    first_frame = K if first_frame is None else first_frame
    ehat = oracle.l2_normalize(emb, dtype).astype(dtype)
    W, I = lists(ehat, K, cxt, radius, temp, knn, first_frame, dtype, defect)
    L0, p0 = initial_labels(cls_front, first_frame, N, nclasses, F, dtype)
    if ring or defect == "bank_frame_in_ring":
        L, pred = ring_gather(W, I, N, nclasses, cxt, K, first_frame, L0, p0, dtype, defect)
    else:
        L, pred = sliding_ref.gather(None, W, rows(I, N, cxt, K, first_frame, defect), nclasses, first_frame, L0, p0, dtype)
    return pred, L, W, I


def violations(ehat, W, I, L, pred, M, cxt, K, radius, temp, knn, first_frame, L_init, pred_init, lists_fn=None, gather_fn=None):
    """The check of every long-memory test, CPU and GPU: lists and labels of one call against the definition.
      * lists: (W, I) of frame n against `lists_fn(ehat, n) -> (W [knn, N], I [knn, N])`, by default `frame_lists` in fp32 -- on the
        GPU the existing top-k entry point on the gathered copy [key frames..., frame n]: bit equality;
      * labels: `sliding_ref.definition_violations` on the rows translated by the rule -- bit equality with
        `gather_fn(seed, W, R, L_init, pred_init)` on numpy lists (default: `sliding_ref.gather`) and `oracle.gather_audit`'s (knn + 2) * 2^-24;
      * the frames before first_frame untouched.
    -> dict of violation counts (all zero = passes)."""
    as_np = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    Wn, In, Ln, pn = as_np(W), as_np(I), as_np(L), as_np(pred)
    N = Wn.shape[2]
    lists_fn = lists_fn or (lambda e, n: frame_lists(as_np(e), n, K, cxt, radius, temp, knn))
    out = dict(lists_W=0, lists_I=0)
    for n in range(first_frame, first_frame + Wn.shape[0]):
        Wd, Id = (as_np(x) for x in lists_fn(ehat, n))
        out["lists_W"] += int((Wd.astype(np.float32).view(np.uint32) != Wn[n - first_frame].view(np.uint32)).sum())
        out["lists_I"] += int((Id != In[n - first_frame]).sum())
    R = rows(In, N, cxt, K, first_frame)
    gather_fn = gather_fn or (lambda seed, W_, R_, Li, pi: sliding_ref.gather(seed, W_, R_, M, first_frame, Li, pi))
    out.update(sliding_ref.definition_violations(gather_fn, None, Wn, R, M, first_frame, L, pred, L_init, pred_init))
    L0, p0 = as_np(L_init), as_np(pred_init)
    out["front_L"] = int((Ln[:first_frame * N].view(np.uint32) != L0[:first_frame * N].view(np.uint32)).sum())
    out["front_pred"] = int((pn[:, :first_frame] != p0[:, :first_frame]).sum())
    return out


def campaign_item(camp, seed, T, N, C, M, amp, up, emerging=False, off=0.0, start=0.0):
    """`sliding_ref.drifting_item` with prototypes shared by a campaign, the appearance walk started at a per-item offset and a
    per-item row offset in the class rule; emerging: class M - 1 folds into M - 2 in the first third of the item.
    -> (emb [T, N, C] float32, cls [T, N] int)."""
    proto = np.random.default_rng(1000 + camp).standard_normal((M, C))
    rng = np.random.default_rng(seed)
    walk = rng.standard_normal((T, C)).cumsum(0) * 0.15 + start * rng.standard_normal(C)
    emb = np.empty((T, N, C))
    cls = np.empty((T, N), np.int64)
    for t in range(T):
        for i in range(N):
            d = amp * t / (T - 1)
            k = int(np.clip(np.floor((i + off + (d if up else -d)) * M / N), 0, M - 1))
            if emerging and t < T // 3 and k == M - 1:
                k = M - 2
            cls[t, i] = k
            emb[t, i] = proto[k] + walk[t] + 0.35 * rng.standard_normal(C)
    return emb.astype(np.float32), cls


BANKS = {1: lambda T: [T - 1], 4: lambda T: [0, T // 3, 2 * T // 3, T - 1], 8: lambda T: list(np.linspace(0, T - 1, 8).astype(int))}
STARTS = (0.0, 0.5, 1.0)


def bank_case(shape, s, B, start, emerging):
    """One cell of the tables (every item of the cell, labelled or target, starts its appearance walk at its own draw of `start`): the virtual item [bank of B traces of the labelled item A (+ the target's own frame 0 when emerging),
    target...] -> (emb, cls_true [F, N], K, first_frame, f0): f0 the frame of the virtual item from which wrong labels are counted."""
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    ea, ca = campaign_item(7, 100 + s, T, N, C, M, 0.6 * amp, True, False, 0.5, start)
    frames = BANKS[B](T)
    if emerging:
        et, ct = campaign_item(7, s, T, N, C, M, amp, True, True, 0.0, start)
        return np.concatenate([ea[frames], et]), np.concatenate([ca[frames], ct]), B + 1, B + 1, B + T // 3
    et, ct = campaign_item(7, s, T, N, C, M, amp, False, False, 0.0, start)
    return np.concatenate([ea[frames], et]), np.concatenate([ca[frames], ct]), B, B, B


def bank_errors(shape, s, B, start, emerging, dtype=np.float64):
    """(wrong labels, labels) of one cell under the plain-loop rule"""
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    emb, cls, K, ff, f0 = bank_case(shape, s, B, start, emerging)
    pred, _, _, _ = labelprop_long(emb, cls[:ff], M, cxt, K, radius, temp, knn, ff, dtype)
    return int((pred.T[f0:] != cls[f0:]).sum()), int(cls[f0:].size)


def own_seed_errors(shape, s, start=0.0, dtype=np.float64):
    """the emerging target seeded with its own frame 0 alone, wrong labels among the frames >= T // 3"""
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    et, ct = campaign_item(7, s, T, N, C, M, amp, True, True, 0.0, start)
    pred, _, _, _ = labelprop_long(et, ct[:1], M, cxt, 1, radius, temp, knn, 1, dtype)
    return int((pred.T[T // 3:] != ct[T // 3:]).sum()), int(ct[T // 3:].size)
