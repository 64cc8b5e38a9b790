"""Aligning a memory bank to its item (include/crw_hip_align.h) as plain definitions on top of
tests/longmem_ref.py -- what the device code is held to.

CENTRING.  The raw features emb [rows, C] are cut into segments of consecutive rows by offsets 0 = b_0 <= ... <= b_S = rows; for
`propagate(memory=, memory_align='center')` these are the bank's B * N rows and the item's T * N rows (its seed frame included).

    mean[s]  = the per-channel mean over the segment's rows                              (fp64)
    y        = emb[r] - mean[s]                  (the device: the subtraction in fp64, rounded ONCE to fp32)
    ehat[r]  = y / max(|y|, 1e-12)                                                       (`oracle.l2_normalize` on y)

A one-row segment is its own mean: y = 0, ehat = the all-zero row.

BIAS.  Under the long-memory rule (longmem_ref) frame n scores against nf = min(n, K + cxt) key frames of which the first
min(n, K) are long-term.  `b` is added to the cosine of every in-band key of those: logit = (cos + b) / temp there, cos / temp on
the recent keys, masked keys stay masked.  Everything else -- selection, ties, softmax, empty slots, the rows read -- is
longmem_ref's, reached through `frame_lists(weights_fn=)`.

Also here: the planted defects, the error bound of the centring kernel, and the checkers that the CPU and the GPU tests apply.
"""
import functools

import numpy as np

import longmem_ref as lm
import oracle.crw_oracle as orc
import sliding_ref

CENTER_DEFECTS = ("mean_over_whole_item", "center_after_normalize")
BIAS_DEFECTS = ("bias_recent_keys", "bias_after_temperature", "bias_masked_keys")
DEFECTS = CENTER_DEFECTS + BIAS_DEFECTS

U32, U64 = 2.0 ** -24, 2.0 ** -53


# ---- centring ----------------------------------------------------------------------------------------------------------------------
def center_normalize(emb, bounds, dtype=np.float64, defect=None):
    """emb [rows, C], bounds [S + 1] -> (ehat [rows, C] dtype, mean [S, C] float64).  The means are always fp64; dtype is that of the
    subtraction's result and of the normalisation (float32: the device's one rounding)."""
    emb = np.asarray(emb)
    rows, C = emb.shape
    b = [int(x) for x in bounds]
    assert b[0] == 0 and b[-1] == rows and all(y >= x for x, y in zip(b, b[1:])), b
    x = emb.astype(np.float64)
    if defect == "center_after_normalize":     # normalised first, centred (and normalised again) afterwards
        x = orc.l2_normalize(x, np.float64)
    if defect == "mean_over_whole_item":       # one mean for every segment
        b_mean = [(0, rows)] * (len(b) - 1)
    else:
        b_mean = list(zip(b, b[1:]))
    mean = np.zeros((len(b) - 1, C))
    y = np.zeros((rows, C), dtype)
    for s, ((lo, hi), (mlo, mhi)) in enumerate(zip(zip(b, b[1:]), b_mean)):
        if hi > lo:
            mean[s] = x[mlo:mhi].sum(0) / (mhi - mlo)
            y[lo:hi] = (x[lo:hi] - mean[s]).astype(dtype)
    return orc.l2_normalize(y, dtype).astype(dtype), mean


def center_bound(emb, bounds):
    """Entry-wise bound [rows, C] on |device ehat - fp64 definition| (DESIGN.md section 2 derives it), u = 2^-24, e* the fp64 result,
    y* = x - mean in fp64, n_s the rows of the segment:

        |e*_c| (C / 2 + 6) u  +  2 (1 + sqrt(C)) dm / max(|y*|, 1e-12)  +  2^-126,        dm = n_s 2^-53 max_r |x_rc|

    first term: the one rounding of the subtraction, seen in the entry (u) and in the norm (u); the fp32 sum of C squares, C
    roundings on positive terms, halved by the root (C u / 2); root and division, 2 u each (correctly rounded they take u each).
    second term: the fp64 mean itself, a sum of n_s terms in any order, moves every y by at most dm -- the entry directly, the norm
    by at most sqrt(C) dm.  Nothing in it comes from what a kernel returns."""
    emb = np.asarray(emb, np.float64)
    rows, C = emb.shape
    estar, _ = center_normalize(emb, bounds, np.float64)
    out = np.empty((rows, C))
    for lo, hi in zip(bounds, bounds[1:]):
        if hi > lo:
            seg = emb[lo:hi]
            ystar = seg - seg.mean(0)
            dm = (hi - lo) * U64 * np.abs(seg).max(0)                                 # [C]
            norm = np.maximum(np.sqrt((ystar ** 2).sum(1, keepdims=True)), 1e-12)      # [n_s, 1]
            out[lo:hi] = np.abs(estar[lo:hi]) * (C / 2 + 6) * U32 + 2 * (1 + np.sqrt(C)) * dm[None] / norm + 2.0 ** -126
    return out


def center_violations(emb, bounds, ehat, mean=None):
    """ehat (and mean) of one call against the definition -> dict(outside=entries beyond `center_bound`, worst=the largest error as
    a fraction of its bound, mean=entries of mean further than n_s 2^-53 max|x| from the fp64 mean)."""
    emb = np.asarray(emb, np.float64)
    estar, mstar = center_normalize(emb, bounds, np.float64)
    frac = np.abs(np.asarray(ehat, np.float64) - estar) / center_bound(emb, bounds)
    out = dict(outside=int((~(frac <= 1)).sum()), worst=float(frac.max()), mean=0)
    if mean is not None:
        for s, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
            tol = (hi - lo) * U64 * np.abs(emb[lo:hi]).max(0) if hi > lo else 0.0
            out["mean"] += int((~(np.abs(np.asarray(mean)[s] - mstar[s]) <= tol)).sum())
    return out


# ---- the biased lists ----------------------------------------------------------------------------------------------------------------
def biased_weights(n_long_keys, bias, defect=None):
    """`oracle.labelprop_weights` for `longmem_ref.frame_lists(weights_fn=)` -- the gathered copy [key frames..., frame n], nothing
    truncated -- with `bias` on the cosine of the first n_long_keys key frames."""
    def fn(ehat, n, cxt_size, radius, temp, knn, dtype=np.float32, grid_w=1, return_scores=False):
        T, N, C = ehat.shape
        assert cxt_size >= n                                                       # (the copy is its own context bound)
        keys = ehat[:n].reshape(n * N, C).astype(dtype)
        q = ehat[n].astype(dtype)
        cos = (keys @ q.T).reshape(n, N, N)
        band = orc.band_bias(N, radius, dtype, grid_w)[None]
        b, kl = dtype(bias), (n if defect == "bias_recent_keys" else min(n_long_keys, n))
        S = cos.copy()
        if defect == "bias_after_temperature":
            S = (S + band) / dtype(temp)
            S[:kl] = S[:kl] + b
        elif defect == "bias_masked_keys":            # the long-term keys lose their mask: (cos + b) / temp whatever the band says
            S = S + band
            S[:kl] = cos[:kl] + b
            S = S / dtype(temp)
        else:
            S[:kl] = S[:kl] + b                       # one rounded add ...
            S = (S + band) / dtype(temp)              # ... the mask as it was, then the temperature
        S = S.reshape(n * N, N)
        I = np.argsort(-S, axis=0, kind="stable")[:knn]
        Vl = np.take_along_axis(S, I, 0)
        Wl = np.exp(Vl - Vl.max(0, keepdims=True))
        W = Wl / Wl.sum(0, keepdims=True)
        return (W.astype(dtype), I, Vl) if return_scores else (W.astype(dtype), I)
    return fn


def frame_lists(ehat, n, K, cxt, radius, temp, knn, bias, dtype=np.float32, defect=None):
    """(W [knn, N], I [knn, N]) of frame n under the rule with the bias (empty slots W = 0, I = 0)"""
    return lm.frame_lists(ehat, n, K, cxt, radius, temp, knn, dtype, None, biased_weights(min(n, K), bias, defect))


def lists(ehat, K, cxt, radius, temp, knn, first_frame, bias, dtype=np.float32, defect=None):
    out = [frame_lists(ehat, n, K, cxt, radius, temp, knn, bias, dtype, defect) for n in range(first_frame, ehat.shape[0])]
    return np.stack([w for w, _ in out]), np.stack([i for _, i in out])


def scores(ehat, K, cxt, radius, temp, knn, first_frame, bias, dtype=np.float32, defect=None):
    """V [F - first_frame, knn, N]: the selected logits that go with `lists` (what raw = 1 returns; an empty slot -inf)"""
    out = []
    for n in range(first_frame, ehat.shape[0]):
        keys = lm.key_frames(n, K, cxt)
        sub = np.concatenate([ehat[keys], ehat[n:n + 1]]).astype(dtype)
        V = biased_weights(min(n, K), bias, defect)(sub, len(keys), len(keys), radius, temp, knn, dtype, 1, True)[2]
        V = np.concatenate([V, np.full((max(knn - V.shape[0], 0), V.shape[1]), -np.inf, V.dtype)])
        out.append(np.where(V < orc.MASK_NEG / 2 / temp, -np.inf, V).astype(dtype))
    return np.stack(out)


def features(emb, n_bank, align, dtype=np.float32, defect=None):
    """emb [F, N, C] raw features of the virtual item [bank's n_bank frames..., item] -> ehat [F, N, C]"""
    F, N, C = emb.shape
    if align is None:
        return orc.l2_normalize(emb, dtype).astype(dtype)
    assert align == "center", align
    return center_normalize(emb.reshape(F * N, C), [0, n_bank * N, F * N], dtype, defect)[0].reshape(F, N, C)


def labelprop_aligned(emb, cls_front, nclasses, cxt, K, radius, temp, knn, first_frame, n_bank, align=None, bias=0.0, dtype=np.float32,
                      defect=None):
    """`longmem_ref.labelprop_long` on the virtual item emb [F, N, C] whose first n_bank frames are the bank's, with the two options
    -> (pred [N, F], L [F*N, M], W, I).  align None and bias 0: labelprop_long's bits."""
    F, N, _ = emb.shape
    ehat = features(emb, n_bank, align, dtype, defect if defect in CENTER_DEFECTS else None)
    W, I = lists(ehat, K, cxt, radius, temp, knn, first_frame, bias, dtype, defect if defect in BIAS_DEFECTS else None)
    L0, p0 = lm.initial_labels(cls_front, first_frame, N, nclasses, F, dtype)
    L, pred = sliding_ref.gather(None, W, lm.rows(I, N, cxt, K, first_frame), nclasses, first_frame, L0, p0, dtype)
    return pred, L, W, I


@functools.lru_cache(maxsize=None)
def _campaign_item(*args):
    return lm.campaign_item(*args)


def bank_case(shape, s, B, start, emerging):
    """`longmem_ref.bank_case`, its items made once per (seed, start) and shared by the cells that differ in the bank size or in the
    options alone (tests/test_align.py holds the two against each other)"""
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    ea, ca = _campaign_item(7, 100 + s, T, N, C, M, 0.6 * amp, True, False, 0.5, start)
    frames = lm.BANKS[B](T)
    if emerging:
        et, ct = _campaign_item(7, s, T, N, C, M, amp, True, True, 0.0, start)
        return np.concatenate([ea[frames], et]), np.concatenate([ca[frames], ct]), B + 1, B + 1, B + T // 3
    et, ct = _campaign_item(7, s, T, N, C, M, amp, False, False, 0.0, start)
    return np.concatenate([ea[frames], et]), np.concatenate([ca[frames], ct]), B, B, B


def aligned_errors(shape, s, B, start, emerging, align=None, bias=0.0, dtype=np.float64):
    """`longmem_ref.bank_errors` -- (wrong labels, labels) of one cell of the README's tables -- under the two options"""
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    emb, cls, K, ff, f0 = bank_case(shape, s, B, start, emerging)
    pred, _, _, _ = labelprop_aligned(emb, cls[:ff], M, cxt, K, radius, temp, knn, ff, B, align, bias, dtype)
    return int((pred.T[f0:] != cls[f0:]).sum()), int(cls[f0:].size)


# ---- the checker of the biased lists -------------------------------------------------------------------------------------------------
AUDIT_MAX_BIAS = 1.0 / 3


def biased_lists_audit(ehat, K, cxt, radius, temp, knn, first_frame, W, I, V, bias):
    """`oracle.topk_lists_audit` -- every slot of every list against fp64, the checker of tests/test_labelprop_lists_gpu.py -- applied
    to lists made under the long-memory rule with a bias.  Frame by frame the audit gets the gathered copy [key frames..., frame n]
    (its own context bound, so an index is a list position, as in `longmem_ref.frame_lists`) with TWO more channels: (b, 0) on the
    long-term keys, (0, 0) on the recent ones, (1, 0) on the query, b the fp32 number the device was given.  In fp64 the audit's
    logit is then exactly (cos + b) / temp on the long-term keys and cos / temp elsewhere -- the definition -- and its own bound
    eps_s = (C' + 2) u / temp is taken at C' = C + 2 channels: (C + 4) u / temp.
    That is the bound of the unbiased lists, (C + 2) u / temp, widened by the one rounded add: the add rounds by u |cos + b| <=
    u (1 + |b|), and the two roundings of the division now act on |cos + b| <= 1 + |b| instead of 1 -- together
    (C + 3 (1 + |b|)) u / temp <= (C + 4) u / temp for |b| <= 1 / 3 (asserted).
    numpy arrays or torch tensors (the work is done on W's device).  -> dict(violations, worst, eps_s) summed / maximised over the
    frames."""
    import torch
    assert abs(bias) <= AUDIT_MAX_BIAS, bias
    b = float(np.float32(bias))
    eh = ehat if torch.is_tensor(ehat) else torch.from_numpy(np.asarray(ehat))
    dev = W.device if torch.is_tensor(W) else torch.device("cpu")
    eh = eh.to(dev, torch.float64)
    as_t = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
    W, I, V = as_t(W), as_t(I), (None if V is None else as_t(V))
    F, N, C = eh.shape
    total, worst, eps = None, None, None
    for n in range(first_frame, F):
        keys = lm.key_frames(n, K, cxt)
        kl = min(n, K)
        sub = torch.zeros(len(keys) + 1, N, C + 2, dtype=torch.float64, device=dev)
        sub[:-1, :, :C], sub[-1, :, :C] = eh[keys], eh[n]
        sub[:kl, :, C] = b
        sub[-1, :, C] = 1.0
        f = n - first_frame
        res = orc.topk_lists_audit(sub, len(keys), radius, temp, knn, len(keys), 1, W[f:f + 1], I[f:f + 1], None if V is None else V[f:f + 1])
        eps = res["eps_s"]
        if total is None:
            total, worst = dict(res["violations"]), dict(res["worst"])
        else:
            total = {k: total[k] + v for k, v in res["violations"].items()}
            worst = {k: max(worst[k], v) for k, v in res["worst"].items()}
    return dict(violations=total, worst=worst, eps_s=eps)
