"""CPU oracle for the contrastive-random-walk hot path.  TEST INFRASTRUCTURE ONLY.

This file is a from-scratch CPU restatement (numpy + torch-CPU) of the algorithm that
jdalcorso/radar-sounder-crw runs on its hot path.  It is the *checker*: only ``tests/``,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import it.  The product
path (``radar-sounder-crw_amd/``) never imports it and fails loudly when the HIP library is missing.

Parity status: PINNED.  Every function below is checked in ``tests/test_oracle_golden.py`` against
fixtures in ``tests/golden/`` that were produced by importing and running the reference itself on
CPU in the build container (``tests/golden/make_golden.py``; the reference repo has no tests or
golden vectors of its own).

Reference lines each function follows (paths under the reference repo):
  l2_normalize ............ src/model.py:22            (F.normalize, eps 1e-12)
  affinity ................ src/model.py:26
  walk_reference_form ..... src/model.py:31-46         (literal palindrome / O(T^2) chain)
  walk_prefix_form ........ same value, O(T) products  
  walk_backward ........... analytic gradient of the above (checked against reference autograd)
  cnn_forward ............. src/encoder.py:13-57
  pos_embed ............... src/utils.py:76-90
  crw_forward ............. src/model.py:15-46
  band_bias ............... src/imported/maskedatt.py:222-245 + labelprop.py:89-96 (w == 1)
  labelprop_weights ....... src/imported/maskedatt.py:151-175
  labelprop ............... src/utils.py:134-161 + src/imported/labelprop.py:67-115
  labelprop_tie_audit ..... same lines, fp64, teacher-forced per frame (near-tie proof for label maps)
  labelprop_lists ......... labelprop_weights of every frame, in the layout of the device's lists
  topk_lists_audit ........ maskedatt.py:151-175 in fp64 against a device's (W, I, V) lists, every slot, derived fp32 bounds
  gather_audit ............ labelprop.py:103-107 in fp64, teacher-forced per frame, against a device's soft labels / label map
  seed_labels ............. src/utils.py:139-147       (NEAREST resize to (N,1))
  xent_metric ............. src/utils.py:117-125
  unfold_item ............. src/dataset.py:19-39
"""
import numpy as np

EPS_NORM = 1e-12


# --------------------------------------------------------------------------------------------
# training forward
# --------------------------------------------------------------------------------------------
def l2_normalize(e, dtype=np.float64):
    e = np.asarray(e, dtype=dtype)
    nrm = np.sqrt((e * e).sum(-1, keepdims=True))
    return e / np.maximum(nrm, EPS_NORM)


def affinity(ehat, tau):
    """A[b,j,n,m] = <ehat[b,j,n], ehat[b,j+1,m]> / tau ; ehat [B,T,N,C] -> [B,T-1,N,N]."""
    return np.einsum("btnc,btmc->btnm", ehat[:, :-1], ehat[:, 1:]) / ehat.dtype.type(tau)


def _softmax(x, axis):
    m = x.max(axis=axis, keepdims=True)
    e = np.exp(x - m)
    return e / e.sum(axis=axis, keepdims=True)


def _cycle_loss_terms(At):
    """-(1/(B*N)) sum_{b,d} log softmax(At[b,d,:])[d]   (cross_entropy with class dim 1 on At^T)."""
    B, N, _ = At.shape
    m = At.max(-1, keepdims=True)
    lse = np.log(np.exp(At - m).sum(-1)) + m[..., 0]
    diag = np.einsum("bdd->bd", At)
    return -(diag - lse).sum() / (B * N)


def walk_reference_form(A):
    """Literal restatement: palindrome AA, for each k a fresh chain of 2k-1 left-multiplications."""
    B, Tm1, N, _ = A.shape
    T = Tm1 + 1
    AA = np.concatenate([A, np.flip(A, 1).transpose(0, 1, 3, 2)], 1)  # [B, 2T-2, N, N]
    loss = A.dtype.type(0)
    Ats = []
    for k in range(1, T - 1):
        At = np.broadcast_to(np.eye(N, dtype=A.dtype), (B, N, N)).copy()
        AA_this = np.concatenate([AA[:, :k], AA[:, -k:]], 1) if k > 0 else AA[:, :0]
        for t in range(1, 2 * k):
            At = _softmax(AA_this[:, t], -1) @ At
        Ats.append(At)
        loss = loss + _cycle_loss_terms(At)
    At_all = np.stack(Ats, 1) if Ats else np.zeros((B, 0, N, N), A.dtype)
    return loss / N, At_all


def softmax_pair(A):
    """F_j = row-softmax(A_j);  Gt_j = column-softmax(A_j) kept in A's layout (G_j = Gt_j^T)."""
    return _softmax(A, -1), _softmax(A, -2)


def walk_prefix_form(A, return_state=False):
    """Lt_1 = Gt_0, Lt_{k+1} = Gt_k Lt_k ; R_1 = I, R_{k+1} = F_k R_k ; At_k = Lt_k^T R_k."""
    B, Tm1, N, _ = A.shape
    T = Tm1 + 1
    F, Gt = softmax_pair(A)
    Lt, R, Ats = [], [], []
    loss = A.dtype.type(0)
    for k in range(1, T - 1):
        if k == 1:
            Lt.append(Gt[:, 0].copy())
            R.append(np.broadcast_to(np.eye(N, dtype=A.dtype), (B, N, N)).copy())
        else:
            Lt.append(Gt[:, k - 1] @ Lt[-1])
            R.append(F[:, k - 1] @ R[-1])
        At = Lt[-1].transpose(0, 2, 1) @ R[-1]
        Ats.append(At)
        loss = loss + _cycle_loss_terms(At)
    At_all = np.stack(Ats, 1) if Ats else np.zeros((B, 0, N, N), A.dtype)
    if return_state:
        return loss / N, At_all, dict(F=F, Gt=Gt, Lt=Lt, R=R)
    return loss / N, At_all


def walk_backward(A, gloss=1.0):
    """dLoss/dA by hand (reverse of the prefix recurrences, Appendix A.3), [B,T-1,N,N]."""
    B, Tm1, N, _ = A.shape
    T = Tm1 + 1
    _, At_all, st = walk_prefix_form(A, return_state=True)
    F, Gt, Lt, R = st["F"], st["Gt"], st["Lt"], st["R"]
    dF = np.zeros_like(A)
    dGt = np.zeros_like(A)
    K = T - 2
    if K < 1:
        return np.zeros_like(A)
    coef = gloss / (N * B * N)
    dLt_next = dR_next = None
    for k in range(K, 0, -1):  # k = K..1 ; lists are 0-based (index k-1)
        At = At_all[:, k - 1]
        dAt = coef * (_softmax(At, -1) - np.eye(N, dtype=A.dtype))
        dLt = R[k - 1] @ dAt.transpose(0, 2, 1)
        dR = Lt[k - 1] @ dAt
        if k < K:
            dLt = dLt + Gt[:, k].transpose(0, 2, 1) @ dLt_next
            dGt[:, k] = dLt_next @ Lt[k - 1].transpose(0, 2, 1)
            dR = dR + F[:, k].transpose(0, 2, 1) @ dR_next
            dF[:, k] = dR_next @ R[k - 1].transpose(0, 2, 1)
        dLt_next, dR_next = dLt, dR
    dGt[:, 0] = dLt_next
    dA = F * (dF - (dF * F).sum(-1, keepdims=True)) + Gt * (dGt - (dGt * Gt).sum(-2, keepdims=True))
    return dA


def affinity_backward(dA, e, tau):
    """dLoss/d(raw features) through affinity + L2 normalisation."""
    e = np.asarray(e, dtype=dA.dtype)
    nrm = np.maximum(np.sqrt((e * e).sum(-1, keepdims=True)), EPS_NORM)
    eh = e / nrm
    deh = np.zeros_like(eh)
    deh[:, :-1] += np.einsum("btnm,btmc->btnc", dA, eh[:, 1:]) / tau
    deh[:, 1:] += np.einsum("btnm,btnc->btmc", dA, eh[:, :-1]) / tau
    return (deh - eh * (eh * deh).sum(-1, keepdims=True)) / nrm


def crw_from_features(emb, tau, dtype=np.float64):
    """emb [B,T,N,C] raw encoder outputs -> dict(loss, A, At, demb)."""
    eh = l2_normalize(emb, dtype)
    A = affinity(eh, tau)
    loss, At = walk_prefix_form(A)
    dA = walk_backward(A)
    demb = affinity_backward(dA, np.asarray(emb, dtype), tau)
    return dict(loss=loss, A=A, At=At, dA=dA, demb=demb)


# --------------------------------------------------------------------------------------------
# encoder (torch CPU; the oracle may use torch ops, it is never the thing measured on the GPU)
# --------------------------------------------------------------------------------------------
def pos_embed(x):
    """x [P,1,h,w] torch -> [P,2,h,w]; prepended channel pe[r,:] = r/h - 0.5."""
    import torch
    P, _, h, w = x.shape
    pe = (torch.arange(h, dtype=torch.float32) / h - 0.5).view(1, 1, h, 1).expand(P, 1, h, w)
    return torch.cat([pe.to(x.dtype), x], 1)


def cnn_forward(x, sd):
    """x [P,cin,h,w] torch, sd: dict name -> torch tensor (conv{1..5}.{weight,bias}, fc.*)."""
    import torch.nn.functional as TF
    x = TF.max_pool2d(TF.relu(TF.conv2d(x, sd["conv1.weight"], sd["conv1.bias"], padding=1)), 2, 1)
    x = TF.max_pool2d(TF.relu(TF.conv2d(x, sd["conv2.weight"], sd["conv2.bias"], padding=1)), 2, 1)
    x = TF.relu(TF.conv2d(x, sd["conv3.weight"], sd["conv3.bias"], padding=1))
    x = TF.relu(TF.conv2d(x, sd["conv4.weight"], sd["conv4.bias"], padding=1))
    x = TF.relu(TF.conv2d(x, sd["conv5.weight"], sd["conv5.bias"], padding=1))
    x = x.mean((2, 3))
    return TF.linear(x, sd["fc.weight"], sd["fc.bias"])


def crw_forward_torch(seq, sd, tau, use_pos_embed=False, dtype=None):
    """Whole training forward in torch-CPU with autograd (used for weight-gradient parity and as
    the timed CPU baseline): seq [B,T,N,h,w] -> (loss, A, emb)."""
    import torch
    B, T, N, h, w = seq.shape
    x = seq.reshape(-1, h, w).unsqueeze(1)
    if use_pos_embed:
        x = pos_embed(x)
    emb = cnn_forward(x, sd).reshape(B, T, N, -1)
    loss, A = walk_loss_torch(emb, tau)
    return loss, A, emb


def walk_loss_torch(emb, tau, At_out=None):
    """Prefix-form walk in torch (differentiable, any device / dtype); emb [B,T,N,C] raw -> (loss, A).  `At_out`: a list that
    receives every cycle product At_k (detached), k = 1..T-2."""
    import torch
    B, T, N, C = emb.shape
    eh = emb / emb.norm(dim=-1, keepdim=True).clamp_min(EPS_NORM)
    A = torch.einsum("btnc,btmc->btnm", eh[:, :-1], eh[:, 1:]) / tau
    if T < 3:
        return emb.new_zeros(()), A
    F = torch.softmax(A, -1)
    Gt = torch.softmax(A, -2)
    eye = torch.eye(N, dtype=emb.dtype, device=emb.device)
    loss = emb.new_zeros(())
    Lt = R = None
    for k in range(1, T - 1):
        if k == 1:
            Lt, R = Gt[:, 0], eye.expand(B, N, N)
        else:
            Lt, R = Gt[:, k - 1] @ Lt, F[:, k - 1] @ R
        At = Lt.transpose(1, 2) @ R
        if At_out is not None:
            At_out.append(At.detach())
        lse = torch.logsumexp(At, -1)
        loss = loss - (torch.diagonal(At, dim1=1, dim2=2) - lse).sum() / (B * N)
    return loss / N, A


# --------------------------------------------------------------------------------------------
# inference: label propagation
# --------------------------------------------------------------------------------------------
MASK_NEG = -1e10


def band_bias(N, radius, dtype=np.float32, grid_w=1):
    """bias[m,q] = 0 if the nodes m and q are closer than `radius` else -1e10.  The N nodes form an (N / grid_w) x grid_w grid in
    row-major order and the distance is Euclidean (MaskedAttention.make, src/imported/maskedatt.py:232-245); a radargram's patch
    grid is N x 1 (grid_w = 1), where the mask degenerates to the band |m-q| < radius."""
    i, j = np.arange(N) // grid_w, np.arange(N) % grid_w
    d = np.sqrt(((i[:, None] - i[None, :]) ** 2 + (j[:, None] - j[None, :]) ** 2).astype(np.float32))
    return np.where(d < radius, 0.0, MASK_NEG).astype(dtype)


def seed_labels(seg_ref, N):
    """NEAREST resize of seg_ref [rows, w] to (N,1): row floor(i*rows/N), column 0."""
    seg_ref = np.asarray(seg_ref)
    rows = seg_ref.shape[0]
    idx = np.floor(np.arange(N) * (rows / N)).astype(np.int64)
    idx = np.minimum(idx, rows - 1)
    return seg_ref[idx, 0].astype(np.float32)


def labelprop_weights(ehat, n, cxt_size, radius, temp, knn, dtype=np.float32, grid_w=1, return_scores=False):
    """Top-k neighbour weights/indices of frame n against frames 0..n-1.
    Returns (W [knn,N], I [knn,N]) with I addressing the (possibly truncated) key list; with `return_scores` also the
    selected logits [knn,N] (a masked key's is -1e10 / temp)."""
    T, N, C = ehat.shape
    keys = ehat[:n].reshape(n * N, C).astype(dtype)
    q = ehat[n].astype(dtype)
    S = (keys @ q.T).reshape(n, N, N) + band_bias(N, radius, dtype, grid_w)[None]
    S = S.reshape(n * N, N) / dtype(temp)
    if S.shape[0] > (cxt_size + 1) * N:
        S = np.concatenate([S[:N], S[-N * cxt_size:]], 0)
    # top-k along keys, descending (ties: any order -- masked keys carry weight exactly 0)
    I = np.argsort(-S, axis=0, kind="stable")[:knn]
    Vl = np.take_along_axis(S, I, 0)
    Wl = np.exp(Vl - Vl.max(0, keepdims=True))
    W = Wl / Wl.sum(0, keepdims=True)
    if return_scores:
        return W.astype(dtype), I, Vl
    return W.astype(dtype), I


def labelprop_lists(ehat, cxt_size, radius, temp, knn, first_frame=1, grid_w=1, dtype=np.float32):
    """`labelprop_weights` of every frame n >= first_frame in the layout of the device's lists: (W, I, V), each
    [T - first_frame, knn, N], I int32.  Where a frame has fewer in-band keys than knn the reference's top-k goes on into masked
    keys (weight exactly 0, logit -1e10 / temp); the device leaves those slots empty, and so does this: W = 0, I = 0, V = -inf."""
    T, N, _ = ehat.shape
    Ws, Is, Vs = [], [], []
    for n in range(first_frame, T):
        W, I, V = labelprop_weights(ehat, n, cxt_size, radius, temp, knn, dtype, grid_w, return_scores=True)
        pad = knn - W.shape[0]  # fewer keys than knn at all (the reference would fail there; the device leaves empty slots)
        if pad > 0:
            W, I = np.concatenate([W, np.zeros((pad, N), dtype)]), np.concatenate([I, np.zeros((pad, N), I.dtype)])
            V = np.concatenate([V, np.full((pad, N), -np.inf, dtype)])
        empty = V < MASK_NEG / 2 / temp
        Ws.append(np.where(empty, 0, W).astype(dtype))
        Is.append(np.where(empty, 0, I).astype(np.int32))
        Vs.append(np.where(empty, -np.inf, V).astype(dtype))
    return np.stack(Ws), np.stack(Is), np.stack(Vs)


def labelprop(emb, seed, nclasses, cxt_size, radius, temp, knn, dtype=np.float32, grid_w=1, return_soft=False):
    """emb [T,N,C] raw features (already flipped by the caller if use_last), seed [N] float labels
    of frame 0 -> pred [N,T] float labels.  Indices returned for the truncated key list are used
    against the *untruncated* label list (quirk Q7).  grid_w: see band_bias.  return_soft: (pred, L [T*N, nclasses])."""
    T, N, C = emb.shape
    ehat = l2_normalize(emb, dtype).astype(dtype)
    L = np.zeros((T * N, nclasses), dtype)
    L[np.arange(N), :] = (seed[:, None] == np.arange(nclasses)[None, :]).astype(dtype)
    pred = np.zeros((N, T), np.float32)
    pred[:, 0] = seed
    for n in range(1, T):
        W, I = labelprop_weights(ehat, n, cxt_size, radius, temp, knn, dtype, grid_w)
        p = (L[I] * W[..., None]).sum(0)  # [N, M]
        L[n * N:(n + 1) * N] = p
        pred[:, n] = p.argmax(-1)
    if return_soft:
        return pred, L
    return pred


def labelprop_tie_audit(ehat, L_dev, pred_dev, cxt_size, radius, temp, knn, eps=1e-5):
    """Frame-by-frame (teacher-forced) fp64 audit of a propagated label map -- how the tests prove that every label
    on which a device run and the fp32 oracle disagree is a floating-point near-tie, not a defect.

    Label propagation is argmax / top-k over floating-point scores, so two correct fp32 implementations (different
    summation orders) can legitimately pick different labels where two class probabilities or the k-th and (k+1)-th key
    logits coincide to rounding, and one such flip then cascades through every later frame that uses the flipped
    labels as context.  This audit removes the cascade: for every frame n it recomputes, in fp64 and with the DEVICE's
    own soft labels of frames < n as context (``L_dev`` [T*N, M]; same index quirk Q7 as ``labelprop``), the scores of
    frame n from the device's normalised features ``ehat`` [T,N,C], and compares argmax with ``pred_dev`` [N,T].

    Returns dict(step_mismatches, not_ties, worst_margin, max_soft_err): a step mismatch is a *tie* when the fp64
    top-2 class-probability margin is < eps or the top-k boundary logit gap (k-th minus (k+1)-th key logit of that
    query) is < eps; ``not_ties`` must be 0.  ``max_soft_err`` = max |L_dev - fp64 soft labels| over the queries
    without a boundary tie (the gathered weights themselves)."""
    T, N, C = ehat.shape
    eh = np.asarray(ehat, np.float64)
    L = np.asarray(L_dev, np.float64)
    M = L.shape[1]
    bias = band_bias(N, radius, np.float64)
    out = dict(step_mismatches=0, not_ties=0, worst_margin=0.0, max_soft_err=0.0, boundary_ties=0)
    for n in range(1, T):
        S = (eh[:n].reshape(n * N, C) @ eh[n].T).reshape(n, N, N) + bias[None]
        S = S.reshape(n * N, N) / temp
        if S.shape[0] > (cxt_size + 1) * N:
            S = np.concatenate([S[:N], S[-N * cxt_size:]], 0)
        order = np.argsort(-S, axis=0, kind="stable")
        I = order[:knn]
        top = np.take_along_axis(S, I, 0)
        if S.shape[0] > knn:
            nxt = np.take_along_axis(S, order[knn:knn + 1], 0)[0]
            gap = top[-1] - nxt                      # masked keys sit at -1e10/temp: a huge gap, never a tie
        else:
            gap = np.full(N, np.inf)
        # ties INSIDE the selected set do not matter (same keys, same weights); only the boundary does
        Wl = np.exp(top - top.max(0, keepdims=True))
        W = Wl / Wl.sum(0, keepdims=True)
        p = (L[I] * W[..., None]).sum(0)             # [N, M]
        ps = np.sort(p, -1)
        margin = ps[:, -1] - ps[:, -2] if M > 1 else np.full(N, np.inf)
        lab = p.argmax(-1)
        dev = np.asarray(pred_dev[:, n]).astype(np.int64)
        boundary_tie = gap < eps
        out["boundary_ties"] += int(boundary_tie.sum())
        clean = ~boundary_tie
        if clean.any():
            out["max_soft_err"] = max(out["max_soft_err"], float(np.abs(L[n * N:(n + 1) * N][clean] - p[clean]).max()))
        bad = lab != dev
        # a device label different from the fp64 argmax is fine when the device's class is within eps of the best one
        dev_short = ps[:, -1] - p[np.arange(N), dev]
        out["step_mismatches"] += int(bad.sum())
        nt = bad & ~boundary_tie & ~(dev_short < eps)
        out["not_ties"] += int(nt.sum())
        if bad.any():
            out["worst_margin"] = max(out["worst_margin"], float(np.where(boundary_tie, 0.0, dev_short)[bad].max()))
    return out


U_FP32 = 2.0 ** -24  # unit roundoff of fp32 (round to nearest)
TOPK_CONDITIONS = ("range", "disc", "distinct", "count", "empty", "selection", "scores", "order", "weights", "sum")
GATHER_CONDITIONS = ("index", "soft", "pred", "frame0", "untouched")


def topk_score_bound(C, temp):
    """eps_s: how far a correct fp32 logit <k, q> / temp of two unit vectors of C channels may lie from its fp64 value.

    A dot product summed in fp32 in ANY order carries each product through at most C roundings (its multiplication and at most
    C - 1 additions), so |fl(k.q) - k.q| <= C u sum_i |k_i q_i| to first order, u = 2^-24, and sum_i |k_i q_i| <= |k| |q| = 1
    (Cauchy-Schwarz).  This holds for the vector kernel's order (partial sums per lane, then a butterfly), for the matrix cores'
    (two chains of 16x16x4 steps) and for a BLAS.  The division by temp rounds once more (u |k.q| / temp) and temp itself is
    given to the device rounded to fp32 (another u |k.q| / temp); |k.q| <= 1.  Together (C + 2) u / temp.  Not tuned: nothing in
    it comes from what a kernel returns."""
    return (C + 2) * U_FP32 / temp


def _to_t64(x, dev, integer=False):
    """numpy array or torch tensor -> float64 (int64) tensor on dev; fp32 -> fp64 is exact, so equalities on a device's values survive"""
    import torch
    dt, nt = (torch.int64, np.int64) if integer else (torch.float64, np.float64)
    if torch.is_tensor(x):
        return x.to(dev, dt)
    return torch.from_numpy(np.asarray(x).astype(nt)).to(dev)


def topk_lists_audit(ehat, cxt_size, radius, temp, knn, first_frame, grid_w, W, I, V=None):
    """fp64 audit of top-k lists in the device's layout -- W (softmax weights), I (int32 indices into the truncated key list),
    V (the selected logits, optional), each [T - first_frame, knn, N] -- against the logits of `labelprop_weights` recomputed in
    fp64 from the SAME normalised features `ehat` [T,N,C]: Euclidean-disc mask of `band_bias`, context truncated to frame 0 + the
    last cxt_size frames when n > cxt_size + 1, index p * N + node on the truncated list.  numpy arrays or torch tensors; the work
    is done in torch float64 on W's device.  No query is exempted; every condition holds for every slot of every list.

    Returns dict(violations={condition: count}, worst={toleranced condition: worst error / its bound}, eps_s=...).  Conditions:
      range ...... a non-empty slot's index is in [0, min(n, cxt_size + 1) * N)                                  (exact)
      disc ....... its key node lies inside the query's disc                                                      (exact)
      distinct ... no index twice in a list                                                                       (exact)
      count ...... (with V) the slots that hold a logit are exactly the first min(knn, in-band candidates)        (exact)
      empty ...... every slot behind those reads W == 0, I == 0 (and V == -inf)                                   (exact)
      selection .. every selected candidate's fp64 logit >= the query's fp64 k-th best - 2 eps_s, and every in-band candidate
                   left out has an fp64 logit <= the smallest selected one + 2 eps_s.  (The device ranked its own fp32 values,
                   each within eps_s of fp64: preferring a to b means v_a >= v_b, hence s_a >= s_b - 2 eps_s.)
      scores ..... |V - fp64 logit at the device's own index| <= eps_s
      order ...... on the device's own values: V[j] >= V[j+1], and where V[j] == V[j+1] bit for bit, I[j] < I[j+1] (the rule
                   "highest value, then lowest candidate index"; candidate order is ascending I).  Without V: W[j] >= W[j+1]
                   alone -- equal weights can come from different logits, so the index rule cannot be read off W.     (exact)
      weights .... W against the fp64 softmax of the fp64 logits at the device's own indices (see the bound below)
      sum ........ |sum_j W - 1| within the same relative bound
    """
    import torch
    dev = W.device if torch.is_tensor(W) else torch.device("cpu")
    eh, Wd, Id = _to_t64(ehat, dev), _to_t64(W, dev), _to_t64(I, dev, True)
    Vd = _to_t64(V, dev) if V is not None else None
    T, N, C = eh.shape
    eps = topk_score_bound(C, temp)
    # Weights.  The device forms W_j = exp(v_j - v_max) / sum_i exp(v_i - v_max) from logits v = s + d, |d| <= eps_s: against the
    # softmax of s that is the factor exp(d_j) / sum_i p_i exp(d_i), inside [exp(-2 eps_s), exp(2 eps_s)] -- relative 2 eps_s.
    # On top, in ulps of fp32 (1 ulp <= 2^-23 relative): expf of the numerator 1 (the documented bound of the device's expf),
    # expf of the terms of the sum 1 (positive terms: the sum inherits their relative error), the division 0.5 -- 3 rounded up --
    # and the sequential fp32 sum of knn positive terms (knn - 1) / 2.  The fp32 subtraction v_j - v_max rounds by at most
    # u |v_j - v_max| <= 2 u / temp; it is not budgeted apart: eps_s charges a dot product C roundings, the sequential worst
    # case, and neither kernel's order comes within 2 of that (partial sums per lane + 4 butterfly steps; two chains of C / 2).
    # Below the smallest normal number fp32 has no relative precision (and may flush): absolute floor 2^-126.
    ulps = 3 + (knn - 1) / 2
    rel_w = 2 * eps + ulps * 2.0 ** -23
    abs_w = 2.0 ** -126
    inband0 = torch.as_tensor(band_bias(N, radius, np.float64, grid_w) == 0).to(dev)   # [key node, query node]
    slot = torch.arange(knn, device=dev)[:, None]
    ninf = float("-inf")
    viol = {k: 0 for k in TOPK_CONDITIONS}
    worst = dict(selection=0.0, scores=0.0, weights=0.0, sum=0.0)

    def _worst(key, x):
        x = x[torch.isfinite(x)]
        if x.numel():
            worst[key] = max(worst[key], float(x.max()))

    for n in range(first_frame, T):
        f = n - first_frame
        frames = list(range(n)) if n <= cxt_size + 1 else [0] + list(range(n - cxt_size, n))
        nf = len(frames)
        S = (eh[frames].reshape(nf * N, C) @ eh[n].T) / temp                       # [nf * N keys, N queries]
        inband = inband0.repeat(nf, 1)
        Sm = torch.where(inband, S, torch.full_like(S, ninf))
        cnt = torch.clamp(inband0.sum(0) * nf, max=knn)                              # slots that must be filled, per query
        full = slot < cnt[None]
        Wn, In = Wd[f], Id[f]
        Vn = Vd[f] if Vd is not None else None
        if Vn is not None:
            viol["count"] += int(((Vn != ninf) != full).sum())
        bad_empty = (Wn != 0) | (In != 0)
        if Vn is not None:
            bad_empty = bad_empty | (Vn != ninf)
        viol["empty"] += int((bad_empty & ~full).sum())
        inrange = (In >= 0) & (In < nf * N)
        viol["range"] += int((full & ~inrange).sum())
        valid = full & inrange
        Ic = torch.where(valid, In, torch.zeros_like(In))
        viol["disc"] += int((valid & ~torch.gather(inband, 0, Ic)).sum())
        keyed = torch.where(valid, In, -1 - slot.expand_as(In)).sort(0).values
        viol["distinct"] += int((keyed[1:] == keyed[:-1]).sum())
        # selection
        s_raw = torch.gather(S, 0, Ic)
        s_sel = torch.gather(Sm, 0, Ic)
        best = torch.topk(Sm, min(knn, nf * N), dim=0).values
        kth = torch.gather(best, 0, (cnt - 1)[None])[0]
        short = kth[None] - s_sel                                                   # > 0: worse than the fp64 k-th best
        viol["selection"] += int((valid & (short > 2 * eps)).sum())
        _worst("selection", (short / (2 * eps))[valid])
        chosen = torch.zeros(S.shape, dtype=torch.int32, device=dev).scatter_add_(0, Ic, valid.to(torch.int32)) > 0
        min_sel = torch.where(valid, s_sel, torch.full_like(s_sel, float("inf"))).min(0).values
        over = torch.where(inband & ~chosen, S, torch.full_like(S, ninf)) - min_sel[None]   # > 0: better than a selected one
        viol["selection"] += int((over > 2 * eps).sum())
        _worst("selection", over.max(0).values / (2 * eps))
        # scores, order
        if Vn is not None:
            err = (Vn - s_raw).abs()
            viol["scores"] += int((valid & ~(err <= eps)).sum())
            _worst("scores", (err / eps)[valid])
            pair = full[:-1] & full[1:]
            wrong = (Vn[:-1] < Vn[1:]) | ((Vn[:-1] == Vn[1:]) & (In[:-1] >= In[1:]))
            viol["order"] += int((pair & wrong).sum())
        else:
            viol["order"] += int((full[:-1] & full[1:] & (Wn[:-1] < Wn[1:])).sum())
        # weights
        x = torch.where(valid, s_raw, torch.full_like(s_raw, ninf))
        e = torch.exp(x - x.max(0, keepdim=True).values)
        p = e / e.sum(0, keepdim=True)
        werr, wtol = (Wn - p).abs(), p * rel_w + abs_w
        viol["weights"] += int((valid & ~(werr <= wtol)).sum())
        _worst("weights", (werr / wtol)[valid])
        serr = (Wn.sum(0) - 1).abs() / (rel_w + knn * abs_w)
        viol["sum"] += int((~(serr <= 1)).sum())
        _worst("sum", serr)
    return dict(violations=viol, worst=worst, eps_s=eps, weight_rel_bound=rel_w)


def gather_bound(knn):
    """Bound of one propagated soft label against its fp64 value from the same fp32 inputs.  p = sum_j W_j L_j over knn
    neighbours, summed in fp32 in any order: each product passes at most knn roundings (its multiplication, at most knn - 1
    additions), so |fl(p) - p| <= knn u sum_j |W_j L_j| to first order, and sum_j W_j L_j <= max L * sum_j W_j, both 1 up to a
    few u (soft labels are convex combinations of one-hot rows, the weights a softmax).  A convex combination does not amplify
    the error of its inputs, and the audit is teacher-forced on the device's own earlier labels, so nothing accumulates from
    frame to frame: (knn + 2) u per label, the 2 covering those excesses over 1 and the second-order terms (knn <= 64)."""
    return (knn + 2) * U_FP32


def gather_audit(W, I, seed, M, first_frame, cxt_size, L, pred, L_init=None, pred_init=None):
    """fp64 audit of propagated soft labels, teacher-forced per frame: for every frame n >= first_frame,
    L64[n] = sum_j W[j] * L[I[j]] with the DEVICE's own L of the earlier frames and the indices applied to the UNtruncated label
    list (quirk Q7, as in `labelprop`), against the device's L[n].  W, I [T - first_frame, knn, N]; seed [N] or None; L [T*N, M];
    pred [N, T]; L_init / pred_init: the buffers as they were before the call (for a run with a later first frame).

    Returns dict(violations={condition: count}, worst=dict(soft=worst error / bound), bound=...).  Conditions:
      index ...... 0 <= I < min(n, cxt_size + 1) * N (n * N when cxt_size is None): a frame reads labels that exist        (exact)
      soft ....... |L[n] - L64[n]| <= gather_bound(knn)
      pred ....... pred[:, n] is the FIRST maximum of the device's own row of L                                            (exact)
      frame0 ..... frame 0 of L is the one-hot seed (and pred[:, 0] the seed where the call wrote it)                       (exact)
      untouched .. frames before first_frame are bitwise those of L_init / pred_init                                       (exact)
    """
    import torch
    dev = W.device if torch.is_tensor(W) else torch.device("cpu")
    Wd, Id, Ld, pd = _to_t64(W, dev), _to_t64(I, dev, True), _to_t64(L, dev), _to_t64(pred, dev)
    knn, N = Wd.shape[1], Wd.shape[2]
    T = Ld.shape[0] // N
    bound = gather_bound(knn)
    viol = {k: 0 for k in GATHER_CONDITIONS}
    worst = dict(soft=0.0)
    classes = torch.arange(M, device=dev)
    if seed is not None:
        sd = _to_t64(seed, dev)
        onehot = (sd[:, None] == classes[None].to(torch.float64)).to(torch.float64)
        viol["frame0"] += int((Ld[:N] != onehot).sum())
        if pred_init is None:
            viol["frame0"] += int((pd[:, 0] != sd).sum())
    if L_init is not None:
        viol["untouched"] += int((Ld[:first_frame * N] != _to_t64(L_init, dev)[:first_frame * N]).sum())
    if pred_init is not None:
        viol["untouched"] += int((pd[:, :first_frame] != _to_t64(pred_init, dev)[:, :first_frame]).sum())
    for n in range(first_frame, T):
        Wn, In = Wd[n - first_frame], Id[n - first_frame]
        hi = (min(n, cxt_size + 1) if cxt_size is not None else n) * N
        ok = (In >= 0) & (In < hi)
        viol["index"] += int((~ok).sum())
        Ic = torch.where(ok, In, torch.zeros_like(In))
        p = (Wn[..., None] * Ld[Ic]).sum(0)                                         # [N, M]; Ld[Ic]: the untruncated list (Q7)
        row = Ld[n * N:(n + 1) * N]
        err = (row - p).abs() / bound
        viol["soft"] += int((~(err <= 1)).sum())
        worst["soft"] = max(worst["soft"], float(err[torch.isfinite(err)].max()) if torch.isfinite(err).any() else 0.0)
        is_max = row == row.max(-1, keepdim=True).values
        first_max = torch.where(is_max, classes[None].expand_as(row), torch.full_like(row, M, dtype=torch.int64)).min(-1).values
        viol["pred"] += int((pd[:, n] != first_max.to(torch.float64)).sum())
    return dict(violations=viol, worst=worst, bound=bound)


def xent_metric(emb, dtype=np.float32):
    """'Horizontality' metric: within-frame affinity on channel-shifted features (quirk Q8),
    temperature 0.1, CE of A_i^T against the identity -> xent [N, T-1]."""
    T, N, C = emb.shape
    eh = l2_normalize(emb, dtype).astype(dtype)
    A = np.einsum("tnc,tmc->tnm", eh[:, :, :-1], eh[:, :, 1:]) / dtype(0.1)
    out = np.zeros((N, T - 1), np.float32)
    for i in range(T - 1):
        X = A[i].T  # input [N(batch), N(class)]
        m = X.max(-1, keepdims=True)
        lse = np.log(np.exp(X - m).sum(-1)) + m[:, 0]
        out[:, i] = -(np.diag(X) - lse)
    return out


# --------------------------------------------------------------------------------------------
# dataset
# --------------------------------------------------------------------------------------------
def dataset_geometry(H, W, length, dim, overlap):
    h, w = dim
    oh, ow = overlap
    nh = (H - oh) // (h - oh)
    pxw = length * w - ow * (length - 1)
    nw = (W - (length * (w - ow) + ow)) // (w - ow) + 1
    pxh = nh * h - oh * (nh - 1)
    return nh, nw, pxh, pxw


def unfold_item(rg, index, length, dim, overlap):
    h, w = dim
    oh, ow = overlap
    nh, nw, pxh, pxw = dataset_geometry(rg.shape[0], rg.shape[1], length, dim, overlap)
    out = np.empty((length, nh, h, w), np.float32)
    c_item = (w - ow) * index
    for t in range(length):
        for n in range(nh):
            out[t, n] = rg[n * (h - oh):n * (h - oh) + h, c_item + t * (w - ow):c_item + t * (w - ow) + w]
    return out
