"""The two fp64 audits of label-propagation lists (`oracle.topk_lists_audit`, `oracle.gather_audit`) on the CPU: they pass the
lists of the fp32 oracle -- a correct fp32 implementation with another summation order than the kernels' --, and they report
every defect planted into those lists, one at a time.  `tests/test_labelprop_lists_gpu.py` runs the same audits, on inputs from
the same generators, over every route of `csrc/labelprop.hip`; this file is what shows that those tests would fail on a subtly
wrong kernel."""
import functools

import numpy as np
import pytest
import torch

from oracle import crw_oracle as orc


# ---- inputs, shared with the GPU test ----------------------------------------------------------------------------------------
def lp_embeddings(T, N, C, seed):
    """Raw features base + 0.5 * noise [T,N,C] (normalised by the caller: by the device on the GPU, by the oracle here)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).float()


def twin_frames(feats):
    """Every odd frame repeats the frame before it: each key has a twin with the same score bit for bit (exact ties)."""
    out = feats.clone() if torch.is_tensor(feats) else feats.copy()
    out[1::2] = out[0:out.shape[0] - 1:2][: out[1::2].shape[0]]
    return out


def scrambled_seed(N, M):
    """Neighbouring nodes carry different labels, so every index and every weight of a list shows in the soft labels."""
    return ((7 * torch.arange(N)) % M).float()


# (T, N, C, cxt, radius, knn, first, grid_w): the vector-kernel shapes of the GPU test and its two-halves 48-node shape
VECTOR_SHAPES = [(6, 5, 7, 100, 2, 2, 1, 1), (10, 12, 16, 3, 2, 5, 1, 1), (12, 30, 16, 4, 3, 7, 1, 5), (9, 33, 20, 3, 9, 8, 2, 11)]
SHAPE_48 = (90, 48, 128, 80, 10, 20, 1, 1)
TRUNC = (10, 12, 16, 3, 2, 5, 1, 1)   # truncated context, empty slots in frame 1
GRID = (12, 30, 16, 4, 3, 7, 1, 5)


def _ehat32(shape, twin=False):
    T, N, C = shape[:3]
    eh = orc.l2_normalize(lp_embeddings(T, N, C, T + N).numpy(), np.float32).astype(np.float32)
    return twin_frames(eh) if twin else eh


@functools.lru_cache(maxsize=None)
def _lists(shape, temp, twin=False):
    T, N, C, cxt, radius, knn, first, gw = shape
    eh = _ehat32(shape, twin)
    W, I, V = orc.labelprop_lists(eh, cxt, radius, temp, knn, first, gw)
    for a in (eh, W, I, V):
        a.setflags(write=False)   # shared among the tests: planted defects go into copies
    return eh, W, I, V


def _audit(shape, temp, eh, W, I, V):
    T, N, C, cxt, radius, knn, first, gw = shape
    return orc.topk_lists_audit(eh, cxt, radius, temp, knn, first, gw, W, I, V)


def _fired(res):
    return {k for k, v in res["violations"].items() if v}


def _softmax32(v):
    """fp32 softmax of a list's logits (empty slots -inf -> 0)"""
    e = np.exp((v - v.max()).astype(np.float32))
    return (e / e.sum(dtype=np.float32)).astype(np.float32)


def _logits64(shape, temp, eh, n):
    """fp64 logits of frame n [keys of the truncated list, queries] and the in-band mask of the same shape"""
    T, N, C, cxt, radius, knn, first, gw = shape
    frames = list(range(n)) if n <= cxt + 1 else [0] + list(range(n - cxt, n))
    e = eh.astype(np.float64)
    S = e[frames].reshape(-1, C) @ e[n].T / temp
    return S, np.tile(orc.band_bias(N, radius, np.float64, gw) == 0, (len(frames), 1))


# ---- the audits pass a correct fp32 implementation ---------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [0.1, 0.01, 0.001])
@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("shape", VECTOR_SHAPES + [SHAPE_48])
def test_fp32_oracle_lists_pass_the_topk_audit(shape, temp, twin):
    eh, W, I, V = _lists(shape, temp, twin)
    res = _audit(shape, temp, eh, W, I, V)
    print("worst error / bound:", res["worst"])
    assert not _fired(res), res
    assert all(v <= 1 for v in res["worst"].values()), res
    noV = _audit(shape, temp, eh, W, I, None)
    assert not _fired(noV), noV


def test_the_oracle_lists_hold_what_the_defects_need():
    """empty slots, truncation and ties are really there -- otherwise the planted-defect tests below would be vacuous"""
    eh, W, I, V = _lists(TRUNC, 0.1)
    assert np.isinf(V[0]).any() and not np.isinf(V[-1]).any()   # frame 1: 3 in-band keys < knn = 5
    assert TRUNC[0] - 1 > TRUNC[3] + 1                          # frames beyond cxt + 1: truncated context
    eh, W, I, V = _lists(TRUNC, 0.1, True)
    assert (V[:, :-1] == V[:, 1:])[~np.isinf(V[:, 1:])].any()   # exact ties between twins


# ---- planted defects ---------------------------------------------------------------------------------------------------------
def _copies(shape, temp=0.1):
    eh, W, I, V = _lists(shape, temp)
    return eh, W.copy(), I.copy(), V.copy()


def _report(shape, eh, W, I, V, temp=0.1):
    """(conditions violated with V, conditions violated without V)"""
    return _fired(_audit(shape, temp, eh, W, I, V)), _fired(_audit(shape, temp, eh, W, I, None))


@pytest.mark.parametrize("shape", [TRUNC, GRID, SHAPE_48])
def test_defect_index_shifted_by_one_node(shape):
    eh, W, I, V = _copies(shape)
    q = shape[1] // 2
    I[-1, 1, q] += 1
    withV, noV = _report(shape, eh, W, I, V)
    assert "scores" in withV, withV
    assert noV, "not reported without V"


@pytest.mark.parametrize("shape", [TRUNC, GRID, SHAPE_48])
def test_defect_kth_neighbour_replaced_by_a_candidate_well_below_the_boundary(shape):
    """consistent in everything else (its own logit, weights renormalised, order kept): only the selection condition can see it"""
    eh, W, I, V = _copies(shape)
    T, N, C, cxt, radius, knn, first, gw = shape
    q = N // 2
    S, inband = _logits64(shape, 0.1, eh, T - 1)
    cand = np.where(inband[:, q])[0]
    assert len(cand) > knn
    worst = cand[np.argmin(S[cand, q])]
    assert worst not in I[-1, :, q] and S[worst, q] < V[-1, -1, q] - 1.0
    I[-1, -1, q] = worst
    V[-1, -1, q] = np.float32(S[worst, q])
    W[-1, :, q] = _softmax32(V[-1, :, q])
    withV, noV = _report(shape, eh, W, I, V)
    assert withV == {"selection"}, withV
    assert noV == {"selection"}, noV


@pytest.mark.parametrize("shape", [TRUNC, SHAPE_48])
def test_defect_key_one_node_outside_the_disc(shape):
    eh, W, I, V = _copies(shape)
    T, N, C, cxt, radius, knn, first, gw = shape
    q, node = 0, radius                      # |node - q| == radius: the first node that is NOT closer than the radius
    S, inband = _logits64(shape, 0.1, eh, T - 1)
    idx = (S.shape[0] // N - 1) * N + node   # in the last context frame
    assert not inband[idx, q] and inband[idx - 1, q]
    I[-1, -1, q] = idx
    V[-1, -1, q] = np.float32(S[idx, q])
    W[-1, :, q] = _softmax32(V[-1, :, q])
    withV, noV = _report(shape, eh, W, I, V)
    assert "disc" in withV and "disc" in noV, (withV, noV)


@pytest.mark.parametrize("shape", [TRUNC, GRID])
def test_defect_truncation_without_frame_0(shape):
    """the last cxt + 1 frames as context where the reference keeps frame 0 + the last cxt"""
    eh, W, I, V = _copies(shape)
    T, N, C, cxt, radius, knn, first, gw = shape
    assert T - 1 > cxt + 1
    for n in range(cxt + 2, T):
        w, i, v = orc.labelprop_weights(eh[n - cxt - 1:n + 1], cxt + 1, cxt, radius, 0.1, knn, np.float32, gw, return_scores=True)
        W[n - first], I[n - first], V[n - first] = w, i, v
    withV, noV = _report(shape, eh, W, I, V)
    assert "scores" in withV, withV
    assert noV, "not reported without V"


@pytest.mark.parametrize("shape", [TRUNC, GRID, SHAPE_48])
def test_defect_weight_row_made_with_twice_the_temperature(shape):
    eh, W, I, V = _copies(shape)
    q = shape[1] // 2
    W[-1, :, q] = _softmax32(V[-1, :, q] / np.float32(2))
    withV, noV = _report(shape, eh, W, I, V)
    assert withV == {"weights"} and noV == {"weights"}, (withV, noV)


@pytest.mark.parametrize("shape", [TRUNC, GRID, SHAPE_48])
def test_defect_two_slots_swapped(shape):
    eh, W, I, V = _copies(shape)
    q = shape[1] // 2
    for a in (W, I, V):
        a[-1, [1, 2], q] = a[-1, [2, 1], q]
    withV, noV = _report(shape, eh, W, I, V)
    assert withV == {"order"}, withV
    assert noV <= {"order"}   # two neighbours of equal fp32 weight cannot be told apart without their logits
    if W[-1, 1, q] != W[-1, 2, q]:
        assert noV == {"order"}


def test_defect_twins_swapped():
    """two candidates with the same logit bit for bit in the wrong order: only the tie rule on the device's own values sees it"""
    eh, W, I, V = (a.copy() for a in _lists(TRUNC, 0.1, True))
    f, j, q = np.argwhere((V[:, :-1] == V[:, 1:]) & ~np.isinf(V[:, 1:]))[0]
    I[f, [j, j + 1], q] = I[f, [j + 1, j], q]
    assert _fired(_audit(TRUNC, 0.1, eh, W, I, V)) == {"order"}


@pytest.mark.parametrize("shape", [TRUNC, GRID, SHAPE_48])
def test_defect_duplicate_index(shape):
    eh, W, I, V = _copies(shape)
    q = shape[1] // 2
    I[-1, 1, q] = I[-1, 0, q]
    V[-1, 1, q] = V[-1, 0, q]
    W[-1, :, q] = _softmax32(V[-1, :, q])
    withV, noV = _report(shape, eh, W, I, V)
    assert "distinct" in withV and "distinct" in noV, (withV, noV)


def test_defect_nonzero_weight_in_an_empty_slot():
    eh, W, I, V = _copies(TRUNC)
    assert np.isinf(V[0, -1, 3])
    W[0, -1, 3] = np.float32(1e-3)
    withV, noV = _report(TRUNC, eh, W, I, V)
    assert "empty" in withV and "empty" in noV, (withV, noV)
    eh, W, I, V = _copies(TRUNC)
    I[0, -1, 3] = 1                          # an index left in an empty slot
    assert _report(TRUNC, eh, W, I, V)[0] == {"empty"}


# ---- the gather audit --------------------------------------------------------------------------------------------------------
def _gather32(W, I, seed, M, T, N, cxt=None, last_max=False):
    """The weighted label sums of `orc.labelprop` on given lists, fp32.  cxt: DROP quirk Q7 -- apply the indices to the truncated
    label list [frame 0] + last cxt frames, as they address the keys.  last_max: the label is the LAST maximum of a row."""
    L = np.zeros((T * N, M), np.float32)
    L[:N] = (seed[:, None] == np.arange(M)[None]).astype(np.float32)
    pred = np.zeros((N, T), np.float32)
    pred[:, 0] = seed
    for n in range(1, T):
        Ln = L if cxt is None or n <= cxt + 1 else np.concatenate([L[:N], L[(n - cxt) * N:n * N]])
        p = (Ln[I[n - 1]] * W[n - 1][..., None]).sum(0)
        L[n * N:(n + 1) * N] = p
        pred[:, n] = M - 1 - p[:, ::-1].argmax(-1) if last_max else p.argmax(-1)
    return L, pred


GATHER_SHAPES = [(TRUNC, 16), (TRUNC, 3), (GRID, 16), ((14, 10, 16, 3, 4, 5, 1, 1), 16)]


@pytest.mark.parametrize("shape,M", GATHER_SHAPES)
@pytest.mark.parametrize("temp", [0.1, 0.01, 0.001])
def test_fp32_oracle_soft_labels_pass_the_gather_audit(shape, M, temp):
    T, N, C, cxt, radius, knn, first, gw = shape
    eh, W, I, V = _lists(shape, temp)
    seed = scrambled_seed(N, M).numpy()
    # the raw features: `labelprop` normalises them as `_ehat32` does, so its lists are bit for bit those of `_lists`
    pred, L = orc.labelprop(lp_embeddings(T, N, C, T + N).numpy(), seed, M, cxt, radius, temp, knn, grid_w=gw, return_soft=True)
    res = orc.gather_audit(W, I, seed, M, 1, cxt, L, pred)
    print("worst error / bound:", res["worst"])
    assert not _fired(res), res
    L2, pred2 = _gather32(W, I, seed, M, T, N)
    assert not _fired(orc.gather_audit(W, I, seed, M, 1, cxt, L2, pred2))
    assert np.array_equal(L2, L) and np.array_equal(pred2, pred)
    assert (seed[1:] != seed[:-1]).all()     # scrambled: neighbouring nodes carry different labels


@pytest.mark.parametrize("shape,M", [(TRUNC, 16), (GRID, 16), ((14, 10, 16, 3, 4, 5, 1, 1), 16)])
def test_defect_soft_labels_gathered_on_the_truncated_label_list(shape, M):
    """quirk Q7 dropped: the indices address [frame 0] + the last cxt frames of L too"""
    T, N, C, cxt, radius, knn, first, gw = shape
    eh, W, I, V = _lists(shape, 0.1)
    seed = scrambled_seed(N, M).numpy()
    L, pred = _gather32(W, I, seed, M, T, N, cxt=cxt)
    res = orc.gather_audit(W, I, seed, M, 1, cxt, L, pred)
    assert _fired(res) == {"soft"}, res


def test_defect_label_is_the_last_maximum_of_a_row_with_two_equal_maxima():
    shape, M = TRUNC, 16
    T, N, C, cxt, radius, knn, first, gw = shape
    eh, W, I, V = _copies(shape)
    seed = scrambled_seed(N, M).numpy()
    # frame 1, query 4: two neighbours of weight 1/2 with different labels -> two classes at exactly 0.5
    W[0, :, 4] = 0
    W[0, :2, 4] = 0.5
    I[0, :, 4] = 0
    I[0, :2, 4] = (4, 5)
    assert seed[4] != seed[5]
    L, pred = _gather32(W, I, seed, M, T, N)
    assert sorted(L[N + 4])[-2:] == [0.5, 0.5]
    assert not _fired(orc.gather_audit(W, I, seed, M, 1, cxt, L, pred))
    L, pred = _gather32(W, I, seed, M, T, N, last_max=True)
    res = orc.gather_audit(W, I, seed, M, 1, cxt, L, pred)
    assert _fired(res) == {"pred"} and res["violations"]["pred"] >= 1, res


def test_gather_audit_reports_a_wrong_seed_frame_and_touched_earlier_frames():
    shape, M = TRUNC, 16
    T, N, C, cxt, radius, knn, first, gw = shape
    eh, W, I, V = _lists(shape, 0.1)
    seed = scrambled_seed(N, M).numpy()
    L, pred = _gather32(W, I, seed, M, T, N)
    first = 3
    L_init, pred_init = L.copy(), pred.copy()
    L_init[first * N:], pred_init[:, first:] = -7, -1
    ok = orc.gather_audit(W[first - 1:], I[first - 1:], seed, M, first, cxt, L, pred, L_init, pred_init)
    assert not _fired(ok), ok
    Lb = L.copy()
    Lb[2 * N + 1, 0] += 1e-3                 # a frame before first_frame rewritten
    assert "untouched" in _fired(orc.gather_audit(W[first - 1:], I[first - 1:], seed, M, first, cxt, Lb, pred, L_init, pred_init))
    Lb = L.copy()
    Lb[2, :] = Lb[3, :]                      # a wrong one-hot row in frame 0
    assert "frame0" in _fired(orc.gather_audit(W, I, seed, M, 1, cxt, Lb, pred))
