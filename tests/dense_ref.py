"""fp64 reference of the dense label map (`crw_hip.labelmap_dense`, csrc/labelmap_dense.hip), built from the integer formula of
include/crw_hip.h: exact knots, weights as exact rationals rounded once to fp64 -- no source coordinate in floating point.  Shared by
test_dense.py and test_dense_gpu.py; a reference is computed once per case (`reference` is cached) and never modified."""
import functools

import numpy as np
import torch

B = 12 * 2.0 ** -24  # the bound on an interpolated probability in fp32 (DESIGN.md section 3 derives it)

# (T, N, M, rows, cols)
SHAPES = [(1, 1, 2, 3, 5), (2, 2, 2, 4, 4), (5, 7, 3, 37, 29), (9, 12, 6, 50, 61), (8, 8, 4, 5, 3), (4, 3, 16, 9, 130)]
SLAB = (24, 48, 6, 410, 768)
EXACT = [(3, 2, 2, 16, 48), (4, 6, 3, 48, 32)]
KINDS = ("maxprob", "margin", "entropy")


def knots(n_in, n_out):
    """-> (i0, i1 int64 [n_out], w float64 [n_out]): a = (2x + 1) n_in - n_out, d = 2 n_out."""
    x = np.arange(n_out, dtype=np.int64)
    a, d = (2 * x + 1) * n_in - n_out, 2 * n_out
    i0 = np.where(a <= 0, 0, a // d)
    edge = (a <= 0) | (i0 >= n_in - 1)
    i0 = np.minimum(i0, n_in - 1)
    i1 = np.where(edge, i0, i0 + 1)
    w = np.where(edge, 0.0, (a - i0 * d).astype(np.float64) / np.float64(d))
    return i0, i1, w


def probabilities(L, T, N, M, rows, cols):
    """L [T*N, M] -> the interpolated probabilities [M, rows, cols] in fp64 (node (n, t) is row t*N + n; image rows along n)."""
    P = np.asarray(L, dtype=np.float64).reshape(T, N, M)
    i0, i1, wr = knots(N, rows)
    j0, j1, wc = knots(T, cols)
    corner = lambda i, j: P[j[None, :], i[:, None]]  # [rows, cols, M]
    wr, wc = wr[:, None, None], wc[None, :, None]
    top = (1 - wc) * corner(i0, j0) + wc * corner(i0, j1)
    bot = (1 - wc) * corner(i1, j0) + wc * corner(i1, j1)
    return np.ascontiguousarray(((1 - wr) * top + wr * bot).transpose(2, 0, 1))


def confidences(p):
    """p [M, rows, cols] fp64 -> dict kind -> [rows, cols] fp64, the formulas of `crw_hip.labelprop_confidence`."""
    M = p.shape[0]
    s = np.sort(p, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, p * np.log(p), 0.0)
    return dict(maxprob=np.minimum(s[-1], 1.0), margin=np.minimum(s[-1] - s[-2], 1.0),
                entropy=np.clip(1 + plogp.sum(0) / np.log(M), 0.0, 1.0))


class Ref:
    """probs [M, rows, cols], labels [rows, cols] (lowest class among equal maxima), gap [rows, cols] (largest minus second
    largest probability) and conf[kind] [rows, cols], all fp64 / int64 numpy, read-only."""

    def __init__(self, L, T, N, M, rows, cols):
        self.probs = probabilities(L, T, N, M, rows, cols)
        self.labels = self.probs.argmax(0)
        s = np.sort(self.probs, axis=0)
        self.gap = s[-1] - s[-2]
        self.conf = confidences(self.probs)
        for a in (self.probs, self.labels, self.gap, *self.conf.values()):
            a.setflags(write=False)


def dirichlet_rows(T, N, M, seed=0):
    """Dirichlet(1) probability rows [T*N, M], float32 (what the kernel reads; the reference reads the same float32 values)."""
    g = np.random.default_rng(1000 * seed + 7 * T + 3 * N + M)
    return torch.tensor(g.dirichlet(np.ones(M), size=T * N).astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference(shape, seed=0):
    """(T, N, M, rows, cols) -> (L float32 [T*N, M] torch, Ref) on Dirichlet(1) rows; computed once per process."""
    T, N, M, rows, cols = shape
    L = dirichlet_rows(T, N, M, seed)
    return L, Ref(L.numpy(), T, N, M, rows, cols)


def exact_rows(T, N, M, seed=0):
    """Rows for the exact cases (rows = N 2^k, cols = T 2^j: every weight is an odd multiple of a power of two, every product and
    sum exact in fp32): random one-hot rows -- between one-hot nodes such weights leave no two classes equal at the top --, and
    frames 0 and 1 set to the dyadic tie row (0, ..., 1/2, 1/2), so that every pixel between those two frames is an EXACT tie of
    the two highest classes."""
    g = np.random.default_rng(50 + seed)
    L = torch.nn.functional.one_hot(torch.tensor(g.integers(0, M, size=T * N)), M).float()
    L[:2 * N] = 0
    L[:2 * N, M - 2:] = 0.5
    return L


def entropy_tolerance(ref):
    """Tolerance for the entropy confidence on rows with every entry >= 1e-3 -> (mask [rows, cols], tol [rows, cols]): 4 x what
    the formula in fp32 torch misses fp64 by on the reference's own rows (the rule of the confidence kernel's test), plus the
    bound B on every probability propagated through the formula, B sum_m |1 + ln p_m| / ln M."""
    p = torch.tensor(ref.probs)
    M = p.shape[0]
    ok = (p >= 1e-3).all(0)
    f = lambda q: (1 + (q * q.log()).sum(0) / np.log(M)).clamp(0, 1)
    miss = (f(p.float()).double() - f(p))[ok].abs().max() if ok.any() else torch.tensor(0.0)
    tol = 4 * float(miss) + B * (1 + p.clamp(min=1e-3).log()).abs().sum(0) / np.log(M)
    return ok.numpy(), tol.numpy()


def check_outputs(ref, labels, conf=None, kind=None, what=""):
    """Item 2 of the issue for one call's outputs (numpy / torch, [rows, cols]) against `ref`: a label may differ from the
    reference's only where the reference's top-two gap is <= 2B, and such pixels are at most 1e-3 of the map; the class a label
    names has, in the reference, a probability within 2B of the largest (both computed values are within B of theirs); maxprob
    within B, margin within 2B, entropy within `entropy_tolerance`.  Prints the figures before it asserts."""
    labels = np.asarray(labels).astype(np.int64)
    rows, cols = ref.labels.shape
    assert labels.shape == (rows, cols)
    M = ref.probs.shape[0]
    assert labels.min() >= 0 and labels.max() < M
    diff = labels != ref.labels
    share = diff.mean()
    worst_gap = float(ref.gap[diff].max()) if diff.any() else 0.0
    # the class the map names, in the reference's probabilities: a maximum of a row computed within B lies within 2B of the true one
    chosen = np.take_along_axis(ref.probs, labels[None], 0)[0]
    short = float((ref.probs.max(0) - chosen).max())
    print(f"{what}: labels differ at {int(diff.sum())} of {diff.size} pixels (share {share:.2e}), largest reference gap there "
          f"{worst_gap:.3e} (2B = {2 * B:.3e}), chosen class short of the maximum by {short:.3e}")
    assert worst_gap <= 2 * B and short <= 2 * B
    assert share <= 1e-3
    if conf is None:
        return
    conf = np.asarray(conf).astype(np.float64)
    assert conf.shape == (rows, cols) and conf.min() >= 0 and conf.max() <= 1
    err = np.abs(conf - ref.conf[kind])
    if kind == "entropy":
        ok, tol = entropy_tolerance(ref)
        print(f"{what}: entropy on {int(ok.sum())} pixels, worst error {float(err[ok].max()) if ok.any() else 0.0:.3e}, "
              f"tolerance there {float(tol[ok].min()) if ok.any() else 0.0:.3e} ... {float(tol[ok].max()) if ok.any() else 0.0:.3e}")
        assert (err[ok] <= tol[ok]).all()
    else:
        bound = B if kind == "maxprob" else 2 * B
        print(f"{what}: {kind} worst error {float(err.max()):.3e} (bound {bound:.3e})")
        assert err.max() <= bound
