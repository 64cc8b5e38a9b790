"""The joint ordered label map (include/crw_hip.h, crw_labelmap_ordered_joint) in fp64: the probabilities of a source's window
(`dense_ref.probabilities`, mirrored and cut as the definition says), the rows selected under a given `took`, the geometry cases the
CPU route and the kernel are held to, and the paired layered items of the quality claim.  It imports `dense_ref` and `ordered_ref`
unchanged and shares no code with `crw_hip` or the kernel.  Shared by test_joint.py and test_joint_gpu.py; a reference is computed
once per case and never modified."""
import functools

import numpy as np
import torch

import dense_ref as dr
import ordered_ref as od


def window_probs(L, T, N, M, rows, cols, col0, ncols, flip):
    """A source's window in fp64 -> [M, rows, ncols]: output column x is column col0 + x of the source's `cols`-wide map, which
    with `flip` holds what column cols - 1 - (col0 + x) of the unflipped map holds."""
    p = dr.probabilities(np.asarray(L), T, N, M, rows, cols)
    if flip:
        p = p[:, :, ::-1]
    return np.ascontiguousarray(p[:, :, col0:col0 + ncols])


def selected(took, probs_a, probs_b):
    """The rows the decode runs over, teacher-forced on `took` [rows, ncols] (True: source b's)."""
    return np.where(np.asarray(took, dtype=bool)[None], probs_b, probs_a)


# Geometry cases: N, M, rows, ncols, order, source a, source b; a source is (T, cols, col0, flip).
# ncols 1 / 20 / 64 / 65 / 84: a dead-lane tail, exactly one wave, two waves; rows 1 / 2 / 8 / 9 / 64 / 65 / 83: the edges of the
# backward scan's 8 words and of the 64 row knots a wave holds, rows < N and rows > N; N 1 / 10 / 12; T = 1; the four flip
# combinations; M 3 / 4 / 6 / 16 with S < M and orders that are no identity; (T, cols) that differ between the sources with
# col0 > 0 -- the corrected tail: a 3-frame item's whole 20-column map against columns 64 ... 83 of a 12-frame item's.
CASES = [
    dict(N=10, M=3, rows=83, ncols=84, order=(0, 1, 2), a=(12, 84, 0, False), b=(12, 84, 0, True)),
    dict(N=12, M=4, rows=64, ncols=64, order=(2, 0, 3), a=(8, 64, 0, False), b=(8, 64, 0, True)),
    dict(N=10, M=4, rows=65, ncols=20, order=(0, 1, 2, 3), a=(3, 20, 0, False), b=(12, 84, 64, True)),
    dict(N=1, M=6, rows=9, ncols=65, order=(5, 1, 3, 0), a=(5, 65, 0, True), b=(7, 100, 30, False)),
    dict(N=12, M=16, rows=8, ncols=1, order=(3, 15, 0, 7, 9), a=(1, 1, 0, False), b=(1, 5, 2, True)),
    dict(N=10, M=16, rows=2, ncols=20, order=tuple(range(15, -1, -1)), a=(4, 40, 20, True), b=(6, 20, 0, True)),
    dict(N=12, M=6, rows=1, ncols=84, order=(1, 0), a=(9, 84, 0, False), b=(9, 90, 6, False)),
    dict(N=10, M=3, rows=64, ncols=65, order=(2, 0), a=(5, 65, 0, False), b=(12, 130, 65, False)),
]
case_id = lambda c: f"N{c['N']}M{c['M']}_{c['rows']}x{c['ncols']}"


class Case:
    """A geometry case with its Dirichlet soft labels (float32 torch, what the code under test reads) and the fp64 probabilities
    of both windows, read-only."""

    def __init__(self, index):
        c = CASES[index]
        self.N, self.M, self.rows, self.ncols, self.order = c["N"], c["M"], c["rows"], c["ncols"], c["order"]
        self.geo = (c["a"], c["b"])
        self.L = tuple(dr.dirichlet_rows(T, self.N, self.M, seed=40 + 2 * index + k) for k, (T, _, _, _) in enumerate(self.geo))
        self.probs = tuple(window_probs(L.numpy(), T, self.N, self.M, self.rows, cols, col0, self.ncols, flip)
                           for L, (T, cols, col0, flip) in zip(self.L, self.geo))
        for p in self.probs:
            p.setflags(write=False)

    def source(self, k, L=None):
        """Source k as `labelmap_ordered_joint` takes it (L: this case's, or the same values elsewhere, e.g. on a device)."""
        T, cols, col0, flip = self.geo[k]
        return (self.L[k] if L is None else L, T, cols, col0, flip)

    @property
    def shared(self):
        return (self.N, self.M, self.rows, self.ncols, self.order)


@functools.lru_cache(maxsize=None)
def case(index):
    return Case(index)


def dense_confidence(hip, src, N, M, rows, ncols, kind):
    """conf_k of the definition on the route of `src`'s tensor: `labelmap_dense` on the source's own geometry, cut to the window."""
    L, T, cols, col0, flip = src
    return hip.labelmap_dense(L, T, N, M, rows, cols, confidence=kind, flip=flip)[1][:, col0:col0 + ncols]


def check_against_the_definition(hip, c, labels, conf, kind, La=None, Lb=None, what=""):
    """The two halves of the definition for one call's outputs on case `c`: conf is `merge_confidence`'s of the two dense confidence
    maps, bit for bit; the labels, teacher-forced on that `took`, pass `ordered_ref.check` against the selected fp64 rows."""
    ca, cb = (dense_confidence(hip, c.source(k, L), c.N, c.M, c.rows, c.ncols, kind) for k, L in ((0, La), (1, Lb)))
    took = cb > ca
    want = torch.where(took, cb, ca)
    assert torch.equal(conf.view(torch.int32), want.view(torch.int32)), f"{what}: conf is not the confidence merge's"
    od.check(selected(took.cpu().numpy(), *c.probs), labels.cpu().numpy(), c.order, what=f"{what} took {int(took.sum())} of {took.numel()}")


# ---- the quality claim: a forward and a reverse pass over one ground truth ----------------------------------------------------------
PAIRS = [(q, seed) for q in od.QUALITY for seed in od.SEEDS]


@functools.lru_cache(maxsize=None)
def paired_case(index):
    """-> (gt, L_fwd, L_rev float32 torch, (T, N, rows, cols, M)): forward `layered_case(seed)`, reverse `layered_case(seed + 100)`
    on the same ground truth with its frames reversed, to be passed with flip=True."""
    q, seed = PAIRS[index]
    T, N, rows, cols, temp, M, share = q
    gt, Lf = od.layered_case(*q, seed)
    _, Lr = od.layered_case(*q, seed + 100)
    Lr = np.ascontiguousarray(Lr.reshape(T, N, M)[::-1]).reshape(T * N, M)
    gt.setflags(write=False)
    return gt, torch.tensor(Lf), torch.tensor(Lr), (T, N, rows, cols, M)


def steps_back(labels, order):
    """Columns of `labels` whose position in `order` decreases somewhere down the column."""
    pos = od.positions(np.asarray(labels).astype(np.int64), order)
    return int((pos[1:] < pos[:-1]).any(0).sum())


def quality_counts(hip, index, device="cpu"):
    """One paired case on `device` -> (wrong pixels of the confidence merge of the two ordered maps, its columns that step back,
    wrong pixels of the joint map, its columns that step back, its most class changes in a column, M); prints them."""
    gt, Lf, Lr, (T, N, rows, cols, M) = paired_case(index)
    Lf, Lr = Lf.to(device), Lr.to(device)
    order = tuple(range(M))
    fl, fc = hip.labelmap_ordered(Lf, T, N, M, rows, cols, order, confidence="maxprob")
    rl, rc = hip.labelmap_ordered(Lr, T, N, M, rows, cols, order, confidence="maxprob", flip=True)
    merged, mconf, _ = hip.merge_confidence(fl, fc, rl, rc)
    joint, jconf = hip.labelmap_ordered_joint((Lf, T, cols, 0, False), (Lr, T, cols, 0, True), N, M, rows, cols, order, confidence="maxprob")
    assert torch.equal(jconf.view(torch.int32), mconf.view(torch.int32))
    merged, joint = merged.cpu().numpy().astype(np.int64), joint.cpu().numpy().astype(np.int64)
    out = (int((merged != gt).sum()), steps_back(merged, order), int((joint != gt).sum()), steps_back(joint, order),
           int(od.changes(joint).max()), M)
    print(f"{PAIRS[index]} on {device}: wrong pixels merge {out[0]} ({out[1]} columns step back) -> joint {out[2]} ({out[3]} step back), "
          f"at most {out[4]} changes in a column")
    return out


def check_quality(counts):
    """The per-case assertions of the quality claim on `quality_counts`' tuple."""
    wm, _, wj, bj, ch, M = counts
    assert bj == 0
    assert wj <= 1.05 * wm
    assert ch <= M - 1
