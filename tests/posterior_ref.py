"""The posterior of the ordered label maps (include/crw_hip.h, crw_labelmap_ordered_posterior) restated in fp64 over the fp64
probabilities of `dense_ref.probabilities` / `joint_ref.window_probs`: plain loops over rows and states, every column at once.  It
shares no code with `crw_hip` or the kernel, and not their route either: the messages are rescaled by their sums, the boundary's
distribution is read from the marginals (P(B_k <= r) = sum_{s >= k} gamma[r][s], differenced), the mean as sum_r P(B_k > r).
`enumerate_paths` is the definition itself -- every monotone path of a small column, weighed and counted -- and proves `posterior`.
Also here: the derived accuracy bound rho and `check`.  Shared by test_posterior.py and test_posterior_gpu.py."""
import itertools

import numpy as np

import dense_ref as dr
import ordered_ref as od

FLOOR = 1e-4  # the host side's default


def positions(labels, order):
    """labels [rows, cols] (any integers) -> the position of every label in `order`, -1 outside it."""
    labels = np.asarray(labels).astype(np.int64)
    pos = np.full(labels.shape, -1, dtype=np.int64)
    for s, k in enumerate(order):
        pos[labels == int(k)] = s
    return pos


def picks(labels, order):
    """-> b^ [S-1, cols] int64: per boundary k = 1 ... S-1 the first row whose label's position is >= k, `rows` if none."""
    pos = positions(labels, order)
    rows, cols = pos.shape
    out = np.full((len(order) - 1, cols), rows, dtype=np.int64)
    for k in range(1, len(order)):
        for r in range(rows - 1, -1, -1):
            out[k - 1] = np.where(pos[r] >= k, r, out[k - 1])
    return out


def evidence(probs, order, floor):
    """probs [M, rows, cols] fp64 -> f [rows, S, cols] = max(probs[order[s]], floor)."""
    return np.maximum(np.stack([probs[int(k)] for k in order], 1), floor)


def marginals(f):
    """f [rows, S, cols] -> gamma [rows, S, cols], the marginals of the monotone paths under the product of f along the path."""
    rows, S, cols = f.shape
    alpha, beta = np.empty_like(f), np.empty_like(f)
    for r in range(rows):
        for s in range(S):
            before = np.ones(cols) if r == 0 else sum(alpha[r - 1, t] for t in range(s + 1))
            alpha[r, s] = f[r, s] * before
        alpha[r] /= alpha[r].sum(0)
    for r in range(rows - 1, -1, -1):
        for s in range(S):
            beta[r, s] = np.ones(cols) if r == rows - 1 else sum(f[r + 1, t] * beta[r + 1, t] for t in range(s, S))
        beta[r] /= beta[r].sum(0)
    gamma = alpha * beta
    return gamma / gamma.sum(1, keepdims=True)


def posterior(probs, order, labels, floor=FLOOR):
    """-> (post [rows, cols], hz [3, S-1, cols]) in fp64: the definition's outputs for the label map `labels`; hz[2] is the rms."""
    f = evidence(probs, order, floor)
    rows, S, cols = f.shape
    gamma = marginals(f)
    pos = positions(labels, order)
    post = np.where(pos >= 0, np.take_along_axis(gamma, np.maximum(pos, 0)[:, None], 1)[:, 0], 0.0)
    pick = picks(labels, order)
    hz = np.empty((3, S - 1, cols))
    hz[0] = pick
    for k in range(1, S):
        cdf = np.concatenate([gamma[:, k:].sum(1), np.ones((1, cols))])  # P(B_k <= r), r = 0 ... rows
        pmf = np.diff(cdf, axis=0, prepend=0.0)
        at = np.arange(rows + 1, dtype=np.float64)[:, None]
        hz[1, k - 1] = (1.0 - cdf[:rows]).sum(0)
        hz[2, k - 1] = np.sqrt(np.maximum((pmf * (at - pick[k - 1][None]) ** 2).sum(0), 0.0))
    return post, hz


def enumerate_paths(f_col, pick):
    """The definition on ONE column by enumeration: f_col [rows, S], pick [S-1] -> (gamma [rows, S], E[B_k] [S-1],
    E[(B_k - pick_k)^2] [S-1]) over every monotone path."""
    rows, S = f_col.shape
    gamma, m1, m2, total = np.zeros((rows, S)), np.zeros(S - 1), np.zeros(S - 1), 0.0
    for x in itertools.product(range(S), repeat=rows):
        if any(x[r] > x[r + 1] for r in range(rows - 1)):
            continue
        w = float(np.prod([f_col[r, x[r]] for r in range(rows)]))
        total += w
        for r in range(rows):
            gamma[r, x[r]] += w
        for k in range(1, S):
            b = next((r for r in range(rows) if x[r] >= k), rows)
            m1[k - 1] += w * b
            m2[k - 1] += w * (b - pick[k - 1]) ** 2
    return gamma / total, m1 / total, m2 / total


def rho(probs, order, floor=FLOOR):
    """The derived bound per column -> [cols].  Every interpolated probability is within B of its fp64 value, so every f is off by a
    relative eps[r][s] = B / max(e, floor), and by nothing where e <= floor - B (both sides read the floor); a path's weight by at
    most exp(+-Delta), Delta_c = sum_r max_s eps[r][s] + rows (S + 4) 2^-23 for the roundings of the scans; a posterior expectation
    of a non-negative quantity -- a ratio of two sums of such weights -- by a relative exp(2 Delta_c) - 1."""
    e = np.stack([probs[int(k)] for k in order], 1)  # [rows, S, cols]
    rows, S, _ = e.shape
    eps = np.where(e <= floor - dr.B, 0.0, dr.B / np.maximum(e, floor))
    delta = eps.max(1).sum(0) + rows * (S + 4) * 2.0 ** -23
    return np.expm1(2 * delta)


RHO_MAX = 0.05  # the condition on every column of every accuracy case


def check(probs, order, labels, post, hz, floor=FLOOR, what="", slack=1.0, against=None):
    """One call's outputs against the reference on the fp64 probabilities [M, rows, cols] (teacher-forced for a joint call):
    hz[0] exact; post, hz[1] and hz[2]^2 within `slack` * rho_c relative of the reference plus `slack` * 1e-6 absolute.
    against: another route's (post, hz) to compare with in place of the reference -- both lie within rho of it, so within 2 rho of
    each other: pass slack=2.  Prints the worst ratio error / tolerance before it asserts -> that ratio."""
    want_post, want_hz = posterior(probs, order, labels, floor) if against is None else against
    want_post, want_hz = np.asarray(want_post, dtype=np.float64), np.asarray(want_hz, dtype=np.float64)
    ref_post, ref_hz = (want_post, want_hz) if against is None else posterior(probs, order, labels, floor)
    post, hz = np.asarray(post, dtype=np.float64), np.asarray(hz, dtype=np.float64)
    bound = rho(probs, order, floor)
    assert bound.max() <= RHO_MAX, f"{what}: rho {bound.max():.3e} on a column: not an accuracy case"
    assert post.shape == want_post.shape and hz.shape == want_hz.shape
    assert np.isfinite(post).all() and np.isfinite(hz).all(), f"{what}: a value that is not finite"
    assert post.min() >= 0 and post.max() <= 1
    assert np.array_equal(hz[0], want_hz[0]), f"{what}: a pick differs"
    worst = 0.0
    for name, got, want, ref in (("post", post, want_post, ref_post), ("E[B]", hz[1], want_hz[1], ref_hz[1]),
                                 ("E[(B - pick)^2]", hz[2] ** 2, want_hz[2] ** 2, ref_hz[2] ** 2)):
        tol = slack * (bound * np.abs(ref) + 1e-6)
        ratio = float((np.abs(got - want) / tol).max())
        worst = max(worst, ratio)
        print(f"{what}: {name} worst error / tolerance {ratio:.3e} (largest rho {bound.max():.3e}, largest error {np.abs(got - want).max():.3e})")
    assert worst <= 1.0, f"{what}: outside the bound by a factor {worst:.3f}"
    return worst


# ---- the quality claim ---------------------------------------------------------------------------------------------------------------
def ece_aurc(conf, right, bins=10):
    """`metrics.Calibration`'s rule on the host: bin b = min(bins - 1, floor(conf * bins)), ECE = sum_b |accuracy_b - mean conf_b|
    n_b / n; the AURC through that class itself."""
    import torch
    from metrics import Calibration
    conf, right = np.asarray(conf, dtype=np.float64).ravel(), np.asarray(right, dtype=bool).ravel()
    b = np.minimum(bins - 1, np.floor(conf.astype(np.float32) * np.float32(bins)).astype(np.int64))
    counts = np.stack([np.bincount(b, minlength=bins), np.bincount(b, weights=right, minlength=bins).astype(np.int64)], 1)
    sums = np.bincount(b, weights=conf, minlength=bins)
    cal = Calibration(torch.tensor(counts), torch.tensor(sums), None)
    return cal.ece, cal.aurc


def bar_coverage(hz, gt, order, z=2.0, slack=1.0):
    """The share of columns whose true boundary lies within z * rms + slack rows of the pick, per boundary -> [S-1] (columns in
    which the ground truth has the boundary)."""
    hz = np.asarray(hz, dtype=np.float64)
    truth = picks(gt, order)
    rows = np.asarray(gt).shape[0]
    out = []
    for k in range(hz.shape[1]):
        has = truth[k] < rows
        out.append(float((np.abs(truth[k] - hz[0, k]) <= z * hz[2, k] + slack)[has].mean()) if has.any() else float("nan"))
    return np.asarray(out)


def quality(gt, labels, maxprob, post, hz, order, what=""):
    """The quality figures of one case, printed, then asserted: ECE of post <= 0.5 x ECE of maxprob (both against `labels`), mean
    bar coverage at z = 2, slack = 1 >= 0.85; the AURC of both is printed and not asserted."""
    gt, labels = np.asarray(gt), np.asarray(labels).astype(np.int64)
    right = labels == gt
    ece_m, aurc_m = ece_aurc(maxprob, right)
    ece_p, aurc_p = ece_aurc(post, right)
    cover = bar_coverage(hz, gt, order)
    truth = picks(gt, order)
    rmse = np.sqrt(((truth - np.asarray(hz[0], dtype=np.float64)) ** 2).mean(1))
    print(f"{what}: accuracy {right.mean():.4f}; ECE maxprob {ece_m:.4f} -> post {ece_p:.4f} (ratio {ece_p / ece_m:.3f}); AURC maxprob "
          f"{aurc_m:.5f}, post {aurc_p:.5f}; bar coverage {np.round(cover, 3)} (mean {np.nanmean(cover):.3f}); mean predicted rms "
          f"{np.asarray(hz[2]).mean(1).round(2)} against true RMSE {rmse.round(2)}")
    assert ece_p <= 0.5 * ece_m
    assert np.nanmean(cover) >= 0.85
    return ece_p / ece_m, float(np.nanmean(cover))
