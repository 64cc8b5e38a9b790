"""The definition of layer horizons and thickness (include/crw_hip.h, crw_horizons) restated literally: plain Python loops over
numpy arrays, per column, per run.  It shares no code with `crw_hip._horizons_cpu` or the kernel and is the reference both are
compared with, integer for integer.  Also here: the comparison helper of the tests (`compare`) and the invariants every result
must satisfy (`check_invariants`)."""
import numpy as np

NSTATS = 18
QUANTITIES = ("top", "bottom", "count")


def classes_of(gt, pred, K, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1):
    """-> (class of every pixel in gt, in pred: int, -1 = none; masked pixels; invalid pixels)."""
    g, p = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    masked = np.zeros(g.shape, dtype=bool)
    if ignore_gt >= 0:
        masked |= g == ignore_gt
    if ignore_pred >= 0:
        masked |= p == ignore_pred
    if ignore_aux >= 0:
        masked |= np.asarray(aux, dtype=np.float64) == ignore_aux
    with np.errstate(invalid="ignore"):
        is_class = lambda v: (v == np.floor(v)) & (v >= 0) & (v < K)  # NaN fails every comparison
        invalid = ~masked & ~(is_class(g) & is_class(p))
    none = masked | invalid
    cg = np.where(none, -1, np.where(none, 0, g)).astype(np.int64)
    cp = np.where(none, -1, np.where(none, 0, p)).astype(np.int64)
    return cg, cp, int(masked.sum()), int(invalid.sum())


def runs_of(column):
    """Maximal runs of equal entries of a 1-D sequence -> [(label, first row, length)]."""
    n = len(column)
    if n == 0:
        return []
    column = np.asarray(column)
    starts = [0] + [int(r) + 1 for r in np.flatnonzero(column[1:] != column[:-1])]
    ends = starts[1:] + [n]
    return [(int(column[a]), a, b - a) for a, b in zip(starts, ends)]


def picks_of(classes, K, min_run):
    """[3, K, cols] int32 of one map's classes [rows, cols]: top, bottom, count."""
    rows, cols = classes.shape
    out = np.zeros((3, K, cols), dtype=np.int32)
    out[:2] = -1
    for c in range(cols):
        for lab, start, length in runs_of(classes[:, c]):
            if lab < 0 or length < min_run:
                continue
            if out[0, lab, c] < 0:
                out[0, lab, c] = start
            out[1, lab, c] = start + length - 1
            out[2, lab, c] += length
    return out


def stats_of(picks, K, tol):
    """[K, 18] int64 from picks [2, 3, K, cols]."""
    cols = picks.shape[3]
    stats = np.zeros((K, NSTATS), dtype=np.int64)
    for k in range(K):
        for c in range(cols):
            hg, hp = picks[0, 2, k, c] > 0, picks[1, 2, k, c] > 0
            if hg and hp:
                stats[k, 0] += 1
                for q in range(3):
                    d = int(picks[1, q, k, c]) - int(picks[0, q, k, c])
                    stats[k, 3 + 5 * q] += abs(d)
                    stats[k, 4 + 5 * q] += d * d
                    stats[k, 5 + 5 * q] = max(stats[k, 5 + 5 * q], abs(d))
                    stats[k, 6 + 5 * q] += abs(d) <= tol
                    stats[k, 7 + 5 * q] += d
            elif hg:
                stats[k, 1] += 1
            elif hp:
                stats[k, 2] += 1
    return stats


def horizons_ref(gt, pred, K, aux=None, ignore_gt=-1, ignore_pred=-1, ignore_aux=-1, min_run=1, tol=2):
    """-> (stats [K, 18] int64, dropped [2] int64, picks [2, 3, K, cols] int32)."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    cg, cp, masked, invalid = classes_of(gt, pred, K, None if aux is None else np.asarray(aux), ignore_gt, ignore_pred, ignore_aux)
    picks = np.stack([picks_of(cg, K, min_run), picks_of(cp, K, min_run)])
    return stats_of(picks, K, tol), np.array([masked, invalid], dtype=np.int64), picks


def compare(got, want):
    """Differences between two (stats, dropped, picks) results (picks may be None on either side) -> list of strings, empty when
    every integer agrees."""
    out = []
    names = ("stats", "dropped", "picks")
    for name, a, b in zip(names, got, want):
        if a is None or b is None:
            continue
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            out.append(f"{name}: shape {a.shape} != {b.shape}")
            continue
        bad = np.argwhere(a != b)
        if len(bad):
            i = tuple(bad[0])
            out.append(f"{name}: {len(bad)} differ, first at {i}: {a[i]} != {b[i]}")
    return out


def check_invariants(stats, dropped, picks, rows, cols, K, min_run):
    """The invariants of the definition, on any result."""
    picks, stats = np.asarray(picks).astype(np.int64), np.asarray(stats)
    assert picks.shape == (2, 3, K, cols) and stats.shape == (K, NSTATS) and len(dropped) == 2
    top, bottom, count = picks[:, 0], picks[:, 1], picks[:, 2]
    has = count > 0
    assert ((top >= 0) == has).all() and ((bottom >= 0) == has).all()
    assert (top[~has] == -1).all() and (bottom[~has] == -1).all() and (count >= 0).all()
    assert (top[has] <= bottom[has]).all() and (bottom[has] < rows).all()
    assert (count[has] >= min_run).all() and (count[has] <= bottom[has] - top[has] + 1).all()
    assert (count.sum(1) <= rows).all()  # a pixel has one class per map
    assert (stats[:, :3].sum(1) <= cols).all() and (stats[:, :3] >= 0).all()
    assert (stats[:, 0] == (has[0] & has[1]).sum(1)).all()
    assert 0 <= int(dropped[0]) + int(dropped[1]) <= rows * cols
    for q in range(3):
        sa, sq, mx, nw, sd = (stats[:, 3 + 5 * q + j] for j in range(5))
        assert (mx <= sa).all() and (sa <= sq).all() and (abs(sd) <= sa).all() and (nw <= stats[:, 0]).all() and (mx * mx <= sq).all()
