"""Layer horizons and thickness, host side: the case table of the feature (shared with tests/test_horizons_gpu.py), the vectorised
CPU route `crw_hip._horizons_cpu` against the literal reference tests/horizons_ref.py, the invariants of the definition, the
arithmetic of `metrics.Horizons`, the argument checks, the comparison helper against planted defects, the measurement that motivates
`min_run`, and the command line with a stubbed label propagation."""
import functools
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG
from horizons_ref import check_invariants, compare, horizons_ref, picks_of, stats_of

import crw_hip

F32, I8 = torch.float32, torch.int8
DTYPES = [(F32, F32), (F32, I8), (I8, I8)]
AUX = [None, F32, I8]
AUX_IGNORE = 9


# ---- maps -------------------------------------------------------------------------------------------------------------------------
def layered(rows, cols, K, seed, speckle=0.05):
    """(a) K undulating bands, the prediction's interfaces displaced, `speckle` of the pixels of both relabelled at random."""
    rng = np.random.default_rng(seed)
    r, c = np.arange(rows, dtype=np.float64)[:, None], np.arange(cols, dtype=np.float64)[None, :]
    gt = np.clip(np.floor((r + 0.04 * rows * np.sin(2 * np.pi * c / 90.0)) * K / max(rows, 1)), 0, K - 1)
    pr = np.clip(np.floor((r + 0.05 * rows * np.sin(2 * np.pi * c / 70.0 + seed) + 0.02 * rows) * K / max(rows, 1)), 0, K - 1)
    for m in (gt, pr):
        hit = rng.random(m.shape) < speckle
        m[hit] = rng.integers(0, K, int(hit.sum()))
    return gt, pr


def run_at_every_offset(rows, min_run):
    """(b) column j: background 0 with one run of class 1 starting at row j -- of length min_run in gt (it just qualifies) and
    min_run - 1 in pred (it just does not), for every j at which the longer run fits; then the same with the maps swapped."""
    n = rows - min_run + 1
    a, b = np.zeros((rows, n)), np.zeros((rows, n))
    for j in range(n):
        a[j:j + min_run, j] = 1
        b[j:j + min_run - 1, j] = 1
    return np.concatenate([a, b], 1), np.concatenate([b, a], 1)


def spanning(rows, cols):
    """(c) even columns: one class over the whole column; odd columns: a run from row 1 to rows - 2 (gt) / rows - 1 (pred)."""
    gt, pr = np.ones((rows, cols)), np.ones((rows, cols))
    gt[0, 1::2] = gt[rows - 1, 1::2] = 0
    pr[0, 1::2] = 0
    return gt, pr


def alternating(rows, cols):
    """(d) labels alternate every row, in opposite phase in the two maps."""
    gt = (np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2
    return gt.astype(np.float64), 1.0 - gt


def broken_runs(rows, cols, K, fp32):
    """(e) class 1 down every column of both maps, with one pixel in the middle that is masked (gt == ignore_gt = 0) or no label
    at all -- in gt for even columns, in pred for odd ones.  fp32: NaN, 2.5, K, -1; int8: K, -1."""
    gt, pr = np.ones((rows, cols)), np.ones((rows, cols))
    bad = ([float("nan"), 2.5, float(K), -1.0] if fp32 else [float(K), -1.0]) + [0.0]
    for c in range(cols):
        v = bad[(c // 2) % len(bad)]
        (gt if (c % 2 == 0 or v == 0.0) else pr)[rows // 2 - (c % 3 == 0), c] = v
    return gt, pr


def uniform(rows, cols, K, seed):
    """(f) uniformly random labels."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, K, (rows, cols)).astype(np.float64), rng.integers(0, K, (rows, cols)).astype(np.float64)


def extremes(rows, cols):
    """(g) class 1 at row 0 in gt and at row rows - 1 in pred, background 0."""
    gt, pr = np.zeros((rows, cols)), np.zeros((rows, cols))
    gt[0], pr[rows - 1] = 1, 1
    return gt, pr


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# a case: (kind, rows, cols, K, min_run, dtype pair index, aux index, row_slabs); the maps depend on all but the last
def _cases():
    out, n = [], 0

    def add(kind, rows, cols, K, min_run, slabs=(0,), dt=None, aux=None):
        nonlocal n
        for s in slabs:
            out.append((kind, rows, cols, K, max(1, min_run), n % 3 if dt is None else dt, (n // 3) % 3 if aux is None else aux, s))
        n += 1

    all_slabs = (0, 1, 2, 3, 5, 8)
    Ks, runs = (2, 6, 16), (1, 2, 3, 7, None)
    # (a) layered + speckle: every rows with every cols once, K / min_run / dtypes / aux cycling; every dtype route at one shape
    i = 0
    for rows in (1, 2, 37, 70, 410):
        for cols in (1, 63, 64, 65, 257, 1000):
            if rows == 410 and cols in (257, 1000) and i % 2:
                i += 1
                continue
            mr = runs[i % 5] or rows
            add("a", rows, cols, Ks[i % 3], mr, slabs=all_slabs if (rows in (37, 70) and cols in (65, 257)) else (8,) if rows == 2 else (0,))
            i += 1
    for dt in range(3):
        for aux in range(3):
            add("a", 37, 65, 6, 3, slabs=(0, 3), dt=dt, aux=aux)
            add("a", 70, 130, 16, 2, slabs=(5,), dt=dt, aux=aux)
    for mr in (1, 2, 3, 7, 70):
        for K in Ks:
            add("a", 70, 65, K, mr, slabs=(0, 8))
    # (b) a run at every offset: every slab border is crossed by a run that just qualifies and one that just does not
    for rows in (37, 70):
        for mr in (1, 2, 3, 7, rows):
            add("b", rows, 0, 2, mr, slabs=all_slabs)
    add("b", 2, 0, 2, 2, slabs=(8,))
    add("b", 410, 0, 6, 7)
    # (c) runs that span three and more slabs
    for rows in (37, 70):
        for mr in (1, 7, rows - 2, rows):
            add("c", rows, 65, 2, mr, slabs=all_slabs)
    add("c", 410, 64, 6, 408)
    # (d) alternating labels, min_run 2: nothing qualifies
    add("d", 37, 65, 2, 2, slabs=all_slabs)
    add("d", 70, 257, 6, 2, slabs=(0, 8))
    add("d", 2, 63, 2, 2, slabs=(8,))
    # (e) masked and invalid pixels inside a long run
    for rows in (37, 70):
        for dt in range(3):
            add("e", rows, 65, 6, 3, slabs=(0, 2, 5, 8), dt=dt, aux=0)
    add("e", 410, 63, 16, 7, dt=0, aux=0)
    # (f) uniformly random labels, K = 16
    for rows, cols in ((37, 65), (70, 257), (410, 64)):
        for mr in (1, 2):
            add("f", rows, cols, 16, mr, slabs=(0, 8) if rows < 410 else (0,))
    # (g) the largest differences: the maxima and the squares
    add("g", 37, 65, 2, 1, slabs=all_slabs)
    add("g", 410, 63, 6, 1)
    add("g", 32768, 3, 2, 1, slabs=(0, 8), dt=0, aux=0)
    # (h) empty maps
    for rows, cols in ((0, 65), (37, 0), (0, 0)):
        add("h", rows, cols, 6, 1, slabs=(0, 3), dt=0, aux=0)
    return out


CASES = _cases()
MAP_CASES = sorted({c[:7] for c in CASES})  # what the maps and the reference depend on (not the slabs)
case_id = lambda c: "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def build(case):
    """case[:7] -> (gt, pred, aux | None: CPU tensors of the case's dtypes; keyword arguments; the reference's result)."""
    kind, rows, cols, K, min_run, dt, aux_i = case
    seed = rows * 131 + cols * 7 + K
    kw = dict(min_run=min_run, tol=2)
    if kind == "a":
        gt, pr = layered(rows, cols, K, seed)
    elif kind == "b":
        gt, pr = run_at_every_offset(rows, min_run)
    elif kind == "c":
        gt, pr = spanning(rows, cols)
    elif kind == "d":
        gt, pr = alternating(rows, cols)
    elif kind == "e":
        gt, pr = broken_runs(rows, cols, K, fp32=DTYPES[dt][0] == F32 and DTYPES[dt][1] == F32)
        kw["ignore_gt"] = 0
    elif kind == "f":
        gt, pr = uniform(rows, cols, K, seed)
    elif kind == "g":
        gt, pr = extremes(rows, cols)
    else:
        gt, pr = np.zeros((rows, cols)), np.zeros((rows, cols))
    aux = None
    if AUX[aux_i] is not None:
        rng = np.random.default_rng(seed + 1)
        aux = np.where(rng.random(gt.shape) < 0.03, float(AUX_IGNORE), 0.0)
        kw["ignore_aux"] = AUX_IGNORE
    tg, tp = torch.from_numpy(gt).to(DTYPES[dt][0]), torch.from_numpy(pr).to(DTYPES[dt][1])
    ta = None if aux is None else torch.from_numpy(aux).to(AUX[aux_i])
    ref = horizons_ref(tg.numpy(), tp.numpy(), K, None if ta is None else ta.numpy(), **kw)
    return tg, tp, ta, kw, ref


# ---- 1-3. the CPU route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MAP_CASES, ids=case_id)
def test_cpu_route_equals_the_reference(case):
    gt, pred, aux, kw, ref = build(case)
    K = case[3]
    got = crw_hip.horizons(gt, pred, K, aux=aux, want_picks=True, **kw)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64 and got[2].dtype == torch.int32
    assert compare([t.numpy() for t in got], ref) == []
    check_invariants(*[t.numpy() for t in got], gt.shape[0], gt.shape[1], K, kw["min_run"])
    check_invariants(*ref, gt.shape[0], gt.shape[1], K, kw["min_run"])
    mask = {k: v for k, v in kw.items() if k.startswith("ignore")}
    assert torch.equal(got[1], crw_hip.confusion(gt, pred, K, aux=aux, **mask)[1])
    two = crw_hip.horizons(gt, pred, K, aux=aux, **kw)
    assert len(two) == 2 and torch.equal(two[0], got[0])


def test_the_case_table_covers_what_it_claims():
    assert 200 <= len(CASES) <= 600
    kinds = {c[0] for c in CASES}
    assert kinds == set("abcdefgh")
    for rows in (37, 70):
        assert {c[7] for c in CASES if c[1] == rows} == {0, 1, 2, 3, 5, 8}
    assert any(c[1] == 2 and c[7] == 8 for c in CASES)
    assert {(c[5], c[6]) for c in CASES} == {(d, a) for d in range(3) for a in range(3)}
    assert {c[3] for c in CASES} == {2, 6, 16} and {1, 2, 3, 7} <= {c[4] for c in CASES}
    assert any(c[4] == c[1] for c in CASES if c[1] > 7)
    # (b): the run of min_run in gt qualifies in every column, the run of min_run - 1 in pred in none
    gt, pred, aux, kw, (stats, dropped, picks) = build(("b", 37, 0, 2, 3, 0, 0))
    n = 37 - 3 + 1
    assert gt.shape == (37, 2 * n) and (picks[0, 2, 1, :n] == 3).all() and (picks[1, 2, 1, :n] == 0).all()
    assert (picks[0, 0, 1, :n] == np.arange(n)).all() and stats[1, 1] == n and stats[1, 2] == n and stats[1, 0] == 0
    # (d): everything absent
    _, _, _, _, (stats, dropped, picks) = build(("d", 37, 65, 2, 2, 0, 0))
    assert (stats == 0).all() and (picks[:, :2] == -1).all() and (picks[:, 2] == 0).all()
    # (e): the bad pixel splits the run and is counted
    gt, _, _, _, (stats, dropped, picks) = build(("e", 37, 65, 6, 3, 0, 0))
    assert dropped[0] > 0 and dropped[1] > 0 and dropped.sum() == 65 and (picks[:, 2, 1] == 36).all()
    # (g): the largest difference and its square
    _, _, _, _, (stats, _, _) = build(("g", 32768, 3, 2, 1, 0, 0))
    assert stats[1, 5] == 32767 and stats[1, 4] == 3 * 32767 ** 2 and stats[1, 7] == 3 * 32767 and stats[1, 0] == 3


# ---- 4. the report ----------------------------------------------------------------------------------------------------------------
def test_report_arithmetic_by_hand():
    """Three columns, K = 3.  Class 0: found in all three, top differences +1, -3, 0, bottom 0, 0, +2, thickness -1, +3, +2.  Class 1:
    found in one column (d = 0 throughout), missing in one, spurious in one.  Class 2: in neither map."""
    from metrics import Horizons
    stats = np.zeros((3, 18), dtype=np.int64)
    stats[0] = [3, 0, 0, 4, 10, 3, 2, -2, 2, 4, 2, 3, 2, 6, 14, 3, 2, 4]
    stats[1] = [1, 1, 1] + [0, 0, 0, 1, 0] * 3
    hz = Horizons(torch.from_numpy(stats), torch.tensor([5, 0]), rows=50, cols=3, min_run=3, tol=2)
    assert hz.mae(0, "top") == pytest.approx(4 / 3) and hz.mae(0, "bottom") == pytest.approx(2 / 3) and hz.mae(0, "thickness") == 2.0
    assert hz.mae(0, "count") == hz.mae(0, "thickness")
    e = hz.errors["top"]
    assert e["rmse"][0] == pytest.approx(math.sqrt(10 / 3)) and e["bias"][0] == pytest.approx(-2 / 3) and e["max"][0] == 3.0
    assert e["within"][0] == pytest.approx(2 / 3) and hz.errors["thickness"]["within"][0] == pytest.approx(2 / 3)
    assert hz.mae(1) == 0.0 and hz.errors["top"]["within"][1] == 1.0
    assert hz.presence_precision[1] == 0.5 and hz.presence_recall[1] == 0.5 and hz.presence_recall[0] == 1.0
    assert all(math.isnan(v) for v in (hz.mae(2), hz.errors["top"]["rmse"][2], hz.errors["bottom"]["max"][2], hz.presence_precision[2],
                                       hz.presence_recall[2], hz.errors["thickness"]["within"][2]))
    assert hz.mean_mae("top") == pytest.approx((4 / 3 + 0) / 2) and hz.mean_mae() == hz.mean_mae("top")
    assert hz.dropped == (5, 0) and list(hz.n_both) == [3, 1, 0] and list(hz.n_missing) == [0, 1, 0] and list(hz.n_spurious) == [0, 1, 0]
    # row_spacing scales the distances and nothing else
    m = Horizons(stats, None, 50, 3, 3, 2, row_spacing=2.5, unit="m")
    assert m.mae(0, "top") == pytest.approx(2.5 * 4 / 3) and m.errors["top"]["max"][0] == 7.5 and m.errors["top"]["bias"][0] == pytest.approx(-5 / 3)
    assert m.errors["top"]["rmse"][0] == pytest.approx(2.5 * math.sqrt(10 / 3)) and m.errors["top"]["within"][0] == pytest.approx(2 / 3)
    assert np.array_equal(m.stats, stats) and m.sum_abs["top"][0] == 4 and m.max_abs["top"][0] == 3 and m.dropped is None
    d = m.to_dict()
    assert d["unit"] == "m" and d["row_spacing"] == 2.5 and d["top"]["sum_abs_rows"] == [4, 0, 0] and d["n_both"] == [3, 1, 0]
    assert d["top"]["mean_mae"] == pytest.approx(2.5 * 2 / 3) and math.isnan(d["top"]["mae"][2]) and "dropped" not in d
    assert json.loads(json.dumps(hz.to_dict()))["dropped"] == dict(masked=5, invalid=0)
    text = str(hz)
    lines = text.splitlines()
    assert "min_run 3" in lines[0] and "tol 2" in lines[0] and len({len(l) for l in lines[1:] if l.strip() and "mean" not in l}) == 1
    assert sum("thickness" in l for l in lines) == 4 and " in m)" in str(m).splitlines()[0]
    # no class found anywhere
    none = Horizons(np.zeros((2, 18), dtype=np.int64), [0, 0], 10, 4, 1, 2)
    assert math.isnan(none.mean_mae("top")) and math.isnan(none.mean_mae("thickness")) and "-" in str(none)
    for bad in (np.zeros((3, 17)), np.zeros(18)):
        with pytest.raises(ValueError):
            Horizons(bad, None, 10, 4, 1, 2)
    with pytest.raises(ValueError):
        Horizons(stats, None, 50, 2, 3, 2)  # more columns counted than there are
    with pytest.raises(ValueError):
        Horizons(stats, None, 50, 3, 3, 2, row_spacing=0)
    with pytest.raises(ValueError):
        hz.mae(0, "middle")


# ---- 5. argument checks -----------------------------------------------------------------------------------------------------------
def test_argument_checks():
    g = torch.zeros(4, 5)
    ok = lambda **kw: crw_hip.horizons(g, g, 2, **kw)
    assert len(ok()) == 2 and len(ok(want_picks=True)) == 3
    for K in (1, 17):
        with pytest.raises(ValueError, match="K must be in 2 ... 16"):
            crw_hip.horizons(g, g, K)
    with pytest.raises(ValueError, match="an ignore label is a class id"):
        ok(ignore_gt=-2)
    with pytest.raises(ValueError, match="ignore_aux needs aux"):
        ok(ignore_aux=4)
    with pytest.raises(ValueError, match="must hold the same number of labels"):
        crw_hip.horizons(g, torch.zeros(4, 6), 2)
    with pytest.raises(ValueError, match="must hold the same number of labels"):
        ok(aux=torch.zeros(5, 4), ignore_aux=1)
    with pytest.raises(ValueError, match=r"\[rows, cols\]"):
        crw_hip.horizons(g.flatten(), g.flatten(), 2)
    for kw in (dict(min_run=0), dict(tol=-1), dict(row_slabs=9), dict(row_slabs=-1)):
        with pytest.raises(ValueError):
            ok(**kw)
    with pytest.raises(ValueError, match="at most 32768"):
        crw_hip.horizons(torch.zeros(32769, 1), torch.zeros(32769, 1), 2)
    with pytest.raises(ValueError, match="picks_out"):
        ok(picks_out=torch.zeros(2, 3, 2, 4, dtype=torch.int32))
    assert crw_hip.HORIZONS_ENTRY_POINTS == ("crw_horizons_ws_bytes", "crw_horizons")
    assert len(crw_hip.SIGNATURES["crw_horizons"][1]) == 22 and len(crw_hip.SIGNATURES["crw_horizons_ws_bytes"][1]) == 3
    assert set(crw_hip.HORIZONS_ENTRY_POINTS) <= set(crw_hip.SIGNATURES)
    head = open(crw_hip.HEADER_PATH).read()
    assert "#define CRW_ABI_VERSION 8" in head and "crw_hip.has_horizons()" in head


def test_windows_and_other_dtypes_on_the_cpu():
    wide = torch.from_numpy(layered(37, 200, 6, 3)[0]).float()
    wide_p = torch.from_numpy(layered(37, 200, 6, 3)[1]).float()
    a, b = 3, 140
    got = crw_hip.horizons(wide[:, a:b], wide_p[:, a:b], 6, min_run=3, want_picks=True)
    ref = horizons_ref(wide[:, a:b].numpy(), wide_p[:, a:b].numpy(), 6, min_run=3)
    assert compare([t.numpy() for t in got], ref) == []
    same = crw_hip.horizons(wide[:, a:b].long(), wide_p[:, a:b].double(), 6, min_run=3, want_picks=True)
    assert all(torch.equal(x, y) for x, y in zip(got, same))
    out = torch.full((2, 3, 6, b - a), 77, dtype=torch.int32)
    assert crw_hip.horizons(wide[:, a:b], wide_p[:, a:b], 6, min_run=3, picks_out=out)[2] is out and torch.equal(out, got[2])


# ---- 6. the comparison helper sees planted defects ---------------------------------------------------------------------------------
def _defects():
    """Ten wrong implementations of the picks, as functions of (classes [rows, cols], K, min_run) -> [3, K, cols]."""
    from horizons_ref import runs_of

    def variant(qualifies=lambda lab, n, mr: n >= mr, split=None, bottom_first=False, count_all=False, top_last=False, cut=None,
                off=None, count_span=False, ignore_none=False):
        def f(classes, K, min_run):
            rows, cols = classes.shape
            out = np.zeros((3, K, cols), dtype=np.int32)
            out[:2] = -1
            for c in range(cols):
                col = classes[:, c].copy()
                if ignore_none:  # a masked pixel does not end a run: it takes the label above it
                    for r in range(1, rows):
                        if col[r] < 0:
                            col[r] = col[r - 1]
                runs = runs_of(col)
                if cut is not None:  # runs are cut at a slab border and never joined
                    runs = [x for lab, s, n in runs for x in ([(lab, s, cut - s), (lab, cut, s + n - cut)] if s < cut < s + n else [(lab, s, n)])]
                for lab, s, n in runs:
                    if lab < 0:
                        continue
                    if count_all:
                        out[2, lab, c] += n
                    if not qualifies(lab, n, min_run):
                        continue
                    if off is not None and s <= off < s + n and s > 0:
                        s, n = s - 1, n + 1  # a pick off by one where the run crosses the border
                    if out[0, lab, c] < 0 or top_last:
                        out[0, lab, c] = s
                    if not (bottom_first and out[1, lab, c] >= 0):
                        out[1, lab, c] = s + n - 1
                    if not count_all:
                        out[2, lab, c] += n
                if count_span:
                    has = out[0, :, c] >= 0
                    out[2, has, c] = out[1, has, c] - out[0, has, c] + 1
            return out
        return f

    return {
        "off by one at a slab border": variant(off=18),
        "a run of min_run - 1 accepted": variant(qualifies=lambda lab, n, mr: n >= mr - 1),
        "a masked pixel does not end a run": variant(ignore_none=True),
        "bottom of the first run": variant(bottom_first=True),
        "count includes short runs": variant(count_all=True),
        "runs never joined across a border": variant(cut=18),
        "top of the last run": variant(top_last=True),
        "count is bottom - top + 1": variant(count_span=True),
        "min_run + 1 required": variant(qualifies=lambda lab, n, mr: n > mr),
        "class 0 never qualifies": variant(qualifies=lambda lab, n, mr: n >= mr and lab > 0),
    }


def test_planted_defects_are_reported():
    from horizons_ref import classes_of
    seen = {}
    probes = [("a", 37, 65, 6, 3, 0, 1), ("b", 37, 0, 2, 3, 0, 0), ("b", 37, 0, 2, 2, 0, 0), ("e", 37, 65, 6, 3, 0, 0), ("c", 37, 65, 2, 7, 0, 0)]
    defects = _defects()
    assert len(defects) == 10
    for case in probes:
        gt, pred, aux, kw, ref = build(case)
        K, mr = case[3], kw["min_run"]
        mask = {k: v for k, v in kw.items() if k.startswith("ignore")}
        cg, cp, _, _ = classes_of(gt.numpy(), pred.numpy(), K, None if aux is None else aux.numpy(), **mask)
        assert np.array_equal(np.stack([picks_of(cg, K, mr), picks_of(cp, K, mr)]), ref[2])
        for name, f in defects.items():
            picks = np.stack([f(cg, K, mr), f(cp, K, mr)])
            diff = compare((stats_of(picks, K, 2), ref[1], picks), ref)
            if diff:
                seen.setdefault(name, diff)
    assert set(seen) == set(defects), set(defects) - set(seen)
    # and in the statistics and dropped alone
    gt, pred, aux, kw, ref = build(probes[0])
    for j in range(18):
        s = ref[0].copy()
        s[2, j] += 1
        assert compare((s, ref[1], None), ref) and compare((s, ref[1], None), ref)[0].startswith("stats")
    assert compare((ref[0], ref[1] + [0, 1], ref[2]), ref)[0].startswith("dropped")
    assert compare((ref[0], ref[1], ref[2][:, :, :, :-1]), ref)[0].startswith("picks: shape")
    assert compare(ref, ref) == []


# ---- 7. why min_run ----------------------------------------------------------------------------------------------------------------
def test_run_length_awareness_is_what_makes_the_pick_usable():
    """410 x 600, 4 layered classes, 2 % of the pixels relabelled at random (seeded): the top of every class but the topmost, picked
    in the noisy map, against the clean map's.  With min_run = 3 the mean error is at most a tenth of the first-row pick's."""
    spec = importlib.util.spec_from_file_location("segment_all_for_horizons", os.path.join(PKG, "scripts", "segment_all.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    K = 4
    clean = cli.synthetic_reference(410, 600, K)
    g = torch.Generator().manual_seed(5)
    hit = torch.rand(clean.shape, generator=g) < 0.02
    noisy = torch.where(hit, torch.randint(0, K, clean.shape, generator=g).float(), clean)
    from metrics import Horizons
    mae = {}
    for mr in (1, 3):
        stats, dropped = crw_hip.horizons(clean, noisy, K, min_run=mr)
        hz = Horizons(stats, dropped, 410, 600, mr, 2)
        assert (hz.n_both[1:] == 600).all() and hz.dropped == (0, 0)
        mae[mr] = [hz.mae(k, "top") for k in range(1, K)]
    print("top MAE, classes 1..3: min_run 1", mae[1], "min_run 3", mae[3])
    for k in range(K - 1):
        assert mae[1][k] > 5 and mae[3][k] <= mae[1][k] / 10


# ---- 8-9. command line (label propagation stubbed: no GPU) -------------------------------------------------------------------------
from test_confidence import Flatten, stub_propagate  # noqa: E402  (the stub the recorded stdout was made with)

CLI_ARGS = ["--synthetic", "40", "384", "--dataset", "1", "--patch_size", "8", "8", "--overlap", "4", "0", "--seq_length", "8", "-c", "4",
            "-r", "4", "-k", "5", "--use_last", "true", "--model", "0", "--iou"]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_cli(monkeypatch, capsys, tmp_path, extra, parser=None):
    import inference as crw_inference
    cli = _load("segment_all")
    monkeypatch.setattr(crw_inference, "propagate", stub_propagate)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    out_dir, js = tmp_path / "out", tmp_path / "r.json"
    torch.manual_seed(11)
    cli.main((parser or cli.get_args_parser()).parse_args(CLI_ARGS + ["--output_folder", str(out_dir), "--report_json", str(js)] + extra))
    text = capsys.readouterr().out.replace(str(tmp_path), "TMP")
    text = re.sub(r"(Time elapsed \([a-z +]+\):) [0-9.e-]+", r"\1 *", text)
    return text, sorted(os.listdir(out_dir)), json.load(open(js))


def test_cli_with_horizons(monkeypatch, capsys, tmp_path):
    text, files, d = run_cli(monkeypatch, capsys, tmp_path, ["--horizons", "--save_horizons", "--row_spacing", "0.5", "--row_unit", "m"])
    assert files == ["horizons.pt", "predicted_map.pt"]
    h = d["horizons"]
    rows, cols = d["map_shape"]
    assert h["min_run"] == 3 and h["tol"] == 2 and h["unit"] == "m" and h["row_spacing"] == 0.5 and (h["rows"], h["cols"]) == (rows, cols)
    n = np.array(h["n_both"]) + np.array(h["n_missing"]) + np.array(h["n_spurious"])
    assert (n <= cols).all() and n.max() > 0 and h["dropped"] == d["dropped"]
    picks = torch.load(tmp_path / "out" / "horizons.pt")
    assert picks.dtype == torch.int32 and tuple(picks.shape) == (2, 3, h["K"], cols) and not picks.is_cuda
    assert [int(v) for v in ((picks[0, 2] > 0) & (picks[1, 2] > 0)).sum(1)] == h["n_both"]
    assert "Horizons (min_run 3, tol 2 rows, distances in m):" in text and "thickness" in text
    assert text.index("Horizons (") > text.index("Computing reports") and text.index("Horizons (") < text.rindex("iou")
    assert "horizons=True" in text and "min_run=3" in text
    for bad in (["--save_horizons"], ["--horizons", "--min_run", "0"], ["--horizons", "--tol", "-1"], ["--horizons", "--row_spacing", "0"]):
        cli = _load("segment_all")
        with pytest.raises(SystemExit):
            cli.check_horizon_flags(cli.get_args_parser().parse_args(CLI_ARGS + bad))


def test_cli_without_the_flag_prints_what_the_parser_without_it_prints(monkeypatch, capsys, tmp_path):
    """Without --horizons the bytes on stdout, the files and the json keys are those of a run whose parser does not know the new
    flags at all (the flags' defaults set on the namespace afterwards, so that only their parsing is bypassed)."""
    plain, files, d = run_cli(monkeypatch, capsys, tmp_path / "a", [])
    cli = _load("segment_all")

    shown = []

    class Bypassed:
        def parse_args(self, argv):
            p = cli.get_args_parser()
            new = [a for a in p._actions if a.dest in cli.HORIZON_FLAGS]
            assert len(new) == len(cli.HORIZON_FLAGS)
            old = cli.argparse.ArgumentParser(add_help=True)
            for a in p._actions:
                if a.dest not in cli.HORIZON_FLAGS and a.dest != "help":
                    old._add_action(a)
            with pytest.raises(SystemExit):
                old.parse_args(argv + ["--horizons"])  # the bypassed parser does not know the flag
            args = old.parse_args(argv)
            shown.append(str(args))
            for a in new:
                setattr(args, a.dest, a.default)
            return args

    text2, files2, d2 = run_cli(monkeypatch, capsys, tmp_path / "b", [], parser=Bypassed())
    assert len(shown) == 1 and not any(f in shown[0] for f in cli.HORIZON_FLAGS)
    assert "Horizons" not in plain and not any(f in plain for f in cli.HORIZON_FLAGS)
    assert plain == text2
    assert files == files2 == ["predicted_map.pt"] and sorted(d) == sorted(d2) and "horizons" not in d


def test_sweep_cli_flags():
    sw = _load("segment_sweep")
    p = sw.get_args_parser(horizons=True)
    a = sw.check_confidence_flags(sw.with_defaults(p.parse_args(["--model_path", "x.pt", "--horizons", "--select", "horizon_mae"])))
    assert a.horizons and a.min_run == 3 and a.tol == 2 and a.select == "horizon_mae"
    with pytest.raises(SystemExit):
        sw.check_confidence_flags(sw.with_defaults(p.parse_args(["--model_path", "x.pt", "--select", "horizon_mae"])))
    with pytest.raises(SystemExit):  # without --horizons on the command line the choice is not offered at all
        sw.get_args_parser().parse_args(["--model_path", "x.pt", "--select", "horizon_mae"])
    plain = sw.check_confidence_flags(sw.with_defaults(sw.get_args_parser().parse_args(["--model_path", "x.pt"])))
    assert (plain.horizons, plain.select) == (False, "macro_f1")
    with pytest.raises(SystemExit):
        sw.check_confidence_flags(sw.with_defaults(p.parse_args(["--model_path", "x.pt", "--horizons", "--min_run", "0"])))
    assert sw.pick_best([float("nan"), 2.0, 1.0, 1.0], lower_is_better=True) == 2


def test_inference_horizons_on_cpu_maps():
    import inference as crw_inference
    gt, pred, _, _, _ = build(("a", 37, 65, 6, 3, 0, 0))
    hz, picks = crw_inference.horizons(pred, gt, 1, nclasses=6, min_run=3, want_picks=True)
    ref = horizons_ref(gt.numpy(), pred.numpy(), 6, ignore_gt=5, ignore_pred=5, min_run=3)
    assert compare((hz.stats, np.array(hz.dropped), picks.numpy()), ref) == []
    rep = crw_inference.evaluate(pred, gt, 1, nclasses=6)
    assert hz.dropped == tuple(rep.dropped) and (hz.rows, hz.cols, hz.min_run, hz.tol) == (37, 65, 3, 2)
    three = crw_inference.horizons_sweep(torch.stack([pred, gt, pred]), gt, 1, nclasses=6, min_run=3)
    assert len(three) == 3 and np.array_equal(three[0].stats, hz.stats) and np.array_equal(three[2].stats, hz.stats)
    assert (three[1].n_missing == 0).all() and three[1].mean_mae("top") == 0.0
    bad = pred.clone()
    bad[5, 5] = 7
    with pytest.raises(crw_hip.LabelError):
        crw_inference.horizons(bad, gt, 3, nclasses=6)
    with pytest.raises(ValueError):
        crw_inference.horizons_sweep(pred, gt, 3, nclasses=6)
