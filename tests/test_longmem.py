"""The sliding rule with K long-term frames (tests/longmem_ref.py) on the CPU: the checker on planted defects, K = 1 against the
sliding rule, the fixtures made from the reference's own `predict`, and the bank tables of the README.  No GPU."""
import glob
import os

import numpy as np
import pytest

import longmem_ref as lm
import sliding_ref as slr
from oracle import crw_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# wrong labels of the [30, 13] item, seeds 0 / 1 / 2: (bank traces, start, emerging) -> counts.  Not emerging: the target has no
# label of its own, of 390; emerging: the target seeded with its own frame 0, among the frames >= T // 3, of 260.  The GPU test
# (tests/test_longmem_gpu.py) reproduces these through `LabelPropVOS_CRW.propagate_all(memory=)`.
TABLE_30_13 = {
    (1, 0.0, False): (39, 16, 5), (4, 0.0, False): (0, 0, 0), (8, 0.0, False): (0, 0, 0),
    (1, 0.5, False): (158, 4, 9), (4, 0.5, False): (0, 0, 0), (8, 0.5, False): (0, 0, 0),
    (1, 1.0, False): (188, 5, 210), (4, 1.0, False): (0, 0, 1), (8, 1.0, False): (0, 0, 0),
    (1, 0.0, True): (0, 0, 0), (4, 0.0, True): (0, 0, 0), (8, 0.0, True): (0, 0, 0),
    (1, 0.5, True): (2, 0, 0), (4, 0.5, True): (0, 0, 0), (8, 0.5, True): (0, 0, 0),
    (1, 1.0, True): (144, 0, 0), (4, 1.0, True): (143, 0, 0), (8, 1.0, True): (143, 0, 0),
}


def _case(K, first, shape=slr.DRIFT_SHAPES[0], seed=0):
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    emb, cls = slr.drifting_item(seed, T, N, C, M, amp)
    ehat = orc.l2_normalize(emb, np.float32).astype(np.float32)
    return emb, cls, ehat, (M, cxt, K, radius, temp, knn, first)


@pytest.mark.parametrize("K,first", [(3, 3), (3, 2), (6, 1), (2, 5)])
def test_the_rule_passes_its_own_checker_through_the_gather_and_through_the_ring(K, first):
    emb, cls, ehat, (M, cxt, K, radius, temp, knn, first) = _case(K, first)
    T, N, _ = emb.shape
    init = lm.initial_labels(cls, first, N, M, T)
    outs = []
    for ring in (False, True):
        pred, L, W, I = lm.labelprop_long(emb, cls[:first], M, cxt, K, radius, temp, knn, first, ring=ring)
        v = lm.violations(ehat, W, I, L, pred, M, cxt, K, radius, temp, knn, first, *init)
        assert not any(v.values()), (ring, v)
        outs.append((pred, L))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


@pytest.mark.parametrize("defect", lm.DEFECTS)
def test_every_planted_defect_is_reported(defect):
    K, first = (3, 2) if defect == "bank_frame_in_ring" else (3, 3)
    emb, cls, ehat, (M, cxt, K, radius, temp, knn, first) = _case(K, first)
    T, N, _ = emb.shape
    pred, L, W, I = lm.labelprop_long(emb, cls[:first], M, cxt, K, radius, temp, knn, first, defect=defect)
    v = lm.violations(ehat, W, I, L, pred, M, cxt, K, radius, temp, knn, first, *lm.initial_labels(cls, first, N, M, T))
    print(defect, {k: x for k, x in v.items() if x})
    assert any(v.values()), defect
    in_lists = defect in ("window_overlaps_bank", "limit_cxt_plus_1")
    assert bool(v["lists_W"] or v["lists_I"]) == in_lists and bool(v["bits_L"]) != in_lists, v   # each is seen where it was planted


def test_the_checker_sees_a_touched_front_frame():
    emb, cls, ehat, (M, cxt, K, radius, temp, knn, first) = _case(3, 3)
    T, N, _ = emb.shape
    pred, L, W, I = lm.labelprop_long(emb, cls[:first], M, cxt, K, radius, temp, knn, first)
    L[N + 1, 0] += 0.5
    v = lm.violations(ehat, W, I, L, pred, M, cxt, K, radius, temp, knn, first, *lm.initial_labels(cls, first, N, M, T))
    assert v["front_L"] == 1


@pytest.mark.parametrize("shape", slr.DRIFT_SHAPES, ids=lambda s: f"T{s[0]}N{s[1]}")
def test_one_long_term_frame_is_the_sliding_rule(shape):
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    emb, cls = slr.drifting_item(0, T, N, C, M, amp)
    for dtype in (np.float32, np.float64):
        p1, L1, W1, I1 = slr.labelprop_sliding(emb, cls[0].astype(np.float32), M, cxt, radius, temp, knn, dtype)
        for ring in (False, True):
            p2, L2, W2, I2 = lm.labelprop_long(emb, cls[:1], M, cxt, 1, radius, temp, knn, 1, dtype, ring=ring)
            assert np.array_equal(p1, p2) and np.array_equal(L1, L2) and np.array_equal(W1, W2)
            assert np.array_equal(np.where(W1 > 0, I1, 0), np.where(W2 > 0, I2, 0))       # (an empty slot: the reference goes on into masked keys)
            assert np.array_equal(slr.rows(I1, N, cxt)[W1 > 0], lm.rows(I2, N, cxt, 1)[W2 > 0])


FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "longmem_*.npz")))


def test_the_fixtures_are_there():
    names = {os.path.basename(p)[len("longmem_"):-len(".npz")] for p in FIXTURES}
    assert names == {"T14N10K2", "T30N13K3", "T20N24K4", "T12N10K5", "T14N10K3F2"}, names


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_fixtures_from_the_reference(path):
    """The reference's own `predict` on the lists feats[:K] + feats[max(K, n - cxt):n] (tests/golden/make_golden_longmem.py) against
    the plain-loop rule: labels exact in fp32 and fp64, L within the recorded deviation (fp64) plus the project's bound (fp32)."""
    g = np.load(path)
    emb, M, cxt, K, radius, temp, knn, first = g["emb"], int(g["M"]), int(g["cxt"]), int(g["K"]), int(g["radius"]), float(g["temp"]), \
        int(g["knn"]), int(g["first_frame"])
    F, N, _ = emb.shape
    assert first in (K, K - 1) and g["cls_front"].shape == (first, N)
    for dtype, tol in ((np.float64, float(g["deviation"])), (np.float32, float(g["deviation"]) + orc.gather_bound(knn))):
        for ring in (False, True):
            pred, L, _, _ = lm.labelprop_long(emb, g["cls_front"], M, cxt, K, radius, temp, knn, first, dtype, ring=ring)
            err = float(np.abs(L - g["L"]).max())
            print(f"{os.path.basename(path)} {np.dtype(dtype).name} ring={ring}: max |L - reference| = {err:.3g} (tolerance {tol:.3g})")
            assert np.array_equal(pred, g["pred"]) and err <= tol * (1 + 1e-6)


@pytest.fixture(scope="module")
def tables():
    """every cell of the README's tables, fp64, once: {(shape index, B, start, emerging): [(wrong, of)] per seed} and the own-seed row"""
    out = {(k, B, start, e): [lm.bank_errors(shape, s, B, start, e) for s in range(3)]
           for k, shape in enumerate(slr.DRIFT_SHAPES) for B in (1, 4, 8) for start in lm.STARTS for e in (False, True)}
    own = {(k, start): [lm.own_seed_errors(shape, s, start) for s in range(3)] for k, shape in enumerate(slr.DRIFT_SHAPES) for start in lm.STARTS}
    return out, own


def test_a_bank_of_four_traces_labels_an_item_that_has_none_and_finds_the_emerging_layer(tables):
    cells, own = tables
    for (k, B, start, e), res in sorted(cells.items()):
        T, N = slr.DRIFT_SHAPES[k][:2]
        print(f"[{T}, {N}] B = {B} start = {start} {'emerging, frames >= f0' if e else 'no seed'}: "
              + " / ".join(str(w) for w, _ in res) + f" of {res[0][1]}")
    for (k, start), res in sorted(own.items()):
        T, N = slr.DRIFT_SHAPES[k][:2]
        print(f"[{T}, {N}] start = {start} own seed alone, frames >= f0: " + " / ".join(str(w) for w, _ in res) + f" of {res[0][1]}")
    for k in range(len(slr.DRIFT_SHAPES)):
        for start in (0.0, 0.5):
            for e in (False, True):
                for w, n in cells[(k, 4, start, e)]:
                    assert w <= 0.01 * n, (k, start, e, w, n)                        # at most 1 % wrong with four bank traces
            for w, n in own[(k, start)]:
                assert w >= 0.40 * n, (k, start, w, n)                               # the own seed alone: at least 40 % wrong
    for key, want in TABLE_30_13.items():
        assert tuple(w for w, _ in cells[(0,) + key]) == want, key


def test_propagate_all_refuses_what_a_bank_cannot_do():
    """the host checks of `LabelPropVOS_CRW.propagate_all(memory=)`, CPU tensors: each raises before anything touches the library"""
    import torch
    from imported.labelprop import LabelPropVOS_CRW
    T, N, C, M, B = 6, 5, 4, 3, 2
    feats, seed = torch.zeros(T, N, C), torch.zeros(N)
    mem = (torch.zeros(B, N, C), torch.zeros(B, N, dtype=torch.int8))
    cfg = dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2)
    sliding = LabelPropVOS_CRW(dict(cfg, CONTEXT="sliding"))
    with pytest.raises(ValueError, match="memory needs CONTEXT 'sliding'.*consistently"):
        LabelPropVOS_CRW(cfg).propagate_all(feats, seed, M, memory=mem)
    with pytest.raises(ValueError, match="restart"):
        sliding.propagate_all(feats, seed, M, memory=mem, anchors=torch.zeros(T, N, dtype=torch.int8), anchor_context="restart")
    with pytest.raises(ValueError, match="nodes"):
        sliding.propagate_all(feats, seed, M, memory=(torch.zeros(B, N + 1, C), torch.zeros(B, N + 1, dtype=torch.int8)))
    with pytest.raises(ValueError, match="fully labelled"):
        sliding.propagate_all(feats, seed, M, memory=(mem[0], torch.full((B, N), -1, dtype=torch.int8)))
    with pytest.raises(ValueError, match="seed=None needs memory"):
        sliding.propagate_all(feats, None, M)
    with pytest.raises(ValueError, match="N x 1"):
        sliding.propagate_all(feats, seed, M, grid_w=5, memory=mem)
