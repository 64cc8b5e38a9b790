"""Aligning a memory bank to its item (tests/align_ref.py) on the CPU: the README's tables re-measured in fp64, the checkers on
planted defects, and the options switched off against `longmem_ref.labelprop_long`.  No GPU.

Wrong labels of the three `sliding_ref.DRIFT_SHAPES`, seeds 0 / 1 / 2, `longmem_ref.bank_case` as it stands.  Emerging: the target
seeded with its own frame 0, counted among the frames >= T // 3 (of 260, 648, 2 064); no seed: the whole target (of 390, 960, 3 072)."""
import numpy as np
import pytest

import align_ref as ar
import longmem_ref as lm
import sliding_ref as slr
from oracle import crw_oracle as orc

SHAPES = slr.DRIFT_SHAPES
NAMES = ["[%d, %d]" % s[:2] for s in SHAPES]
BIAS = 0.1

# memory_bias = 0.1, no centring, emerging items at start = 1.0: shape -> seeds 0 / 1 / 2 (without the bias: 143 / 0 / 0, 0 / 0 / 0,
# 893 / 898 / 898 at B = 4 and 143 / 0 / 0, 0 / 0 / 0, 843 / 898 / 898 at B = 8 -- tests/test_longmem.py).  Two seeds of [64, 48]
# are not repaired.
BIASED_START_1 = {4: ((24, 0, 0), (0, 0, 0), (1, 898, 898)), 8: ((20, 0, 0), (0, 0, 0), (0, 898, 898))}
# memory_align = 'center', no seed, [30, 13] (C = 8, M = 3): B -> seeds 0 / 1 / 2 of 390, at every start.  Without the option these
# cells are 0 / 0 / 0 to 0 / 0 / 1: the cost of centring on the smallest geometry.  The GPU test reproduces them.
CENTRED_30_13 = {4: (23, 13, 9), 8: (19, 23, 12)}


def _row(k, B, start, emerging, **kw):
    return tuple(ar.aligned_errors(SHAPES[k], s, B, start, emerging, **kw)[0] for s in range(3))


def _show(title, table):
    print(title)
    for key, row in sorted(table.items()):
        print("   ", key, " / ".join(str(x) for x in row))


@pytest.fixture(scope="module")
def centred():
    """(emerging {(shape, B, start): seeds}, no seed {(shape, B, start): seeds}) under memory_align = 'center'"""
    em = {(NAMES[k], B, st): _row(k, B, st, True, align="center") for k in range(3) for B in (1, 4, 8) for st in lm.STARTS}
    un = {(NAMES[k], B, 1.0): _row(k, B, 1.0, False, align="center") for k in (1, 2) for B in (4, 8)}
    un.update({(NAMES[0], B, st): _row(0, B, st, False, align="center") for B in (4, 8) for st in lm.STARTS})
    _show("memory_align='center', emerging items, wrong labels among the frames >= T // 3 (shape, B, start):", em)
    _show("memory_align='center', no seed, wrong labels of the target (shape, B, start):", un)
    return em, un


def test_centring_clears_the_emerging_table(centred):
    em, _ = centred
    assert len(em) == 27 and all(row == (0, 0, 0) for row in em.values()), {k: r for k, r in em.items() if any(r)}   # 81 cells


def test_centring_costs_labels_on_the_smallest_geometry_only(centred):
    _, un = centred
    for k in (1, 2):
        for B in (4, 8):
            assert un[(NAMES[k], B, 1.0)] == (0, 0, 0), (NAMES[k], B)
    worst = 0
    for B in (4, 8):
        for st in lm.STARTS:
            row = un[(NAMES[0], B, st)]
            worst = max(worst, *row)
            assert all(w <= 30 for w in row), (B, st, row)                      # of 390 per cell: the cost stays visible
            assert row == CENTRED_30_13[B], (B, st, row)                          # ... and does not depend on the start
    print("[30, 13] no seed, centred: worst cell", worst, "of 390")


@pytest.fixture(scope="module")
def biased():
    """memory_bias = 0.1, no centring: emerging rows at start 1.0 (B 4 / 8) and 0 (B 1 / 4 / 8); no seed, B >= 4, with and without"""
    em1 = {(NAMES[k], B): _row(k, B, 1.0, True, bias=BIAS) for k in range(3) for B in (4, 8)}
    em0 = {(NAMES[k], B): _row(k, B, 0.0, True, bias=BIAS) for k in range(3) for B in (1, 4, 8)}
    un = {(NAMES[k], B, st): (_row(k, B, st, False, bias=BIAS), _row(k, B, st, False)) for k in range(3) for B in (4, 8) for st in lm.STARTS}
    _show("memory_bias=0.1, emerging items at start 1.0 (shape, B):", em1)
    _show("memory_bias=0.1, emerging items at start 0 (shape, B):", em0)
    _show("memory_bias=0.1, no seed (shape, B, start): with the bias, without:", {k: (" / ".join(map(str, a)), " / ".join(map(str, b))) for k, (a, b) in un.items()})
    return em1, em0, un


def test_the_bias_repairs_part_of_the_emerging_table(biased):
    em1, em0, _ = biased
    for B, want in BIASED_START_1.items():
        assert tuple(em1[(NAMES[k], B)] for k in range(3)) == want, (B, [em1[(NAMES[k], B)] for k in range(3)])
    assert len(em0) == 9 and all(row == (0, 0, 0) for row in em0.values()), em0                                        # 27 cells stay 0


def test_the_bias_changes_no_unseeded_cell_of_four_or_more_traces(biased):
    _, _, un = biased
    assert len(un) == 18 and all(with_b == without for with_b, without in un.values()), {k: v for k, v in un.items() if v[0] != v[1]}


def test_the_shared_items_are_bank_case_as_it_stands():
    for args in ((SHAPES[0], 1, 4, 1.0, True), (SHAPES[1], 2, 8, 0.5, False), (SHAPES[0], 0, 1, 0.0, False)):
        a, b = ar.bank_case(*args), lm.bank_case(*args)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- the options switched off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,first,n_bank", [(3, 3, 3), (3, 2, 2), (5, 5, 4), (1, 1, 0)])
def test_without_the_options_the_rule_is_labelprop_long_bit_for_bit(K, first, n_bank):
    T, N, C, M, cxt, radius, temp, knn, amp = SHAPES[0]
    emb, cls = slr.drifting_item(0, T, N, C, M, amp)
    for dtype in (np.float32, np.float64):
        p1, L1, W1, I1 = lm.labelprop_long(emb, cls[:first], M, cxt, K, radius, temp, knn, first, dtype)
        p2, L2, W2, I2 = ar.labelprop_aligned(emb, cls[:first], M, cxt, K, radius, temp, knn, first, n_bank, None, 0.0, dtype)
        bits = lambda x: x.view(np.uint32 if dtype == np.float32 else np.uint64)
        assert np.array_equal(p1, p2) and np.array_equal(bits(L1), bits(L2)) and np.array_equal(bits(W1), bits(W2)) and np.array_equal(I1, I2)


# ---- the checkers ------------------------------------------------------------------------------------------------------------------
def _bank_item():
    """the virtual item of an emerging cell at start 1.0 -- bank and item a class distance apart -- and its geometry"""
    T, N, C, M, cxt, radius, temp, knn, amp = SHAPES[0]
    emb, cls, K, first, _ = lm.bank_case(SHAPES[0], 0, 4, 1.0, True)
    return emb, cls, (N, C, M, cxt, radius, temp, knn, K, first, 4)


def test_the_definitions_pass_their_own_checkers():
    emb, cls, (N, C, M, cxt, radius, temp, knn, K, first, B) = _bank_item()
    F = emb.shape[0]
    bounds = [0, B * N, F * N]
    ehat, mean = ar.center_normalize(emb.reshape(F * N, C), bounds, np.float32)
    v = ar.center_violations(emb.reshape(F * N, C), bounds, ehat, mean)
    print("centring in fp32 against fp64: worst error / bound", v["worst"])
    assert v["outside"] == 0 and v["mean"] == 0 and 0 < v["worst"] <= 1, v
    eh = ehat.reshape(F, N, C)
    W, I = ar.lists(eh, K, cxt, radius, temp, knn, first, BIAS)
    V = ar.scores(eh, K, cxt, radius, temp, knn, first, BIAS)
    res = ar.biased_lists_audit(eh, K, cxt, radius, temp, knn, first, W, I, V, BIAS)
    print("biased lists in fp32 against fp64: worst error / bound", res["worst"])
    assert not any(res["violations"].values()) and all(x <= 1 for x in res["worst"].values()), res
    assert res["eps_s"] == (C + 4) * 2.0 ** -24 / temp                              # the unbiased bound, (C + 2) u / temp, widened
    # the bias is live in these lists: without it other keys are chosen
    W0, I0 = ar.lists(eh, K, cxt, radius, temp, knn, first, 0.0)
    assert not np.array_equal(I0, I)


@pytest.mark.parametrize("defect", ar.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    emb, cls, (N, C, M, cxt, radius, temp, knn, K, first, B) = _bank_item()
    F = emb.shape[0]
    bounds = [0, B * N, F * N]
    flat = emb.reshape(F * N, C)
    if defect in ar.CENTER_DEFECTS:
        ehat, _ = ar.center_normalize(flat, bounds, np.float32, defect)
        v = ar.center_violations(flat, bounds, ehat)
        print(defect, v)
        assert v["outside"] > 0 and v["worst"] > 1, v
        return
    eh = ar.center_normalize(flat, bounds, np.float32)[0].reshape(F, N, C)
    W, I = ar.lists(eh, K, cxt, radius, temp, knn, first, BIAS, defect=defect)
    V = ar.scores(eh, K, cxt, radius, temp, knn, first, BIAS, defect=defect)
    res = ar.biased_lists_audit(eh, K, cxt, radius, temp, knn, first, W, I, V, BIAS)
    seen = {k for k, x in res["violations"].items() if x}
    print(defect, {k: res["violations"][k] for k in seen})
    assert seen, defect
    if defect == "bias_masked_keys":
        assert "disc" in seen, seen                  # a key outside the band was chosen
    else:
        assert "scores" in seen and "weights" in seen, seen


def test_a_defect_is_also_seen_in_the_labels():
    """the whole rule under each defect gives other soft labels than the definition: in fp64, far above its rounding (the labels of
    this item are nearly one-hot, so a defect of the features moves them little)"""
    emb, cls, (N, C, M, cxt, radius, temp, knn, K, first, B) = _bank_item()
    ref = ar.labelprop_aligned(emb, cls[:first], M, cxt, K, radius, temp, knn, first, B, "center", BIAS, np.float64)[1]
    for defect in ar.DEFECTS:
        L = ar.labelprop_aligned(emb, cls[:first], M, cxt, K, radius, temp, knn, first, B, "center", BIAS, np.float64, defect)[1]
        assert float(np.abs(L - ref).max()) > 1e-10, defect


# ---- the CPU route of the binding ----------------------------------------------------------------------------------------------------
def test_center_normalize_on_cpu_tensors_is_the_definition():
    import torch
    import crw_hip
    rng = np.random.default_rng(5)
    rows, C = 37, 8
    emb = (rng.standard_normal((rows, C)) + 3.0 * rng.standard_normal(C)).astype(np.float32)
    bounds = [0, 11, 12, 12, 37]                                                   # unequal, one row, empty
    ehat, mean = crw_hip.center_normalize(torch.from_numpy(emb), bounds, return_mean=True)
    want, wmean = ar.center_normalize(emb, bounds, np.float32)
    v = ar.center_violations(emb, bounds, ehat.numpy(), mean.numpy())
    assert v["outside"] == 0 and v["mean"] == 0, v
    assert np.abs(ehat.numpy() - want).max() <= 2.0 ** -22 and ehat.dtype == torch.float32 and mean.dtype == torch.float64
    assert not ehat[11].any() and not np.signbit(ehat[11].numpy()).any()         # the one-row segment: the all-zero row, +0
    assert not mean[2].any()                                                      # the empty segment's mean
    three = crw_hip.center_normalize(torch.from_numpy(emb).reshape(1, rows, C), torch.tensor(bounds, dtype=torch.int32))
    assert three.shape == (1, rows, C) and torch.equal(three[0], ehat)
    # all means zero: the plain normalisation
    x = rng.standard_normal((6, C)).astype(np.float32)
    sym = torch.from_numpy(np.concatenate([x, -x]))
    assert torch.equal(crw_hip.center_normalize(sym, [0, 12]), torch.from_numpy(orc.l2_normalize(sym.numpy(), np.float32)))
    for bad in ([0, 5], [1, 37], [0, 20, 10, 37]):
        with pytest.raises(ValueError, match="row offsets"):
            crw_hip.center_normalize(torch.from_numpy(emb), bad)
