"""CPU proof of the references and bars that tests/test_walk_routes_gpu.py holds the walk's dA to (tests/walk_ref.py).

Per-slice bars, as fractions of max|dA_ref[b,t]| (derivation: DESIGN.md section 3):
    fp32 chain .... 1e-3
    bf16x3 chain .. 1e-3 + 4 * E_x3[b,t]
    bf16 chain .... 1e-3 + 4 * E_bf16[b,t]
with E = slice_report(dA_rounded(A, mode), dA_fp64(A)): the error of the same formulas in float64 with the chain's bf16
images emulated -- computed from the reference and the number format, never from a kernel.  A case may be judged per slice only
if a plain fp32 evaluation of the formulas (the oracle on float32 A) stays within 1e-4 of every non-zero slice maximum: the
kernel then gets ten times what fp32 needs.  A case that misses gets another seed (walk_ref._SEED), never another bar.
"""
import numpy as np
import pytest
import torch

import walk_ref as wr
from oracle import crw_oracle as orc

_CACHE = {}


def _case(kind, B, T, N):
    """logits, the fp64 reference and the two emulated rounding errors of one table case, computed once"""
    key = (kind, B, T, N)
    if key not in _CACHE:
        A = wr.inputs(kind, B, T, N, wr.case_seed(kind, B, T, N))
        At = torch.from_numpy(A)
        big = N >= 256                                    # the torch forms (what the GPU tests use from there on)
        ref = wr.dA_fp64(At if big else A, wr.GLOSS)
        E = {mode: wr.slice_report(wr.dA_rounded(At if big else A, wr.GLOSS, mode), ref)["ratio"] for mode in ("bf16x3", "bf16")}
        _CACHE[key] = (A, ref.numpy() if big else ref, E)
    return _CACHE[key]


def bars(E):
    return {"none": 1e-3, "bf16x3": 1e-3 + 4 * E["bf16x3"], "bf16": 1e-3 + 4 * E["bf16"]}


CASES = wr.route_cases(with_chain=False)


@pytest.mark.parametrize("kind,B,T,N", [c for c in CASES if c[3] < 256])
def test_rounded_without_rounding_is_the_oracle(kind, B, T, N):
    """mode 'none' is `oracle.walk_backward` bit for bit (numpy), so the emulation adds nothing but its roundings."""
    A = _case(kind, B, T, N)[0]
    assert np.array_equal(wr.dA_rounded(A, wr.GLOSS, "none"), orc.walk_backward(A.astype(np.float64), wr.GLOSS))


@pytest.mark.parametrize("kind,B,T,N", [c for c in CASES if c[3] <= 257 and wr.per_slice(c[0])] + [("randn3", 40, 5, 5)])
def test_torch_references_agree_with_the_oracle(kind, B, T, N):
    """The autograd reference (what the GPU tests use for N >= 256 and the batch split) and the torch form of the emulation
    against `oracle.walk_backward`: 1e-12 of every slice's own maximum; At and the loss against walk_prefix_form."""
    A = wr.inputs(kind, B, T, N, wr.case_seed(kind, B, T, N))
    ref = orc.walk_backward(A.astype(np.float64), wr.GLOSS)
    loss, At, dA = wr.walk_fp64_torch(torch.from_numpy(A), wr.GLOSS)
    loss_ref, At_ref = orc.walk_prefix_form(A.astype(np.float64))
    assert abs(loss - loss_ref) <= 1e-12 * max(1.0, abs(loss_ref))
    assert np.abs(At.numpy() - At_ref).max() <= 1e-12
    for name, got in (("autograd", dA), ("emulation", wr.dA_rounded(torch.from_numpy(A), wr.GLOSS, "none"))):
        rep = wr.slice_report(got, ref)
        assert rep["ratio"].max() <= 1e-12 and not rep["zero_bad"].any(), (name, rep["ratio"].max())


@pytest.mark.parametrize("kind,B,T,N", CASES)
def test_admission_and_emulated_rounding_error(kind, B, T, N):
    """Every case of the GPU table: (a) the admission condition -- the fp32 oracle within 1e-4 of every non-zero slice
    maximum -- for every case judged per slice; (b) E_x3 <= 1e-4 per slice; (c) dA[:, -1], which never enters the loss, is an
    exactly zero reference slice, and for N = 1 every slice is."""
    A, ref, E = _case(kind, B, T, N)
    f32 = orc.walk_backward(A, np.float32(wr.GLOSS))
    assert f32.dtype == np.float32
    rep = wr.slice_report(f32, ref)
    print(f"{kind} {(B, T, N)}: fp32 oracle {rep['ratio'].max():.2e}, E_x3 {E['bf16x3'].max():.2e}, E_bf16 {E['bf16'].max():.2e}, "
          f"slice maxima {rep['scale'][:, :-1].min():.1e} .. {rep['scale'].max():.1e}")
    assert rep["zero_ref"][:, -1].all() and not rep["zero_bad"].any()
    assert rep["zero_ref"].all() == (N == 1) and (N == 1 or not rep["zero_ref"][:, :-1].any())
    if wr.per_slice(kind):
        assert rep["ratio"].max() <= 1e-4, "not admissible per slice: change the seed or the shape, never the bar"
    assert E["bf16x3"].max() <= 1e-4
    assert not wr.audit(ref, ref, 0.0)


@pytest.mark.parametrize("B,T,N", [(2, 5, 7), (1, 3, 33), (3, 4, 1), (1, 4, 130)])
@pytest.mark.parametrize("c", [3.25, -100.0, 1000.0])
def test_const_closed_form(B, T, N, c):
    """Constant logits: loss = (T-2) ln N / N, dA[:,0] = gloss / (B N^3) (1/N - I), every other slice 0 -- the oracle in
    float64 agrees to 1e-18 absolute (dA[:,0] is ~1e-3 .. 1e-7)."""
    A = wr.inputs("const", B, T, N, 0, c=c)
    loss, dA = wr.const_closed_form(B, T, N, wr.GLOSS)
    loss64, _ = orc.walk_prefix_form(A.astype(np.float64))
    assert abs(loss64 - loss) <= 1e-14 * max(1.0, loss)
    assert np.abs(wr.dA_fp64(A, wr.GLOSS) - dA).max() <= 1e-18
    assert wr.slice_report(dA, dA)["zero_ref"][:, 1:].all()


def test_slice_report_and_audit():
    """The report's own edge cases: a slice judged on its own maximum, zero reference slices apart, NaN an offence."""
    ref = np.zeros((2, 3, 4, 4))
    ref[0, 0], ref[0, 1], ref[1, 0], ref[1, 1] = 1.0, 1e-6, -2.0, 3e-9
    got = ref.copy()
    got[0, 1, 2, 3] += 2e-9            # 2e-3 of its slice, 1e-9 of the tensor
    rep = wr.slice_report(got, ref)
    assert rep["zero_ref"].tolist() == [[False, False, True], [False, False, True]] and not rep["zero_bad"].any()
    np.testing.assert_allclose(rep["ratio"], [[0, 2e-3, 0], [0, 0, 0]], rtol=1e-9)
    bad = wr.audit(got, ref, 1e-3)
    assert [(o["b"], o["t"], o["index"]) for o in bad] == [(0, 1, (2, 3))] and abs(bad[0]["ratio"] - 2e-3) < 1e-12
    assert not wr.audit(got, ref, 3e-3) and not wr.audit(got, ref, np.array([[0, 2.1e-3, 0], [0, 0, 0]]))
    assert wr.global_bar_misses(got, ref) == 0                     # the single-scale bar cannot see it
    got = ref.copy()
    got[1, 2, 0, 0] = 1e-300                                      # zero reference: nothing but zeros passes, whatever the bar
    assert wr.slice_report(got, ref)["zero_bad"].tolist() == [[False, False, False], [False, False, True]]
    assert [(o["b"], o["t"]) for o in wr.audit(got, ref, 1e3)] == [(1, 2)]
    got = ref.copy()
    got[1, 1, 3, 3] = np.nan
    assert [(o["b"], o["t"], o["index"]) for o in wr.audit(got, ref, 1e3)] == [(1, 1, (3, 3))]
    assert wr.slice_report(got, ref)["ratio"][1, 1] == np.inf
    assert wr.audit(torch.from_numpy(got), ref, 1e3)[0]["t"] == 1  # torch in, the same answer


# ------------------------------------------------------------------------------------------------ planted defects
DEFECT_CASES = [("randn3", 1, 4, 64), ("peaked", 1, 6, 130), ("randn3", 2, 7, 33), ("peaked", 2, 7, 33), ("randn3", 2, 5, 129),
                ("peaked", 2, 5, 129), ("randn3", 1, 9, 250), ("peaked", 1, 9, 250)]
LO_DEFECTS = tuple("lo_dropped:" + f for f in wr.LO_FAMILIES)
ALL_DEFECTS = LO_DEFECTS + wr.FORMULA_DEFECTS + wr.RESULT_DEFECTS

# What the bar the suite had before -- |got - ref| <= 1e-3 |ref| + 1e-4 max|ref|, one maximum for the whole tensor -- lets
# through, as run on DEFECT_CASES (asserted below, so this stays true): defect -> the cases it passes on.
OLD_BAR_LETS_THROUGH = {
    "edge_column_zeroed": [("randn3", 1, 9, 250)],
    "last_slice_nonzero": [("randn3", 2, 7, 33), ("peaked", 2, 7, 33), ("randn3", 2, 5, 129), ("randn3", 1, 9, 250)],
}


def _planted(A, ref, defect):
    if defect in LO_DEFECTS:
        return wr.dA_rounded(A, wr.GLOSS, "bf16x3", defect)        # the rest of the chain keeps both images
    if defect in wr.FORMULA_DEFECTS:
        return wr.dA_rounded(A, wr.GLOSS, "none", defect)
    return wr.plant(ref, defect)


@pytest.mark.parametrize("kind,B,T,N", DEFECT_CASES)
def test_planted_defects(kind, B, T, N):
    """Each defect, planted into the fp64 result or into the emulation, is reported by `audit` at the bar of the chain it
    imitates: a lost lo image of one operand family (F, Gt, Lt, R, dAt, dLt, dR in turn) at the bf16x3 bar, on the cases with
    T >= 5; the others at the fp32 AND the bf16x3 bar: column N-1 (the padded edge) of the last live slice zeroed, the two
    smallest adjacent slices swapped, the column-softmax dot taken over rows, dGt_0 = dLt_1 omitted, gloss ignored, dA[:, -1]
    not zero.

    Measured with this list (not asserted: the bf16 chain is the throughput mode): at the bf16 bar, 1e-3 + 4 E_bf16 with
    E_bf16 up to 1.4e-2 per slice here, every defect is still reported, except the zeroed edge column on peaked (2,7,33),
    peaked (2,5,129) and both kinds at (1,9,250) -- that column's entries are below 4 E_bf16 of the slice maximum there --
    and, on peaked (2,7,33), one of the ten slices of the row-for-column dot.

    The same list against the bar the suite had before (rtol 1e-3, atol 1e-4 of ONE maximum for the whole tensor):
    OLD_BAR_LETS_THROUGH, asserted here.  It lets dA[:, -1] != 0 (one entry at 1e-3 of the smallest slice) through on four of
    the eight cases and the zeroed edge column on randn3 (1,9,250).  It does see the swapped slices, the formula defects and
    every lost lo image on these cases: its rtol term is tight on the largest slices, which these defects reach too, and
    the smallest slice here is 7e-4 of the largest, not below the 1e-4 of its atol term."""
    A, ref, E = _case(kind, B, T, N)
    bar = bars(E)
    at_bar = {"none": "fp32", "bf16x3": "bf16x3"}
    let_through = {}
    for defect in ALL_DEFECTS:
        if defect in LO_DEFECTS and T < 5:
            continue
        got = _planted(A, ref, defect)
        modes = ("bf16x3",) if defect in LO_DEFECTS else ("none", "bf16x3")
        for mode in modes:
            found = wr.audit(got, ref, bar[mode])
            assert found, (defect, "not reported at the bar of", at_bar[mode])
        if defect == "last_slice_nonzero":
            assert {o["t"] for o in wr.audit(got, ref, bar["none"])} == {T - 2}
        if defect == "edge_column_zeroed":
            assert [(o["b"], o["t"], o["index"][1]) for o in wr.audit(got, ref, bar["none"])] == [(0, T - 3, N - 1)]
        if wr.global_bar_misses(got, ref) == 0:
            let_through[defect] = True
    want = {d for d, cases in OLD_BAR_LETS_THROUGH.items() if (kind, B, T, N) in cases}
    assert set(let_through) == want, (sorted(let_through), sorted(want))


@pytest.mark.parametrize("kind,B,T,N", [("randn3", 2, 7, 33), ("peaked", 1, 9, 250)])
def test_honest_emulations_pass_their_own_bars(kind, B, T, N):
    """The bars are not so tight that the format's own rounding trips them: each emulation passes its bar (trivially, 4 E
    against E) -- and the plain bf16 emulation does NOT pass the bf16x3 bar: E_bf16 / E_x3 >= 100 on the worst slice."""
    A, ref, E = _case(kind, B, T, N)
    bar = bars(E)
    for mode in ("bf16x3", "bf16"):
        assert not wr.audit(wr.dA_rounded(A, wr.GLOSS, mode), ref, bar[mode])
    assert wr.audit(wr.dA_rounded(A, wr.GLOSS, "bf16"), ref, bar["bf16x3"])
    assert E["bf16"].max() >= 100 * E["bf16x3"].max()
