"""Anchor marks in the lists, on the CPU: `crw_hip.mark_anchors` against the numpy marking (tests/anchor_lists_ref.py), the literal
loop over marked lists against the definition of anchored propagation (`anchored_ref.gather_anchored`), and what the change may
not move -- the header's declarations, `SIGNATURES`, the ABI number.  The device side is tests/test_anchor_lists_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import anchor_lists_ref as al
import anchored_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ar.SHAPES + al.EXTRA_SHAPES


def random_lists(shape, first_frame=1, G=None, seed=0):
    """lists of the right shapes and value ranges (weights in (0, 1], indices anywhere in the window): the marking reads neither"""
    T, N, C, M, cxt, radius, knn = shape
    rng = np.random.default_rng(seed)
    lead = (T - first_frame, knn, N) if G is None else (G, T - first_frame, knn, N)
    return rng.random(lead, np.float32) + np.float32(1e-3), rng.integers(0, (cxt + 1) * N, lead).astype(np.int32)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mark_anchors_is_the_numpy_marking_on_every_pattern(shape):
    import crw_hip
    T, N, C, M, cxt, radius, knn = shape
    for name, (anchor, ff) in al.all_patterns(T, N, M, cxt).items():
        W, I = random_lists(shape, ff)
        Wm, Im = al.mark(W, I, anchor, M, ff)
        Wt, It = torch.from_numpy(W.copy()), torch.from_numpy(I.copy())
        got = crw_hip.mark_anchors(Wt, It, torch.from_numpy(anchor), M, ff)
        assert got[0] is Wt and got[1] is It, name                                           # in place
        assert np.array_equal(bits(Wt.numpy()), bits(Wm)) and np.array_equal(It.numpy(), Im), name
        # slot 0 only; exactly the clamped nodes of frames >= first_frame carry the mark, with their class as the index
        assert np.array_equal(bits(Wm[:, 1:]), bits(W[:, 1:])) and np.array_equal(Im[:, 1:], I[:, 1:]), name
        v = ar.clamped(anchor[ff:], M)
        assert np.array_equal(al.is_mark(Wm), v) and np.array_equal(Im[:, 0][v], anchor[ff:][v]), name
        assert np.array_equal(bits(Wm[:, 0][~v]), bits(W[:, 0][~v])) and np.array_equal(Im[:, 0][~v], I[:, 0][~v]), name


def test_mark_anchors_on_the_stacked_form_and_on_a_shared_index_list():
    import crw_hip
    shape = ar.SHAPES[0]
    T, N, C, M, cxt, radius, knn = shape
    anchor, ff = ar.patterns(T, N, M, cxt)["a frame of out-of-range values"]
    W, I = random_lists(shape, ff, G=3)
    Wm, Im = al.mark(W, I, anchor, M, ff)
    for shared in (False, True):                               # I [G, F, knn, N], or one [F, knn, N] for all G
        Wt, It = torch.from_numpy(W.copy()), torch.from_numpy((I[0] if shared else I).copy())
        crw_hip.mark_anchors(Wt, It, torch.from_numpy(anchor), M, ff)
        assert np.array_equal(bits(Wt.numpy()), bits(Wm)) and np.array_equal(It.numpy(), Im[0] if shared else Im)
        for g in range(3):                                     # slice g is the single form's marking of slice g
            one = al.mark(W[g], I[g], anchor, M, ff)
            assert np.array_equal(bits(Wm[g]), bits(one[0])) and np.array_equal(Im[g], one[1])
    assert al.is_mark(Wm).sum() == 3 * ar.clamped(anchor[ff:], M).sum() > 0
    with pytest.raises(ValueError, match="anchors must be"):
        crw_hip.mark_anchors(torch.from_numpy(W), torch.from_numpy(I), torch.from_numpy(anchor[:-1]), M, ff)
    with pytest.raises(ValueError, match="same frames"):
        crw_hip.mark_anchors(torch.from_numpy(W), torch.from_numpy(I[:, 1:]), torch.from_numpy(anchor), M, ff)


def test_labelprop_gather_marks_a_copy_and_makes_one_call(monkeypatch):
    """The binding's default route without a device: the entry point is replaced by a recorder.  The caller's lists keep their bits,
    the ONE call sees marked lists in other storage; CRW_ANCHORS_SEGMENTED=1 takes `_propagate_anchored`."""
    import crw_hip
    shape = ar.SHAPES[0]
    T, N, C, M, cxt, radius, knn = shape
    anchor, ff = ar.patterns(T, N, M, cxt)["partial rows: a third of the nodes at three frames"]
    W, I = (torch.from_numpy(x) for x in random_lists(shape, ff))
    W0, I0 = W.clone(), I.clone()
    calls, seen = [], {}

    class Lib:
        def crw_labelprop_propagate_sliding(self, *a):
            calls.append(a)
            return crw_hip.CRW_OK

    def dev(t, name, dtype=torch.float32):
        seen[name] = t
        return t

    monkeypatch.setattr(crw_hip, "_sliding_lib", lambda: Lib())
    monkeypatch.setattr(crw_hip, "has_anchor_lists", lambda: True)
    monkeypatch.setattr(crw_hip, "_dev", dev)
    monkeypatch.setattr(crw_hip, "_stream", lambda: None)
    monkeypatch.delenv("CRW_ANCHORS_SEGMENTED", raising=False)
    crw_hip.labelprop_gather(torch.zeros(N), W, I, T, N, M, cxt_size=cxt, context="sliding", anchors=torch.from_numpy(anchor))
    assert len(calls) == 1 and calls[0][3:9] == (T, N, M, knn, ff, cxt)
    assert torch.equal(W.view(torch.int32), W0.view(torch.int32)) and torch.equal(I, I0)
    Wm, Im = al.mark(W0.numpy(), I0.numpy(), anchor, M, ff)
    assert seen["W"].data_ptr() != W.data_ptr() and seen["I"].data_ptr() != I.data_ptr()
    assert np.array_equal(bits(seen["W"].numpy()), bits(Wm)) and np.array_equal(seen["I"].numpy(), Im)
    routed = []
    monkeypatch.setattr(crw_hip, "_propagate_anchored", lambda *a: routed.append(a) or (None, None))
    monkeypatch.setenv("CRW_ANCHORS_SEGMENTED", "1")           # read per call
    crw_hip.labelprop_gather(torch.zeros(N), W, I, T, N, M, cxt_size=cxt, context="sliding", anchors=torch.from_numpy(anchor))
    assert len(routed) == 1 and len(calls) == 1
    monkeypatch.delenv("CRW_ANCHORS_SEGMENTED")
    monkeypatch.setattr(crw_hip, "has_anchor_lists", lambda: False)   # a library from before the marks: the segments
    crw_hip.labelprop_gather(torch.zeros(N), W, I, T, N, M, cxt_size=cxt, context="sliding", anchors=torch.from_numpy(anchor))
    assert len(routed) == 2 and len(calls) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_loop_over_marked_lists_is_the_definition(shape):
    """`anchor_lists_ref.gather_marked` on the marked lists == `anchored_ref.gather_anchored` on the same anchors, bit for bit."""
    T, N, C, M, cxt, radius, knn = shape
    rng = np.random.default_rng(sum(shape))
    emb = (rng.standard_normal((1, N, C)) + 0.5 * rng.standard_normal((T, N, C))).astype(np.float32)
    W1, I1, _ = ar.lists(emb, cxt, radius, knn)
    seen = 0
    for name, (anchor, ff) in al.all_patterns(T, N, M, cxt).items():
        W, I = W1[ff - 1:], I1[ff - 1:]
        R = al.sr.rows(I, N, cxt, ff)
        seed = (np.arange(N) * M // N).astype(np.float32) if ff == 1 else None
        Li, pi = (None, None) if ff == 1 else ar.soft_init(T, N, M, ff)
        want = ar.gather_anchored(seed, W, R, M, anchor, ff, Li, pi)
        Wm, Im = al.mark(W, I, anchor, M, ff)
        got = al.gather_marked(seed, Wm, Im, M, cxt, ff, Li, pi)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), name
        assert np.isfinite(got[0]).all(), name
        seen += int(al.is_mark(Wm).sum())
    assert seen > 0


def test_the_header_names_the_mark_and_declares_what_it_declared():
    import crw_hip
    text = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"#define\s+CRW_LABELPROP_ANCHOR_WEIGHT\b", text) and "0xFF800000" in text
    at = text.index("ANCHOR MARKS")
    assert at < text.index("int crw_labelprop_propagate_sliding(")       # in the comment of the two entry points
    assert np.array([crw_hip.ANCHOR_WEIGHT], np.float32).view(np.uint32)[0] == al.ANCHOR_BITS
    declared = set(re.findall(r"\b(crw_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(crw_hip.SIGNATURES) and not [n for n in declared if "anchor" in n]
    assert crw_hip.ABI_VERSION == 8
    assert len(crw_hip.SIGNATURES["crw_labelprop_propagate_sliding"][1]) == 12
    assert len(crw_hip.SIGNATURES["crw_labelprop_propagate_sliding_batch"][1]) == 14
    assert crw_hip.SLIDING_ENTRY_POINTS == ("crw_labelprop_propagate_sliding", "crw_labelprop_propagate_sliding_batch")


def test_the_sweep_surface_takes_anchors_and_refuses_what_segment_refuses():
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    T, N, M = 6, 4, 3
    anchors = torch.full((T, N), -1, dtype=torch.int8)
    feats, seed = torch.zeros(T, N, 8), torch.zeros(N)
    for fn in (LabelPropSweep.propagate_all, crw_utils.propagate_sweep, crw_inference.segment_sweep):
        assert inspect.signature(fn).parameters["anchors"].default is None
    ref = LabelPropSweep(3, [2], [0.1], [2])
    with pytest.raises(ValueError) as sweep_err:
        ref.propagate_all(feats, seed, M, anchors=anchors)
    with pytest.raises(ValueError) as one_err:
        LabelPropVOS_CRW(dict(CXT_SIZE=3, RADIUS=2, TEMP=0.1, KNN=2)).propagate_all(feats, seed, M, anchors=anchors)
    assert str(sweep_err.value) == str(one_err.value) and "CONTEXT 'sliding'" in str(one_err.value)
    sl = LabelPropSweep(3, [2], [0.1], [2], context="sliding")
    for bad in (anchors[:-1], anchors.to(torch.int32)):
        with pytest.raises(ValueError, match="int8"):
            sl.propagate_all(feats, seed, M, anchors=bad)
    with pytest.raises(ValueError, match="127 classes"):
        sl.propagate_all(feats, seed, 128, anchors=anchors)
    with pytest.raises(ValueError, match=rf"\[{T}, {N}\]"):
        crw_utils.propagate_sweep(torch.zeros(T, N, 4, 4), torch.zeros(8, 4), None, sl, M, False, False, anchors=anchors[1:])
    with pytest.raises(ValueError, match="correction"):
        crw_inference.segment_sweep(None, None, None, sl, M, T, (4, 4), (0, 0), correction=True, anchors=(torch.zeros(8, 24), [3]))
