"""Context novelty and anchor picks on the CPU (no library needed): the definition of tests/novelty_ref.py on the items in which a
layer enters after the seed trace, `crw_hip.suggest_frames` against it, the planted defects, the column round trip of
`inference.segment`'s picks, and the option checks.  Defaults everywhere: top = N // 4, min_gap = 2."""
import os
import sys

import numpy as np
import pytest
import torch

import anchored_ref as ar
import novelty_ref as nr
import restart_ref as rr
import sliding_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(shape, s) for shape in sr.DRIFT_SHAPES for s in sr.DRIFT_SEEDS]
ids = lambda v: f"{v[0][0]}x{v[0][1]}-seed{v[1]}"


def anchored_at(cls, frames):
    a = np.full(cls.shape, ar.FREE, np.int8)
    for f in frames:
        a[f] = cls[f]
    return a


def wrong(emb, cls, M, cxt, radius, knn, temp, anchor, lo, restart=True):
    """(wrong, labels) among the un-annotated frames >= lo, under restart or under clamp"""
    seed = cls[0].astype(np.float32)
    if restart:
        pred = rr.propagate(emb, seed, M, cxt, radius, knn, temp, anchor)[1]
    else:
        W, _, R = ar.lists(emb, cxt, radius, knn, temp)
        pred = ar.gather_anchored(seed, W, R, M, anchor)[1]
    return ar.emergence_errors(pred, cls, lo, anchor)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_first_pick_is_the_onset_and_a_trace_there_repairs_everything(case):
    (T, N, C, M, cxt, radius, temp, knn, amp), s = case
    emb, cls, f0 = ar.emerging_item(s, T, N, C, M, amp)
    got = nr.suggest(emb, cxt, radius, 2)
    print(f"[{T}, {N}] seed {s}: onset {f0}, picks {[(f, round(z, 3)) for f, z, _ in got]}")
    assert got[0][0] == f0, (got, f0)
    anchor = anchored_at(cls, [got[0][0]])
    for restart in (False, True):
        e = wrong(emb, cls, M, cxt, radius, knn, temp, anchor, f0, restart)
        assert e[0] == 0 and e[1] == (T - f0 - 1) * N, (restart, e)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_both_onsets_are_among_the_first_three_picks(case):
    (T, N, C, M, cxt, radius, temp, knn, amp), s = case
    emb, cls, (fa, fb) = nr.two_onsets_item(s, T, N, C, M + 1, amp)
    assert (fa, fb) == (T // 4, (5 * T) // 8) and cls[:fa].max() == M - 2 and cls[fa:fb].max() == M - 1 and cls[fb:].max() == M
    frames = [f for f, _, _ in nr.suggest(emb, cxt, radius, 3)]
    assert {fa, fb} <= set(frames), (frames, fa, fb)
    # printed, not asserted
    none = wrong(emb, cls, M + 1, cxt, radius, knn, temp, anchored_at(cls, []), 1, restart=False)
    two = wrong(emb, cls, M + 1, cxt, radius, knn, temp, anchored_at(cls, frames[:2]), 1)
    print(f"[{T}, {N}] seed {s}: onsets {(fa, fb)}, picks {frames}, first two are the onsets: {set(frames[:2]) == {fa, fb}}; wrong labels "
          f"in the un-annotated frames >= 1: {none[0]} of {none[1]} without anchors, {two[0]} of {two[1]} with the first two picks anchored (restart)")


def test_print_change_point_and_the_drifting_items():
    """Printed, not asserted: what the xent metric with PELT (`utils.change_point`'s arithmetic, pelt.py) finds on the emerging
    items, and the largest z of the items in which nothing emerges -- it overlaps the weakest true onset, so no threshold."""
    sys.path.insert(0, os.path.join(ROOT, "radar-sounder-crw_amd"))
    import pelt
    for (T, N, C, M, cxt, radius, temp, knn, amp), s in CASES:
        emb, _, f0 = ar.emerging_item(s, T, N, C, M, amp)
        x = rr.oracle.xent_metric(emb)
        try:
            bk = pelt.pelt_rbf(np.abs(x[:, :-1] - x[:, 1:]).sum(0), pen=5)[:-1]
        except Exception as e:
            bk = repr(e)
        onset = nr.suggest(emb, cxt, radius, 1)[0]
        drift = nr.suggest(sr.drifting_item(s, T, N, C, M, amp)[0], cxt, radius, 1)[0]
        print(f"[{T}, {N}] seed {s}: onset {f0}; PELT interior breakpoints {list(bk) if not isinstance(bk, str) else bk}; first pick "
              f"{onset[0]} z {onset[1]:.3f}; drifting item: largest z {drift[1]:.3f} at frame {drift[0]}")


# ------------------------------------------------------------------------------------------------ suggest_frames
def test_suggest_frames_is_the_definition_and_its_unit_cases():
    import crw_hip
    sf = crw_hip.suggest_frames
    rng = np.random.default_rng(5)
    for F, cxt, gap, first, anchored in ((29, 4, 2, 1, ()), (39, 6, 2, 1, (13, 14)), (10, 80, 0, 3, (3,)), (1, 4, 2, 1, ()), (7, 1, 3, 1, (4,))):
        s = rng.random(F).astype(np.float32)
        want = nr.picks(s, cxt, F, gap, first, anchored)
        for arg in (s, torch.from_numpy(s), s.tolist()):
            assert sf(arg, cxt, F, gap, first, anchored) == want, (F, cxt, gap, first)
        assert sf(s, cxt, 2, gap, first, anchored) == want[:2]
    # ties go to the lowest frame; the neighbours within min_gap leave with a pick
    s = [0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert [f for f, _, _ in sf(s, 3, 2, 2)] == [2, 6]
    assert sf(s, 3, 1, 2)[0] == (2, 1.0, 1.0)
    got = [f for f, _, _ in sf([0.0, 5.0, 4.0, 3.0, 0.5, 0.0, 0.0, 2.0], 9, 9, 2)]
    assert got[0] == 2 and all(abs(a - b) > 2 for i, a in enumerate(got) for b in got[:i]), got
    assert got == [f for f, _, _ in nr.picks([0.0, 5.0, 4.0, 3.0, 0.5, 0.0, 0.0, 2.0], 9, 9, 2)]
    # fully anchored frames are not proposed again, nor their neighbours
    assert sf(s, 3, 1, 2, anchored=[2])[0][0] == 6
    assert all(f not in (1, 2, 3, 4) for f, _, _ in sf(s, 3, 9, 2, anchored=[2]))
    # budget larger than the frames left: what there is
    assert len(sf(s, 3, 50, 2)) == len(nr.picks(s, 3, 50, 2)) < 9 and sf(s, 3, 0, 2) == []
    assert sf(s, 3, 50, 0, anchored=range(1, 10)) == []
    # T = 2: one scored frame, no neighbour, z = s
    assert sf([0.25], 4, 3) == [(1, 0.25, 0.25)] and sf(torch.tensor([0.25]), 4, 3, first_frame=1, anchored=[1]) == []
    # the excess is over the median of the neighbours inside the window, in float64
    z = nr.excess([1.0, 2.0, 4.0, 8.0, 16.0], 2)
    assert z.tolist() == [1 - 3.0, 2 - 4.0, 4 - 5.0, 8 - 4.0, 16 - 6.0]
    with pytest.raises(ValueError):
        sf(s, 0, 1)


# ------------------------------------------------------------------------------------------------ planted defects
def test_planted_defects_change_a_pick_or_a_value():
    T, N, C, M, cxt, radius, temp, knn, amp = sr.DRIFT_SHAPES[0]
    emb, cls, f0 = ar.emerging_item(0, T, N, C, M, amp)
    ehat = nr.normalized(emb)
    good = nr.novelty(ehat, cxt, radius)
    assert np.abs(good - nr.novelty_fast(ehat, cxt, radius)).max() < 1e-12                # the loops and the matrix form agree
    f32 = nr.novelty(ehat, cxt, radius, dtype=np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - good).max() <= nr.nov_bound(C)
    v = nr.violations(ehat, cxt, radius, None, None, 1, f32, nr.frame_scores(f32, None, np.float32))
    assert not any(v.values()), v
    # the window reaching before the origin: a restart two frames after the onset (the README's "two frames late") -- the frames
    # behind it find the pre-restart frames among their keys
    origin = rr.origins(anchored_at(cls, [f0 + 2]), M)
    assert origin[f0 + 3] == f0 + 2 and origin[f0 + 2] == 0
    right, bad = nr.novelty(ehat, cxt, radius, origin), nr.novelty(ehat, cxt, radius, origin, defect="window_before_origin")
    assert np.array_equal(right[:f0 + 2], bad[:f0 + 2]) and (bad[f0 + 3:f0 + 2 + cxt] < right[f0 + 3:f0 + 2 + cxt]).any()
    assert (bad <= right).all()
    v = nr.violations(ehat, cxt, radius, None, origin, 1, bad.astype(np.float32), nr.frame_scores(bad, None, np.float32))
    assert v["nov"] > 0 and v["score"] > 0, v
    # the band <= radius: one more node on each side, so a maximum can only grow
    wide = nr.novelty(ehat, cxt, radius, defect="band_le")
    assert (wide <= good).all() and (wide < good).any()
    assert np.array_equal(wide, nr.novelty(ehat, cxt, radius + 1))
    assert nr.violations(ehat, cxt, radius, None, None, 1, wide.astype(np.float32), nr.frame_scores(wide, None, np.float32))["nov"] > 0
    # the mean in place of the median: the onset's own peak and the young context after frame 0 enter their neighbours' baseline
    s = nr.frame_scores(good)
    z, zm = nr.excess(s, cxt), nr.excess(s, cxt, defect="mean")
    assert not np.allclose(z, zm)
    emb2, _, _ = ar.emerging_item(2, T, N, C, M, amp)                                     # the weakest onset: 0.145 against 0.086
    a, b = nr.suggest(emb2, cxt, radius, 3), nr.suggest(emb2, cxt, radius, 3, defect="mean")
    print("median:", a, "mean:", b)
    assert a != b and a[0][0] == f0
    # top smallest instead of largest: the new layer's nodes -- the deepest few -- no longer carry the frame
    a, b = nr.suggest(emb, cxt, radius, 1), nr.suggest(emb, cxt, radius, 1, defect="top_smallest")
    print("largest:", a, "smallest:", b)
    assert a[0][0] == f0 and (b[0][0] != f0 or b[0][1] < 0.5 * a[0][1])
    assert nr.violations(ehat, cxt, radius, None, None, 1, good.astype(np.float32), nr.frame_scores(good, None, np.float32, "top_smallest"))["score"] > 0


# ------------------------------------------------------------------------------------------------ segment's picks, options
def test_the_column_of_a_pick_maps_back_to_its_frame():
    import inference
    import utils
    T, N, (H, W), (oh, ow), K = 10, 6, (16, 32), (0, 4), 3
    step, rg_len, rg_h = W - ow, T * (W - ow) + ow, N * (H - oh) + oh
    rng = np.random.default_rng(3)
    novs = [(torch.zeros(N, T), torch.cat([torch.zeros(1), torch.from_numpy(rng.random(T - 1)).float()])) for _ in range(2)]
    novs[1][1][T - 1] = 5.0                                                # the last frame: its columns run to the radargram's end
    out = inference._suggested(novs, 4, 3, 2, N, K, T, (H, W), (oh, ow), None)
    assert tuple(out["novelty"].shape) == (2, T) and out["novelty"].device.type == "cpu" and len(out["suggested"]) == 2
    assert out["suggested"][1][0]["frame"] == T - 1
    annot = torch.zeros(rg_h, 2 * rg_len, dtype=torch.int64)
    for t, picks in enumerate(out["suggested"]):
        assert [(p["frame"], p["z"], p["score"]) for p in picks] == nr.picks(novs[t][1][1:].numpy(), 4, 3, 2)
        for p in picks:
            assert set(p) == {"radargram", "item", "frame", "column", "columns", "z", "score"}
            assert p["radargram"] == t and p["item"] == t * T and p["columns"][0] == p["column"] < p["columns"][1] <= (t + 1) * rg_len
            for col in (p["column"], p["columns"][1] - 1):
                nodes = utils.anchor_nodes(annot, [col], rg_len, T, N, rg_h, step)
                hit = [(r, f) for r in range(2) for f in range(T) if (nodes[r][f] >= 0).any()]
                assert hit == [(t, p["frame"])], (p, col, hit)
    # the loop: a suggested trace, labelled and passed as an anchor, is not suggested again -- nor are its neighbours
    first = out["suggested"][0][0]
    again = inference._suggested(novs, 4, 3, 2, N, K, T, (H, W), (oh, ow), (annot, [first["column"]]))
    assert all(abs(p["frame"] - first["frame"]) > 2 for p in again["suggested"][0])
    assert again["suggested"][1] == out["suggested"][1]
    part = annot.clone()
    part[: rg_h // 2] = -1                                                 # a partially labelled trace excludes nothing
    assert inference._suggested(novs, 4, 3, 2, N, K, T, (H, W), (oh, ow), (part, [first["column"]]))["suggested"] == out["suggested"]


def test_option_checks():
    import crw_hip
    import inference
    import utils
    from imported.labelprop import LabelPropVOS_CRW
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding"))
    seq = torch.zeros(6, 4, 16, 16)
    with pytest.raises(ValueError, match="novelty needs a label propagation"):
        utils.propagate(seq, None, None, object(), 2, False, False, novelty=True)
    for top in (0, 5):
        with pytest.raises(ValueError, match="top must lie in 1 .. N = 4"):
            utils.propagate(seq, None, None, lp, 2, False, False, novelty=True, novelty_top=top)
    assert crw_hip.novelty_top(13) == 3 and crw_hip.novelty_top(3) == 1 and crw_hip.novelty_top(48, 48) == 48
    with pytest.raises(ValueError, match="suggest and suggest_gap must be >= 0"):
        inference.segment(None, None, None, lp, 2, 6, (16, 16), (0, 0), suggest=-1)
    with pytest.raises(ValueError, match="suggest and suggest_gap must be >= 0"):
        inference.segment(None, None, None, lp, 2, 6, (16, 16), (0, 0), suggest=1, suggest_gap=-1)
    with pytest.raises(ValueError, match="suggest needs a label propagation with `novelty`"):
        inference.segment(None, None, None, object(), 2, 6, (16, 16), (0, 0), suggest=1)
    feats = torch.zeros(6, 4, 8)
    with pytest.raises(ValueError, match="route must be one of"):
        crw_hip.labelprop_novelty(feats, 2, 2, route="mfma")
    with pytest.raises(ValueError, match="breaks the chain rule"):
        crw_hip.labelprop_novelty(feats, 2, 2, origin=torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="anchor_context='restart' needs anchors"):
        lp.novelty(feats, anchor_context="restart")
    assert set(crw_hip.NOVELTY_ROUTES) == {"auto", "vector", "matrix"}


def test_script_flags():
    sys.path.insert(0, os.path.join(ROOT, "radar-sounder-crw_amd", "scripts"))
    import segment_all
    parse = segment_all.get_args_parser().parse_args
    a = parse(["--synthetic", "40", "128"])
    assert a.suggest_anchors is None and segment_all.check_suggest_flags(a) is a and a.suggest_gap is None
    a = segment_all.check_suggest_flags(parse(["--synthetic", "40", "128", "--suggest_anchors", "3"]))
    assert (a.suggest_anchors, a.suggest_gap, a.suggest_top) == (3, 2, None)
    for bad, msg in ((["--suggest_gap", "1"], "need --suggest_anchors"), (["--suggest_top", "2"], "need --suggest_anchors"),
                     (["--suggest_anchors", "0"], "at least 1"), (["--suggest_anchors", "2", "--single"], "not available with --single"),
                     (["--suggest_anchors", "2", "--suggest_gap", "-1"], "at least 0")):
        with pytest.raises(SystemExit, match=msg):
            segment_all.check_suggest_flags(parse(["--synthetic", "40", "128"] + bad))
    table = segment_all.suggested_table([[dict(radargram=0, item=0, frame=3, column=84, columns=(84, 112), z=0.5, score=0.75)], []])
    lines = table.split("\n")
    assert len(lines) == 3 and len(lines[1]) == len(lines[2]) and lines[2].split() == ["0", "3", "84-111", "0.5000", "0.7500"]
