"""anchor_context='restart' on the CPU: the definition of tests/restart_ref.py against the construction by cutting the item, against
clamp mode where nothing restarts, the checker against planted defects, the option checks of the binding, and the README's table --
wrong labels behind a fully labelled trace that comes after a layer's onset, clamp mode against restart."""
import numpy as np
import pytest
import torch

import anchored_ref as ar
import restart_ref as rr
import sliding_ref as sr


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def case(shape, name, anchor, ff):
    T, N, C, M, cxt, radius, knn = shape
    emb = rr.item(shape)
    if ff == 1:
        return emb, (np.arange(N) * M // N).astype(np.float32), None, None
    return (emb, None) + ar.soft_init(T, N, M, ff)


@pytest.mark.parametrize("shape", ar.SHAPES, ids=str)
def test_the_definition_is_the_item_cut_at_every_origin(shape):
    T, N, C, M, cxt, radius, knn = shape
    for name, (anchor, ff) in rr.patterns(T, N, M, cxt).items():
        emb, seed, Li, pi = case(shape, name, anchor, ff)
        L, pred, W, R, origin = rr.propagate(emb, seed, M, cxt, radius, knn, ar.TEMP, anchor, ff, Li, pi)
        assert rr.chain_rule_ok(origin), name
        ref = rr.cut(emb, seed, M, cxt, radius, knn, ar.TEMP, anchor, ff, Li, pi)
        v = rr.violations(seed, W, R, M, anchor, ff, L, pred, Li, pi, ref=ref)
        assert not any(v.values()), (name, v)
        # the lists: frame n scores against key_frames(n, a, cxt) and nothing else -- the explicit-key construction, bit for bit
        ehat = rr.oracle.l2_normalize(emb, np.float32).astype(np.float32)
        for n in (ff, min(ff + cxt + 2, T - 1), T - 1):
            keys = rr.key_frames(n, int(origin[n]), cxt)
            We, Ie, _ = rr._frame_lists(ehat, n, keys, radius, ar.TEMP, knn)
            assert np.array_equal(bits(We), bits(W[n - ff])), (name, n)
            live = We > 0
            assert np.array_equal((np.asarray(keys)[Ie // N] * N + Ie % N)[live], R[n - ff][live]), (name, n)
        if not origin.any():                                   # nothing restarts: clamp mode on the sliding lists, bit for bit
            Wc, Ic, Rc = ar.lists(emb, cxt, radius, knn, ar.TEMP, ff)
            Lc, pc = ar.gather_anchored(seed, Wc, Rc, M, anchor, ff, Li, pi)
            assert np.array_equal(bits(W), bits(Wc)) and np.array_equal(R, Rc), name
            assert np.array_equal(bits(L), bits(Lc)) and np.array_equal(pred, pc), name
    names = list(rr.patterns(T, N, M, cxt))
    assert {"none", "partial rows only", "every frame full"} <= set(names)
    for name in ("none", "partial rows only"):
        assert not rr.origins(rr.patterns(T, N, M, cxt)[name][0], M).any(), name


def test_origins_and_stretches():
    M, T, N = 3, 9, 4
    a = np.full((T, N), -1, np.int8)
    a[2], a[3, :2], a[5], a[6] = 1, 0, 2, [0, 1, 2, M]         # 2 and 5 full, 3 partial, 6 holds an out-of-range value
    assert rr.origins(a, M).tolist() == [0, 0, 0, 2, 2, 2, 5, 5, 5]
    assert rr.origins(a, M, first_frame=3).tolist() == [0, 0, 0, 0, 0, 0, 5, 5, 5]      # frame 2 is the caller's: never clamped
    assert rr.origins(a, M, partial=True).tolist() == [0, 0, 0, 2, 3, 3, 5, 6, 6]
    assert rr.stretches(rr.origins(a, M)) == [(0, 2), (2, 5), (5, 8)]
    assert rr.stretches(rr.origins(a, M), first_frame=4) == [(2, 5), (5, 8)]
    assert rr.key_frames(8, 5, 2) == [5, 6, 7] and rr.key_frames(8, 2, 3) == [2, 5, 6, 7] and rr.key_frames(3, 2, 3) == [2]
    import crw_hip
    o = crw_hip.anchor_origins(torch.from_numpy(a), M, T)
    assert o.dtype == torch.int32 and o.tolist() == rr.origins(a, M).tolist()
    assert crw_hip.anchor_origins(torch.from_numpy(a), M, T, first_frame=3).tolist() == rr.origins(a, M, 3).tolist()
    assert crw_hip.origin_stretches(o.tolist(), T) == rr.stretches(rr.origins(a, M))
    # n = 8, a = 5, cxt = 1: n' = 3 > cxt + 1, the keys are frames [5, 7] -- list frame 1 is frame 7; at cxt = 2 it is frame 6
    I = np.array([1, N + 1]).reshape(1, 2, 1)
    assert rr.rows_of(I, rr.origins(a, M), N, 1, first_frame=8).ravel().tolist() == [5 * N + 1, 7 * N + 1]
    assert rr.rows_of(I, rr.origins(a, M), N, 2, first_frame=8).ravel().tolist() == [5 * N + 1, 6 * N + 1]


@pytest.mark.parametrize("defect", rr.DEFECTS)
def test_the_checker_reports_each_planted_defect(defect):
    shape = ar.SHAPES[0]                                       # (14, 10, 8, 3, cxt 4, 3, 4)
    T, N, C, M, cxt, radius, knn = shape
    pats = rr.patterns(T, N, M, cxt)
    name = {"partial_restarts": "partial rows only", "late": "two consecutive full frames"}.get(
        defect, "a restart at 2, after which the window slides again")
    anchor, ff = pats[name]
    emb, seed, Li, pi = case(shape, name, anchor, ff)
    L, pred, W, R, _ = rr.propagate(emb, seed, M, cxt, radius, knn, ar.TEMP, anchor, ff, Li, pi)
    ref = rr.cut(emb, seed, M, cxt, radius, knn, ar.TEMP, anchor, ff, Li, pi)
    assert not any(rr.violations(seed, W, R, M, anchor, ff, L, pred, ref=ref).values())
    Ld, pd, *_ = rr.propagate(emb, seed, M, cxt, radius, knn, ar.TEMP, anchor, ff, Li, pi, defect=defect)
    v = rr.violations(seed, W, R, M, anchor, ff, Ld, pd, ref=ref)
    assert v["bits_L"] and v["soft"], (defect, v)              # ... against the cut construction AND against the fp64 sums
    assert not (v["onehot"] or v["frame0"]), (defect, v)


def test_option_checks_and_their_messages():
    import crw_hip
    assert crw_hip.ANCHOR_CONTEXTS == ("clamp", "restart") and crw_hip.check_anchor_context("restart") == "restart"
    with pytest.raises(ValueError, match=r"anchor_context must be one of \('clamp', 'restart'\) \(got 'cut'\)"):
        crw_hip.check_anchor_context("cut")
    T = 6
    ok = torch.tensor([0, 0, 0, 2, 2, 4], dtype=torch.int32)
    assert crw_hip.check_origin(ok, T) == ok.tolist()
    for bad in ([0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 4, 4], [0, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 5], [0, -1, 0, 0, 0, 0]):
        with pytest.raises(ValueError, match="breaks the chain rule"):
            crw_hip.check_origin(torch.tensor(bad, dtype=torch.int32), T)
    with pytest.raises(ValueError, match=r"origin must be \[6\] int32"):
        crw_hip.check_origin(ok[:5], T)
    with pytest.raises(ValueError, match=r"origin must be \[6\] int32"):
        crw_hip.check_origin(ok.float(), T)
    W, I = torch.zeros(T - 1, 2, 3), torch.zeros(T - 1, 2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="origin needs context='sliding'"):
        crw_hip.labelprop_gather(None, W, I, T, 3, 2, cxt_size=2, origin=ok)
    with pytest.raises(ValueError, match="origin needs context='sliding'"):
        crw_hip.labelprop_propagate_batch(None, W[None], I, T, 3, 2, cxt_size=2, origin=ok)
    with pytest.raises(ValueError, match="breaks the chain rule"):
        crw_hip.labelprop_gather(None, W, I, T, 3, 2, cxt_size=2, context="sliding", origin=torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32))
    from imported.labelprop import LabelPropVOS_CRW
    feats, seed = torch.zeros(T, 3, 4), torch.zeros(3)
    anchors = torch.full((T, 3), -1, dtype=torch.int8)
    with pytest.raises(ValueError, match="anchor_context must be one of"):
        LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding")).propagate_all(feats, seed, 2, anchors=anchors,
                                                                                                      anchor_context="cut")
    with pytest.raises(ValueError, match="anchor_context='restart' needs anchors"):
        LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2, CONTEXT="sliding")).propagate_all(feats, seed, 2, anchor_context="restart")
    with pytest.raises(ValueError, match="anchors need CONTEXT 'sliding'"):
        LabelPropVOS_CRW(dict(CXT_SIZE=2, RADIUS=2, TEMP=0.1, KNN=2)).propagate_all(feats, seed, 2, anchors=anchors, anchor_context="restart")
    from imported.labelprop import LabelPropSweep
    with pytest.raises(ValueError, match="anchor_context='restart' needs anchors"):
        LabelPropSweep(2, [2], [0.1], [2], context="sliding").propagate_all(feats, seed, 2, anchor_context="restart")
    with pytest.raises(ValueError, match="anchors need CONTEXT 'sliding'"):
        LabelPropSweep(2, [2], [0.1], [2]).propagate_all(feats, seed, 2, anchors=anchors, anchor_context="restart")
    import inference
    import utils
    seq = torch.zeros(T, 3, 16, 16)
    for fn in (utils.propagate, utils.propagate_sweep):
        with pytest.raises(ValueError, match="anchor_context='restart' needs anchors"):
            fn(seq, None, None, None, 2, False, False, anchor_context="restart")
        with pytest.raises(ValueError, match="anchor_context must be one of"):
            fn(seq, None, None, None, 2, False, False, anchors=anchors, anchor_context="origin")
    for fn in (inference.segment, inference.segment_sweep):
        with pytest.raises(ValueError, match="anchor_context='restart' needs anchors"):
            fn(None, None, None, None, 2, T, (16, 16), (0, 0), anchor_context="restart")
        with pytest.raises(ValueError, match="anchors and correction=True do not combine"):
            fn(None, None, None, None, 2, T, (16, 16), (0, 0), correction=True, anchors=(None, [1]), anchor_context="restart")


def test_script_flag():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radar-sounder-crw_amd", "scripts"))
    import segment_all
    import segment_sweep
    for mod in (segment_all, segment_sweep):
        parse = mod.get_args_parser().parse_args
        assert parse(["--synthetic", "40", "128"]).anchor_context is None and "anchor_context" in segment_all.ANCHOR_FLAGS
        assert parse(["--synthetic", "40", "128", "--anchor_every", "3", "--anchor_context", "restart"]).anchor_context == "restart"
        with pytest.raises(SystemExit):
            parse(["--synthetic", "40", "128", "--anchor_context", "cut"])
    with pytest.raises(SystemExit, match="--anchor_context needs --anchors or --anchor_every"):
        segment_all.check_anchor_flags(segment_all.get_args_parser().parse_args(["--synthetic", "40", "128", "--anchor_context", "restart"]))


# ---- the README's table: a full trace after a layer's onset, clamp mode -> restart (wrong labels among un-annotated frames >= f0)
TABLE = {(30, 13): ((12, 247), (36, 234)), (40, 24): ((20, 624), (31, 576)), (64, 48): ((32, 2016), (49, 1824))}


def _both(emb, seed, M, cxt, radius, knn, temp, anchor):
    Wc, _, Rc = ar.lists(emb, cxt, radius, knn, temp)
    clamp = ar.gather_anchored(seed, Wc, Rc, M, anchor)
    L, pred, *_ = rr.propagate(emb, seed, M, cxt, radius, knn, temp, anchor)
    return clamp, (L, pred)


def test_a_full_trace_after_the_onset_is_as_good_as_a_seed():
    for T, N, C, M, cxt, radius, temp, knn, amp in sr.DRIFT_SHAPES:
        for s in sr.DRIFT_SEEDS:
            emb, cls, f0 = ar.emerging_item(s, T, N, C, M, amp)
            seed = cls[0].astype(np.float32)
            sets = ar.emergence_anchors(cls, f0, M)
            for k, name in enumerate(("two frames late", "every 8 frames")):
                anchor = sets[name]
                (Lc, pc), (Lr, pr) = _both(emb, seed, M, cxt, radius, knn, temp, anchor)
                ec, er = ar.emergence_errors(pc, cls, f0, anchor), ar.emergence_errors(pr, cls, f0, anchor)
                print(f"[{T}, {N}] seed {s} {name}: clamp {ec[0]} -> restart {er[0]} of {er[1]}")
                a1 = min(f for f in range(f0, T) if ar.clamped(anchor[f], M).all())          # the first origin >= f0
                wrong = pr.T != cls
                assert not wrong[a1:].any() and not wrong[:f0].any(), (T, N, s, name)
                deep = np.zeros_like(wrong)
                deep[f0:a1] = cls[f0:a1] == M - 1
                assert np.array_equal(wrong, deep), (T, N, s, name)                          # exactly the new layer's nodes of [f0, a1)
                assert er[0] <= ec[0] and er == TABLE[(T, N)][k], (T, N, s, name, ec, er)
            onset = sets["onset, full"]
            (_, pc), (_, pr) = _both(emb, seed, M, cxt, radius, knn, temp, onset)
            assert ar.emergence_errors(pc, cls, f0 + 1, onset)[0] == ar.emergence_errors(pr, cls, f0 + 1, onset)[0] == 0
            # no new layer: restart never does worse than clamp mode
            emb, cls = sr.drifting_item(s, T, N, C, M, amp)
            anchor = np.full((T, N), -1, np.int8)
            anchor[8::8] = cls[8::8]
            (_, pc), (_, pr) = _both(emb, cls[0].astype(np.float32), M, cxt, radius, knn, temp, anchor)
            ec, er = ar.emergence_errors(pc, cls, 0, anchor), ar.emergence_errors(pr, cls, 0, anchor)
            print(f"[{T}, {N}] seed {s} drifting, every 8 frames: clamp {ec[0]} -> restart {er[0]} of {er[1]}")
            assert er[0] <= ec[0], (T, N, s, ec, er)


def test_print_the_two_sided_combination():
    """Printed, not asserted: restart forward plus restart reverse (seeded with the last trace, anchors mirrored), merged by maxprob."""
    for T, N, C, M, cxt, radius, temp, knn, amp in sr.DRIFT_SHAPES[:2]:
        for s in sr.DRIFT_SEEDS:
            emb, cls, f0 = ar.emerging_item(s, T, N, C, M, amp)
            anchor = ar.emergence_anchors(cls, f0, M)["two frames late"]
            Lf, pf, *_ = rr.propagate(emb, cls[0].astype(np.float32), M, cxt, radius, knn, temp, anchor)
            Lb, pb, *_ = rr.propagate(emb[::-1].copy(), cls[-1].astype(np.float32), M, cxt, radius, knn, temp, anchor[::-1].copy())
            Lb, pb = Lb.reshape(T, N, M)[::-1], pb[:, ::-1]
            take = Lb.max(-1) > Lf.reshape(T, N, M).max(-1)
            merged = np.where(take, pb.T, pf.T)
            wrong = merged != cls
            print(f"[{T}, {N}] seed {s}: forward {int((pf.T != cls)[f0:].sum())} wrong in frames >= f0; merged with the reverse pass "
                  f"{int(wrong[f0:].sum())}, and {int(wrong[:f0].sum())} before f0")
