"""GPU side of anchor_context='restart': the three entry points of include/crw_hip_restart.h through the C ABI, held to the
definition of tests/restart_ref.py (whose checker tests/test_restart.py proves on planted defects).
  * lists: `crw_labelprop_topk_origin` against the entry points WITHOUT origins called on the sub-item of every stretch between
    origins -- I equal and W / V bit-equal where the sub-item's call takes the same kernel route (a shorter item has fewer
    candidates: always so on the vector and the matrix-core route), `oracle.topk_lists_audit`'s derived bounds where a sub-item leaves
    the long-list route; origin NULL and origin all zero bit-equal to crw_labelprop_topk_grid / _topk_scores.
  * L, pred: `crw_labelprop_propagate_origin` bit-equal to crw_labelprop_propagate_sliding called once per stretch on the sub-item
    with seed = NULL on the same L, free rows within `oracle.gather_bound(knn)` of the fp64 sum on the rule's absolute rows
    (`restart_ref.violations`), on the ring route (its second long-term slot flips at every restart) and on the general route
    (CRW_LABELPROP_SLIDING_GENERAL=1); the batch entry point at G = 3 with different knn padding, slice by slice; all-zero origins
    bit-equal to crw_labelprop_propagate_sliding[_batch], marked lists included.
  * every entry point under `run_banded` and `run_twice` of tests/stale_ref.py.
Shapes: `anchored_ref.SHAPES` (what each exercises: tests/test_anchored_gpu.py) x `restart_ref.patterns`, and one shape per top-k
route from tests/test_labelprop_lists_gpu.py.  Nothing here provokes a fault."""
import ctypes

import numpy as np
import pytest
import torch

import anchored_ref as ar
import restart_ref as rr
import sliding_ref as slr
import stale_ref as sr
from oracle import crw_oracle as orc

pytestmark = pytest.mark.gpu

RING = ar.SHAPES[:5]          # the shapes the ring kernel takes, with and without origins
F32, I32 = torch.float32, torch.int32


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_sliding() and crw_hip.has_sweep() and crw_hip.has_anchor_restart()
    return crw_hip


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(status, what):
    assert status == 0, (what, status)


def topk_origin(lib, ehat, cxt, radius, temp, k, first, gw, origin, raw, out=None):
    T, N, C = ehat.shape
    WV, I = out or (torch.empty(T - first, k, N, device="cuda"), torch.empty(T - first, k, N, device="cuda", dtype=I32))
    _ok(lib.crw_labelprop_topk_origin(_p(ehat), T, N, C, cxt, radius, temp, k, first, gw, _p(origin), _p(WV), _p(I), raw, _stream()),
        "crw_labelprop_topk_origin")
    return WV, I


def topk_plain(lib, ehat, cxt, radius, temp, k, first, gw, raw, out=None):
    T, N, C = ehat.shape
    WV, I = out or (torch.empty(T - first, k, N, device="cuda"), torch.empty(T - first, k, N, device="cuda", dtype=I32))
    fn = lib.crw_labelprop_topk_scores if raw else lib.crw_labelprop_topk_grid
    _ok(fn(_p(ehat), T, N, C, cxt, radius, temp, k, first, gw, _p(WV), _p(I), _stream()), "crw_labelprop_topk_grid / _scores")
    return WV, I


def topk_cut(hip, ehat, cxt, radius, temp, k, first, gw, origin, raw):
    """the lists from the entry points without origins, one call per stretch on the sub-item"""
    T, N, C = ehat.shape
    WV, I = torch.zeros(T - first, k, N, device="cuda"), torch.zeros(T - first, k, N, device="cuda", dtype=I32)
    for a, e in hip.origin_stretches(origin.tolist(), T, first):
        ff = max(first - a, 1)
        at = a + ff - first
        topk_plain(hip.lib(), ehat[a:e + 1], cxt, radius, temp, k, ff, gw, raw, out=(WV[at:], I[at:]))
    return WV, I


def eq_bits(a, b):
    return torch.equal(a.view(I32), b.view(I32))


def propagate_origin(lib, seed, W, I, T, N, M, first, cxt, origin, L, pred):
    _ok(lib.crw_labelprop_propagate_origin(_p(seed), _p(W), _p(I), T, N, M, W.shape[1], first, cxt, _p(origin), _p(L), _p(pred), _stream()),
        "crw_labelprop_propagate_origin")
    return L, pred


@pytest.mark.parametrize("shape", ar.SHAPES, ids=str)
def test_every_pattern_on_every_route_is_the_definition(hip, monkeypatch, shape):
    T, N, C, M, cxt, radius, knn = shape
    lib = hip.lib()
    feats = hip.normalize(torch.from_numpy(rr.item(shape)).cuda())
    routes = (False, True) if shape in RING else (False,)
    knns = (knn, max(knn - 2, 1), 1)                                   # the batch: G = 3, padded to knn
    for name, (anchor_np, ff) in rr.patterns(T, N, M, cxt).items():
        anchor = torch.from_numpy(anchor_np)
        origin = hip.anchor_origins(anchor, M, T, ff)
        assert origin.tolist() == rr.origins(anchor_np, M, ff).tolist(), name
        od = origin.cuda()
        # ---- lists: the sub-item calls of the entry points without origins, bit for bit (the vector route in every shape here)
        W, I = topk_origin(lib, feats, cxt, radius, ar.TEMP, knn, ff, 1, od, 0)
        V, Iv = topk_origin(lib, feats, cxt, radius, ar.TEMP, knn, ff, 1, od, 1)
        Wc, Ic = topk_cut(hip, feats, cxt, radius, ar.TEMP, knn, ff, 1, origin, 0)
        Vc, _ = topk_cut(hip, feats, cxt, radius, ar.TEMP, knn, ff, 1, origin, 1)
        assert torch.equal(I, Ic) and torch.equal(Iv, Ic) and eq_bits(W, Wc) and eq_bits(V, Vc), name
        R = rr.rows_of(I.cpu().numpy(), origin.numpy(), N, cxt, ff)
        Wm, Im = hip.mark_anchors(W.clone(), I.clone(), anchor, M, ff)
        if ff == 1:
            seed, L_init, p_init = (torch.arange(N) * M // N).float().cuda(), None, None
        else:
            seed = None
            L_init, p_init = (torch.from_numpy(x).cuda() for x in ar.soft_init(T, N, M, ff))

        def fresh(fill, lead=()):
            L, p = torch.empty(*lead, T * N, M, device="cuda"), torch.empty(*lead, N, T, device="cuda")
            for t in (L, p):
                t.view(torch.uint8).fill_(fill)
            if L_init is not None:
                L[..., :ff * N, :], p[..., :ff] = L_init[:ff * N], p_init[:, :ff]
            return L, p

        # the segmented construction: crw_labelprop_propagate_sliding per stretch on the sub-item, seed = NULL, on the same L
        ref = hip._propagate_origin_segmented(seed, Wm, Im, origin.tolist(), T, N, M, knn, ff, cxt, *fresh(0))
        for general in routes:
            if general:
                monkeypatch.setenv("CRW_LABELPROP_SLIDING_GENERAL", "1")
            else:
                monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
            got = propagate_origin(lib, seed, Wm, Im, T, N, M, ff, cxt, od, *fresh(0x00))
            init = (None, None) if L_init is None else fresh(0)
            v = rr.violations(seed, W, R, M, anchor_np, ff, *got, *init, ref=ref)
            assert not any(v.values()), (name, "general" if general else "default", v)
            again = propagate_origin(lib, seed, Wm, Im, T, N, M, ff, cxt, od, *fresh(0xFF))
            assert eq_bits(again[0], got[0]) and torch.equal(again[1], got[1]), (name, general)
            if not origin.any():                                       # nothing restarts: the entry point without origins, marks and all
                for o in (od, None):
                    z = propagate_origin(lib, seed, Wm, Im, T, N, M, ff, cxt, o, *fresh(0x00))
                    L2, p2 = fresh(0x00)
                    _ok(lib.crw_labelprop_propagate_sliding(_p(seed), _p(Wm), _p(Im), T, N, M, knn, ff, cxt, _p(L2), _p(p2), _stream()), name)
                    assert eq_bits(z[0], L2) and torch.equal(z[1], p2) and eq_bits(z[0], got[0]), (name, general)
        monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
        # ---- the batch entry point: three configurations with different knn, padded, sharing I and the origins
        W3 = hip.labelprop_sweep_weights(V, knns)
        W3m, I3m = hip.mark_anchors(W3.clone(), I.clone(), anchor, M, ff)
        L3, p3 = fresh(0x00, (3,))
        _ok(lib.crw_labelprop_propagate_origin_batch(_p(seed), _p(W3m), _p(I3m), 0, 3, T, N, M, knn, ff, cxt, _p(od), _p(L3), _p(p3), _stream()),
            "crw_labelprop_propagate_origin_batch")
        for g in range(3):
            one = propagate_origin(lib, seed, W3m[g].contiguous(), I3m, T, N, M, ff, cxt, od, *fresh(0x00))
            assert eq_bits(L3[g], one[0]) and torch.equal(p3[g], one[1]), (name, g)
        assert eq_bits(L3[0], got[0]) and torch.equal(p3[0], got[1]), name
        if not origin.any():
            for o in (od, None):
                Lz, pz = fresh(0xFF, (3,))
                _ok(lib.crw_labelprop_propagate_origin_batch(_p(seed), _p(W3m), _p(I3m), 0, 3, T, N, M, knn, ff, cxt, _p(o), _p(Lz), _p(pz),
                                                             _stream()), name)
                Ls, ps = fresh(0x00, (3,))
                _ok(lib.crw_labelprop_propagate_sliding_batch(_p(seed), _p(W3m), _p(I3m), 0, 3, T, N, M, knn, ff, cxt, _p(Ls), _p(ps), _stream()),
                    name)
                assert eq_bits(Lz, Ls) and torch.equal(pz, ps), name


# (T, N, C, cxt, radius, knn, first, grid_w) of tests/test_labelprop_lists_gpu.py, one per top-k route, and the frames that restart
TOPK_ROUTES = [
    ((10, 12, 16, 3, 2, 5, 1, 1), (2, 3, 7)),            # vector kernel
    ((12, 30, 16, 4, 3, 7, 1, 5), (1, 6)),               # vector kernel on a 6 x 5 grid
    ((40, 21, 64, 6, 4, 9, 1, 1), (3, 20, 21, 38)),      # matrix cores in one piece
    ((90, 48, 128, 80, 10, 20, 1, 1), (5, 50)),          # matrix cores in two halves
    ((100, 48, 64, 80, 30, 20, 7, 1), (40, 95)),         # long-list form, first frame 7: the sub-items at 40 and 95 leave it
]


def topk_route(T, N, C, cxt, radius, gw):
    """`topk_grid`'s choice, as the comment over TOPK_CASES in tests/test_labelprop_lists_gpu.py derives it"""
    max_nf, max_bi = min(cxt + 1, T - 1), min(2 * radius - 1, N // gw)
    maxcand = max_nf * max_bi
    column = gw == 1 and N >= 16
    if column and C in (64, 128, 256) and maxcand <= 2048 and 64 * maxcand <= 150 * 1024:
        return "matrix cores"
    if column and C in (64, 128) and max_bi <= 1024:
        return "long lists"
    return "vector"


@pytest.mark.parametrize("shape,restarts", TOPK_ROUTES, ids=lambda v: "x".join(map(str, v)))
def test_topk_origin_on_every_route(hip, shape, restarts):
    from test_labelprop_lists import lp_embeddings
    T, N, C, cxt, radius, knn, first, gw = shape
    lib, temp = hip.lib(), 0.1
    feats = hip.normalize(lp_embeddings(T, N, C, T + N).cuda())
    origin = torch.zeros(T, dtype=I32)
    for n in range(1, T):
        origin[n] = n - 1 if n - 1 in restarts else origin[n - 1]
    assert hip.check_origin(origin, T) and origin.max() == max(restarts)
    od, zero = origin.cuda(), torch.zeros(T, dtype=I32, device="cuda")
    whole = topk_route(T, N, C, cxt, radius, gw)
    for raw in (0, 1):
        plain = topk_plain(lib, feats, cxt, radius, temp, knn, first, gw, raw)
        for o in (None, zero):
            got = topk_origin(lib, feats, cxt, radius, temp, knn, first, gw, o, raw)
            assert torch.equal(got[1], plain[1]) and eq_bits(got[0], plain[0]), (raw, o is None)
        WV, I = topk_origin(lib, feats, cxt, radius, temp, knn, first, gw, od, raw)
        cutWV, cutI = topk_cut(hip, feats, cxt, radius, temp, knn, first, gw, origin, raw)
        if raw == 0:
            V = topk_origin(lib, feats, cxt, radius, temp, knn, first, gw, od, 1)[0]
        for a, e in hip.origin_stretches(origin.tolist(), T, first):
            ff = max(first - a, 1)
            lo, hi = a + ff - first, e + 1 - first
            if topk_route(e + 1 - a, N, C, cxt, radius, gw) == whole:
                assert torch.equal(I[lo:hi], cutI[lo:hi]) and eq_bits(WV[lo:hi], cutWV[lo:hi]), (raw, a, e)
            elif raw == 0:                                             # the sub-item leaves the long-list route: the derived bounds
                assert whole == "long lists"
                res = orc.topk_lists_audit(feats[a:e + 1], cxt, radius, temp, knn, ff, gw, WV[lo:hi], I[lo:hi], V[lo:hi])
                print(f"{shape} stretch ({a}, {e}): worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in res["worst"].items()))
                assert not any(res["violations"].values()) and all(v <= 1 for v in res["worst"].values()), (a, e, res)


# ================================================================================================ stale memory and guard bands
def _out(*shape, dtype=F32, init=None):
    like = torch.empty(shape, dtype=dtype, device="meta")
    return sr.Buf(like.numel() * like.element_size(), dtype if dtype.is_floating_point else None, step=sr.largest_step(like), init=init)


def _as(t, name, dtype, *shape):
    like = torch.empty(shape, dtype=dtype, device="meta")
    return t[name][:like.numel() * like.element_size()].view(dtype).view(shape)


def banded_case(hip, home, shape, general):
    """the three entry points on one shape with two restarts (one of them at consecutive frames) and a partially anchored frame"""
    T, N, C, M, cxt, radius, knn = shape
    lib, G = hip.lib(), 3
    anchor = np.full((T, N), -1, np.int8)
    for f in (2, 3, T - 4):
        anchor[f] = (np.arange(N) + f) % M
    anchor[5, ::3] = 1
    anchor = torch.from_numpy(anchor)
    origin = hip.anchor_origins(anchor, M, T)
    feats = hip.normalize(torch.from_numpy(rr.item(shape)).cuda())
    V, I = hip.labelprop_topk_scores(feats, cxt, radius, ar.TEMP, knn, origin=origin)
    W3, I3 = hip.mark_anchors(hip.labelprop_sweep_weights(V, (knn, max(knn - 2, 1), 1)), I.clone(), anchor, M)
    ehat, od, W3, I3, seed = home.many(ehat=feats, origin=origin.cuda(), W3=W3, I3=I3, seed=(torch.arange(N) * M // N).float().cuda())
    F = T - 1
    bufs = dict(W=_out(F, knn, N), I=_out(F, knn, N, dtype=I32), V=sr.Buf(F * knn * N * 4, None, step=knn * N * 4), Iv=_out(F, knn, N, dtype=I32),
                L=_out(T * N, M), pred=_out(N, T), L3=_out(G, T * N, M), pred3=_out(G, N, T))

    def run(_, t):
        for raw, (w, i) in enumerate((("W", "I"), ("V", "Iv"))):
            _ok(lib.crw_labelprop_topk_origin(_p(ehat), T, N, C, cxt, radius, ar.TEMP, knn, 1, 1, _p(od), _p(t[w]), _p(t[i]), raw, _stream()),
                "crw_labelprop_topk_origin")
        _ok(lib.crw_labelprop_propagate_origin(_p(seed), _p(W3), _p(I3), T, N, M, knn, 1, cxt, _p(od), _p(t["L"]), _p(t["pred"]), _stream()),
            "crw_labelprop_propagate_origin")
        _ok(lib.crw_labelprop_propagate_origin_batch(_p(seed), _p(W3), _p(I3), 0, G, T, N, M, knn, 1, cxt, _p(od), _p(t["L3"]), _p(t["pred3"]),
                                                     _stream()), "crw_labelprop_propagate_origin_batch")
        torch.cuda.synchronize()

    case = sr.Case("crw_labelprop_topk_origin / _propagate_origin / _propagate_origin_batch" + (" (general route)" if general else ""),
                   None, bufs, run, device="cuda", home=home)

    def check(t):
        L, L3 = _as(t, "L", F32, T, N, M), _as(t, "L3", F32, G, T, N, M)
        assert torch.allclose(L.sum(-1), torch.ones(T, N, device="cuda"), atol=1e-4) and torch.equal(L, L3[0])
        assert torch.allclose(_as(t, "W", F32, F, knn, N).sum(1), torch.ones(F, N, device="cuda"), atol=1e-5)
        assert torch.equal(_as(t, "I", I32, F, knn, N), _as(t, "Iv", I32, F, knn, N))
        for f in (2, 3, T - 4):
            assert torch.equal(_as(t, "pred", F32, N, T)[:, f].cpu(), anchor[f].float())
    return case, check


@pytest.mark.parametrize("shape,general", [(ar.SHAPES[0], False), (ar.SHAPES[0], True), (ar.SHAPES[2], False), (ar.SHAPES[5], False)], ids=str)
def test_entry_points_over_stale_memory_and_between_guard_bands(hip, monkeypatch, shape, general):
    if general:
        monkeypatch.setenv("CRW_LABELPROP_SLIDING_GENERAL", "1")
    else:
        monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
    case, check = banded_case(hip, sr.Home("cuda"), shape, general)
    assert case.home.operands
    check(sr.run_banded(case))
    check(sr.run_twice(case))


# ================================================================================================ end to end
def test_a_full_trace_after_the_onset_on_the_device(hip, monkeypatch):
    """The first emerging item [30, 13] through `LabelPropVOS_CRW.propagate_all(anchor_context='restart')`: the CPU test's counts,
    the same labels under CRW_ANCHORS_RESTART_SEGMENTED=1, and the sweep's slices."""
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    from test_restart import TABLE
    T, N, C, M, cxt, radius, temp, knn, amp = slr.DRIFT_SHAPES[0]
    emb, cls, f0 = ar.emerging_item(0, T, N, C, M, amp)
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=cxt, RADIUS=radius, TEMP=temp, KNN=knn, CONTEXT="sliding"))
    sweep = LabelPropSweep(cxt, [radius], [temp], [knn, 2], context="sliding")
    feats, seed = hip.normalize(torch.tensor(emb).cuda()), torch.tensor(cls[0]).float().cuda()
    for k, name in enumerate(("two frames late", "every 8 frames")):
        anchor = ar.emergence_anchors(cls, f0, M)[name]
        a = torch.from_numpy(anchor).cuda()
        monkeypatch.delenv("CRW_ANCHORS_RESTART_SEGMENTED", raising=False)
        pred, L = lp.propagate_all(feats, seed, M, anchors=a, anchor_context="restart")
        clamp, _ = lp.propagate_all(feats, seed, M, anchors=a)
        ps, Ls = sweep.propagate_all(feats, seed, M, soft=True, anchors=a, anchor_context="restart")
        monkeypatch.setenv("CRW_ANCHORS_RESTART_SEGMENTED", "1")
        pred2, L2 = lp.propagate_all(feats, seed, M, anchors=a, anchor_context="restart")
        ps2, Ls2 = sweep.propagate_all(feats, seed, M, soft=True, anchors=a, anchor_context="restart")
        assert torch.equal(pred, pred2) and eq_bits(L, L2) and torch.equal(ps, ps2) and eq_bits(Ls, Ls2), name
        assert torch.equal(ps[0], pred) and eq_bits(Ls[0], L), name
        e, ec = ar.emergence_errors(pred.cpu().numpy(), cls, f0, anchor), ar.emergence_errors(clamp.cpu().numpy(), cls, f0, anchor)
        want = ar.emergence_errors(rr.propagate(emb, cls[0].astype(np.float32), M, cxt, radius, knn, temp, anchor)[1], cls, f0, anchor)
        print(f"{name}: clamp {ec[0]} -> restart {e[0]} of {e[1]} (CPU definition {want[0]})")
        assert e == want == TABLE[(T, N)][k], (name, e, want)


def test_segment_and_segment_sweep_restart_at_three_columns(hip, monkeypatch):
    """The 96 x 320 case of tests/test_anchored_gpu.py (two radargrams of T = 10, reverse pass, 'maxprob', merge='confidence', full
    traces at three columns) under anchor_context='restart': the one-launch route against CRW_ANCHORS_RESTART_SEGMENTED=1 -- labels
    equal, confidences bit for bit --, the sweep's 2 x 1 x 2 grid likewise and slice by slice against `segment`."""
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case
    enc, fresh, seg, _, N = e2e_case(0, n_rg=2, H=100)
    T, step = T_E2E, PATCH[1] - OVERLAP[1]
    rg_len = T * step + OVERLAP[1]
    assert (seg.shape[0], 2 * rg_len) == (96, 320)
    cols = [2 * step + 5, 6 * step, rg_len + 4 * step + 9]                    # frames 2 and 6 of radargram 0, frame 4 of radargram 1
    kw = dict(use_last=True, dataset_id=2, confidence="maxprob", merge="confidence", anchors=(seg, cols))
    keys = ("pred", "forward", "conf", "forward_conf")
    same = lambda a, b: all(torch.equal(a[k].view(I32) if a[k].dtype == F32 else a[k], b[k].view(I32) if b[k].dtype == F32 else b[k]) for k in keys)
    sweep = LabelPropSweep(6, context="sliding", radii=[4, 6], temps=[0.1], knns=[4, 8])
    seg_one = lambda cfg, **k: crw_inference.segment(fresh(), seg, enc, LabelPropVOS_CRW(dict(cfg)), M_E2E, T, PATCH, OVERLAP, **kw, **k)
    seg_all = lambda **k: crw_inference.segment_sweep(fresh(), seg, enc, sweep, M_E2E, T, PATCH, OVERLAP, **kw, **k)
    monkeypatch.delenv("CRW_ANCHORS_RESTART_SEGMENTED", raising=False)
    cfg = dict(CXT_SIZE=6, RADIUS=6, TEMP=0.1, KNN=8, CONTEXT="sliding")
    out, clamp, outs = seg_one(cfg, anchor_context="restart"), seg_one(cfg), seg_all(anchor_context="restart")
    assert out["anchor_context"] == "restart" and out["origin_traces"] == 3 and clamp["anchor_context"] == "clamp"
    assert "origin_traces" not in clamp and outs["anchor_context"] == "restart" and outs["origin_traces"] == 3
    assert same(clamp, seg_one(cfg, anchor_context="clamp")) and not torch.equal(out["pred"], clamp["pred"])     # the option is live
    per_cfg = [seg_one(c, anchor_context="restart") for c in sweep.configs]
    monkeypatch.setenv("CRW_ANCHORS_RESTART_SEGMENTED", "1")
    assert same(out, seg_one(cfg, anchor_context="restart")) and same(outs, seg_all(anchor_context="restart"))
    assert sweep.configs[3] == cfg
    for g, one in enumerate(per_cfg):
        for k in keys:
            a, b = outs[k][g], one[k]
            assert torch.equal(a, b.to(a.dtype)) if a.dtype != F32 else torch.equal(a.view(I32), b.view(I32)), (g, k)
    assert same(out, per_cfg[3])
