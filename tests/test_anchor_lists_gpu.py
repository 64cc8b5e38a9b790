"""Anchor marks in the lists, on the device: crw_labelprop_propagate_sliding and crw_labelprop_propagate_sliding_batch through the C
ABI on MARKED lists (`crw_hip.mark_anchors`), every operand between poisoned guard bands (`stale_ref.run_banded`: finite outputs,
the same bits under 0xFF and 0x00 bands, no band byte changed).  Held per case:
  * L and pred bit for bit those of the segmented route, `crw_hip.labelprop_gather(anchors=)` under CRW_ANCHORS_SEGMENTED=1 -- the
    K + 1 launches on UNMARKED lists that tests/test_anchored_gpu.py holds to the definition;
  * `anchored_ref.violations` against the loop definition reports nothing (clamped rows exactly one-hot, free rows within the
    fp32 bound of the fp64 sum over the pair's own earlier rows, pred the first maximum, earlier frames untouched);
  * lists without a mark: the bits of the un-anchored call.
Routes: the ring kernel (the first five of `anchored_ref.SHAPES` and `anchor_lists_ref.EXTRA_SHAPES`), the general kernels (the
same shapes under CRW_LABELPROP_SLIDING_GENERAL=1, and the sixth shape, whose lists do not fit the ring kernel's loader), and the
batch kernel (G = 3 on a shared and on a per-configuration I, one configuration padded from a smaller knn).
Patterns: `anchor_lists_ref.all_patterns` -- first_frame, cxt + 1, cxt + 2, T - 1, two consecutive frames, whole frames, node 0
only, node N - 1 only, class 0 and class M - 1, out-of-range values, first_frame 3 with marks in the ignored rows.
Nothing here provokes a fault: the marked lists' indices are classes in [0, M) and the lists' own in-range rows."""
import functools

import numpy as np
import pytest
import torch

import anchor_lists_ref as al
import anchored_ref as ar
import stale_ref as sr
from stale_ref import Buf, Case, Home
from test_encoder_stale_gpu import _ok, _p, _stream

pytestmark = pytest.mark.gpu

F32 = torch.float32
RING = ar.SHAPES[:5] + al.EXTRA_SHAPES      # the shapes crw_labelprop_propagate_sliding sends to the ring kernel
SHAPES = ar.SHAPES + al.EXTRA_SHAPES


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_sliding() and crw_hip.has_sweep()
    return crw_hip


def _out(*shape, init=None):
    like = torch.empty(shape, dtype=F32, device="meta")
    return Buf(like.numel() * 4, F32, step=sr.largest_step(like), init=init)


def _as(t, name, *shape):
    like = torch.empty(shape, dtype=F32, device="meta")
    return t[name][:like.numel() * 4].view(F32).view(shape)


@functools.lru_cache(maxsize=None)
def features(shape):
    import crw_hip
    T, N, C, M, cxt, radius, knn = shape
    g = torch.Generator().manual_seed(sum(shape))
    return crw_hip.normalize((torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).cuda())


def start_of(shape, ff):
    """(seed, L_init, pred_init) of a call from frame ff: a seed at ff = 1, else the caller's soft frames and no seed"""
    T, N, C, M, cxt, radius, knn = shape
    if ff == 1:
        return (torch.arange(N) * M // N).float().cuda(), None, None
    return (None,) + tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(T, N, M, ff))


def banded_call(entry, lib_call, shape, ff, lists, seed, L_init, p_init, G=None):
    """One C call on `lists` = (W, I), every operand between guard bands -> (L, pred) of the run with 0x00 bands.
    lib_call(seed, W, I, L, pred) makes the call on the banded operands."""
    T, N, C, M, cxt, radius, knn = shape
    home = Home("cuda")
    W, I, s = home.many(W=lists[0], I=lists[1], seed=seed)
    lead = () if G is None else (G,)
    rep = (lambda x: x) if G is None else (lambda x: x[None].expand(G, *x.shape).contiguous())
    init = lambda x: None if x is None else rep(x).reshape(-1).view(torch.uint8)
    bufs = dict(L=_out(*lead, T * N, M, init=init(L_init)), pred=_out(*lead, N, T, init=init(p_init)))

    def run(_, t):
        _ok(entry, lib_call(s, W, I, t["L"], t["pred"]))
        torch.cuda.synchronize()

    t = sr.run_banded(Case(entry, None, bufs, run, device="cuda", home=home))
    return _as(t, "L", *lead, T * N, M).clone(), _as(t, "pred", *lead, N, T).clone()


def segmented(hip, monkeypatch, shape, ff, W, I, anchor, seed, L_init, p_init):
    """the parent route: the binding under CRW_ANCHORS_SEGMENTED=1, K + 1 launches on the unmarked lists"""
    T, N, C, M, cxt, radius, knn = shape
    L, p = torch.zeros(T * N, M, device="cuda"), torch.zeros(N, T, device="cuda")
    if L_init is not None:
        L[:ff * N], p[:, :ff] = L_init[:ff * N], p_init[:, :ff]
    monkeypatch.setenv("CRW_ANCHORS_SEGMENTED", "1")
    try:
        return hip.labelprop_gather(seed, W, I, T, N, M, first_frame=ff, cxt_size=cxt, context="sliding", L=L, pred=p, anchors=anchor)
    finally:
        monkeypatch.delenv("CRW_ANCHORS_SEGMENTED")


def same_bits(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_marked_lists_on_every_route_are_the_segmented_route_and_the_definition(hip, monkeypatch, shape):
    T, N, C, M, cxt, radius, knn = shape
    lib = hip.lib()
    W1, I1 = hip.labelprop_topk(features(shape), cxt, radius, ar.TEMP, knn)
    routes = (False, True) if shape in RING else (False,)
    marked_nodes = 0
    for name, (anchor_np, ff) in al.all_patterns(T, N, M, cxt).items():
        W, I = W1[ff - 1:].contiguous(), I1[ff - 1:].contiguous()
        anchor = torch.from_numpy(anchor_np).cuda()
        seed, L_init, p_init = start_of(shape, ff)
        ref = segmented(hip, monkeypatch, shape, ff, W, I, anchor, seed, L_init, p_init)
        Wm, Im = hip.mark_anchors(W.clone(), I.clone(), anchor, M, ff)
        want_marks = al.mark(W.cpu().numpy(), I.cpu().numpy(), anchor_np, M, ff)
        assert np.array_equal(Wm.cpu().numpy().view(np.uint32), want_marks[0].view(np.uint32)) and np.array_equal(Im.cpu().numpy(), want_marks[1])
        marked_nodes += int(al.is_mark(want_marks[0]).sum())
        R = hip.sliding_rows(I, N, cxt, ff)
        call = lambda s, w, i, L, p: lib.crw_labelprop_propagate_sliding(_p(s), _p(w), _p(i), T, N, M, knn, ff, cxt, _p(L), _p(p), _stream())
        for general in routes:
            if general:
                monkeypatch.setenv("CRW_LABELPROP_SLIDING_GENERAL", "1")
            else:
                monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
            got = banded_call("crw_labelprop_propagate_sliding", call, shape, ff, (Wm, Im), seed, L_init, p_init)
            assert same_bits(got, ref), (name, "general" if general else "default")
            v = ar.violations(seed, W, R, M, anchor_np, ff, *got, L_init, p_init, ref=ref)
            assert not any(v.values()), (name, "general" if general else "default", v)
            if not ar.clamped(anchor_np[ff:], M).any():        # no mark: the lists are the caller's bits, the result the plain call's
                assert torch.equal(Wm.view(torch.int32), W.view(torch.int32)) and torch.equal(Im, I)
                L, p = torch.zeros(T * N, M, device="cuda"), torch.zeros(N, T, device="cuda")
                if L_init is not None:
                    L[:ff * N], p[:, :ff] = L_init[:ff * N], p_init[:, :ff]
                plain = hip.labelprop_gather(seed, W, I, T, N, M, first_frame=ff, cxt_size=cxt, context="sliding", L=L, pred=p)
                assert same_bits(plain, got), name
        monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
    assert marked_nodes > 0


@pytest.mark.parametrize("general", (False, True), ids=("ring", "general"))
def test_a_marked_node_is_exactly_one_hot_and_every_label_is_finite(hip, monkeypatch, general):
    """What a library without the marks cannot pass: there the -inf weight makes the marked rows, and every row that reads them,
    non-finite.  Straight through the C entry point, no binding route in between: exact 1.0f / +0.0f bits at the marked nodes, the
    class in pred, finite L everywhere -- with every other slot of a marked list holding NaN weights and the index of the last
    row of L (NaN here until frame T - 1 is written), which the header says are ignored."""
    shape = ar.SHAPES[0]
    T, N, C, M, cxt, radius, knn = shape
    if general:
        monkeypatch.setenv("CRW_LABELPROP_SLIDING_GENERAL", "1")
    W, I = hip.labelprop_topk(features(shape), cxt, radius, ar.TEMP, knn)
    anchor_np, ff = ar.patterns(T, N, M, cxt)["partial rows: a third of the nodes at three frames"]
    anchor_np = anchor_np.copy()
    anchor_np[T - 1] = np.arange(N) % M
    Wm, Im = hip.mark_anchors(W.clone(), I.clone(), torch.from_numpy(anchor_np).cuda(), M, ff)
    v = torch.from_numpy(ar.clamped(anchor_np[ff:], M)).cuda()
    Wm[:, 1:] = torch.where(v[:, None], torch.full_like(Wm[:, 1:], float("nan")), Wm[:, 1:])
    Im[:, 1:] = torch.where(v[:, None], torch.full_like(Im[:, 1:], T * N - 1), Im[:, 1:])   # a row no frame may read (still inside L)
    seed = (torch.arange(N) * M // N).float().cuda()
    L, pred = torch.full((T * N, M), float("nan"), device="cuda"), torch.full((N, T), float("nan"), device="cuda")
    _ok("crw_labelprop_propagate_sliding", hip.lib().crw_labelprop_propagate_sliding(_p(seed), _p(Wm), _p(Im), T, N, M, knn, ff, cxt, _p(L),
                                                                                     _p(pred), _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(L).all() and torch.isfinite(pred).all()
    rows = L.view(T, N, M)[ff:][v]
    cls = torch.from_numpy(anchor_np[ff:]).cuda()[v].long()
    want = torch.nn.functional.one_hot(cls, M).float()
    assert v.sum() > N and torch.equal(rows.view(torch.int32), want.view(torch.int32))      # 0x3F800000 and 0x00000000, no -0.0f
    assert torch.equal(pred.t()[ff:][v], cls.float())
    free = L.view(T, N, M)[ff:][~v]
    assert torch.allclose(free.sum(-1), torch.ones(free.shape[0], device="cuda"), atol=1e-4)


def test_a_slot0_index_outside_the_classes_is_clamped_and_other_negative_weights_are_no_mark(hip):
    """The class is the slot-0 index clamped into [0, M - 1]; a weight of -1, of -FLT_MAX or of +inf is a weight like before."""
    T, N, M, cxt, knn = 4, 3, 3, 2, 2
    seed = torch.tensor([0.0, 1.0, 2.0], device="cuda")
    W = torch.zeros(T - 1, knn, N, device="cuda")
    I = torch.zeros(T - 1, knn, N, device="cuda", dtype=torch.int32)
    W[:, 0] = 1.0
    I[:, 0] = torch.arange(N, dtype=torch.int32)               # every node copies itself from frame 0
    W[0, 0, 0], I[0, 0, 0] = float("-inf"), 7                   # frame 1, node 0: class clamps to M - 1
    W[0, 0, 1], I[0, 0, 1] = float("-inf"), -5                  # frame 1, node 1: class clamps to 0
    W[1, 0, 2] = -1.0                                           # frame 2, node 2: an ordinary (negative) weight
    L, pred = torch.zeros(T * N, M, device="cuda"), torch.zeros(N, T, device="cuda")
    _ok("crw_labelprop_propagate_sliding", hip.lib().crw_labelprop_propagate_sliding(_p(seed), _p(W), _p(I), T, N, M, knn, 1, cxt, _p(L),
                                                                                     _p(pred), _stream()))
    torch.cuda.synchronize()
    L = L.view(T, N, M)
    assert L[1, 0].tolist() == [0, 0, 1] and L[1, 1].tolist() == [1, 0, 0] and L[1, 2].tolist() == [0, 0, 1]
    assert L[2, 2].tolist() == [0, 0, -1] and pred[:, 1].tolist() == [2, 0, 2]


@pytest.mark.parametrize("shared", (True, False), ids=("i_stride 0", "per-configuration I"))
def test_the_batch_kernel_honours_the_marks_of_every_configuration(hip, monkeypatch, shared):
    """G = 3 on the lists of a sweep: knn (3, 5, 5) at two temperatures' worth of weights -- configuration 0 is padded from knn 3
    to 5 with zero weights, slot 0 stays a real slot.  Slice g equals the segmented route on configuration g's unmarked lists."""
    shape = ar.SHAPES[1]
    T, N, C, M, cxt, radius, knn = shape
    G, feats, lib = 3, features(shape), hip.lib()
    V, I = hip.labelprop_topk_scores(feats, cxt, radius, ar.TEMP, knn)
    W3 = hip.labelprop_sweep_weights(V, [3, knn])                                          # [2, F, knn, N]
    V2, I2 = hip.labelprop_topk_scores(feats, cxt, radius, 0.5, knn)
    W3 = torch.cat([W3, hip.labelprop_sweep_weights(V2, [knn])]).contiguous()
    assert torch.equal(I, I2) and (W3[0][:, 3:] == 0).all() and (W3[0][:, :3] > 0).any()
    I3 = I if shared else I[None].expand(G, *I.shape).contiguous()
    for name in ("two consecutive frames", "partial rows: a third of the nodes at three frames", "every frame", "none",
                 "first_frame 3, no seed: anchors on frames 1 - 2 ignored"):
        anchor_np, ff = ar.patterns(T, N, M, cxt)[name]
        anchor = torch.from_numpy(anchor_np).cuda()
        seed, L_init, p_init = start_of(shape, ff)
        Wf, If = W3[:, ff - 1:].contiguous(), I3[..., ff - 1:, :, :].contiguous()
        Wm, Im = hip.mark_anchors(Wf.clone(), If.clone(), anchor, M, ff)
        stride = 0 if shared else (T - ff) * knn * N
        call = lambda s, w, i, L, p: lib.crw_labelprop_propagate_sliding_batch(_p(s), _p(w), _p(i), stride, G, T, N, M, knn, ff, cxt, _p(L), _p(p),
                                                                               _stream())
        L, pred = banded_call("crw_labelprop_propagate_sliding_batch", call, shape, ff, (Wm, Im), seed, L_init, p_init, G=G)
        for g in range(G):
            Ig = If if shared else If[g]
            ref = segmented(hip, monkeypatch, shape, ff, Wf[g], Ig, anchor, seed, L_init, p_init)
            assert same_bits((L[g], pred[g]), ref), (name, g)
            v = ar.violations(seed, Wf[g], hip.sliding_rows(Ig, N, cxt, ff), M, anchor_np, ff, L[g], pred[g], L_init, p_init, ref=ref)
            assert not any(v.values()), (name, g, v)


def test_the_library_says_that_it_honours_the_marks_and_the_binding_takes_one_launch(hip, monkeypatch):
    monkeypatch.delenv("CRW_ANCHORS_SEGMENTED", raising=False)
    assert hip.has_anchor_lists() and not hip.anchors_segmented()
    monkeypatch.setenv("CRW_ANCHORS_SEGMENTED", "1")
    assert hip.anchors_segmented()
    monkeypatch.delenv("CRW_ANCHORS_SEGMENTED")
    shape = ar.SHAPES[1]
    T, N, C, M, cxt, radius, knn = shape
    W, I = hip.labelprop_topk(features(shape), cxt, radius, ar.TEMP, knn)
    anchor_np, ff = ar.patterns(T, N, M, cxt)["partial rows: a third of the nodes at three frames"]
    anchor, (seed, _, _) = torch.from_numpy(anchor_np).cuda(), start_of(shape, ff)
    W0, I0 = W.clone(), I.clone()
    calls = []
    real = hip.lib().crw_labelprop_propagate_sliding
    monkeypatch.setattr(hip, "_sliding_lib", lambda: type("L", (), {"crw_labelprop_propagate_sliding": staticmethod(lambda *a: calls.append(1) or real(*a))}))
    got = hip.labelprop_gather(seed, W, I, T, N, M, cxt_size=cxt, context="sliding", anchors=anchor)
    assert len(calls) == 1 and torch.equal(W.view(torch.int32), W0.view(torch.int32)) and torch.equal(I, I0)
    monkeypatch.undo()
    ref = segmented(hip, monkeypatch, shape, ff, W, I, anchor, seed, None, None)
    assert same_bits(got, ref)
