"""GPU side of the memory bank in the parameter sweep: crw_labelprop_propagate_long_batch (include/crw_hip_sweepmem.h) through the
C ABI, and the sweep's host path on top of it.
  * n_long = 1, frame 0 from a seed: the bits of crw_labelprop_propagate_sliding_batch;
  * n_long in {2, 3, 6}, G = 4: slice g bit-equal to crw_labelprop_propagate_long on configuration g's lists on routes 1 and 2, and
    inside (knn + 2) * 2^-24 of `longmem_ref.ring_gather` in fp64 -- distinct I per configuration, one shared I with configurations
    padded from a smaller knn, first frames inside the bank, at its end and behind it;
  * a ring smaller than the context that wraps more than twice; the LDS edge and the binding's fallback; anchor marks; planted
    out-of-range indices; stale memory and guard bands; argument checks;
  * `segment_sweep(bank=)` against `segment(memory=, memory_bias=)` configuration by configuration, and the [30, 13] rows of the
    bank tables through the sweep.
Nothing here provokes a fault: every index the kernel sees is clamped by the kernel, which is what the planted indices show."""
import os

import numpy as np
import pytest
import torch

import anchored_ref as ar
import longmem_ref as lm
import sliding_ref as slr
import stale_ref as sr
from test_longmem_gpu import (EINVAL, F32, I32, LONG_SHAPES, _as, _out, _p, _stream, eq_bits, features, fresh, prop_long, ring_fits,
                              topk_long, topk_plain)

pytestmark = pytest.mark.gpu

ROUTE = "labelprop.batch_slide"  # the sliding batch's route: the bank's instance is logged through the same site


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_sweep_memory() and crw_hip.has_long_memory() and crw_hip.has_sweep() and crw_hip.has_routes()
    return crw_hip


def prop_batch(lib, W, I, T, N, M, first, cxt, K, L, pred, want=0):
    """crw_labelprop_propagate_long_batch on W [G, F, knn, N] and I of that shape (its own per configuration) or [F, knn, N] (shared)"""
    G, F, knn = W.shape[0], W.shape[1], W.shape[2]
    stride = F * knn * N if I.dim() == 4 else 0
    st = lib.crw_labelprop_propagate_long_batch(_p(W), _p(I), stride, G, T, N, M, knn, first, cxt, K, _p(L), _p(pred), _stream())
    assert st == want, ("crw_labelprop_propagate_long_batch", st)
    return L, pred


def fresh_batch(G, T, N, M, first, init, fill=0):
    parts = [fresh(T, N, M, first, init, fill) for _ in range(G)]
    return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])


def slices_equal(lib, W, I, T, N, M, first, cxt, K, init, got, routes):
    """slice g of `got` against crw_labelprop_propagate_long on configuration g's lists, on each of `routes`"""
    for g in range(W.shape[0]):
        Ig = I[g] if I.dim() == 4 else I
        for route in routes:
            L, p = prop_long(lib, W[g].contiguous(), Ig.contiguous(), T, N, M, first, cxt, K, *fresh(T, N, M, first, init, 0xFF), route)
            assert eq_bits(got[0][g], L) and torch.equal(got[1][g], p), (g, route, first)


# ================================================================================================ n_long = 1: the sliding batch
@pytest.mark.parametrize("shape", [(14, 10, 8, 3, 4, 3, 4), LONG_SHAPES[1]], ids=lambda v: "x".join(map(str, v)))
def test_one_long_term_frame_is_the_sliding_batch(hip, shape):
    F, N, C, M, cxt, radius, knn = shape
    lib, G = hip.lib(), 3
    feats = features(hip, F, N, C, sum(shape))
    lists = [topk_plain(lib, feats, cxt, radius + g, 0.05 * (g + 1), knn, 1, 0) for g in range(G)]
    W, I = torch.stack([w for w, _ in lists]), torch.stack([i for _, i in lists])
    seed = (torch.arange(N, device="cuda") * M // N).float()
    L0, p0 = torch.empty(G, F * N, M, device="cuda"), torch.empty(G, N, F, device="cuda")
    with hip.routes() as hit:
        assert lib.crw_labelprop_propagate_sliding_batch(_p(seed), _p(W), _p(I), (F - 1) * knn * N, G, F, N, M, knn, 1, cxt, _p(L0), _p(p0),
                                                         _stream()) == 0
    assert set(hit) == {"labelprop.batch_slide"}, hit
    L, p = torch.empty_like(L0), torch.empty_like(p0)
    for t in (L, p):
        t.view(torch.uint8).fill_(0xFF)
    L[:, :N] = (seed[:, None] == torch.arange(M, device="cuda")).float()
    p[:, :, 0] = seed
    with hip.routes() as hit:
        prop_batch(lib, W, I, F, N, M, 1, cxt, 1, L, p)
    assert set(hit) == {ROUTE}, hit
    assert eq_bits(L, L0) and torch.equal(p, p0)
    via = hip.labelprop_propagate_batch(seed, W, I, F, N, M, 1, cxt, context="sliding", n_long=1)
    assert eq_bits(via[0], L0) and torch.equal(via[1], p0)


# ================================================================================================ n_long > 1 against the one-configuration kernel
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("K", (2, 3, 6))
def test_a_bank_in_the_batch_is_the_one_configuration_kernel(hip, shape, K):
    F, N, C, M, cxt, radius, knn = shape
    lib, G = hip.lib(), 4
    feats = features(hip, F, N, C, sum(shape) + K)
    assert ring_fits(N, M, cxt, K, knn)
    bound = (knn + 2) * 2.0 ** -24
    for first in sorted({1, K, K + 2}):
        init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 11 * first + K))
        # distinct I per configuration: four (radius, temp) selections
        own = [topk_long(lib, feats, cxt, K, radius + g % 2, 0.05 * (g + 1), knn, first, 0) for g in range(G)]
        Wd, Id = torch.stack([w for w, _ in own]), torch.stack([i for _, i in own])
        # one shared I: the sweep's weights of one selection, two configurations padded from a smaller knn
        V, Is = topk_long(lib, feats, cxt, K, radius, 0.1, knn, first, 1)
        Ws = hip.labelprop_sweep_weights(V, [knn, knn - 1, knn, 1])
        assert not Ws[1][:, knn - 1:].any() and not Ws[3][:, 1:].any()
        for W, I in ((Wd, Id), (Ws, Is)):
            with hip.routes() as hit:
                got = prop_batch(lib, W, I, F, N, M, first, cxt, K, *fresh_batch(G, F, N, M, first, init, 0xFF))
            assert set(hit) == {ROUTE}, hit
            slices_equal(lib, W, I, F, N, M, first, cxt, K, init, got, (1, 2))
            worst = 0.0
            for g in range(G):
                Ig = I[g] if I.dim() == 4 else I
                Lr, pr = lm.ring_gather(W[g].cpu().numpy(), Ig.cpu().numpy(), N, M, cxt, K, first, init[0].cpu().numpy(),
                                        init[1].cpu().numpy(), np.float64)
                worst = max(worst, float(np.abs(got[0][g].cpu().numpy().astype(np.float64) - Lr).max()))
                assert eq_bits(got[0][g][:first * N], init[0][:first * N]) and torch.equal(got[1][g][:, :first], init[1][:, :first])
            print(f"{shape} K = {K} first = {first} ({'own' if I.dim() == 4 else 'shared'} I): max |L - fp64 ring| = {worst:.3g}, "
                  f"bound {bound:.3g}")
            assert worst <= bound, (first, worst, bound)


def test_a_ring_smaller_than_the_context_that_wraps_more_than_twice(hip):
    """N M 4 = 6 KiB: R = 25 - 3 = 22 < cxt + 1 = 31, 67 chained frames: rows older than the ring from global memory, long-term rows
    and ring rows from LDS in one list"""
    F, N, M, cxt, knn, K, C, radius = 70, 96, 16, 30, 8, 3, 16, 5
    lib, G = hip.lib(), 2
    assert 150 * 1024 // (4 * N * M) - K == 22
    feats = features(hip, F, N, C, 41)
    init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 5))
    own = [topk_long(lib, feats, cxt, K, radius, 0.07 * (g + 1), knn, K, 0) for g in range(G)]
    W, I = torch.stack([w for w, _ in own]), torch.stack([i for _, i in own])
    rows_read = lm.rows(I[0].cpu().numpy(), N, cxt, K, K)
    n = np.arange(K, F)[:, None, None]
    assert ((rows_read >= K * N) & (rows_read < (n - 22 + 1) * N)).any()  # a list does reach behind the ring
    with hip.routes() as hit:
        got = prop_batch(lib, W, I, F, N, M, K, cxt, K, *fresh_batch(G, F, N, M, K, init, 0xFF))
    assert set(hit) == {ROUTE}, hit
    slices_equal(lib, W, I, F, N, M, K, cxt, K, init, got, (0, 1))


def test_the_lds_edge(hip):
    """N M = 7 680 (30 KiB a frame, five in 150 KiB): n_long = 3 leaves a two-frame ring and runs, 4 is CRW_EINVAL from the C entry
    point and the one-configuration routes, slice by slice, from the binding"""
    F, N, M, C, cxt, radius, knn = 8, 96, 80, 8, 4, 4, 4
    lib, G = hip.lib(), 2
    feats = features(hip, F, N, C, 3)
    for K in (3, 4):
        assert hip.sweep_memory_fits(N, M, K) == (K == 3)
        init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, K))
        own = [topk_long(lib, feats, cxt, K, radius, 0.1 * (g + 1), knn, K, 0) for g in range(G)]
        W, I = torch.stack([w for w, _ in own]), torch.stack([i for _, i in own])
        with hip.routes() as one:
            want = [prop_long(lib, W[g], I[g], F, N, M, K, cxt, K, *fresh(F, N, M, K, init), 0) for g in range(G)]
        if K == 4:
            L, p = fresh_batch(G, F, N, M, K, init)
            before = L.clone()
            prop_batch(lib, W, I, F, N, M, K, cxt, K, L, p, want=EINVAL)
            assert eq_bits(L, before)
        with hip.routes() as hit:
            got = hip.labelprop_propagate_batch(None, W, I, F, N, M, K, cxt, *fresh_batch(G, F, N, M, K, init, 0xFF), context="sliding",
                                                n_long=K)
        assert set(hit) == ({ROUTE} if K == 3 else set(one)), (K, hit, one)
        assert ROUTE not in one and all(r.startswith("labelprop.slide_general") for r in one), one
        for g in range(G):
            assert eq_bits(got[0][g], want[g][0]) and torch.equal(got[1][g], want[g][1]), (K, g)


# ================================================================================================ anchor marks, planted indices
@pytest.mark.parametrize("pattern", ("two consecutive frames", "partial rows: a third of the nodes at three frames"))
def test_anchor_marks_under_a_bank_of_three(hip, pattern):
    F, N, C, M, cxt, radius, knn = ar.SHAPES[0]
    K, first, lib, G = 3, 3, hip.lib(), 2
    feats = features(hip, F, N, C, 17)
    anchor_np, _ = ar.patterns(F, N, M, cxt)[pattern]
    assert ar.clamped(anchor_np[first:], M).any()
    marked = []
    for g in range(G):
        W, I = topk_long(lib, feats, cxt, K, radius, ar.TEMP * (g + 1), knn, first, 0)
        I[0, 1, ::2] = 10 ** 6                                       # (planted: out of range, the clamp of the rule)
        I[2, 0, 1::2] = -5
        marked.append(hip.mark_anchors(W.clone(), I.clone(), torch.from_numpy(anchor_np), M, first))
    W, I = torch.stack([w for w, _ in marked]), torch.stack([i for _, i in marked])
    init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 3))
    got = prop_batch(lib, W, I, F, N, M, first, cxt, K, *fresh_batch(G, F, N, M, first, init, 0xFF))
    slices_equal(lib, W, I, F, N, M, first, cxt, K, init, got, (0, 1, 2))
    cl = ar.clamped(anchor_np, M)
    for g in range(G):
        pred = got[1][g].cpu().numpy().T
        assert np.array_equal(pred[first:][cl[first:]], anchor_np[first:][cl[first:]].astype(np.float32))


def test_planted_out_of_range_indices_are_clamped(hip):
    F, N, C, M, cxt, radius, knn = LONG_SHAPES[1]
    K, lib, G = 3, hip.lib(), 2
    feats = features(hip, F, N, C, 29)
    init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 4))
    for first in (1, K):
        W, I = topk_long(lib, feats, cxt, K, radius, 0.1, knn, first, 0)
        I = torch.stack([I, I.clone()])
        n = F - first
        I[0, 0, 0, 0], I[0, 1, knn - 1, N - 1], I[1, n - 1, 0, N // 2], I[1, n // 2, 1, 1] = 2 ** 30, -7, min(F - 1, K + cxt) * N, -2 ** 31
        W = torch.stack([W, W.clone()])
        got = prop_batch(lib, W, I, F, N, M, first, cxt, K, *fresh_batch(G, F, N, M, first, init, 0xFF))
        slices_equal(lib, W, I, F, N, M, first, cxt, K, init, got, (1, 2))
        assert torch.isfinite(got[0]).all()


# ================================================================================================ stale memory and guard bands
def banded_case(hip, home, shape, K, shared):
    F, N, C, M, cxt, radius, knn = shape
    lib, n, G = hip.lib(), F - K, 2
    feats = features(hip, F, N, C, 23)
    W, I = topk_long(lib, feats, cxt, K, radius, 0.1, knn, K, 0)
    I[0, 0, 0], I[1, knn - 1, N - 1], I[n - 1, 0, N // 2] = 2 ** 30, -7, min(F - 1, K + cxt) * N
    anchor = np.full((F, N), -1, np.int8)
    anchor[K + 1] = np.arange(N) % M
    W, I = hip.mark_anchors(W, I, torch.from_numpy(anchor), M, K)
    W2, _ = topk_long(lib, feats, cxt, K, radius, 0.3, knn, K, 0)
    W2, _ = hip.mark_anchors(W2, I.clone(), torch.from_numpy(anchor), M, K)
    W = torch.stack([W, W2]).contiguous()
    I = I.contiguous() if shared else torch.stack([I, I]).contiguous()
    L_init, p_init = (torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 9))
    W, I, L_front, p_front = home.many(W=W, I=I, L_front=L_init[:K * N].contiguous(), p_front=p_init[:, :K].contiguous())
    bufs = dict(L=_out(G, F * N, M), pred=_out(G, N, F))

    def run(_, t):
        L, pred = _as(t, "L", F32, G, F * N, M), _as(t, "pred", F32, G, N, F)
        L[:, :K * N], pred[:, :, :K] = L_front, p_front              # the caller's frames: written here, read by the entry point
        pred[:, :, K:] = 0
        prop_batch(lib, W, I, F, N, M, K, cxt, K, L, pred)
        torch.cuda.synchronize()

    case = sr.Case(f"crw_labelprop_propagate_long_batch ({'shared' if shared else 'own'} I)", None, bufs, run, device="cuda", home=home)

    def check(t):
        L, pred = _as(t, "L", F32, G, F, N, M), _as(t, "pred", F32, G, N, F)
        assert torch.allclose(L.sum(-1), torch.ones(G, F, N, device="cuda"), atol=1e-4)
        assert eq_bits(L[:, :K].reshape(G, K * N, M), L_front.expand(G, -1, -1).contiguous())
        assert torch.equal(pred[:, :, :K], p_front.expand(G, -1, -1))
        for g in range(G):
            assert torch.equal(pred[g][:, K + 1].cpu(), torch.from_numpy(anchor[K + 1]).float())
        return L
    return case, check


@pytest.mark.parametrize("shape,K,shared", [(LONG_SHAPES[0], 3, False), (LONG_SHAPES[1], 6, True), (LONG_SHAPES[2], 2, False)], ids=str)
def test_entry_point_over_stale_memory_and_between_guard_bands(hip, shape, K, shared):
    case, check = banded_case(hip, sr.Home("cuda"), shape, K, shared)
    assert case.home.operands
    a = check(sr.run_banded(case))
    b = check(sr.run_twice(case))
    assert eq_bits(a, b)


def test_argument_checks(hip):
    lib = hip.lib()
    F, N, C, M, cxt, knn, G = 8, 10, 8, 3, 3, 4, 2
    feats = features(hip, F, N, C, 1)
    W, I = topk_long(lib, feats, cxt, 2, 3, 0.1, knn, 2, 0)
    W, I = torch.stack([W, W]), torch.stack([I, I])
    L, p = torch.zeros(G, F * N, M, device="cuda"), torch.zeros(G, N, F, device="cuda")
    for K, first in ((0, 1), (F, 1), (-1, 2), (2, 0), (2, F)):
        prop_batch(lib, W, I, F, N, M, first, cxt, K, L, p, want=EINVAL)
    prop_batch(lib, W, I, F, N, M, 2, 0, 2, L, p, want=EINVAL)                       # what the sliding batch refuses: cxt_size < 1
    st = lambda **k: lib.crw_labelprop_propagate_long_batch(*[k.get(a, d) for a, d in (
        ("W", _p(W)), ("I", _p(I)), ("stride", 0), ("G", G), ("T", F), ("N", N), ("M", M), ("knn", knn), ("first", 2), ("cxt", cxt),
        ("K", 2), ("L", _p(L)), ("pred", _p(p)), ("stream", _stream()))])
    for bad in (dict(G=0), dict(G=65536), dict(knn=65), dict(W=None), dict(I=None), dict(L=None), dict(pred=None), dict(M=0), dict(N=0),
                dict(N=96, M=81)):                                                    # a frame above 30 KiB
        assert st(**bad) == EINVAL, bad
    assert not L.any() and not p.any()
    for kw, msg in ((dict(n_long=2, origin=torch.zeros(F, dtype=I32)), "n_long and origin are not combined"),
                    (dict(n_long=2, context="reference"), "n_long needs context='sliding'"), (dict(n_long=F), "n_long must be in 1 .. T - 1")):
        with pytest.raises(ValueError, match=msg):
            hip.labelprop_propagate_batch(None, W, I, F, N, M, 2, cxt, L, p, **{"context": "sliding", **kw})


# ================================================================================================ the host path, end to end
E2E_OPTIONS = {"plain": {}, "seedless": dict(seedless=True), "centred": dict(bank_align="center"),
               "bilinear maps merged by confidence": dict(use_last=True, upsample="bilinear", confidence="maxprob", merge="confidence"),
               "anchors": "anchors", "per configuration": {}}


@pytest.mark.parametrize("name", list(E2E_OPTIONS))
def test_segment_sweep_with_a_bank_is_segment_per_configuration(hip, monkeypatch, name):
    """The 96 x 320 case of tests/test_anchored_gpu.py, a bank of four traces of the first radargram, the grid radii [4, 6] x temp
    [0.1] x biases [0, 0.1] x knns [4, 8]: slice g is `segment(memory=, memory_bias=b_g)` for configs[g] -- labels equal,
    confidences bit for bit."""
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case
    enc, fresh_ds, seg, _, N = e2e_case(0, n_rg=2, H=100)
    T, step = T_E2E, PATCH[1] - OVERLAP[1]
    rg_len = T * step + OVERLAP[1]
    assert (seg.shape[0], 2 * rg_len) == (96, 320)
    sweep = LabelPropSweep(6, [4, 6], [0.1], [4, 8], context="sliding", biases=[0.0, 0.1])
    assert len(sweep) == 8 and [c["MEMORY_BIAS"] for c in sweep.configs] == [0.0, 0.0, 0.1, 0.1] * 2
    bank = crw_utils.bank_from_columns(fresh_ds(), seg, [0, 3 * step, 6 * step + 5, 9 * step])
    opts = E2E_OPTIONS[name]
    if opts == "anchors":
        opts = dict(anchors=(seg, [2 * step + 5, 6 * step, rg_len + 4 * step + 9]), use_last=True, confidence="maxprob", merge="confidence")
    kw = dict(dataset_id=2, **opts)
    if name == "per configuration":
        monkeypatch.setenv("CRW_SWEEP_PER_CONFIG", "1")
    with hip.routes() as hit:
        out = crw_inference.segment_sweep(fresh_ds(), seg, enc, sweep, M_E2E, T, PATCH, OVERLAP, bank=bank, **kw)
    assert (ROUTE in hit) == (name != "per configuration"), hit
    assert out["memory_traces"] == 4 and out["seedless"] is bool(opts.get("seedless", False)) and out["memory_align"] == opts.get("bank_align")
    monkeypatch.delenv("CRW_SWEEP_PER_CONFIG", raising=False)
    skw = {("memory_align" if k == "bank_align" else k): v for k, v in kw.items()}
    differ = 0
    for g, cfg in enumerate(sweep.configs):
        one = crw_inference.segment(fresh_ds(), seg, enc, LabelPropVOS_CRW(cfg), M_E2E, T, PATCH, OVERLAP, memory=bank,
                                    memory_bias=cfg["MEMORY_BIAS"], **skw)
        for k in ("pred", "forward"):
            assert torch.equal(out[k][g].to(one[k].dtype), one[k]), (name, g, k)
        for k in ("conf", "forward_conf"):
            assert (k in out) == (k in one)
            if k in out:
                assert eq_bits(out[k][g].contiguous(), one[k].contiguous()), (name, g, k)
        differ += int(g >= 2 and not torch.equal(out["forward"][g], out["forward"][g - 2]))
    assert differ, "the bias changes no map: the axis is not exercised"


def test_the_tables_rows_of_the_smallest_shape_through_the_sweep(hip):
    """the [30, 13] rows of the README's bank tables through `LabelPropSweep.propagate_all(memory=)`: `longmem_ref.bank_errors`"""
    from imported.labelprop import LabelPropSweep
    shape = slr.DRIFT_SHAPES[0]
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    sweep = LabelPropSweep(cxt, [radius], [temp], [knn], context="sliding")
    for B in (1, 4, 8):
        for start in lm.STARTS:
            for emerging in (False, True):
                got, want = [], []
                for s in range(3):
                    emb, cls, K, ff, f0 = lm.bank_case(shape, s, B, start, emerging)
                    feats = hip.normalize(torch.from_numpy(emb).cuda())
                    memory = (feats[:B], torch.from_numpy(cls[:B]).to(torch.int8).cuda())
                    seed = torch.from_numpy(cls[B]).float().cuda() if emerging else None
                    pred = sweep.propagate_all(feats[B:].contiguous(), seed, M, memory=memory)
                    assert pred.shape == (1, N, T)
                    got.append(int((pred[0].cpu().numpy().T[f0 - B:] != cls[f0:]).sum()))
                    want.append(lm.bank_errors(shape, s, B, start, emerging)[0])
                print(f"B = {B}, start = {start}, {'emerging' if emerging else 'no seed'}: {got} (CPU fp64 {want})")
                assert got == want, (B, start, emerging)
