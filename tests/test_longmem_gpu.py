"""GPU side of the long-term memory bank: the two entry points of include/crw_hip_longmem.h through the C ABI, held to the definition
of tests/longmem_ref.py (whose checker tests/test_longmem.py proves on planted defects).
  * n_long = 1: bit for bit the entry points without a bank (crw_labelprop_topk_grid / _topk_scores / _propagate_sliding), on the
    vector route and on each of the three matrix-core instances, the route names asserted;
  * n_long in {2, 3, 6}: lists bit-equal to the existing top-k entry point on the gathered copy [key frames..., frame n] and inside
    the fp64 list audit's bounds on that copy; labels bit-equal to crw_labelprop_gather on the rows the rule translates to and
    inside `gather_audit`'s (knn + 2) * 2^-24; first frames inside and behind the bank; a ring that wraps twice;
  * the LDS edge of the ring, anchor marks, planted out-of-range indices, stale memory and guard bands;
  * the fixtures made from the reference's own `predict`, the [30, 13] rows of the README's tables, `propagate_all(memory=)`.
Nothing here provokes a fault: every index a kernel sees is clamped by the kernel, which is what the planted indices show."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import anchored_ref as ar
import longmem_ref as lm
import sliding_ref as slr
import stale_ref as sr
from oracle import crw_oracle as orc

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
EINVAL = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_long_memory() and crw_hip.has_sliding() and crw_hip.has_sweep() and crw_hip.has_routes()
    return crw_hip


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def eq_bits(a, b):
    return torch.equal(a.view(I32), b.view(I32))


def topk_long(lib, ehat, cxt, K, radius, temp, k, first, raw, route=0, out=None, want=0):
    T, N, C = ehat.shape
    WV, I = out or (torch.empty(T - first, k, N, device="cuda"), torch.empty(T - first, k, N, device="cuda", dtype=I32))
    st = lib.crw_labelprop_topk_long(_p(ehat), T, N, C, cxt, K, radius, temp, k, first, _p(WV), _p(I), raw, route, _stream())
    assert st == want, ("crw_labelprop_topk_long", st)
    return WV, I


def topk_plain(lib, ehat, cxt, radius, temp, k, first, raw):
    T, N, C = ehat.shape
    WV, I = torch.empty(T - first, k, N, device="cuda"), torch.empty(T - first, k, N, device="cuda", dtype=I32)
    fn = lib.crw_labelprop_topk_scores if raw else lib.crw_labelprop_topk_grid
    assert fn(_p(ehat), T, N, C, cxt, radius, temp, k, first, 1, _p(WV), _p(I), _stream()) == 0
    return WV, I


def prop_long(lib, W, I, T, N, M, first, cxt, K, L, pred, route=0, want=0):
    st = lib.crw_labelprop_propagate_long(_p(W), _p(I), T, N, M, W.shape[1], first, cxt, K, _p(L), _p(pred), route, _stream())
    assert st == want, ("crw_labelprop_propagate_long", st)
    return L, pred


def features(hip, T, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    return hip.normalize((torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).cuda())


def fresh(T, N, M, first, init, fill=0):
    """(L, pred) filled with `fill`, the frames before `first` from init = (L_init, pred_init)"""
    L, p = torch.empty(T * N, M, device="cuda"), torch.empty(N, T, device="cuda")
    for t in (L, p):
        t.view(torch.uint8).fill_(fill)
    L[:first * N], p[:, :first] = init[0][:first * N], init[1][:, :first]
    return L, p


def ring_fits(N, M, cxt, K, knn):
    """the header's condition of route 2"""
    return (cxt + 1 + K) * N * M * 4 + 16 * 1024 <= 150 * 1024 and knn <= 24 and N * M <= 384 and knn * N <= 1024


def other_gather(hip, N):
    """crw_labelprop_gather on absolute rows: `longmem_ref.violations`' gather_fn, another kernel than the one under test"""
    def run(seed, w, r, li, pi):
        assert seed is None
        w, r = torch.as_tensor(w).cuda().contiguous(), torch.as_tensor(r).cuda().to(I32).contiguous()
        li, pi = torch.as_tensor(li).cuda().contiguous(), torch.as_tensor(pi).cuda().contiguous()
        ff = pi.shape[1] - w.shape[0]
        return hip.labelprop_gather(None, w, r, pi.shape[1], N, li.shape[1], first_frame=ff, cxt_size=None, L=li.clone(), pred=pi.clone())
    return run


# ================================================================================================ n_long = 1: the entry points without a bank
# (F, N, C, cxt, radius, knn) and the route `topk_grid` takes: the vector kernel; the matrix cores in one piece (7 * 9 candidates); in
# two halves (81 * 19 = 1539 candidates: 16 * 1539 * 4 > 76 KiB, 41 * 19 <= 1024); the long-list form (41 * 59 = 2419 > 2048)
K1_CASES = [((14, 10, 8, 4, 3, 4), "labelprop.topk_valu"), ((20, 48, 64, 6, 5, 10), "labelprop.topk_mfma_chunks1"),
            ((90, 48, 64, 80, 10, 20), "labelprop.topk_mfma_chunks2"), ((50, 100, 64, 40, 30, 10), "labelprop.topk_mfma_long")]


@pytest.mark.parametrize("shape,route_name", K1_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_one_long_term_frame_is_the_entry_points_without_a_bank(hip, shape, route_name):
    F, N, C, cxt, radius, knn = shape
    lib, temp, M = hip.lib(), 0.1, 3
    feats = features(hip, F, N, C, sum(shape))
    forced = 1 if route_name.endswith("valu") else 2
    for first in (1, 3):
        for raw in (0, 1):
            with hip.routes() as hit:
                plain = topk_plain(lib, feats, cxt, radius, temp, knn, first, raw)
            assert set(hit) == {route_name}, hit
            for route in (0, forced):
                with hip.routes() as hit:
                    got = topk_long(lib, feats, cxt, 1, radius, temp, knn, first, raw, route)
                assert set(hit) == {route_name}, (route, hit)
                assert torch.equal(got[1], plain[1]) and eq_bits(got[0], plain[0]), (first, raw, route)
        if forced == 2:                                              # the vector kernel on the same call: another summation order
            with hip.routes() as hit:
                v = topk_long(lib, feats, cxt, 1, radius, temp, knn, first, 0, 1)
            assert set(hit) == {"labelprop.topk_valu"}, hit
            assert torch.allclose(v[0].sum(1), torch.ones(F - first, N, device="cuda"), atol=1e-5)
        else:
            topk_long(lib, feats, cxt, 1, radius, temp, knn, first, 0, 2, want=EINVAL)   # no matrix-core form of this shape
        W, I = topk_long(lib, feats, cxt, 1, radius, temp, knn, first, 0)
        init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, first))
        L0, p0 = fresh(F, N, M, first, init)
        with hip.routes() as hit:
            assert lib.crw_labelprop_propagate_sliding(None, _p(W), _p(I), F, N, M, knn, first, cxt, _p(L0), _p(p0), _stream()) == 0
        ring = ring_fits(N, M, cxt, 1, knn)
        assert set(hit) == {"labelprop.slide_ring" if ring else "labelprop.slide_general_lds"}, hit
        for route in (0, 1) + ((2,) if ring else ()):
            with hip.routes() as hit2:
                L, p = prop_long(lib, W, I, F, N, M, first, cxt, 1, *fresh(F, N, M, first, init, 0xFF), route)
            assert set(hit2) == {"labelprop.slide_general_lds" if route == 1 or not ring else "labelprop.slide_ring"}, (route, hit2)
            assert eq_bits(L, L0) and torch.equal(p, p0), (first, route)


# ================================================================================================ n_long > 1 against the definition
# (F, N, C, M, cxt, radius, knn): the vector route; a ring that wraps twice at K = 3 (R = 5, 27 frames); the matrix cores
LONG_SHAPES = [(14, 10, 8, 3, 4, 3, 4), (30, 13, 8, 3, 4, 3, 4), (20, 24, 64, 3, 4, 4, 5)]


@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("K", (2, 3, 6))
def test_a_bank_of_long_term_frames_is_the_definition(hip, shape, K):
    F, N, C, M, cxt, radius, knn = shape
    lib, temp = hip.lib(), 0.1
    feats = features(hip, F, N, C, sum(shape) + K)
    matrix = C == 64
    # ---- the definition's lists, once: the existing entry point on the gathered copy of every frame (first_frame = nf, cxt >= nf)
    Wd, Id, Vd = (torch.zeros(F - 1, knn, N, device="cuda", dtype=d) for d in (F32, I32, F32))
    worst = {}
    for n in range(1, F):
        keys = lm.key_frames(n, K, cxt)
        sub = feats[keys + [n]].contiguous()
        with hip.routes() as hit:
            (w, i), (v, iv) = (topk_plain(lib, sub, len(keys), radius, temp, knn, len(keys), raw) for raw in (0, 1))
        assert set(hit) == {"labelprop.topk_mfma_chunks1" if matrix else "labelprop.topk_valu"}, hit
        assert torch.equal(i, iv)
        Wd[n - 1], Id[n - 1], Vd[n - 1] = w[0], i[0], v[0]
        res = orc.topk_lists_audit(sub, len(keys), radius, temp, knn, len(keys), 1, w, i, v)   # (C + 2) * 2^-24 / temp, twice for selection / weights
        assert not any(res["violations"].values()) and all(x <= 1 for x in res["worst"].values()), (n, res)
        worst = {k: max(worst.get(k, 0), x) for k, x in res["worst"].items()}
    print(f"{shape} K = {K}: list audit, worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    gather_fn = other_gather(hip, N)
    for first in sorted({1, K - 1, K, K + 2, F - 1}):
        with hip.routes() as hit:
            W, I = topk_long(lib, feats, cxt, K, radius, temp, knn, first, 0)
            V, Iv = topk_long(lib, feats, cxt, K, radius, temp, knn, first, 1)
        assert set(hit) == {"labelprop.topk_mfma_chunks1" if matrix else "labelprop.topk_valu"}, hit
        assert torch.equal(I, Id[first - 1:]) and torch.equal(Iv, I) and eq_bits(W, Wd[first - 1:]) and eq_bits(V, Vd[first - 1:]), first
        if matrix:                                                   # forced onto the route it takes anyway: the same bits
            Wm, Im = topk_long(lib, feats, cxt, K, radius, temp, knn, first, 0, 2)
            assert torch.equal(Im, I) and eq_bits(Wm, W), first
        init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 11 * first + K))
        ring = ring_fits(N, M, cxt, K, knn)
        assert ring
        lists_fn = lambda e, n: (Wd[n - 1], Id[n - 1])
        outs = []
        for route, name in ((0, "labelprop.slide_ring"), (1, "labelprop.slide_general_lds"), (2, "labelprop.slide_ring")):
            with hip.routes() as hit:
                L, p = prop_long(lib, W, I, F, N, M, first, cxt, K, *fresh(F, N, M, first, init, 0xFF if route else 0), route)
            assert set(hit) == {name}, (route, hit)
            v = lm.violations(feats, W, I, L, p, M, cxt, K, radius, temp, knn, first, *fresh(F, N, M, first, init), lists_fn=lists_fn,
                              gather_fn=gather_fn)
            assert not any(v.values()), (first, route, v)
            outs.append((L, p))
        assert all(eq_bits(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs), first


def test_the_lds_edge_of_the_ring(hip):
    """N 96, M 4, cxt 80, knn 10, F 12: K = 8 takes the ring (89 frames of 1536 B + 16 KiB <= 150 KiB), K = 9 the general route"""
    F, N, C, M, cxt, radius, knn = 12, 96, 16, 4, 80, 5, 10
    lib = hip.lib()
    feats = features(hip, F, N, C, 5)
    assert ring_fits(N, M, cxt, 8, knn) and not ring_fits(N, M, cxt, 9, knn)
    for K, name in ((8, "labelprop.slide_ring"), (9, "labelprop.slide_general_lds")):
        W, I = topk_long(lib, feats, cxt, K, radius, 0.1, knn, K, 0)
        init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, K))
        with hip.routes() as hit:
            L, p = prop_long(lib, W, I, F, N, M, K, cxt, K, *fresh(F, N, M, K, init), 0)
        assert set(hit) == {name}, hit
        L1, p1 = prop_long(lib, W, I, F, N, M, K, cxt, K, *fresh(F, N, M, K, init, 0xFF), 1)
        assert eq_bits(L, L1) and torch.equal(p, p1), K
        if K == 8:
            L2, p2 = prop_long(lib, W, I, F, N, M, K, cxt, K, *fresh(F, N, M, K, init, 0xFF), 2)
            assert eq_bits(L, L2) and torch.equal(p, p2)
        else:
            prop_long(lib, W, I, F, N, M, K, cxt, K, *fresh(F, N, M, K, init), 2, want=EINVAL)
        v = lm.violations(feats, W, I, L, p, M, cxt, K, radius, 0.1, knn, K, *fresh(F, N, M, K, init), lists_fn=lambda e, n: (W[n - K], I[n - K]),
                          gather_fn=other_gather(hip, N))
        assert not any(v.values()), (K, v)


def test_argument_checks(hip):
    lib = hip.lib()
    F, N, C, M, cxt, knn = 8, 10, 8, 3, 3, 4
    feats = features(hip, F, N, C, 1)
    W, I = topk_long(lib, feats, cxt, 2, 3, 0.1, knn, 2, 0)
    L, p = torch.zeros(F * N, M, device="cuda"), torch.zeros(N, F, device="cuda")
    for K, first in ((0, 1), (F, 1), (2, 0), (2, F)):
        topk_long(lib, feats, cxt, K, 3, 0.1, knn, first, 0, out=(W, I), want=EINVAL)
        prop_long(lib, W, I, F, N, M, first, cxt, K, L, p, want=EINVAL)
    topk_long(lib, feats, cxt, 2, 3, 0.1, knn, 2, 0, 3, out=(W, I), want=EINVAL)
    prop_long(lib, W, I, F, N, M, 2, cxt, 2, L, p, 3, want=EINVAL)
    assert not L.any() and not p.any()


# ================================================================================================ anchor marks
@pytest.mark.parametrize("pattern", ("two consecutive frames", "partial rows: a third of the nodes at three frames"))
def test_anchor_marks_under_a_bank_of_three(hip, pattern):
    F, N, C, M, cxt, radius, knn = ar.SHAPES[0]
    K, first, lib = 3, 3, hip.lib()
    feats = features(hip, F, N, C, 17)
    anchor_np, _ = ar.patterns(F, N, M, cxt)[pattern]
    assert ar.clamped(anchor_np[first:], M).any()
    W, I = topk_long(lib, feats, cxt, K, radius, ar.TEMP, knn, first, 0)
    I[0, 1, ::2] = 10 ** 6                                           # (planted: out of range, the clamp of the rule)
    I[2, 0, 1::2] = -5
    Wm, Im = hip.mark_anchors(W.clone(), I.clone(), torch.from_numpy(anchor_np), M, first)
    R = lm.rows(I.cpu().numpy(), N, cxt, K, first)
    init = tuple(torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 3))
    as_np = lambda x: x.cpu().numpy()

    def other_kernel(s, w, r, m, ff, li, pi):                        # `anchored_ref.segmented`'s gather: crw_labelprop_gather on absolute rows
        return tuple(as_np(x) for x in other_gather(hip, N)(s, w, r, li, pi))

    ref = ar.segmented(None, as_np(W), R, M, anchor_np, first, *(as_np(x) for x in fresh(F, N, M, first, init)), gather=other_kernel)
    for route in (0, 1, 2):
        got = prop_long(lib, Wm, Im, F, N, M, first, cxt, K, *fresh(F, N, M, first, init, 0xFF if route else 0), route)
        v = ar.violations(None, W, torch.from_numpy(R).cuda(), M, anchor_np, first, *got, *fresh(F, N, M, first, init), ref=ref)
        assert not any(v.values()), (route, v)
    via = hip.labelprop_gather(None, W, I, F, N, M, first, *fresh(F, N, M, first, init), cxt_size=cxt, context="sliding",
                               anchors=torch.from_numpy(anchor_np), n_long=K)
    assert eq_bits(via[0], got[0]) and torch.equal(via[1], got[1])


# ================================================================================================ stale memory and guard bands
def _out(*shape, dtype=F32):
    like = torch.empty(shape, dtype=dtype, device="meta")
    return sr.Buf(like.numel() * like.element_size(), dtype if dtype.is_floating_point else None, step=sr.largest_step(like))


def _as(t, name, dtype, *shape):
    like = torch.empty(shape, dtype=dtype, device="meta")
    return t[name][:like.numel() * like.element_size()].view(dtype).view(shape)


def banded_case(hip, home, shape, K, route):
    """both entry points on one shape, first_frame = K: lists (weights and logits), then the propagation of lists that hold planted
    out-of-range indices -- a huge one, a negative one, one just past the frame's list -- and an anchored frame"""
    F, N, C, M, cxt, radius, knn = shape
    lib, n = hip.lib(), F - K
    feats = features(hip, F, N, C, 23)
    W, I = topk_long(lib, feats, cxt, K, radius, 0.1, knn, K, 0)
    I[0, 0, 0], I[1, knn - 1, N - 1], I[n - 1, 0, N // 2] = 2 ** 30, -7, min(F - 1, K + cxt) * N
    anchor = np.full((F, N), -1, np.int8)
    anchor[K + 1] = np.arange(N) % M
    W, I = hip.mark_anchors(W, I, torch.from_numpy(anchor), M, K)
    L_init, p_init = (torch.from_numpy(x).cuda() for x in ar.soft_init(F, N, M, 9))
    ehat, W, I, L_front, p_front = home.many(ehat=feats, W=W, I=I, L_front=L_init[:K * N].contiguous(), p_front=p_init[:, :K].contiguous())
    bufs = dict(Wo=_out(n, knn, N), Io=_out(n, knn, N, dtype=I32), Vo=sr.Buf(n * knn * N * 4, None, step=knn * N * 4),
                Ivo=_out(n, knn, N, dtype=I32), L=_out(F * N, M), pred=_out(N, F))

    def run(_, t):
        for raw, (w, i) in enumerate((("Wo", "Io"), ("Vo", "Ivo"))):
            topk_long(lib, ehat, cxt, K, radius, 0.1, knn, K, raw, 0, out=(t[w], t[i]))
        L, pred = _as(t, "L", F32, F * N, M), _as(t, "pred", F32, N, F)
        L[:K * N], pred[:, :K] = L_front, p_front                    # the caller's frames: written here, read by the entry point
        pred[:, K:] = 0                                               # (bytes the fill left: the entry point writes every one of them)
        prop_long(lib, W, I, F, N, M, K, cxt, K, L, pred, route)
        torch.cuda.synchronize()

    case = sr.Case(f"crw_labelprop_topk_long / crw_labelprop_propagate_long (route {route})", None, bufs, run, device="cuda", home=home)

    def check(t):
        L = _as(t, "L", F32, F, N, M)
        assert torch.allclose(L.sum(-1), torch.ones(F, N, device="cuda"), atol=1e-4)
        assert torch.allclose(_as(t, "Wo", F32, n, knn, N).sum(1), torch.ones(n, N, device="cuda"), atol=1e-5)
        assert torch.equal(_as(t, "Io", I32, n, knn, N), _as(t, "Ivo", I32, n, knn, N))
        assert torch.equal(_as(t, "pred", F32, N, F)[:, K + 1].cpu(), torch.from_numpy(anchor[K + 1]).float())
        return L
    return case, check


@pytest.mark.parametrize("shape,K,route", [(LONG_SHAPES[0], 3, 2), (LONG_SHAPES[0], 3, 1), (LONG_SHAPES[1], 6, 2), (LONG_SHAPES[2], 2, 0)],
                         ids=str)
def test_entry_points_over_stale_memory_and_between_guard_bands(hip, shape, K, route):
    case, check = banded_case(hip, sr.Home("cuda"), shape, K, route)
    assert case.home.operands
    a = check(sr.run_banded(case))
    b = check(sr.run_twice(case))
    assert eq_bits(a, b)


# ================================================================================================ fixtures, tables, the host path
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "longmem_*.npz"))), ids=os.path.basename)
def test_fixtures_from_the_reference(hip, path):
    """The reference's own `predict` on the rule's lists: labels exact; L within the fixture's recorded deviation from fp64 plus the
    project's bound (as tests/test_sliding_gpu.py holds its fixtures)."""
    g = np.load(path)
    emb, cxt, K, radius, temp, knn, first, M = g["emb"], *(int(g[k]) for k in ("cxt", "K", "radius")), float(g["temp"]), *(
        int(g[k]) for k in ("knn", "first_frame", "M"))
    F, N, _ = emb.shape
    feats = hip.normalize(torch.from_numpy(emb).cuda())
    init = tuple(torch.from_numpy(x).cuda() for x in lm.initial_labels(g["cls_front"], first, N, M, F))
    W, I = hip.labelprop_topk(feats, cxt, radius, temp, knn, first, n_long=K, route="auto")
    for route in ("general", "ring"):
        L, pred = hip.labelprop_gather(None, W, I, F, N, M, first, *fresh(F, N, M, first, init), cxt_size=cxt, context="sliding", n_long=K,
                                       route=route)
        dev = float(np.abs(L.cpu().numpy()[first * N:] - g["L"][first * N:]).max())
        print(f"{os.path.basename(path)} ({route}): max |L - reference| = {dev:.3g}, recorded deviation {float(g['deviation']):.3g}")
        assert np.array_equal(pred.cpu().numpy()[:, first:], g["pred"][:, first:])
        assert dev <= float(g["deviation"]) + orc.gather_bound(knn)


def test_the_tables_rows_of_the_smallest_shape(hip):
    """the [30, 13] rows of the README's bank tables through `LabelPropVOS_CRW.propagate_all(memory=)`: the CPU counts"""
    from imported.labelprop import LabelPropVOS_CRW
    from test_longmem import TABLE_30_13
    shape = slr.DRIFT_SHAPES[0]
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=cxt, RADIUS=radius, TEMP=temp, KNN=knn, CONTEXT="sliding"))
    for (B, start, emerging), want in TABLE_30_13.items():
        got = []
        for s in range(3):
            emb, cls, K, ff, f0 = lm.bank_case(shape, s, B, start, emerging)
            feats = hip.normalize(torch.from_numpy(emb).cuda())
            memory = (feats[:B], torch.from_numpy(cls[:B]).to(torch.int8).cuda())
            seed = torch.from_numpy(cls[B]).float().cuda() if emerging else None
            pred, L = lp.propagate_all(feats[B:].contiguous(), seed, M, memory=memory)
            assert pred.shape == (N, T) and L.shape == (T * N, M)
            got.append(int((pred.cpu().numpy().T[f0 - B:] != cls[f0:]).sum()))
        print(f"B = {B}, start = {start}, {'emerging' if emerging else 'no seed'}: {got} (CPU fp64 {list(want)})")
        assert tuple(got) == tuple(want), (B, start, emerging)


def test_segment_with_a_bank_and_no_seed_on_the_device(hip):
    """The 96 x 320 case of tests/test_anchored_gpu.py (two radargrams of T = 10, the CNN, reverse pass, 'maxprob',
    merge='confidence') with a bank of four traces of the first radargram and no seed: the maps are `propagate`'s, item by item;
    the bank changes the labels; without the arguments `segment` is bit for bit what it is."""
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case
    enc, fresh_ds, seg, _, N = e2e_case(0, n_rg=2, H=100)
    T, step = T_E2E, PATCH[1] - OVERLAP[1]
    rg_len = T * step + OVERLAP[1]
    assert (seg.shape[0], 2 * rg_len) == (96, 320)
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=6, RADIUS=6, TEMP=0.1, KNN=8, CONTEXT="sliding"))
    kw = dict(use_last=True, dataset_id=2, confidence="maxprob", merge="confidence")
    run = lambda **k: crw_inference.segment(fresh_ds(), seg, enc, lp, M_E2E, T, PATCH, OVERLAP, **kw, **k)
    cols = [0, 3 * step, 6 * step + 5, 9 * step]
    bank = crw_utils.bank_from_columns(fresh_ds(), seg, cols)
    assert len(bank) == 4 and bank.nodes == N
    with hip.routes() as hit:
        out = run(memory=(seg, cols), seedless=True)
    assert out["memory_traces"] == 4 and out["seedless"] is True
    assert {"labelprop.slide_ring", "labelprop.topk_valu"} <= set(hit) or {"labelprop.slide_ring", "labelprop.topk_mfma_chunks1"} <= set(hit), hit
    ds = fresh_ds()
    for t in range(2):                                                   # the forward map, item by item, from `propagate` itself
        seq = ds[t * T].cuda()
        pred, _, _, conf = crw_utils.propagate(seq, None, enc, lp, M_E2E, False, False, confidence="maxprob", memory=bank)
        assert pred.shape == (N, T) and conf.shape == (N, T)
        want = crw_inference._upsample(pred, seg.shape[0], rg_len)
        assert torch.equal(out["forward"][:, t * rg_len:(t + 1) * rg_len], want), t
        assert bool((conf[:, 0] < 1).any())                              # frame 0 is predicted: its confidence is a frame's, not a seed's
    seeded, plain = run(memory=bank), run()
    assert seeded["seedless"] is False and not torch.equal(seeded["pred"], plain["pred"]) and not torch.equal(out["pred"], seeded["pred"])
    for k in ("pred", "forward", "conf", "forward_conf"):                # without the arguments: what it is (two runs, the same bits)
        again = run()[k]
        assert torch.equal(again.view(I32) if again.dtype == F32 else again, plain[k].view(I32) if plain[k].dtype == F32 else plain[k]), k
    assert "memory_traces" not in plain and "seedless" not in plain
