"""Which kernel ran: one or two calls at the smallest shape on either side of every selector's threshold, inside `crw_hip.routes()`
(include/crw_hip_routes.h), asserting the EXACT set of routes the calls took -- a threshold that moves in a `launch_*` selector
fails here instead of silently leaving a route untested.  The expected sets are read off the selectors, never
off a run.  Every case also holds its results to fp64 with the check and the tolerance the suite already has for that kernel: the
bodies of the parity tests are called at these shapes, or the same audits (`oracle.gather_audit`, `oracle.topk_lists_audit`, the
walk's per-slice bars of tests/walk_ref.py) are applied.  No tolerance is new.  The last test holds the whole file to the default
environment: no route that only a variant switch reaches was taken."""
import pytest
import torch

import restart_ref as rre
import routes_ref as rr
import test_conv_chain_gpu as tcc
import test_hip_parity as tp
import test_resnet_hip as trn
import test_walk_routes_gpu as twr
from oracle import crw_oracle as orc
from test_labelprop_lists import lp_embeddings, scrambled_seed

pytestmark = pytest.mark.gpu

SEEN = set()   # every route any call of this file took (the default-route check at the end)


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_routes()
    return crw_hip


def took(hip, fn, *args, **kw):
    """fn(*args) inside crw_hip.routes() -> (its result, the set of routes it took)"""
    with hip.routes() as hit:
        out = fn(*args, **kw)
        torch.cuda.synchronize()
    assert all(v > 0 for v in hit.values()) and set(hit) <= set(rr.ROUTES), hit
    SEEN.update(hit)
    return out, set(hit)


# ------------------------------------------------------------------------------------------------ affinity
def _affinity(hip, B, T, N, C, tau):
    """crw_affinity_fwd and crw_affinity_bwd against fp64 at the tolerances of test_hip_parity.test_affinity_tiles_and_fused_statistics
    -> (routes of the forward, routes of the backward)"""
    g = torch.Generator().manual_seed(N + C)
    emb = (torch.randn(1, 1, N, C, generator=g) + 0.6 * torch.randn(B, T, N, C, generator=g)).float()
    (A, ehat, norm, stats), fwd = took(hip, hip.affinity_fwd, emb.cuda(), tau)
    eh = emb.double() / emb.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    A_ref = torch.einsum("btnc,btmc->btnm", eh[:, :-1], eh[:, 1:]) / tau
    torch.testing.assert_close(A.cpu().double(), A_ref, rtol=1e-5, atol=2e-5 / tau * 1e-1)
    Ad = A.double()
    rmax, cmax = Ad.max(-1).values, Ad.max(-2).values
    rsum, csum = (Ad - rmax[..., None]).exp().sum(-1), (Ad - cmax[..., None, :]).exp().sum(-2)
    for got, want in zip(stats, (rmax, rsum, cmax, csum)):
        torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)
    dA = torch.randn(B, T - 1, N, N, generator=g).float()
    demb, bwd = took(hip, hip.affinity_bwd, dA.cuda(), ehat, norm, tau)
    deh = torch.zeros_like(eh)
    deh[:, :-1] += torch.einsum("btnm,btmc->btnc", dA.double(), eh[:, 1:]) / tau
    deh[:, 1:] += torch.einsum("btnm,btnc->btmc", dA.double(), eh[:, :-1]) / tau
    nrm = emb.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    want = (deh - eh * (eh * deh).sum(-1, keepdim=True)) / nrm
    torch.testing.assert_close(demb.cpu().double(), want, rtol=1e-4, atol=1e-4 * want.abs().max().item())
    return fwd, bwd


# N, C -> forward route, backward route.  The thresholds: N <= 64 one 64-row tile; N >= 256 and C % 32 == 0 bf16 splits in the
# forward, N >= 256 and C == 128 in the backward; N % 4 != 0 element loads of dA in the backward; C outside {32, 64, 128} the
# bounds-checked fallback in the backward, C % 4 != 0 in the forward (then a statistics pass of its own: vector at N % 4 == 0)
AFFINITY = [
    (64, 32, {"affinity.fwd_f32_t64"}, {"affinity.bwd_f32_t64"}),
    (62, 32, {"affinity.fwd_f32_t64"}, {"affinity.bwd_f32_t64_elem"}),
    (68, 32, {"affinity.fwd_f32_t128"}, {"affinity.bwd_f32_t128"}),
    (252, 32, {"affinity.fwd_f32_t128"}, {"affinity.bwd_f32_t128"}),
    (256, 32, {"affinity.fwd_bf16x6"}, {"affinity.bwd_f32_t128"}),
    (252, 128, {"affinity.fwd_f32_t128"}, {"affinity.bwd_f32_t128"}),
    (256, 128, {"affinity.fwd_bf16x6"}, {"affinity.bwd_bf16x6"}),
    (254, 32, {"affinity.fwd_f32_t128"}, {"affinity.bwd_f32_t128_elem"}),
    (258, 128, {"affinity.fwd_bf16x6"}, {"affinity.bwd_f32_t128_elem"}),
    (256, 20, {"affinity.fwd_f32_t128"}, {"gemm_f32.edge"}),
    (8, 6, {"gemm_f32.edge", "softmax.stats_dense_vec"}, {"gemm_f32.edge"}),
    (7, 6, {"gemm_f32.edge", "softmax.stats_dense_scalar"}, {"gemm_f32.edge"}),
]


@pytest.mark.parametrize("N,C,fwd,bwd", AFFINITY, ids=[f"N{a[0]}-C{a[1]}" for a in AFFINITY])
def test_affinity_routes(hip, monkeypatch, N, C, fwd, bwd):
    monkeypatch.delenv("CRW_AFFINITY_F32", raising=False)
    got = _affinity(hip, 1, 3, N, C, 0.07)
    assert got == (fwd, bwd), got


def test_affinity_f32_switch_per_call(hip, monkeypatch):
    """CRW_AFFINITY_F32=1 is read on every call: the shape that takes the bf16 splits in both directions, on the fp32 MFMA"""
    monkeypatch.delenv("CRW_AFFINITY_F32", raising=False)
    with hip.routes() as hit:                                       # (the context manager itself: nothing launched, nothing held)
        pass
    assert not hit
    assert _affinity(hip, 1, 3, 256, 128, 0.07) == ({"affinity.fwd_bf16x6"}, {"affinity.bwd_bf16x6"})
    monkeypatch.setenv("CRW_AFFINITY_F32", "1")
    assert _affinity(hip, 1, 3, 256, 128, 0.07) == ({"affinity.fwd_f32_t128"}, {"affinity.bwd_f32_t128"})
    monkeypatch.setenv("CRW_AFFINITY_F32", "0")
    assert _affinity(hip, 1, 3, 256, 128, 0.07) == ({"affinity.fwd_bf16x6"}, {"affinity.bwd_bf16x6"})


# ------------------------------------------------------------------------------------------------ walk
# (B, T, N) are rows of walk_ref.ROUTE_TABLE: the references are the ones tests/test_walk_routes_gpu.py computes (shared, cached)
WALK = [
    # padded N = 32 / 64: the persistent chain; the batched products behind it on 32-wide tiles (a grid of 2 .. 4 tiles)
    ((1, 5, 32), 0, {"walk.fwd_persistent", "walk.bwd_persistent", "chain_small.n32", "gemm_f32.t32", "softmax.fwd_vec", "softmax.bwd_vec"}),
    ((1, 4, 64), 0, {"walk.fwd_persistent", "walk.bwd_persistent", "chain_small.n64", "gemm_f32.t32", "softmax.fwd_vec", "softmax.bwd_vec"}),
    # N = 65 pads to 96: grouped GEMMs; 65 % 4 != 0: the scalar softmax kernels
    ((2, 5, 65), 0, {"walk.fwd_gemm", "walk.bwd_gemm", "gemm_f32.t32", "softmax.fwd_scalar", "softmax.bwd_scalar"}),
    # the bf16 chains pad to 128: never the persistent kernel, 128-tiles
    ((2, 7, 33), 1, {"walk.fwd_gemm", "walk.bwd_gemm", "gemm_bf16.t128", "softmax.fwd_scalar", "softmax.bwd_scalar"}),
    ((1, 4, 128), 2, {"walk.fwd_gemm", "walk.bwd_gemm", "gemm_bf16.t128", "softmax.fwd_vec", "softmax.bwd_vec"}),
]


@pytest.mark.parametrize("shape,chain,want", WALK, ids=[f"{a[0]}-chain{a[1]}" for a in WALK])
def test_walk_routes(hip, shape, chain, want):
    B, T, N = shape
    ref = twr._reference(hip, "randn3", B, T, N)
    (loss, At, dA), hit = took(hip, twr._walk, hip, ref["A"], chain, None)
    assert hit == want, hit
    twr._check_forward(chain, loss, At, ref)
    twr._check_dA(f"routes {shape} chain {chain}", chain, "randn3", dA, ref)
    (loss, At, dA), hit = took(hip, twr._walk, hip, ref["A"], chain, ref["stats"])
    assert hit == want | {"softmax.stats_import"}, hit
    twr._check_forward(chain, loss, At, ref)


# the tile rules of the chain GEMMs on both sides, through crw_gemm_f32 / crw_gemm_bf16 (bodies: test_hip_parity's GEMM tests)
#   fp32: the largest of 128 / 64 / 32 that divides n and gives (n / tile)^2 * batch >= 512 blocks, else 32
#   bf16: 256-tiles when n % 256 == 0 and (n / 256)^2 * batch >= 256, else 128-tiles; the default 256-tile schedule is the staggered one
GEMM_F32 = [(128, 512, "gemm_f32.t128"), (128, 511, "gemm_f32.t64"), (64, 512, "gemm_f32.t64"), (64, 511, "gemm_f32.t32"),
            (96, 600, "gemm_f32.t32")]
GEMM_BF16 = [(256, 256, "gemm_bf16.t256_stagger"), (256, 255, "gemm_bf16.t128"), (384, 300, "gemm_bf16.t128")]


@pytest.mark.parametrize("n,batch,want", GEMM_F32, ids=[f"n{a[0]}-b{a[1]}" for a in GEMM_F32])
def test_gemm_f32_tile_rule(hip, n, batch, want):
    _, hit = took(hip, tp.test_gemm_f32_matches_torch, hip, n, batch, 0, 1)
    assert hit == {want}, hit


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("n,batch,want", GEMM_BF16, ids=[f"n{a[0]}-b{a[1]}" for a in GEMM_BF16])
def test_gemm_bf16_tile_rule(hip, n, batch, want, split):
    _, hit = took(hip, tp.test_gemm_bf16_matches_torch, hip, n, batch, 1, 0, split)
    assert hit == {want}, hit


# ------------------------------------------------------------------------------------------------ label propagation
LP_T, LP_N, LP_M, LP_C, LP_KNN, LP_RADIUS = 91, 96, 4, 64, 4, 3   # N * M = 384: six compute waves, the most chain_fits admits


def _lp_item(hip, cxt, origin=None):
    feats = hip.normalize(lp_embeddings(LP_T, LP_N, LP_C, LP_T + cxt).cuda())
    seed = scrambled_seed(LP_N, LP_M).cuda()
    (W, I), hit = took(hip, hip.labelprop_topk, feats, cxt, LP_RADIUS, 0.1, LP_KNN, first_frame=1, origin=origin)
    assert hit == {"labelprop.topk_mfma_chunks1"}, hit            # a column of 96 >= 16 nodes, C = 64, (cxt + 1) * 5 <= 450 candidates: 28 KiB
    return feats, seed, W, I


def _audit(what, W, R, seed, cxt, L, pred):
    res = orc.gather_audit(W, R, seed, LP_M, 1, cxt, L, pred)
    print(f"{what}: worst error / bound soft {res['worst']['soft']:.3g} (bound {res['bound']:.3g})")
    assert not any(res["violations"].values()), (what, res["violations"])


def test_propagate_prefix_against_gather_at_the_lds_limit(hip, monkeypatch):
    """crw_labelprop_propagate chains frames 1 .. cxt with cxt + 1 label frames in LDS: chain_fits asks (cxt + 1) * 384 * 4 + 16 KiB
    <= 150 KiB, i.e. cxt + 1 <= 89.  cxt = 88 fits; cxt = 89 goes to the one-workgroup walk (its LDS ring holds 95 frames)."""
    for name in ("CRW_LABELPROP_GATHER_SEQ", "CRW_LABELPROP_GATHER_GLOBAL"):
        monkeypatch.delenv(name, raising=False)
    for cxt, want in ((88, {"labelprop.propagate_prefix"}), (89, {"labelprop.gather_lds"})):
        feats, seed, W, I = _lp_item(hip, cxt)
        (L, pred), hit = took(hip, hip.labelprop_gather, seed, W, I, LP_T, LP_N, LP_M, cxt_size=cxt)
        assert hit == want, (cxt, hit)
        _audit(f"propagate cxt {cxt}", W, I, seed, cxt, L, pred)
    (Lb, pb), hit = took(hip, hip.labelprop_propagate_batch, seed, torch.stack([W, W]), I, LP_T, LP_N, LP_M, cxt_size=89)
    assert hit == {"labelprop.batch_reference"}, hit
    _audit("batch", W, I, seed, 89, Lb[1], pb[1])


def _origin(T, at):
    o = torch.zeros(T, dtype=torch.int32)
    o[at + 1:] = at                                               # the item restarts at frame `at`: origin[n] in {origin[n - 1], n - 1}
    return o


def test_sliding_ring_against_general_at_the_lds_limit(hip, monkeypatch):
    """crw_labelprop_propagate_sliding keeps frame 0 + R = min(cxt + 1, T - 1) ring frames: R + 1 <= 89 -> cxt = 87 rides the ring,
    cxt = 88 the general kernel; with origins two more frames and origin[T] (one frame's room here): R + 3 <= 89 -> cxt = 85
    against 86.  CRW_LABELPROP_SLIDING_GENERAL=1 (read per call) sends the fitting shapes to the general kernel too.  Each result
    against the fp64 audit on the translated rows; the batch entry points have one kernel each."""
    for name in ("CRW_LABELPROP_SLIDING_GENERAL", "CRW_LABELPROP_GATHER_GLOBAL", "CRW_ANCHORS_RESTART_SEGMENTED"):
        monkeypatch.delenv(name, raising=False)
    T, N, M = LP_T, LP_N, LP_M
    for cxt, want in ((87, "labelprop.slide_ring"), (88, "labelprop.slide_general_lds")):
        feats, seed, W, I = _lp_item(hip, cxt)
        R = hip.sliding_rows(I, N, cxt, 1)
        (L, pred), hit = took(hip, hip.labelprop_gather, seed, W, I, T, N, M, cxt_size=cxt, context="sliding")
        assert hit == {want}, (cxt, hit)
        _audit(f"sliding cxt {cxt}", W, R, seed, None, L, pred)
        if cxt == 87:
            monkeypatch.setenv("CRW_LABELPROP_SLIDING_GENERAL", "1")
            (Lg, pg), hit = took(hip, hip.labelprop_gather, seed, W, I, T, N, M, cxt_size=cxt, context="sliding")
            monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL")
            assert hit == {"labelprop.slide_general_lds"}, hit
            assert torch.equal(Lg.view(torch.int32), L.view(torch.int32)) and torch.equal(pg, pred)
            (Lb, pb), hit = took(hip, hip.labelprop_propagate_batch, seed, torch.stack([W, W]), I, T, N, M, cxt_size=cxt, context="sliding")
            assert hit == {"labelprop.batch_slide"}, hit
            assert torch.equal(Lb[1].view(torch.int32), L.view(torch.int32)) and torch.equal(pb[1], pred)
    origin = _origin(T, 40)
    for cxt, want in ((85, "labelprop.slide_ring_origin"), (86, "labelprop.slide_general_origin_lds")):
        feats, seed, W, I = _lp_item(hip, cxt, origin=origin)
        R = torch.as_tensor(rre.rows_of(I.cpu().numpy(), origin, N, cxt)).int().cuda()
        (L, pred), hit = took(hip, hip.labelprop_gather, seed, W, I, T, N, M, cxt_size=cxt, context="sliding", origin=origin)
        assert hit == {want}, (cxt, hit)
        _audit(f"sliding with origins cxt {cxt}", W, R, seed, None, L, pred)
        if cxt == 85:
            monkeypatch.setenv("CRW_LABELPROP_SLIDING_GENERAL", "1")
            (Lg, pg), hit = took(hip, hip.labelprop_gather, seed, W, I, T, N, M, cxt_size=cxt, context="sliding", origin=origin)
            monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL")
            assert hit == {"labelprop.slide_general_origin_lds"}, hit
            assert torch.equal(Lg.view(torch.int32), L.view(torch.int32)) and torch.equal(pg, pred)
            (Lb, pb), hit = took(hip, hip.labelprop_propagate_batch, seed, torch.stack([W, W]), I, T, N, M, cxt_size=cxt, context="sliding",
                                 origin=origin)
            assert hit == {"labelprop.batch_slide_origin"}, hit
            assert torch.equal(Lb[1].view(torch.int32), L.view(torch.int32)) and torch.equal(pb[1], pred)


def test_restart_segmented_switch_per_call(hip, monkeypatch):
    """CRW_ANCHORS_RESTART_SEGMENTED=1 (read per call by the binding): the origin call as one crw_labelprop_propagate_sliding call per
    stretch between origins -- the ring kernel without origins, twice, and the same bits"""
    monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
    T, N, M, cxt = 20, 16, 4, 5
    origin = _origin(T, 9)
    feats = hip.normalize(lp_embeddings(T, N, 16, 5).cuda())
    seed = scrambled_seed(N, M).cuda()
    monkeypatch.delenv("CRW_ANCHORS_RESTART_SEGMENTED", raising=False)
    W, I = hip.labelprop_topk(feats, cxt, 4, 0.1, 4, origin=origin)
    with hip.routes() as one:
        L1, p1 = hip.labelprop_gather(seed, W, I, T, N, M, cxt_size=cxt, context="sliding", origin=origin)
    monkeypatch.setenv("CRW_ANCHORS_RESTART_SEGMENTED", "1")
    with hip.routes() as seg:
        L2, p2 = hip.labelprop_gather(seed, W, I, T, N, M, cxt_size=cxt, context="sliding", origin=origin)
    SEEN.update(one, seg)
    assert dict(one) == {"labelprop.slide_ring_origin": 1}, one
    assert dict(seg) == {"labelprop.slide_ring": 2}, seg
    assert torch.equal(L1.view(torch.int32), L2.view(torch.int32)) and torch.equal(p1, p2)
    R = torch.as_tensor(rre.rows_of(I.cpu().numpy(), origin, N, cxt)).int().cuda()
    res = orc.gather_audit(W, R, seed, M, 1, None, L1, p1)
    assert not any(res["violations"].values()), res["violations"]


# (T, N, C, cxt, radius, knn, first, grid_w) -> route: the choice is by shape (csrc/labelprop.hip topk_grid)
TOPK = [
    ((8, 15, 64, 3, 3, 4, 1, 1), "labelprop.topk_valu"),            # 15 < 16 nodes: no full query tile
    ((8, 16, 64, 3, 3, 4, 1, 1), "labelprop.topk_mfma_chunks1"),    # 16 nodes: matrix cores
    ((8, 16, 32, 3, 3, 4, 1, 1), "labelprop.topk_valu"),            # 32 channels: not a matrix-core width
    ((8, 16, 64, 3, 3, 4, 1, 2), "labelprop.topk_valu"),            # an 8 x 2 grid: not a column
    # 64 * maxcand bytes against 76 KiB = 77 824: maxcand = 81 * 15 = 1215 -> 77 760 one piece; 82 * 15 = 1230 -> 78 720 two halves
    ((90, 16, 64, 80, 8, 6, 1, 1), "labelprop.topk_mfma_chunks1"),
    ((90, 16, 64, 81, 8, 6, 1, 1), "labelprop.topk_mfma_chunks2"),
    # maxcand <= 2048: 64 * 32 = 2048 in two halves (128 KiB); 65 * 32 = 2080 the long-list form
    ((70, 32, 64, 63, 40, 6, 1, 1), "labelprop.topk_mfma_chunks2"),
    ((70, 32, 64, 64, 40, 6, 1, 1), "labelprop.topk_mfma_long"),
]


@pytest.mark.parametrize("shape,want", TOPK, ids=["x".join(map(str, a[0])) for a in TOPK])
def test_topk_routes(hip, monkeypatch, shape, want):
    for name in ("CRW_LABELPROP_TOPK_VALU", "CRW_LABELPROP_TOPK_CHUNKS"):
        monkeypatch.delenv(name, raising=False)
    T, N, C, cxt, radius, knn, first, gw = shape
    f = hip.normalize(lp_embeddings(T, N, C, T + N).cuda())
    (W, I), hit = took(hip, hip.labelprop_topk, f, cxt, radius, 0.1, knn, first_frame=first, grid_w=gw)
    assert hit == {want}, hit
    (V, Iv), hit = took(hip, hip.labelprop_topk_scores, f, cxt, radius, 0.1, knn, first_frame=first, grid_w=gw)
    assert hit == {want} and torch.equal(I, Iv), hit
    res = orc.topk_lists_audit(f, cxt, radius, 0.1, knn, first, gw, W, I, V)
    assert not any(res["violations"].values()) and all(v <= 1 for v in res["worst"].values()), res


# ------------------------------------------------------------------------------------------------ CNN convolutions
# the three layers in patch form: forward, backward-data and weight gradient against fp64 (the body of
# test_hip_parity.test_encoder_conv_kernels_match_torch).  Waves: 8 for hi/lo pairs, 4 for plain bf16; weight gradient: first
# generation at 64 output channels, streamed at 128
CONV = [((32, 64), 3, {"conv.patch_nw8", "wgrad.gen1"}), ((64, 128), 3, {"conv.patch_nw8", "wgrad.streamed"}),
        ((128, 128), 3, {"conv.patch_nw8", "wgrad.streamed"}), ((32, 64), 1, {"conv.patch_nw4", "wgrad.gen1"}),
        ((64, 128), 1, {"conv.patch_nw4", "wgrad.streamed"}), ((128, 128), 1, {"conv.patch_nw4", "wgrad.streamed"})]


@pytest.mark.parametrize("layer,split,want", CONV, ids=[f"{a[0][0]}-{a[0][1]}-split{a[1]}" for a in CONV])
def test_conv_patch_routes(hip, layer, split, want):
    _, hit = took(hip, tp.test_encoder_conv_kernels_match_torch, hip, layer[0], layer[1], split)
    assert hit == want, hit


@pytest.mark.parametrize("split", [3, 1])
def test_conv_map_routes_on_a_14x21_map(hip, split):
    """2 x 3 tiles of 10 x 10: two with 100 in-map pixels (7 row tiles), four with 40, 10, 10 and 4 (at most 64: 4 row tiles) --
    backward-data and the map weight gradient of conv4 against fp64 (test_hip_parity.test_map_backward_kernels_match_torch)"""
    _, hit = took(hip, tp.test_map_backward_kernels_match_torch, hip, split)
    assert hit == {"conv.map_big", "conv.map_small", "wgrad.map"}, hit


def test_conv_map_forward_of_the_three_layers(hip):
    """CNN inference on 20 x 27 patches: front end and conv3 - conv5 on 14 x 21 maps, both tile classes, against the fp64 network"""
    _, hit = took(hip, tp.test_encoder_inference_trunk_any_patch_size, hip, (20, 27), 3)
    assert hit == {"front.fwd_nt512", "conv.map_big", "conv.map_small"}, hit


def test_conv_chain_switch_per_call(hip, monkeypatch):
    """conv3 -> conv5 in one launch against the three launches it replaces (bit for bit), and CRW_CONV_CHAIN=0 (read per call by the
    binding) through the encoder: the chain's route disappears, the per-layer kernel's stays"""
    (xh, xl, packed, biases), ref = tcc._reference(hip, 5)
    got, hit = took(hip, hip.enc_conv_fwd_chain, xh, xl, packed, biases)
    assert hit == {"conv.chain"}, hit
    tcc._assert_equal(dict(zip(tcc.OUTPUTS, got)), ref)
    _, hit = took(hip, tcc._per_layer, hip, xh, xl, packed, biases)
    assert hit == {"conv.patch_nw8"}, hit
    import encoder
    torch.manual_seed(5)
    enc = encoder.CNN(False).cuda()
    x, r = torch.randn(6, 1, 16, 16).cuda(), torch.randn(6, 128).cuda()
    monkeypatch.delenv("CRW_CONV_CHAIN", raising=False)
    with hip.routes() as hit:
        gap1, grads1 = tcc._encoder_step(hip, enc, x, r)
    with_chain = set(hit)
    monkeypatch.setenv("CRW_CONV_CHAIN", "0")
    with hip.routes() as hit:
        gap0, grads0 = tcc._encoder_step(hip, enc, x, r)
    SEEN.update(with_chain, hit)
    step = {"front.fwd_nt512", "front.bwd_saved", "conv.patch_nw8", "wgrad.gen1", "wgrad.streamed"}   # (backward-data is per layer either way)
    assert with_chain == step | {"conv.chain"} and set(hit) == step, (with_chain, set(hit))
    assert torch.equal(gap1, gap0) and all(torch.equal(a, b) for a, b in zip(grads1, grads0))


# ------------------------------------------------------------------------------------------------ Resnet
def test_resnet_product_routes(hip):
    """one product of every kind at P = 128 against fp64 (test_resnet_hip.test_rn_conv_forward_backward_wgrad_match_torch): the
    split-role kernel and the 32-patch weight gradient"""
    _, hit = took(hip, trn.test_rn_conv_forward_backward_wgrad_match_torch, hip, trn.CONVS[1], 128)
    assert hit == {"rn_conv.spec2", "rn_wgrad.bk32"}, hit


# the stem's forward product by patch size: 16 x 16 a patch per wave; other sizes a band of output rows per wave where the geometry
# covers them -- 20 x 27 and 32 x 32 do (W1 = 15 / 17 <= 96 output columns, w + 9 <= 128); the gathered product is left to wider
# patches and to CRW_RN_STEM_BAND=0 (tests/test_variants.py).  The stem's backward-data product exists at the other sizes only and
# is always on the plain kernel, 64 deep.
NET = {"rn_net.fwd_side_stream", "rn_net.bwd_side_stream", "rn_net.bwd_fused_red", "rn_bn.ticket_fence", "rn_conv.spec2", "rn_wgrad.bk32"}
STEM = [("resnet_train_B2T4N5", {"rn_stem.patch_per_wave"}), ("resnet_train_20x27_B2T4N5", {"rn_stem.band", "rn_conv.stem_bwd_bk64"}),
        ("resnet_train_32x32_B2T4N5", {"rn_stem.band", "rn_conv.stem_bwd_bk64"})]


@pytest.mark.parametrize("name,stem", STEM, ids=[a[0] for a in STEM])
def test_resnet_stem_routes(hip, monkeypatch, name, stem):
    """the reference's recorded training step at the three patch sizes (test_resnet_hip.test_resnet_hip_training_step_matches_reference)"""
    _, hit = took(hip, trn.test_resnet_hip_training_step_matches_reference, hip, monkeypatch, name)
    walk = {r for r in hit if r.split(".")[0] in ("affinity", "walk", "chain_small", "softmax", "gemm_f32")}
    assert hit - walk == NET | stem, sorted(hit - walk)


# ------------------------------------------------------------------------------------------------ the default environment
def test_no_variant_only_route_ran_in_this_file(hip):
    """every test above ran in this process, under the default environment (switches were set per call only where a test says
    so): none of the routes that only a variant switch reaches was taken"""
    assert len(SEEN) >= 40, sorted(SEEN)                            # the tests above did run
    assert not SEEN & set(rr.VARIANT_ONLY), sorted(SEEN & set(rr.VARIANT_ONLY))
