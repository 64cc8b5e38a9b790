"""Do the training path, the label propagation and the encoder's packers read or write outside their operands?  Every case calls
the C ABI through crw_hip.lib() with this test's own buffers and runs under `run_banded` of tests/stale_ref.py (its proof on
planted defects: tests/test_stale.py): every input, output and workspace is a view into the middle of a larger allocation, with a
guard band of at least 256 KiB -- and no shorter than the operand's largest index step -- in front of it and behind it, at the
allocator's alignment.  The sequence runs once with every band filled with 0xFF (NaN as fp32 and bf16, a huge index as int32) and
once with 0x00.  Held per case: every output is finite and bit-identical between the two runs (a halo, a padding row, the nodes
N .. 15 of a query tile or a ragged last k-chunk fetched from the neighbouring memory instead of being made would be NaN in one run
and right in the other), and no byte of any band changed.  The property is two runs of the same code: no tolerance, no reference.
A case adds cheap value checks (the result is not all zeros, the lists sum to 1).

The bands see an index that is off by up to one plane, frame or matrix, not a wild pointer; operands that are not 256-byte aligned
are a separate question.  The encoder's kernels run between bands in tests/test_encoder_stale_gpu.py; the last section here bands
the encoder entry points that file reaches through the binding only (packers, crw_enc_gap_bwd, crw_enc_front_fwd_map,
crw_rn_bn_apply, crw_rn_bn_pool, crw_rn_split).  `BANDED` of tests/stale_ref.py lists who bands what."""
import ctypes

import pytest
import torch

import stale_ref as sr
import walk_ref as wr
from stale_ref import Buf, Case
from test_encoder_stale_gpu import _gen, _ok, _p, _randn, _stream
from test_labelprop_lists import lp_embeddings, scrambled_seed
from test_labelprop_lists_gpu import GATHER_CASES, TOPK_CASES

pytestmark = pytest.mark.gpu

F32, BF16, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8
TAU = 0.05


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    assert crw_hip.has_sweep() and crw_hip.has_sliding() and crw_hip.has_confidence()
    return crw_hip


def _out(*shape, dtype=F32, init=None):
    """an output (or, with init, an in/out operand) of that shape: bytes, how to read it for the finiteness check, largest step"""
    like = torch.empty(shape, dtype=dtype, device="meta")
    return Buf(like.numel() * like.element_size(), dtype if dtype.is_floating_point else None, step=sr.largest_step(like), init=init)


def _as(t, name, dtype, *shape):
    like = torch.empty(shape, dtype=dtype, device="meta")
    return t[name][:like.numel() * like.element_size()].view(dtype).view(shape)


def _case(entry, bufs, run, home, check=None, zero_ok=False):
    """check(tensors of the 0x00-banded run): the case's cheap value checks; zero_ok: the right result is all zeros"""
    def synced(inp, t):
        run(inp, t)
        torch.cuda.synchronize()
    case = Case(entry, None, bufs, synced, device="cuda", home=home)
    case.check, case.zero_ok = check, zero_ok
    return case


# ================================================================================================ training path
def normalize(hip, home, rows, C):
    lib = hip.lib()
    emb = home(_randn(_gen(C), rows, C, scale=2.0), "emb")
    bufs = dict(ehat=_out(rows, C), norm=_out(rows))

    def run(_, t):
        _ok("crw_normalize", lib.crw_normalize(_p(emb), rows, C, _p(t["ehat"]), _p(t["norm"]), _stream()))

    def check(t):
        assert torch.allclose(_as(t, "ehat", F32, rows, C).norm(dim=1), torch.ones(rows, device="cuda"), atol=1e-5)
    return _case("crw_normalize", bufs, run, home, check)


def _embeddings(B, T, N, C):
    return torch.from_numpy(wr.embeddings(B, T, N, 1000 * N + C, C=C)).cuda()


def affinity_fwd(hip, home, B, T, N, C):
    lib = hip.lib()
    emb = home(_embeddings(B, T, N, C), "emb")
    nws = lib.crw_affinity_ws_bytes(B, T, N)
    bufs = dict(ehat=_out(B, T, N, C), norm=_out(B, T, N), A=_out(B, T - 1, N, N), stats=_out(4, B, T - 1, N), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_affinity_fwd", lib.crw_affinity_fwd(_p(emb), B, T, N, C, TAU, _p(t["ehat"]), _p(t["norm"]), _p(t["A"]), _p(t["stats"]),
                                                     _p(t["ws"]), nws, _stream()))

    def check(t):
        A, stats = _as(t, "A", F32, B, T - 1, N, N), _as(t, "stats", F32, 4, B, T - 1, N)
        assert torch.allclose(stats[0], A.max(-1).values, rtol=1e-6) and torch.allclose(stats[2], A.max(-2).values, rtol=1e-6)
    return _case("crw_affinity_fwd", bufs, run, home, check)


def affinity_bwd(hip, home, B, T, N, C):
    lib = hip.lib()
    _, ehat, norm, _ = hip.affinity_fwd(_embeddings(B, T, N, C), TAU)
    dA, ehat, norm = home.many(dA=_randn(_gen(N + C), B, T - 1, N, N, scale=0.1), ehat=ehat, norm=norm)
    bufs = dict(dehat_ws=Buf(B * T * N * C * 4, ws=True), demb=_out(B, T, N, C))

    def run(_, t):
        _ok("crw_affinity_bwd", lib.crw_affinity_bwd(_p(dA), _p(ehat), _p(norm), B, T, N, C, TAU, _p(t["dehat_ws"]), _p(t["demb"]),
                                                     _stream()))

    def check(t):
        assert _as(t, "demb", F32, B, T, N, C).abs().amax(dim=(2, 3)).min() > 0                         # every frame gets a gradient
    return _case("crw_affinity_bwd", bufs, run, home, check)


def walk(hip, home, chain, B, T, N, imported):
    """crw_walk_fwd (with At_out) then crw_walk_bwd on the logits and the statistics crw_affinity_fwd made"""
    lib = hip.lib()
    A, _, _, stats = hip.affinity_fwd(_embeddings(B, T, N, 32), TAU)
    A, stats, gloss = home.many(A=A, stats=stats if imported else None, gloss=torch.full((1,), wr.GLOSS, device="cuda"))
    nstate, nscratch = lib.crw_walk_state_bytes(B, T, N, chain), lib.crw_walk_scratch_bytes(B, T, N, chain)
    bufs = dict(state=Buf(nstate, ws=True), scratch=Buf(nscratch, ws=True), loss=_out(1), dA=_out(B, T - 1, N, N))
    if T > 2:
        bufs["At"] = _out(B, T - 2, N, N)

    def run(_, t):
        _ok("crw_walk_fwd", lib.crw_walk_fwd(_p(A), _p(stats), B, T, N, chain, _p(t["state"]), nstate, _p(t.get("At")), _p(t["loss"]),
                                             _stream()))
        _ok("crw_walk_bwd", lib.crw_walk_bwd(_p(gloss), _p(A), B, T, N, chain, _p(t["state"]), nstate, _p(t["scratch"]), nscratch,
                                             _p(t["dA"]), _stream()))

    def check(t):
        dA = _as(t, "dA", F32, B, T - 1, N, N)
        assert torch.count_nonzero(dA[:, -1]).item() == 0                                              # A_{T-2} never enters the loss
        if T > 2:
            assert float(_as(t, "loss", F32, 1)) > 0 and torch.count_nonzero(dA[:, 0]).item() > 0
            assert torch.allclose(_as(t, "At", F32, B, T - 2, N, N).sum(-1), torch.ones(B, T - 2, N, device="cuda"), atol=5e-2)
        else:
            assert float(_as(t, "loss", F32, 1)) == 0
    return _case(f"crw_walk_fwd + crw_walk_bwd chain {chain}", bufs, run, home, check, zero_ok=T == 2)


def gemm_f32(hip, home, n, batch, trans, beta):
    lib, g = hip.lib(), _gen(n + trans + beta)
    A, B = home.many(A=_randn(g, batch, n, n), B=_randn(g, batch, n, n))
    C0 = _randn(g, batch, n, n)
    bufs = dict(C=_out(batch, n, n, init=C0 if beta else None))

    def run(_, t):
        _ok("crw_gemm_f32", lib.crw_gemm_f32(_p(A), _p(B), _p(t["C"]), n, batch, trans, trans, beta, _stream()))

    def check(t):
        ref = (A.mT if trans else A).double() @ (B.mT if trans else B).double() + (C0.double() if beta else 0)
        assert torch.allclose(_as(t, "C", F32, batch, n, n).double(), ref, atol=1e-3)
    return _case("crw_gemm_f32", bufs, run, home, check)


def gemm_bf16(hip, home, n, split, batch=2):
    lib, g = hip.lib(), _gen(n + split)
    A, B = home.many(A=_randn(g, batch, n, n), B=_randn(g, batch, n, n))
    nws = lib.crw_gemm_bf16_ws_bytes(n, batch, split)
    bufs = dict(C=_out(batch, n, n), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_gemm_bf16", lib.crw_gemm_bf16(_p(A), _p(B), _p(t["C"]), n, batch, 0, 0, 0, split, _p(t["ws"]), nws, 1, _stream()))

    def check(t):
        assert _as(t, "C", F32, batch, n, n).abs().amax(dim=(1, 2)).min() > 0
    return _case("crw_gemm_bf16", bufs, run, home, check)


def xent_metric(hip, home, T, N, C):
    lib = hip.lib()
    ehat = home(hip.normalize(_randn(_gen(T + N + C), T, N, C)), "ehat")
    bufs = dict(xent=_out(N, T - 1))

    def run(_, t):
        _ok("crw_xent_metric", lib.crw_xent_metric(_p(ehat), T, N, C, _p(t["xent"]), _stream()))

    def check(t):
        assert _as(t, "xent", F32, N, T - 1).abs().min() > 0
    return _case("crw_xent_metric", bufs, run, home, check)


ADAM = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)


def adam_step(hip, home, n):
    """n = 1027: the scalar tail of adam_kernel (three elements behind the last float4)"""
    lib, g = hip.lib(), _gen(n)
    grad = home(_randn(g, n), "g")
    p0, m0, v0 = _randn(g, n), _randn(g, n, scale=0.1), torch.rand(n, generator=g).cuda() * 0.01
    bufs = dict(p=_out(n, init=p0), m=_out(n, init=m0), v=_out(n, init=v0))

    def run(_, t):
        _ok("crw_adam_step", lib.crw_adam_step(_p(t["p"]), _p(grad), _p(t["m"]), _p(t["v"]), n, ADAM["lr"], ADAM["beta1"], ADAM["beta2"],
                                               ADAM["eps"], 3, _stream()))

    def check(t):
        moved = _as(t, "p", F32, n) != p0
        assert bool(moved[-8:].all()) and float(moved.float().mean()) > 0.99
    return _case("crw_adam_step", bufs, run, home, check)


# ================================================================================================ label propagation
def _feats(hip, T, N, C):
    return hip.normalize(lp_embeddings(T, N, C, T + N).cuda())


def topk(hip, home, T, N, C, cxt, radius, knn, first, gw):
    """crw_labelprop_topk_grid, crw_labelprop_topk_scores and (a column of patches only) crw_labelprop_topk on one route"""
    lib = hip.lib()
    ehat = home(_feats(hip, T, N, C), "ehat")
    F = T - first
    bufs = dict(W=_out(F, knn, N), I=_out(F, knn, N, dtype=I32), V=Buf(F * knn * N * 4, None, step=knn * N * 4),   # V: -inf in empty slots
                Iv=_out(F, knn, N, dtype=I32))
    if gw == 1:
        bufs.update(W1=_out(F, knn, N), I1=_out(F, knn, N, dtype=I32))

    def run(_, t):
        _ok("crw_labelprop_topk_grid", lib.crw_labelprop_topk_grid(_p(ehat), T, N, C, cxt, radius, 0.1, knn, first, gw, _p(t["W"]), _p(t["I"]),
                                                                   _stream()))
        _ok("crw_labelprop_topk_scores", lib.crw_labelprop_topk_scores(_p(ehat), T, N, C, cxt, radius, 0.1, knn, first, gw, _p(t["V"]),
                                                                       _p(t["Iv"]), _stream()))
        if gw == 1:
            _ok("crw_labelprop_topk", lib.crw_labelprop_topk(_p(ehat), T, N, C, cxt, radius, 0.1, knn, first, _p(t["W1"]), _p(t["I1"]), _stream()))

    def check(t):
        W, I = _as(t, "W", F32, F, knn, N), _as(t, "I", I32, F, knn, N)
        assert torch.allclose(W.sum(1), torch.ones(F, N, device="cuda"), atol=1e-5), "a list's weights do not sum to 1"
        assert int(I.min()) >= 0 and int(I.max()) < min(T - 1, cxt + 1) * N and torch.equal(I, _as(t, "Iv", I32, F, knn, N))
        assert not torch.isnan(_as(t, "V", F32, F, knn, N)).any()
        if gw == 1:
            assert torch.equal(W, _as(t, "W1", F32, F, knn, N)) and torch.equal(I, _as(t, "I1", I32, F, knn, N))
    return _case("crw_labelprop_topk_grid / _topk_scores / _topk", bufs, run, home, check)


def sweep_weights(hip, home, knns=(3, 9)):
    """on the scores of the 21-node case"""
    lib = hip.lib()
    T, N, C, cxt, radius, kcap, first, gw = (40, 21, 64, 6, 4, 9, 1, 1)
    V, _ = hip.labelprop_topk_scores(_feats(hip, T, N, C), cxt, radius, 0.1, kcap, first_frame=first, grid_w=gw)
    V = home(V, "V")
    F, nk, kmax = T - first, len(knns), max(knns)
    arr = (ctypes.c_int * nk)(*knns)
    bufs = dict(W=_out(nk, F, kmax, N))

    def run(_, t):
        _ok("crw_labelprop_sweep_weights", lib.crw_labelprop_sweep_weights(_p(V), F, kcap, N, arr, nk, _p(t["W"]), _stream()))

    def check(t):
        W = _as(t, "W", F32, nk, F, kmax, N)
        assert torch.allclose(W.sum(2), torch.ones(nk, F, N, device="cuda"), atol=1e-5) and torch.count_nonzero(W[0, :, knns[0]:]).item() == 0
    return _case("crw_labelprop_sweep_weights", bufs, run, home, check)


BATCH_TEMPS = (0.1, 0.05, 0.02)       # G = 3 configurations


def gather(hip, home, T, N, C, M, cxt, radius, knn, gw, first=1):
    """crw_labelprop_gather, _propagate, _propagate_batch (G = 3), _propagate_sliding and _sliding_batch on the lists of one
    GATHER_CASES shape.  first > 1: no seed, the frames before `first` are the caller's (in/out operands, each run from its copy)."""
    lib, G = hip.lib(), len(BATCH_TEMPS)
    feats = _feats(hip, T, N, C)
    lists = [hip.labelprop_topk(feats, cxt, radius, temp, knn, first_frame=first, grid_w=gw) for temp in BATCH_TEMPS]
    seed = scrambled_seed(N, M).cuda()
    L_init = p_init = L_init3 = p_init3 = None
    if first > 1:
        W1, I1 = hip.labelprop_topk(feats, cxt, radius, BATCH_TEMPS[0], knn, first_frame=1, grid_w=gw)
        L_init, _ = hip.labelprop_gather(seed, W1, I1, T, N, M, first_frame=1)
        L_init[first * N:] = -7.0
        p_init = torch.full((N, T), -1.0, device="cuda")
        L_init3, p_init3 = torch.stack([L_init] * G), torch.stack([p_init] * G)
    W, I, W3, I3, seed = home.many(W=lists[0][0], I=lists[0][1], W3=torch.stack([w for w, _ in lists]), I3=torch.stack([i for _, i in lists]),
                                   seed=seed if first == 1 else None)
    stride = (T - first) * knn * N
    one = ("gather", "propagate", "sliding")
    bufs = {}
    for k in one:
        bufs["L_" + k], bufs["pred_" + k] = _out(T * N, M, init=L_init), _out(N, T, init=p_init)
    for k in ("batch", "sliding_batch"):
        bufs["L_" + k], bufs["pred_" + k] = _out(G, T * N, M, init=L_init3), _out(G, N, T, init=p_init3)

    def run(_, t):
        Lp = lambda k: (_p(t["L_" + k]), _p(t["pred_" + k]), _stream())
        _ok("crw_labelprop_gather", lib.crw_labelprop_gather(_p(seed), _p(W), _p(I), T, N, M, knn, first, *Lp("gather")))
        _ok("crw_labelprop_propagate", lib.crw_labelprop_propagate(_p(seed), _p(W), _p(I), T, N, M, knn, first, cxt, *Lp("propagate")))
        _ok("crw_labelprop_propagate_sliding", lib.crw_labelprop_propagate_sliding(_p(seed), _p(W), _p(I), T, N, M, knn, first, cxt,
                                                                                   *Lp("sliding")))
        _ok("crw_labelprop_propagate_batch", lib.crw_labelprop_propagate_batch(_p(seed), _p(W3), _p(I3), stride, G, T, N, M, knn, first, cxt,
                                                                               *Lp("batch")))
        _ok("crw_labelprop_propagate_sliding_batch", lib.crw_labelprop_propagate_sliding_batch(_p(seed), _p(W3), _p(I3), stride, G, T, N, M,
                                                                                               knn, first, cxt, *Lp("sliding_batch")))

    def check(t):
        Lg, Lb = _as(t, "L_gather", F32, T, N, M), _as(t, "L_batch", F32, G, T, N, M)
        for L in (Lg, _as(t, "L_sliding", F32, T, N, M), Lb[1], _as(t, "L_sliding_batch", F32, G, T, N, M)[2]):
            assert torch.allclose(L[first:].sum(-1), torch.ones(T - first, N, device="cuda"), atol=1e-4), "a soft label does not sum to 1"
        assert torch.equal(Lg, _as(t, "L_propagate", F32, T, N, M)) and torch.equal(Lg, Lb[0])          # the header's "bit-identical"
        assert torch.equal(_as(t, "pred_gather", F32, N, T), _as(t, "pred_batch", F32, G, N, T)[0])
        assert torch.equal(_as(t, "L_sliding", F32, T, N, M), _as(t, "L_sliding_batch", F32, G, T, N, M)[0])
    return _case("crw_labelprop_gather / _propagate / _propagate_batch / _propagate_sliding / _propagate_sliding_batch", bufs, run, home,
                 check)


def confidence(hip, home, M, T=5, N=21):
    """M = 8: 16-byte loads; M = 3: the scalar route"""
    lib = hip.lib()
    L = home(torch.softmax(_randn(_gen(M), T * N, M, scale=2.0), dim=1).contiguous(), "L")
    bufs = {f"conf{kind}": _out(N, T) for kind in (0, 1, 2)}

    def run(_, t):
        for kind in (0, 1, 2):
            _ok("crw_labelprop_confidence", lib.crw_labelprop_confidence(_p(L), T, N, M, kind, 1, _p(t[f"conf{kind}"]), _stream()))

    def check(t):
        c0 = _as(t, "conf0", F32, N, T)
        assert torch.equal(c0[:, 1:], L.view(T, N, M).amax(-1).t()[:, 1:])                              # "bitwise the largest entry"
        for kind in (1, 2):
            c = _as(t, f"conf{kind}", F32, N, T)
            assert bool(((c >= 0) & (c <= 1)).all()) and c.abs().sum() > 0
    return _case("crw_labelprop_confidence", bufs, run, home, check)


# ================================================================================================ encoder: packers and the rest
def enc_pack_weights(hip, home, cout=128, cin=64):
    lib = hip.lib()
    w = home(_randn(_gen(cout), cout, cin, 3, 3, scale=0.05), "w")
    bufs = {k: _out(9, cout * cin, dtype=BF16) for k in ("fwd_hi", "fwd_lo", "bwd_hi", "bwd_lo")}

    def run(_, t):
        _ok("crw_enc_pack_weights", lib.crw_enc_pack_weights(_p(w), cout, cin, _p(t["fwd_hi"]), _p(t["fwd_lo"]), _p(t["bwd_hi"]),
                                                             _p(t["bwd_lo"]), _stream()))
    return _case("crw_enc_pack_weights", bufs, run, home)


def enc_pack_input(hip, home, mapped, P=3, C=32):
    lib = hip.lib()
    H, W = (14, 21) if mapped else (10, 10)
    x = home(_randn(_gen(H), P, C, H, W), "x")
    bufs = dict(x_hi=_out(P, H * W, C, dtype=BF16), x_lo=_out(P, H * W, C, dtype=BF16))

    def run(_, t):
        if mapped:
            _ok("crw_enc_pack_input_map", lib.crw_enc_pack_input_map(_p(x), P, C, H, W, _p(t["x_hi"]), _p(t["x_lo"]), _stream()))
        else:
            _ok("crw_enc_pack_input", lib.crw_enc_pack_input(_p(x), P, C, _p(t["x_hi"]), _p(t["x_lo"]), _stream()))
    return _case("crw_enc_pack_input_map" if mapped else "crw_enc_pack_input", bufs, run, home)


def enc_gap_bwd(hip, home, P=3, C=128, npix=100):
    lib, g = hip.lib(), _gen(npix)
    dgap, yh = home.many(dgap=_randn(g, P, C), y_hi=torch.relu(_randn(g, P, npix, C)).to(BF16))
    bufs = dict(dy_hi=_out(P, npix, C, dtype=BF16), dy_lo=_out(P, npix, C, dtype=BF16))

    def run(_, t):
        _ok("crw_enc_gap_bwd", lib.crw_enc_gap_bwd(_p(dgap), _p(yh), P, C, npix, _p(t["dy_hi"]), _p(t["dy_lo"]), _stream()))
    return _case("crw_enc_gap_bwd", bufs, run, home)


def enc_front_pack(hip, home):
    lib = hip.lib()
    w2 = home(_randn(_gen(32), 32, 8, 5, 5, scale=0.07), "w2")
    bufs = dict(fwd_hi=_out(7, 32, 32, dtype=BF16), fwd_lo=_out(7, 32, 32, dtype=BF16), bwd_hi=_out(25, 8, 32, dtype=BF16),
                bwd_lo=_out(25, 8, 32, dtype=BF16))

    def run(_, t):
        _ok("crw_enc_front_pack", lib.crw_enc_front_pack(_p(w2), _p(t["fwd_hi"]), _p(t["fwd_lo"]), _p(t["bwd_hi"]), _p(t["bwd_lo"]), _stream()))
    return _case("crw_enc_front_pack", bufs, run, home)


def enc_front_fwd_map(hip, home, split, P=2, cin=1, H=20, W=27):
    """14 x 21 output map = 2 x 3 tiles, partial in both directions"""
    lib, g = hip.lib(), _gen(H * W + split)
    x, w1, b1, b2 = home.many(x=_randn(g, P, cin, H, W), w1=_randn(g, 8, cin, 5, 5, scale=0.2), b1=_randn(g, 8, scale=0.1),
                              b2=_randn(g, 32, scale=0.1))
    fh, fl, _, _ = hip.enc_front_pack(_randn(g, 32, 8, 5, 5, scale=0.07), split)
    fh, fl = home.many(w2_hi=fh, w2_lo=fl)
    npix = (H - 6) * (W - 6)
    bufs = dict(y_hi=_out(P, npix, 32, dtype=BF16))
    if split == 3:
        bufs["y_lo"] = _out(P, npix, 32, dtype=BF16)

    def run(_, t):
        _ok("crw_enc_front_fwd_map", lib.crw_enc_front_fwd_map(split, _p(x), P, cin, H, W, _p(w1), _p(b1), _p(fh), _p(fl), _p(b2), _p(t["y_hi"]),
                                                               _p(t.get("y_lo")), _stream()))
    return _case("crw_enc_front_fwd_map", bufs, run, home)


def rn_pack_conv(hip, home, cout=64, cin=64, k=3):
    lib = hip.lib()
    w = home(_randn(_gen(cout + k), cout, cin, k, k, scale=0.04), "w")
    bufs = {key: _out(cout, k * k * cin, dtype=BF16) for key in ("fwd_hi", "fwd_lo", "bwd_hi", "bwd_lo")}

    def run(_, t):
        _ok("crw_rn_pack_conv", lib.crw_rn_pack_conv(_p(w), cout, cin, k, k, _p(t["fwd_hi"]), _p(t["fwd_lo"]), _p(t["bwd_hi"]), _p(t["bwd_lo"]),
                                                     _stream()))
    return _case("crw_rn_pack_conv", bufs, run, home)


def rn_pack_stem(hip, home, h=20, w=27):
    lib = hip.lib()
    w1 = home(_randn(_gen(h * w), 64, 3, 7, 7, scale=0.08), "w1")
    cols, ld = lib.crw_rn_stem_cols(w), lib.crw_rn_stem_toeplitz_ld(w)
    bufs = dict(fwd_hi=_out(64, 256, dtype=BF16), fwd_lo=_out(64, 256, dtype=BF16), toep_hi=_out(h + 2, cols, ld, dtype=BF16),
                toep_lo=_out(h + 2, cols, ld, dtype=BF16))

    def run(_, t):
        _ok("crw_rn_pack_stem", lib.crw_rn_pack_stem(_p(w1), h, w, _p(t["fwd_hi"]), _p(t["fwd_lo"]), _p(t["toep_hi"]), _p(t["toep_lo"]),
                                                     _stream()))
    return _case("crw_rn_pack_stem", bufs, run, home)


def rn_pack_stem16(hip, home):
    lib = hip.lib()
    w1 = home(_randn(_gen(16), 64, 3, 7, 7, scale=0.08), "w1")
    bufs = dict(wf=_out(28672, dtype=BF16), wt=_out(28672, dtype=BF16))

    def run(_, t):
        _ok("crw_rn_pack_stem16", lib.crw_rn_pack_stem16(_p(w1), _p(t["wf"]), _p(t["wt"]), _stream()))
    return _case("crw_rn_pack_stem16", bufs, run, home)


def rn_split(hip, home, P=130, C=128):
    lib = hip.lib()
    Ppad = hip.rn_padded(P)
    x = home(_randn(_gen(P), P, C), "x")
    bufs = dict(hi=_out(Ppad, C, dtype=BF16), lo=_out(Ppad, C, dtype=BF16))

    def run(_, t):
        _ok("crw_rn_split", lib.crw_rn_split(_p(x), P, C, _p(t["hi"]), _p(t["lo"]), _stream()))
    return _case("crw_rn_split", bufs, run, home)


def _bn_inputs(hip, P, npix, C, seed):
    """a raw convolution output [Ppad][npix][C] with zero padding rows, and coefficients [4][C] = scale, shift, mean, invstd"""
    g, Ppad = _gen(seed), hip.rn_padded(P)
    Z = torch.zeros(Ppad, npix * C, device="cuda")
    Z[:P] = _randn(g, P, npix * C, scale=2.0, shift=0.5)
    coef = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1,
                        torch.rand(C, generator=g) + 0.5]).cuda()
    return Ppad, Z, coef


def rn_bn_apply(hip, home, P=130, npix=9, C=128):
    """the shortcut form with a residual: relu(bn(Z) + bn_d(Zd) + res)"""
    lib = hip.lib()
    Ppad, Z, coef = _bn_inputs(hip, P, npix, C, 1)
    _, Zd, coefd = _bn_inputs(hip, P, npix, C, 2)
    rh, rl = hip.rn_split(_randn(_gen(3), P, npix * C), P, npix * C)
    Z, coef, Zd, coefd, rh, rl = home.many(Z=Z, coef=coef, Zd=Zd, coef_d=coefd, res_hi=rh, res_lo=rl)
    bufs = dict(y_hi=_out(Ppad, npix * C, dtype=BF16), y_lo=_out(Ppad, npix * C, dtype=BF16))

    def run(_, t):
        _ok("crw_rn_bn_apply", lib.crw_rn_bn_apply(_p(Z), _p(coef), _p(Zd), _p(coefd), _p(rh), _p(rl), P, npix, C, 1, _p(t["y_hi"]),
                                                   _p(t["y_lo"]), _stream()))
    return _case("crw_rn_bn_apply", bufs, run, home)


def rn_bn_pool(hip, home, P=70, H=7, W=6, C=64):
    """7 x 6 -> 4 x 3: windows that hang over the map's edge on every side"""
    lib = hip.lib()
    Ppad, Z, coef = _bn_inputs(hip, P, H * W, C, 4)
    Z, coef = home.many(Z=Z, coef=coef)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    bufs = dict(y_hi=_out(Ppad, Ho * Wo * C, dtype=BF16), y_lo=_out(Ppad, Ho * Wo * C, dtype=BF16), amax=_out(Ppad, Ho * Wo * C, dtype=U8))

    def run(_, t):
        _ok("crw_rn_bn_pool", lib.crw_rn_bn_pool(_p(Z), _p(coef), P, H, W, C, _p(t["y_hi"]), _p(t["y_lo"]), _p(t["amax"]), _stream()))
    return _case("crw_rn_bn_pool", bufs, run, home)


# ================================================================================================ the table
def _walks():
    """chain 0 at N = 7 (the persistent small chain) and N = 70 (Np = 96); chains 2 and 1 at N = 130 (Np = 256), B = 2, T = 4;
    T = 2 (the memset routes); each with the walk's own statistics and with imported ones"""
    shapes = [(0, 2, 5, 7), (0, 1, 4, 70), (2, 2, 4, 130), (1, 2, 4, 130), (0, 2, 2, 7), (1, 2, 2, 130)]
    return [(f"walk-chain{c}-B{B}-T{T}-N{N}-{'imported' if imp else 'own'}", walk, (c, B, T, N, imp)) for c, B, T, N in shapes
            for imp in (False, True)]


# (B, T, N, C): a small one; a ragged 128-row tile and the backward's bounds-checked fallback (N % 4 != 0); bf16 splits with a ragged
# last k-chunk; an odd channel count (the edge product plus the dense statistics pass)
AFFINITY_SHAPES = [(1, 3, 40, 20), (2, 3, 130, 64), (1, 3, 300, 128), (1, 3, 21, 33)]
TOPK_BANDED = [s for s, _ in TOPK_CASES[:5]] + [s for s, _ in TOPK_CASES[6:10]]     # every route of csrc/labelprop.hip once
assert (40, 21, 64, 6, 4, 9, 1, 1) in TOPK_BANDED and (100, 48, 64, 80, 30, 20, 7, 1) in TOPK_BANDED and len(TOPK_BANDED) == 9

TABLE = (
    [(f"normalize-15x{C}", normalize, (15, C)) for C in (6, 128)]
    + [("affinity_fwd-" + "x".join(map(str, s)), affinity_fwd, s) for s in AFFINITY_SHAPES]
    + [("affinity_bwd-" + "x".join(map(str, s)), affinity_bwd, s) for s in AFFINITY_SHAPES]
    + _walks()
    + [(f"gemm_f32-n{n}-b3-trans{tr}-beta{beta}", gemm_f32, (n, 3, tr, beta)) for n in (32, 96) for tr in (0, 1) for beta in (0, 1)]
    + [(f"gemm_bf16-n{n}-split{s}", gemm_bf16, (n, s)) for n in (128, 384) for s in (1, 3)]
    + [("xent_metric-" + "x".join(map(str, s)), xent_metric, s) for s in ((5, 3, 6), (9, 70, 33), (4, 130, 128))]
    + [(f"adam_step-n{n}", adam_step, (n,)) for n in (1024, 1027)]
    + [("topk-" + "x".join(map(str, s)), topk, s) for s in TOPK_BANDED]
    + [("sweep_weights-21-nodes-knn3,9", sweep_weights, ())]
    + [("gather-" + "x".join(map(str, s)), gather, s) for s in GATHER_CASES[:6]]
    + [("gather-" + "x".join(map(str, GATHER_CASES[0])) + "-from-frame-2", gather, GATHER_CASES[0] + (2,))]
    + [(f"confidence-M{M}", confidence, (M,)) for M in (3, 8)]
    + [("enc_pack_weights-128x64", enc_pack_weights, ()), ("enc_pack_input-P3-C32", enc_pack_input, (False,)),
       ("enc_pack_input_map-14x21", enc_pack_input, (True,)), ("enc_gap_bwd-P3-C128", enc_gap_bwd, ()),
       ("enc_front_pack", enc_front_pack, ()), ("enc_front_fwd_map-20x27-split3", enc_front_fwd_map, (3,)),
       ("enc_front_fwd_map-20x27-split1", enc_front_fwd_map, (1,)), ("rn_pack_conv-64x64x3x3", rn_pack_conv, ()),
       ("rn_pack_stem-20x27", rn_pack_stem, ()), ("rn_pack_stem16", rn_pack_stem16, ()), ("rn_split-P130-C128", rn_split, ()),
       ("rn_bn_apply-shortcut-residual-P130", rn_bn_apply, ()), ("rn_bn_pool-P70-7x6", rn_bn_pool, ())])


@pytest.mark.parametrize("build,args", [pytest.param(f, a, id=i) for i, f, a in TABLE])
def test_stays_inside_its_operands(hip, build, args):
    case = build(hip, sr.Home("cuda"), *args)
    assert case.home.operands, (case.entry, "no input went through `home`")
    out = sr.run_banded(case)
    live = [k for k, b in case.bufs.items() if not b.ws and out[k][:b.nbytes].any()]
    assert live or case.zero_ok, (case.entry, "every output is all zeros: the case computes nothing")
    if case.check is not None:
        case.check(out)


@pytest.mark.parametrize("defect,operand,prop", [("reads in front", "y", sr.SURROUND_READ),
                                                 ("reads a row past the end, times zero", "y", sr.SURROUND_READ),
                                                 ("writes past the output", "y", sr.SURROUND_WRITTEN),
                                                 ("writes in front of an input", "x", sr.SURROUND_WRITTEN)])
def test_planted_defects_are_seen_on_the_device(defect, operand, prop):
    """the planted defects of tests/test_stale.py as torch operations on the GPU, through the device branch of the harness (the
    allocator's addresses, device-side fills and comparisons): each is reported, and the clean routine and the discarded read pass.
    Every access lies inside the routine's own allocations."""
    from test_stale import _banded as planted
    with pytest.raises(sr.StaleError) as e:
        sr.run_banded(planted(defect, "cuda"))
    assert (e.value.buffer, e.value.prop) == (operand, prop), str(e.value)
    sr.run_banded(planted(None, "cuda"))
    sr.run_banded(planted("reads past the end, discarded by select", "cuda"))


def test_adam_scalar_tail_matches_torch_adam(hip):
    """n = 1027 = 256 float4 + 3: the scalar tail of adam_kernel, which the training loop never reaches (dist.FlatGradBucket pads
    its flat buffers to multiples of 4).  Six steps of gradients over six orders of magnitude against torch.optim.Adam with its
    defaults, at the tolerance of test_hip_parity.py test_flat_adam_matches_torch_adam (an update is ~lr = 1e-2: a few of its ulps)."""
    n = 1027
    g = torch.Generator(device="cuda").manual_seed(9)
    p = torch.randn(n, device="cuda", generator=g)
    q = torch.nn.Parameter(p.clone())
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ta = torch.optim.Adam([q], lr=1e-2)
    for step in range(6):
        gr = torch.randn(n, device="cuda", generator=g) * 10.0 ** (step - 3)
        q.grad = gr.clone()
        hip.adam_step(p, gr, m, v, step + 1, lr=1e-2)
        ta.step()
        torch.testing.assert_close(p, q.data, rtol=2e-6, atol=1e-8)
