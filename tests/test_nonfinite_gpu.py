"""NaN and infinite inputs on the training path (include/crw_hip.h, "Non-finite values"): where the reference -- the PyTorch-op
route of the encoders on the CPU, the numpy oracle of the walk, torch.optim.Adam -- turns non-finite, the kernels do (no
laundering: `fmaxf(NaN, 0) = 0` is the ReLU that fails here); what the reference keeps bit-equal to its clean run, the kernels keep
bit-equal to THEIR clean run (no contamination across patches, batch items, elements).  The rules and the references: tests/
nonfinite_ref.py, pinned on the CPU by tests/test_nonfinite.py.  Masks and bits only; the two finite edge classes at the end (an
all-zero embedding row, rows scaled by 2^+-40) use the tolerances of test_hip_parity.test_affinity_tiles_and_fused_statistics.

Every case names the routes it ran on (crw_hip.routes), so that none passes on another kernel than it says.  No kernel under test
derives an address from an activation: the pooling codes are comparison results (0 .. 3, 0 .. 8), the ReLU gates are bits."""
import copy

import numpy as np
import pytest
import torch

import nonfinite_ref as nf

pytestmark = pytest.mark.gpu


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
    return out, set(hit)


def _report(tag, misses):
    """misses: [(what, count)] of broken rules; all of them in one message (the run against the unfixed library is a record)"""
    misses = [(w, c) for w, c in misses if c]
    print(f"{tag}: {'ok' if not misses else misses}")
    assert not misses, (tag, misses)


def _gpu(net, mode):
    net = copy.deepcopy(net).cuda()
    net.hip_convs = mode
    return net


def _patches(P, cin, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(P, cin, h, w, generator=g), torch.randn(P, 128, generator=g)


def _encoder_case(hip, tag, net, mode, x, gy, poisons, must, must_not=(), local=True):
    """one clean and one poisoned step of the module on the kernels against the reference's poisoned step: features with EQUAL
    masks, the clean patches bit-equal to the clean run (local: the reference is patch-local), every gradient and every buffer a
    superset of the reference's mask.  gy None: forward only, under torch.no_grad()"""
    xp = nf.poison_patches(x, poisons)
    ref_y, ref_g, ref_b = nf.module_reference(net, xp, gy)
    rest = nf.others(x.shape[0], nf.poisoned_patches(poisons))
    dev = None if gy is None else gy.cuda()
    misses = []
    if local:
        assert int(nf.nonfinite(ref_y[rest]).sum()) == 0                               # (pinned in tests/test_nonfinite.py)
        (y0, _), _ = took(hip, nf._step, _gpu(net, mode), x.cuda(), dev)
        assert int(nf.nonfinite(y0).sum()) == 0, tag
    run = _gpu(net, mode)
    (y1, g1), hit = took(hip, nf._step, run, xp.cuda(), dev)
    assert set(must) <= hit and not set(must_not) & hit, (tag, sorted(hit))
    misses.append(("features laundered", nf.superset_misses(ref_y, y1)))
    misses.append(("features: mask differs", nf.mask_differences(ref_y, y1)))
    if local:
        misses.append(("clean patches changed", nf.changed_bits(y1, y0, rest)))
    for k in ref_g:
        misses.append((f"d {k} laundered", nf.superset_misses(ref_g[k], g1[k])))
    for k, b in run.named_buffers():
        misses.append((f"buffer {k} laundered", nf.superset_misses(ref_b[k], b)))
    _report(tag, misses)


# ------------------------------------------------------------------------------------------------ CNN
@pytest.fixture(scope="module")
def cnn():
    import encoder
    torch.manual_seed(3)
    return encoder.CNN(False)


@pytest.mark.parametrize("chain", ["1", "0"], ids=["chain", "per-layer"])
@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "mixed"])
@pytest.mark.parametrize("P", [29, 130])
def test_cnn_patch_kernels(hip, cnn, monkeypatch, P, mode, chain):
    """16x16 patches, forward and backward: P = 29 is odd (the front end's workgroups take two patches each and one is left), P =
    130 crosses a 128-patch tile.  The corner-pixel NaN reaches ONE candidate of a pooling window: what a nested fmaxf drops."""
    monkeypatch.setenv("CRW_CONV_CHAIN", chain)
    x, gy = _patches(P, 1, 16, 16, P)
    fwd3, bwd3 = mode != "bf16", mode == "bf16x3"
    chained = fwd3 and chain == "1"
    must = {"front.fwd_nt512", "front.bwd_saved", "conv.patch_nw8" if bwd3 else "conv.patch_nw4"}
    must |= {"conv.chain"} if chained else {"conv.patch_nw8" if fwd3 else "conv.patch_nw4"}
    _encoder_case(hip, f"CNN 16x16 P={P} {mode} CRW_CONV_CHAIN={chain}", cnn, mode, x, gy, nf.patch_poisons(P), must,
                  () if chained else ("conv.chain",))


@pytest.mark.parametrize("train", [True, False], ids=["train", "no_grad"])
@pytest.mark.parametrize("hw", [(20, 27), (32, 32)], ids=["20x27", "32x32"])
def test_cnn_map_kernels(hip, cnn, hw, train):
    """other patch sizes: the tiled kernels, in training (_HipMapEncoder) and under torch.no_grad (_hip_inference_trunk)"""
    x, gy = _patches(5, 1, *hw, hw[1])
    must = {"front.fwd_nt512", "conv.map_big"} | ({"front.bwd_tile", "wgrad.map"} if train else set())
    _encoder_case(hip, f"CNN {hw} P=5 {'train' if train else 'no_grad'}", cnn, "bf16x3", x, gy if train else None, nf.patch_poisons(5),
                  must, () if train else ("front.bwd_tile", "wgrad.map"))


@pytest.mark.parametrize("name", ["conv3.weight", "conv1.bias"])
def test_cnn_poisoned_weight(hip, cnn, name):
    """one NaN in a weight or a bias: every feature of every patch non-finite, as the reference gives"""
    net = nf.cpu_module(cnn)
    with torch.no_grad():
        dict(net.named_parameters())[name].view(-1)[1] = float("nan")
    x, _ = _patches(29, 1, 16, 16, 7)
    ref_y, _, _ = nf.module_reference(net, x)
    assert int(nf.nonfinite(ref_y).sum()) == ref_y.numel()
    with torch.enable_grad():                                                          # the training forward (the patch kernels)
        y, hit = took(hip, lambda: _gpu(net, "bf16x3")(x.cuda()).detach())
    assert {"front.fwd_nt512", "conv.chain"} <= hit, sorted(hit)
    _report(f"CNN NaN in {name}", [("features: mask differs", nf.mask_differences(ref_y, y))])


# ------------------------------------------------------------------------------------------------ Resnet
@pytest.fixture(scope="module")
def resnet():
    import encoder
    torch.manual_seed(4)
    return encoder.Resnet(False)


RN_SIZES = [((16, 16), 70, "rn_stem.patch_per_wave"), ((32, 32), 40, "rn_stem.band"), ((20, 27), 70, "rn_stem.band")]
RN_IDS = ["16x16", "32x32", "20x27"]


@pytest.mark.parametrize("hw,P,stem", RN_SIZES, ids=RN_IDS)
@pytest.mark.parametrize("path", ["bf16x3", "stepwise"])
def test_resnet_train_mode(hip, resnet, path, hw, P, stem):
    """train-mode BatchNorm: the batch statistics carry one patch's poison to every patch -- all features, the running statistics
    and (where the reference's are) the gradients non-finite; nothing is patch-local here"""
    x, gy = _patches(P, 1, *hw, P + hw[1])
    net = copy.deepcopy(resnet).train(True)
    native = {"rn_net.fwd_side_stream", "rn_net.bwd_side_stream"}
    must = {stem, "rn_conv.spec2", "rn_wgrad.bk32"} | (native if path == "bf16x3" else set())
    _encoder_case(hip, f"Resnet train {hw} P={P} {path}", net, path, x, gy, nf.patch_poisons(P), must,
                  () if path == "bf16x3" else native, local=False)


@pytest.mark.parametrize("hw,P,stem", RN_SIZES, ids=RN_IDS)
def test_resnet_train_mode_no_grad(hip, resnet, hw, P, stem):
    """crw_rn_train_fwd_nograd (train-mode BatchNorm under torch.no_grad): as train mode"""
    x, _ = _patches(P, 1, *hw, P + hw[1])
    net = copy.deepcopy(resnet).train(True)
    _encoder_case(hip, f"Resnet train, no_grad {hw} P={P}", net, "bf16x3", x, None, nf.patch_poisons(P),
                  {stem, "rn_net.fwd_side_stream", "rn_conv.spec2"}, ("rn_net.bwd_side_stream", "rn_wgrad.bk32"), local=False)


@pytest.mark.parametrize("hw,P,stem", RN_SIZES, ids=RN_IDS)
def test_resnet_eval_mode(hip, resnet, hw, P, stem):
    """crw_rn_eval_fwd on finite running statistics: patch-local -- the poisoned patches non-finite, the rest bit-equal to the
    clean run"""
    x, _ = _patches(P, 1, *hw, P + hw[1])
    net = copy.deepcopy(resnet).train(False)
    _encoder_case(hip, f"Resnet eval {hw} P={P}", net, "bf16x3", x, None, nf.patch_poisons(P),
                  {stem, "rn_net.fwd_side_stream", "rn_conv.spec2"}, ("rn_net.bwd_side_stream", "rn_wgrad.bk32"))


# ------------------------------------------------------------------------------------------------ affinity and walk
TAU = 0.07
# (B, T, N, C) -> forward route, backward route of the affinity (the selectors' rules: tests/test_routes_gpu.py AFFINITY)
WALK_SHAPES = {
    (3, 4, 7, 8): ("affinity.fwd_f32_t64", "gemm_f32.edge"),                   # the oracle's case of tests/test_nonfinite.py
    (3, 4, 63, 128): ("affinity.fwd_f32_t64", "affinity.bwd_f32_t64_elem"),      # persistent small-N chain; statistics written directly
    (3, 4, 130, 64): ("affinity.fwd_f32_t128", "affinity.bwd_f32_t128_elem"),    # two tiles: merged partials on the fp32 MFMA
    (3, 4, 260, 32): ("affinity.fwd_bf16x6", "affinity.bwd_f32_t128"),           # bf16-split affinity from 256 nodes on; ragged tile
}
CHAINS = (0, 2, 1)                                                               # fp32, bf16x3, bf16: every N offers all three


def _emb(B, T, N, C):
    g = torch.Generator().manual_seed(N + C)
    return (torch.randn(1, 1, N, C, generator=g) + 0.6 * torch.randn(B, T, N, C, generator=g)).float()


def _walk_run(hip, emb, chain, imported):
    """crw_affinity_fwd -> crw_walk_fwd -> crw_walk_bwd (gloss 1, like the oracle) -> crw_affinity_bwd"""
    def run():
        A, ehat, norm, stats = hip.affinity_fwd(emb.cuda(), TAU)
        loss, state, At = hip.walk_fwd(A, chain=chain, want_At=True, stats=stats if imported else None)
        dA = hip.walk_bwd(torch.ones((), dtype=torch.float32, device="cuda"), A, state, chain=chain)
        demb = hip.affinity_bwd(dA, ehat, norm, TAU)
        return dict(A=A, ehat=ehat, norm=norm.reshape(emb.shape[:3]), stats=stats, loss=loss.reshape(1), At=At, dA=dA, demb=demb)
    out, hit = took(hip, run)
    return {k: v.cpu() for k, v in out.items()}, hit


def _walk_routes(shape, chain, imported, hit):
    B, T, N, C = shape
    fwd, bwd = WALK_SHAPES[shape]
    small = chain == 0 and N <= 64                                               # padded to 32 / 64: the persistent chain
    must = {fwd, bwd, "walk.fwd_persistent" if small else "walk.fwd_gemm", "walk.bwd_persistent" if small else "walk.bwd_gemm"}
    must |= {"gemm_f32.t32"} if chain == 0 else {"gemm_bf16.t128"}
    must |= {"chain_small.n32" if N <= 32 else "chain_small.n64"} if small else set()
    assert must <= hit and ("softmax.stats_import" in hit) == imported, (shape, chain, imported, sorted(hit))


_CLEAN = {}


def _clean_run(hip, shape, chain, imported):
    key = (shape, chain, imported)
    if key not in _CLEAN:
        _CLEAN[key], _ = _walk_run(hip, _emb(*shape), chain, imported)
        assert all(int(nf.nonfinite(v).sum()) == 0 for v in _CLEAN[key].values()), key
    return _CLEAN[key]


@pytest.mark.parametrize("frame", [0, 1, -1], ids=["t0", "t1", "tlast"])
@pytest.mark.parametrize("shape", list(WALK_SHAPES), ids=[f"N{s[2]}-C{s[3]}" for s in WALK_SHAPES])
def test_affinity_and_walk(hip, shape, frame):
    """one entry of emb[1, t, n] poisoned with NaN, +inf, -inf; every chain arithmetic; statistics from the affinity epilogue and
    statistics the walk computes.  A and the loss: the oracle's masks exactly (t = T-1: the last logit matrix feeds no cycle -- a
    finite loss, the clean run's bits); ehat, norm, At, dA, demb: supersets; a row / column of A with a non-finite logit has a
    non-finite sum statistic; items 0 and 2 bit-equal to the clean run."""
    B, T, N, C = shape
    t, n, c = frame % T, N // 2, C - 3
    emb = _emb(*shape)
    misses = []
    for v in nf.VALUES:
        bad = nf.poison_entry(emb, (1, t, n, c), v)
        o = nf.oracle_run(bad.numpy(), TAU)
        assert np.isnan(o["loss"]) == (t != T - 1), (t, v, o["loss"])                # (pinned in tests/test_nonfinite.py)
        A_bad = nf.nonfinite(o["A"])
        for chain in CHAINS:
            for imported in (True, False):
                tag = f"{v} chain {chain} {'imported' if imported else 'own'} statistics"
                clean = _clean_run(hip, shape, chain, imported)
                got, hit = _walk_run(hip, bad, chain, imported)
                _walk_routes(shape, chain, imported, hit)
                misses.append((f"{tag}: A mask differs", nf.mask_differences(o["A"], got["A"])))
                misses.append((f"{tag}: loss mask differs", nf.mask_differences(o["loss"], got["loss"][0])))
                if t == T - 1:
                    misses.append((f"{tag}: loss is not the clean run's", nf.changed_bits(got["loss"], clean["loss"])))
                for k in ("ehat", "norm", "At", "dA", "demb"):
                    misses.append((f"{tag}: {k} laundered", nf.superset_misses(o[k], got[k])))
                for k in ("A", "At", "dA", "demb"):
                    misses.append((f"{tag}: {k} of items 0, 2 changed", nf.changed_bits(got[k], clean[k], [0, 2])))
                misses.append((f"{tag}: row sum finite", nf.superset_misses(nf.as_values(A_bad.any(-1)), got["stats"][1])))
                misses.append((f"{tag}: column sum finite", nf.superset_misses(nf.as_values(A_bad.any(-2)), got["stats"][3])))
    _report(f"walk {shape} frame {t}", misses)


def _fp64_affinity(emb, dA):
    """the fp64 expression of test_hip_parity.test_affinity_tiles_and_fused_statistics -> (ehat, norm, A, demb)"""
    e = emb.double()
    nrm = e.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    eh = e / nrm
    A = torch.einsum("btnc,btmc->btnm", eh[:, :-1], eh[:, 1:]) / TAU
    deh = torch.zeros_like(eh)
    deh[:, :-1] += torch.einsum("btnm,btmc->btnc", dA.double(), eh[:, 1:]) / TAU
    deh[:, 1:] += torch.einsum("btnm,btnc->btmc", dA.double(), eh[:, :-1]) / TAU
    return eh, nrm[..., 0], A, (deh - eh * (eh * deh).sum(-1, keepdim=True)) / nrm


def _affinity_edge(hip, shape, emb):
    B, T, N, C = shape
    dA = torch.randn(B, T - 1, N, N, generator=torch.Generator().manual_seed(N)).float()

    def run():
        A, ehat, norm, stats = hip.affinity_fwd(emb.cuda(), TAU)
        only = hip.normalize(emb.cuda())                                           # crw_normalize: the same rows, no norm output
        return A, ehat, norm.reshape(B, T, N), stats, hip.affinity_bwd(dA.cuda(), ehat, norm, TAU), only
    (A, ehat, norm, stats, demb, only), hit = took(hip, run)
    assert set(WALK_SHAPES[shape]) <= hit, sorted(hit)
    assert torch.equal(only, ehat)
    return [v.cpu() for v in (A, ehat, norm, stats, demb)] + list(_fp64_affinity(emb, dA))


@pytest.mark.parametrize("shape", list(WALK_SHAPES), ids=[f"N{s[2]}-C{s[3]}" for s in WALK_SHAPES])
def test_zero_row_is_finite_and_exact(hip, shape):
    """an all-zero embedding row (the eps = 1e-12 branch of the norm): everything finite; A, the statistics and demb against fp64 at
    the tolerances of test_affinity_tiles_and_fused_statistics -- demb of the zero row (1e12 times the others: / 1e-12) scaled by its
    own maximum, the other rows by theirs; the walk on those logits finite too"""
    B, T, N, C = shape
    emb = _emb(*shape)
    emb[1, 1, N // 2] = 0.0
    A, ehat, norm, stats, demb, eh, nrm, A_ref, want = _affinity_edge(hip, shape, emb)
    assert all(int(nf.nonfinite(v).sum()) == 0 for v in (A, ehat, norm, stats, demb))
    assert norm[1, 1, N // 2].item() == np.float32(1e-12) and torch.count_nonzero(ehat[1, 1, N // 2]).item() == 0
    torch.testing.assert_close(A.double(), A_ref, rtol=1e-5, atol=2e-5 / TAU * 1e-1)
    Ad = A.double()
    rmax, cmax = Ad.max(-1).values, Ad.max(-2).values
    rsum, csum = (Ad - rmax[..., None]).exp().sum(-1), (Ad - cmax[..., None, :]).exp().sum(-2)
    for got, ref in zip(stats, (rmax, rsum, cmax, csum)):
        torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=1e-6)
    zero = torch.zeros(B, T, N, dtype=torch.bool)
    zero[1, 1, N // 2] = True
    assert want[zero].abs().max() > 1e9 * want[~zero].abs().max()
    for rows in (zero, ~zero):
        torch.testing.assert_close(demb.double()[rows], want[rows], rtol=1e-4, atol=1e-4 * want[rows].abs().max().item())
    for chain in CHAINS:
        got, hit = _walk_run(hip, emb, chain, True)
        _walk_routes(shape, chain, True, hit)
        assert all(int(nf.nonfinite(v).sum()) == 0 for v in got.values()), chain


@pytest.mark.parametrize("shape", list(WALK_SHAPES), ids=[f"N{s[2]}-C{s[3]}" for s in WALK_SHAPES])
def test_rows_scaled_by_two_to_the_40(hip, shape):
    """one row times 2^40 and one times 2^-40 (exact in fp32; the squares, 2^+-80, are far inside its range): a sum of squares that
    overflows or flushes where it need not shows here.  ehat (entries of a unit vector: the logits' bound at tau = 1) and A against
    fp64 at the tolerances of test_affinity_tiles_and_fused_statistics; the norm, scaled back, at that test's rtol."""
    B, T, N, C = shape
    emb = _emb(*shape)
    big, small = (0, 1, N // 3), (2, 2, N - 1)
    emb[big] *= 2.0 ** 40
    emb[small] *= 2.0 ** -40
    A, ehat, norm, stats, demb, eh, nrm, A_ref, want = _affinity_edge(hip, shape, emb)
    assert all(int(nf.nonfinite(v).sum()) == 0 for v in (A, ehat, norm, stats, demb))
    torch.testing.assert_close(ehat.double(), eh, rtol=1e-5, atol=2e-5 * 1e-1)
    torch.testing.assert_close(A.double(), A_ref, rtol=1e-5, atol=2e-5 / TAU * 1e-1)
    scale = torch.ones(B, T, N, dtype=torch.float64)
    scale[big], scale[small] = 2.0 ** -40, 2.0 ** 40
    torch.testing.assert_close(norm.double() * scale, nrm * scale, rtol=1e-5, atol=0.0)


# ------------------------------------------------------------------------------------------------ whole model
def test_whole_model_loss_and_gradients(hip, cnn):
    """model.CRW(CNN) on [B=2, T=4, N=7, 16, 16].  One NaN pixel in a frame that feeds the cycles: loss NaN and every gradient
    entirely non-finite.  The NaN in the last frame only: the loss finite, the clean run's bits."""
    import model
    B, T, N = 2, 4, 7
    seq = torch.randn(B, T, N, 16, 16, generator=torch.Generator().manual_seed(11))
    must = {"front.fwd_nt512", "conv.chain", "affinity.fwd_f32_t64", "walk.fwd_persistent", "chain_small.n32", "softmax.stats_import"}

    def step(s):
        net = model.CRW(_gpu(cnn, "bf16x3"), 0.05, False).cuda()
        loss, _ = net(s.cuda())
        loss.backward()
        return loss.detach().reshape(1), {k: p.grad for k, p in net.named_parameters()}
    (loss0, g0), hit = took(hip, step, seq)
    assert must | {"front.bwd_saved", "walk.bwd_persistent"} <= hit, sorted(hit)
    assert int(nf.nonfinite(loss0).sum()) == 0 and all(int(nf.nonfinite(g).sum()) == 0 for g in g0.values())
    bad = seq.clone()
    bad[1, 1, 3, 8, 8] = float("nan")
    (loss1, g1), hit = took(hip, step, bad)
    assert must <= hit, sorted(hit)
    misses = [("loss finite", 1 - int(nf.nonfinite(loss1).sum()))]
    misses += [(f"d {k}: finite entries", int((~nf.nonfinite(g)).sum())) for k, g in g1.items()]
    last = seq.clone()
    last[1, T - 1, 3, 8, 8] = float("nan")
    (loss2, _), hit = took(hip, step, last)
    assert must <= hit, sorted(hit)
    misses.append(("NaN in the last frame: loss is not the clean run's", nf.changed_bits(loss2, loss0)))
    _report("CRW(CNN)", misses)


# ------------------------------------------------------------------------------------------------ Adam
def test_adam_step_is_elementwise(hip):
    """crw_adam_step (one kernel, no selector: no route to name) on n = 4 * 256 + 3: the float4 body and the scalar tail.  Gradient NaN
    at index 0, +inf in the last full quad, NaN in the tail, in the first of two steps: the masks of p, m, v equal torch.optim.Adam's
    on the CPU, every other element bit-equal to the clean run"""
    n = 4 * 256 + 3
    g = torch.Generator().manual_seed(9)
    p, g1, g2 = (torch.randn(n, generator=g) for _ in range(3))
    bad = {0: "nan", 4 * 256 - 2: "+inf", n - 2: "nan"}
    g1p = g1.clone()
    for i, v in bad.items():
        g1p[i] = nf.VALUES[v]

    def run(grads):
        q, m, v = p.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
        for step, gr in enumerate(grads, start=1):
            hip.adam_step(q, gr.cuda(), m, v, step, 1e-3)
        return q, m, v
    clean, hit0 = took(hip, run, [g1, g2])
    got, hit1 = took(hip, run, [g1p, g2])
    assert not hit0 and not hit1, (sorted(hit0), sorted(hit1))
    ref = nf.adam_reference(p, [g1p, g2])
    assert all(sorted(torch.nonzero(nf.nonfinite(r)).flatten().tolist()) == sorted(bad) for r in ref)
    misses = []
    for name, r, a, c in zip("pmv", ref, got, clean):
        assert int(nf.nonfinite(c).sum()) == 0
        misses.append((f"{name}: mask differs", nf.mask_differences(r, a)))
        misses.append((f"{name}: other elements changed", nf.changed_bits(a, c, nf.others(n, bad))))
    _report("crw_adam_step", misses)
