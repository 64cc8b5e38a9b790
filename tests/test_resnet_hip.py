"""GPU tests of the Resnet encoder kernels (crw_rn_*, through the C ABI): every kernel against fp64 PyTorch on the same operand
values (the bf16 hi + lo pairs the kernels actually read), then the whole encoder -- forward, backward, BatchNorm running
statistics -- against PyTorch's own modules and against the reference's recorded training step (fixture resnet_train_*)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    return crw_hip


def planes(hip, x_nchw):
    """fp32 [P,C,H,W] -> (hi, lo) planes [Ppad, H*W*C] and the fp64 values they hold, back in NCHW"""
    P, C, H, W = x_nchw.shape
    flat = x_nchw.permute(0, 2, 3, 1).reshape(P, H * W * C).contiguous()
    hi, lo = hip.rn_split(flat, P, H * W * C)
    val = (hi[:P].double() + lo[:P].double()).reshape(P, H, W, C).permute(0, 3, 1, 2).contiguous()
    assert not hi[P:].any() and not lo[P:].any()
    return (hi, lo), val


def wvals(w):
    """the values of a weight after the hi/lo split"""
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi.double() + lo.double()


def nhwc(out, P, H, W, C):
    return out[:P].reshape(P, H, W, C).permute(0, 3, 1, 2)


CONVS = [  # Hin, Win, Cin, Cout, k, stride, pad
    (5, 5, 64, 64, 3, 1, 1), (5, 5, 64, 128, 3, 2, 1), (3, 3, 128, 128, 3, 1, 1), (5, 5, 64, 128, 1, 2, 0),
    (3, 3, 128, 256, 3, 2, 1), (2, 2, 256, 256, 3, 1, 1), (2, 2, 256, 512, 3, 2, 1), (1, 1, 512, 512, 3, 1, 1),
    (2, 2, 256, 512, 1, 2, 0), (1, 1, 512, 128, 1, 1, 0), (4, 6, 64, 64, 3, 1, 1),
    # 32 x 32 patches (scripts/test/test_mc1.py:19): maps 9 -> 9 -> 5 -> 3 -> 2, then the head over the 2 x 2 map as ONE product whose
    # kernel covers the map (global average pool + linear, src/encoder.py:264-266); a 1 x 3 final map (16 x 80 patches) likewise
    (9, 9, 64, 64, 3, 1, 1), (9, 9, 64, 128, 3, 2, 1), (5, 5, 128, 256, 3, 2, 1), (3, 3, 256, 512, 3, 2, 1), (2, 2, 512, 512, 3, 1, 1),
    (2, 2, 512, 128, (2, 2), 1, 0), (1, 3, 512, 128, (1, 3), 1, 0),
    # the row-per-workgroup kernel of the 64 -> 64 layers (csrc/resnet_gemm.hip rn_conv_row_kernel): one-pixel / one-row / two-row maps,
    # a row in three chunks, a chunk of one output
    (1, 1, 64, 64, 3, 1, 1), (1, 7, 64, 64, 3, 1, 1), (2, 3, 64, 64, 3, 1, 1), (3, 11, 64, 64, 3, 1, 1), (6, 2, 64, 64, 3, 1, 1),
    (3, 21, 64, 64, 3, 1, 1)]


@pytest.mark.parametrize("geo", CONVS)
@pytest.mark.parametrize("P", [200, 128])
def test_rn_conv_forward_backward_wgrad_match_torch(hip, geo, P):
    Hin, Win, Cin, Cout, k, s, pad = geo
    kh, kw = k if isinstance(k, tuple) else (k, k)
    Hout, Wout = (Hin + 2 * pad - kh) // s + 1, (Win + 2 * pad - kw) // s + 1
    g = torch.Generator().manual_seed(Hin * 100 + Cin + kh + s)
    x = torch.randn(P, Cin, Hin, Win, generator=g).cuda()
    w = (torch.randn(Cout, Cin, kh, kw, generator=g) / (Cin * kh * kw) ** 0.5).cuda()
    bias = torch.randn(Cout, generator=g).cuda() if Hout * Wout == 1 and Cout == 128 else None
    k = (kh, kw)
    dy = torch.randn(P, Cout, Hout, Wout, generator=g).cuda()
    xp, xv = planes(hip, x)
    dp, dv = planes(hip, dy)
    wp = hip.rn_pack_conv(w)
    wv = wvals(w)
    xv.requires_grad_(True)
    wv.requires_grad_(True)
    ref = TF.conv2d(xv, wv, bias.double() if bias is not None else None, stride=s, padding=pad)
    gx, gw = torch.autograd.grad(ref, (xv, wv), dv)
    scale = ref.abs().max().item()

    out, part = hip.rn_conv(hip.RN_FWD, P, (Hin, Win, Cin), (Hout, Wout), Cout, k, s, pad, xp, wp[:2], bias=bias, stats=True)
    got = nhwc(out, P, Hout, Wout, Cout).double()
    torch.testing.assert_close(got, ref.detach(), rtol=1e-4, atol=2e-5 * scale)
    if bias is None:
        assert not out[P:].any(), "rows of the padding patches must stay zero"
        # per-tile statistics: their sum over tiles and pixels = column sums / sums of squares over (patches, pixels)
        pt = part.reshape(-1, Hout * Wout, Cout, 2).double().sum((0, 1))
        torch.testing.assert_close(pt[:, 0], ref.detach().sum((0, 2, 3)), rtol=1e-4, atol=1e-3 * scale)
        torch.testing.assert_close(pt[:, 1], (ref.detach() ** 2).sum((0, 2, 3)), rtol=1e-4, atol=1e-3 * scale)

    gin, _ = hip.rn_conv(hip.RN_BWD, P, (Hout, Wout, Cout), (Hin, Win), Cin, k, s, pad, dp, wp[2:])
    torch.testing.assert_close(nhwc(gin, P, Hin, Win, Cin).double(), gx, rtol=1e-4, atol=2e-5 * gx.abs().max().item())
    assert not gin[P:].any()

    dw = hip.rn_wgrad(hip.RN_FWD, P, (Hin, Win, Cin), (Hout, Wout, Cout), k, s, pad, xp, dp)
    torch.testing.assert_close(dw.double(), gw, rtol=1e-4, atol=2e-5 * gw.abs().max().item())


class _Stem(torch.nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.fc0 = torch.nn.Conv2d(cin, 3, 1, padding=1)
        self.bn0 = torch.nn.BatchNorm2d(3)
        self.conv1 = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)

    def forward(self, x):
        return self.conv1(torch.relu(self.bn0(self.fc0(x))))


@pytest.mark.parametrize("cin,P", [(1, 200), (2, 130)])
def test_rn_stem_matches_torch(hip, cin, P):
    """fc0 + bn0 (batch statistics from the input moments) + relu0 + the 7x7/2 convolution, forward and backward, against
    fp64 PyTorch modules with the same parameters; bn0's running statistics against nn.BatchNorm2d's update."""
    torch.manual_seed(5 + cin)
    net = _Stem(cin).cuda()
    with torch.no_grad():
        net.bn0.weight.copy_(torch.tensor([0.8, -1.2, 1.5]))
        net.bn0.bias.copy_(torch.tensor([0.3, 0.1, -0.2]))
    ref_net = _Stem(cin).cuda().double()
    ref_net.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in net.state_dict().items()})
    x = torch.randn(P, cin, 16, 16).cuda() * 1.5 + 0.3
    dy = torch.randn(P, 64, 9, 9).cuda()

    ref_net.train()
    y_ref = ref_net(x.double())
    y_ref.backward(dy.double())

    wstem = hip.rn_pack_stem(net.conv1.weight, 16, 16)
    xmap, stem = hip.rn_stem_fwd(x, net.fc0, net.bn0, 24, 24, 0.1)
    torch.testing.assert_close(net.bn0.running_mean.double(), ref_net.bn0.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(net.bn0.running_var.double(), ref_net.bn0.running_var, rtol=1e-5, atol=1e-6)
    m = (xmap[0][:P].double() + xmap[1][:P].double()).reshape(P, 24, 24, 4)
    with torch.no_grad():
        a0 = torch.relu(ref_net.bn0(ref_net.fc0(x.double())))  # second call: running stats move again, the output does not
    torch.testing.assert_close(m[:, 3:21, 3:21, :3].permute(0, 3, 1, 2), a0, rtol=1e-4, atol=1e-5)
    assert not m[:, :3].any() and not m[:, 21:].any() and not m[:, :, :3].any() and not m[:, :, 21:].any() and not m[..., 3].any()
    assert not xmap[0][P:].any()

    Z1, part = hip.rn_conv(hip.RN_STEM_FWD, P, (24, 24, 4), (9, 9), 64, (7, 7), 2, 3, xmap, wstem[:2], stats=True)
    scale = y_ref.abs().max().item()
    torch.testing.assert_close(nhwc(Z1, P, 9, 9, 64).double(), y_ref.detach(), rtol=2e-4, atol=5e-5 * scale)

    dp, dv = planes(hip, dy)
    dw1 = hip.rn_wgrad(hip.RN_STEM_FWD, P, (24, 24, 4), (9, 9, 64), (7, 7), 2, 3, xmap, dp)
    gw = ref_net.conv1.weight.grad
    torch.testing.assert_close(dw1.double(), gw, rtol=2e-4, atol=5e-5 * gw.abs().max().item())

    dX0, _ = hip.rn_conv(hip.RN_STEM_BWD, P, (9, 9, 64), (18, 1), 64, (7, 7), 2, 3, dp, wstem[2:])
    dw0, db0, dg, db = hip.rn_stem_bwd(dX0, x, stem, net.fc0.weight.detach(), net.fc0.bias.detach())
    for got, ref in ((dg, ref_net.bn0.weight.grad), (db, ref_net.bn0.bias.grad)):
        torch.testing.assert_close(got.double(), ref, rtol=1e-3, atol=1e-4 * max(1.0, ref.abs().max().item()))
    # fc0.weight feeds a BatchNorm: with one input channel its gradient survives only through eps (y_hat depends on w through
    # w / sqrt(w^2 var + eps)), i.e. it is the difference of sums ~1e5 times larger -- ill-conditioned in any fp32-grade arithmetic
    ref = ref_net.fc0.weight.grad
    torch.testing.assert_close(dw0.double(), ref, rtol=2e-2, atol=2e-3 * max(1.0, ref.abs().max().item()))
    assert db0.abs().max().item() <= 1e-3 * max(1.0, dg.abs().max().item())  # fc0.bias feeds a BatchNorm: true gradient 0

    # the same layer on the patch-per-wave kernels (what training uses at 16 x 16): map in LDS only, fused backward sums
    rm0 = net.bn0.running_mean.clone()
    stem16 = hip.rn_stem_stats(x, net.fc0, net.bn0, 0.1)
    torch.testing.assert_close(stem16[:21], stem[:21], rtol=1e-6, atol=1e-7)
    assert not torch.equal(rm0, net.bn0.running_mean)  # a second momentum step on the running statistics, like a second forward
    wf, wt = hip.rn_pack_stem16(net.conv1.weight)
    Z16, part16 = hip.rn_stem16_fwd(x, stem, wf)
    torch.testing.assert_close(nhwc(Z16, P, 9, 9, 64).double(), y_ref.detach(), rtol=2e-4, atol=5e-5 * scale)
    pt = part16.double().sum(0)  # sums of P * 81 values that each carry ~1e-5 of relative error: tolerance per sample, not per sum
    torch.testing.assert_close(pt[:, 0], y_ref.detach().sum((0, 2, 3)), rtol=1e-4, atol=1e-6 * P * 81 * scale)
    torch.testing.assert_close(pt[:, 1], (y_ref.detach() ** 2).sum((0, 2, 3)), rtol=1e-4, atol=1e-6 * P * 81 * scale * scale)
    dw16 = hip.rn_stem16_wgrad(x, stem, dp)
    torch.testing.assert_close(dw16.double(), gw, rtol=2e-4, atol=5e-5 * gw.abs().max().item())
    dw0b, db0b, dgb, dbb = hip.rn_stem16_bwd(x, stem, net.fc0.weight.detach(), net.fc0.bias.detach(), wt, dp)
    for got, ref in ((dgb, ref_net.bn0.weight.grad), (dbb, ref_net.bn0.bias.grad)):
        torch.testing.assert_close(got.double(), ref, rtol=1e-3, atol=1e-4 * max(1.0, ref.abs().max().item()))
    ref = ref_net.fc0.weight.grad
    torch.testing.assert_close(dw0b.double(), ref, rtol=2e-2, atol=2e-3 * max(1.0, ref.abs().max().item()))
    assert db0b.abs().max().item() <= 1e-3 * max(1.0, dgb.abs().max().item())


@pytest.mark.parametrize("C,npix,P,mode", [(64, 25, 200, "plain"), (128, 9, 130, "shortcut"), (64, 25, 200, "identity"),
                                           (512, 1, 300, "shortcut"), (256, 4, 128, "plain")])
def test_rn_batchnorm_kernels_match_torch(hip, C, npix, P, mode):
    """statistics (from per-tile partials), apply (+ shortcut BatchNorm | identity), backward: against nn.BatchNorm in fp64"""
    g = torch.Generator().manual_seed(C + npix)
    Ppad = hip.rn_padded(P)
    z = (torch.randn(P, npix, C, generator=g) * 2 + 0.5).cuda()
    zd = (torch.randn(P, npix, C, generator=g) * 0.7 - 0.2).cuda()
    res = torch.randn(P, npix, C, generator=g).cuda()
    gup = torch.randn(P, npix, C, generator=g).cuda()
    gup2 = torch.randn(P, npix, C, generator=g).cuda()

    def padrows(t):
        out = torch.zeros(Ppad, npix * C, device="cuda")
        out[:P] = t.reshape(P, -1)
        return out

    def make_part(t):  # what the convolution epilogue writes: per (128-row tile half, pixel) column sums
        zp = padrows(t).reshape(Ppad // 64, 64, npix, C)
        return torch.stack([zp.sum(1), (zp * zp).sum(1)], -1).contiguous().reshape(-1)

    bn, bnd = torch.nn.BatchNorm2d(C).cuda(), torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        for b_ in (bn, bnd):
            b_.weight.copy_(torch.rand(C, generator=g) + 0.5)
            b_.bias.copy_(torch.randn(C, generator=g) * 0.3)
    ref_bn, ref_bnd = torch.nn.BatchNorm2d(C).cuda().double(), torch.nn.BatchNorm2d(C).cuda().double()
    ref_bn.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    ref_bnd.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bnd.state_dict().items()})
    to4 = lambda t: t.double().reshape(P, npix, 1, C).permute(0, 3, 1, 2)  # [P,C,npix,1]
    zr, zdr = to4(z).requires_grad_(True), to4(zd).requires_grad_(True)
    resv = None
    y = ref_bn(zr)
    if mode == "shortcut":
        y = y + ref_bnd(zdr)
    elif mode == "identity":
        rp, resv = planes(hip, res.reshape(P, npix, 1, C).permute(0, 3, 1, 2).contiguous())
        resv = resv.requires_grad_(True)
        y = y + resv
    y = torch.relu(y)
    y.backward(to4(gup) + to4(gup2))

    coef = hip.rn_bn_stats(make_part(z), P, npix, bn, 0.1)
    torch.testing.assert_close(bn.running_mean.double(), ref_bn.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(bn.running_var.double(), ref_bn.running_var, rtol=1e-5, atol=1e-6)
    coefd = hip.rn_bn_stats(make_part(zd), P, npix, bnd, 0.1) if mode == "shortcut" else None
    Z, Zd = padrows(z), padrows(zd) if mode == "shortcut" else None
    yh, yl = hip.rn_bn_apply(Z, coef, P, npix, C, Zd=Zd, coef_d=coefd, res=rp if mode == "identity" else None)
    got = (yh[:P].double() + yl[:P].double()).reshape(P, npix, 1, C).permute(0, 3, 1, 2)
    torch.testing.assert_close(got, y.detach(), rtol=1e-4, atol=1e-4)
    assert not yh[P:].any() and not yl[P:].any()

    dz, dzd, gres, dg, db, dgd, dbd = hip.rn_bn_bwd(padrows(gup), padrows(gup2), yh, Z, coef, P, npix, C, Zd=Zd, coef_d=coefd,
                                                    want_g=(mode == "identity"))
    val = lambda pl: (pl[0][:P].double() + pl[1][:P].double()).reshape(P, npix, 1, C).permute(0, 3, 1, 2)
    tol = dict(rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(val(dz), zr.grad, **tol)
    torch.testing.assert_close(dg.double(), ref_bn.weight.grad, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(db.double(), ref_bn.bias.grad, rtol=2e-4, atol=2e-3)
    assert not dz[0][P:].any()
    if mode == "shortcut":
        torch.testing.assert_close(val(dzd), zdr.grad, **tol)
        torch.testing.assert_close(dgd.double(), ref_bnd.weight.grad, rtol=2e-4, atol=2e-3)
        torch.testing.assert_close(dbd.double(), ref_bnd.bias.grad, rtol=2e-4, atol=2e-3)
    if mode == "identity":
        torch.testing.assert_close(gres[:P].double().reshape(P, npix, 1, C).permute(0, 3, 1, 2), resv.grad, **tol)


@pytest.mark.parametrize("P,H,W", [(130, 9, 9), (64, 9, 9), (70, 7, 6)])
def test_rn_pool_kernels_match_torch(hip, P, H, W):
    """relu(bn(z)) -> 3x3/2 max-pool, forward and backward (arg-max routing from the recorded codes, relu gate, BatchNorm backward)"""
    g = torch.Generator().manual_seed(P)
    C, Ppad = 64, hip.rn_padded(P)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    z = (torch.randn(P, H * W, C, generator=g) * 1.5).cuda()
    d1 = torch.randn(P, Ho * Wo, C, generator=g).cuda()
    d2 = torch.randn(P, Ho * Wo, C, generator=g).cuda()
    bn = torch.nn.BatchNorm2d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g))  # negative scales too: the pool does not commute with them
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    ref_bn = torch.nn.BatchNorm2d(C).cuda().double()
    ref_bn.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    zr = z.double().reshape(P, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = TF.max_pool2d(torch.relu(ref_bn(zr)), 3, 2, 1)
    y.backward((d1 + d2).double().reshape(P, Ho, Wo, C).permute(0, 3, 1, 2))

    Z = torch.zeros(Ppad, H * W * C, device="cuda")
    Z[:P] = z.reshape(P, -1)
    zp = Z.reshape(Ppad // 64, 64, H * W, C)
    part = torch.stack([zp.sum(1), (zp * zp).sum(1)], -1).contiguous().reshape(-1)
    coef = hip.rn_bn_stats(part, P, H * W, bn, 0.1)
    (yh, yl), amax = hip.rn_bn_pool(Z, coef, P, H, W, C)
    got = (yh[:P].double() + yl[:P].double()).reshape(P, Ho, Wo, C).permute(0, 3, 1, 2)
    torch.testing.assert_close(got, y.detach(), rtol=1e-4, atol=1e-4)
    assert not yh[P:].any()

    padp = lambda t: torch.cat([t.reshape(P, -1), torch.zeros(Ppad - P, Ho * Wo * C, device="cuda")])
    dz, dg, db = hip.rn_pool_bwd(padp(d1), padp(d2), amax, Z, coef, P, H, W, C)
    gotdz = (dz[0][:P].double() + dz[1][:P].double()).reshape(P, H, W, C).permute(0, 3, 1, 2)
    torch.testing.assert_close(gotdz, zr.grad, rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(dg.double(), ref_bn.weight.grad, rtol=2e-4, atol=2e-3)
    torch.testing.assert_close(db.double(), ref_bn.bias.grad, rtol=2e-4, atol=2e-3)
    assert not dz[0][P:].any() and not dz[1][P:].any()


def _no_library_convs(monkeypatch):
    """any PyTorch convolution / batch-norm call raises: the HIP path must not touch MIOpen"""
    def boom(*a, **k):
        raise AssertionError("a PyTorch convolution / batch_norm ran on the HIP Resnet path")
    monkeypatch.setattr(torch.nn.functional, "conv2d", boom)
    monkeypatch.setattr(torch.nn.functional, "batch_norm", boom)
    monkeypatch.setattr(torch.nn.functional, "max_pool2d", boom)
    monkeypatch.setattr(torch.nn.Conv2d, "_conv_forward", boom)


def _device_decisions(enc_stepwise, x):
    """The discrete choices of the device's forward pass: the max-pool's arg-max code per window and every ReLU gate, read from
    what the Python-driven schedule (`resnet_hip.HipResnetFn`, bit for bit the forward of the native pass -- asserted by
    test_resnet_native_and_stepwise_paths_agree) saves for its backward.  Gates are `hi plane > 0`, exactly what the backward
    kernels test."""
    P = x.shape[0]
    y = enc_stepwise(x)
    sv = y.grad_fn.sv  # the autograd node of a custom Function is its ctx
    _, _, _, _, _, _, H1, W1, H2, W2, _, _ = sv["geo"]

    def gate(plane_hi, h, w, C):
        return (plane_hi[:P].float() > 0).reshape(P, h, w, C).permute(0, 3, 1, 2).double()

    dec = {"amax": sv["amax"][:P].reshape(P, H2 * W2, 64).permute(0, 2, 1).long(),  # [P, C, Ho*Wo], code = ky * 3 + kx
           "pool": gate(sv["recs"][0]["Ain"][0], H2, W2, 64), "a": [], "out": []}
    for b, r in zip(sv["blocks"], sv["recs"]):
        dec["a"].append(gate(r["Aa"][0], b.hout, b.wout, b.cout))
        dec["out"].append(gate(r["Aout"][0], b.hout, b.wout, b.cout))
    return dec


def _teacher_forced_forward(ref, x64, dec):
    """`ref` (the fp64 PyTorch modules) with the device's discrete choices imposed: ReLU = multiplication by the recorded gate,
    max-pool = the recorded window position.  Everything else (convolutions, train-mode BatchNorm on fp64 batch statistics,
    average pool, head) is the module's own arithmetic.  Where the device's choice differs from the one fp64 would make, the two
    candidates are within the arithmetic's ~1e-5 of each other (that is what a flip is), so the forward values move by that much;
    the gradients then take the SAME routes on both sides and must agree entry by entry."""
    body = ref.model
    h = ref.relu0(ref.bn0(ref.fc0(x64)))  # the stem's gate feeds activations ~0 into the 7x7 product: not a routing decision
    z1 = body.bn1(body.conv1(h))
    P, C, H1, W1 = z1.shape
    Ho, Wo = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
    win = TF.unfold(TF.pad(z1, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(P, C, 9, Ho * Wo)
    a = win.gather(2, dec["amax"][:, :, None, :]).reshape(P, C, Ho, Wo)
    assert torch.isfinite(a).all()  # the device never picks a padding position
    # how many of the device's choices differ from the ones this fp64 forward would make by itself (reported by the test)
    live = (a.detach() > 0).reshape(P, C, Ho * Wo)  # (an all-negative window passes no gradient whichever position is named)
    flips = {"argmax": int(((win.detach().argmax(2) != dec["amax"]) & live).sum()), "gates": int((live.reshape(a.shape).double() != dec["pool"]).sum())}
    a = a * dec["pool"]
    for i in range(4):
        m = getattr(body, f"layer{i + 1}")[0]
        za = m.bn1(m.conv1(a))
        aa = za * dec["a"][i]
        zb = m.bn2(m.conv2(aa))
        s = zb + (a if m.downsample is None else m.downsample(a))
        a = s * dec["out"][i]
        flips["gates"] += int(((za.detach() > 0).double() != dec["a"][i]).sum()) + int(((s.detach() > 0).double() != dec["out"][i]).sum())
    return body.fc(torch.flatten(body.avgpool(a), 1)), flips


@pytest.mark.parametrize("pos_embed,P,path,hw", [(False, 160, "bf16x3", (16, 16)), (True, 70, "bf16x3", (16, 16)), (False, 130, "stepwise", (16, 16)),
                                                  (False, 140, "bf16x3", (32, 32)), (True, 40, "stepwise", (32, 32)), (False, 70, "bf16x3", (20, 27)),
                                                  (False, 30, "bf16x3", (40, 64))])
def test_resnet_hip_matches_pytorch_modules(hip, monkeypatch, pos_embed, P, path, hw):
    """The whole encoder: HIP forward / backward / running statistics against the same module run on PyTorch ops in fp64.
    path "bf16x3" = the whole pass from native code (crw_rn_train_fwd / _bwd, what training uses), "stepwise" = the same
    kernels launched one by one from Python (resnet_hip.HipResnetFn).  Patch sizes: 16x16 (patch-per-wave stem, 1x1 final map),
    32x32 (the reference's cfg5 encoder input, scripts/test/test_mc1.py:19: gathered stem, 2x2 final map -> the average pool +
    head as one product over the map), 20x27 (stem rows over two column tiles, 1x1 final map), 40x64 (2x3 final map: `resnet_hip.final_map(40, 64)`).

    Two references.  FREE-RUNNING fp64 modules: features, running statistics, and direction + norm of every gradient (an fp32-grade
    forward and an fp64 one may pick different arg-max pixels / ReLU gates where two candidates differ by less than ~1e-5, which
    re-routes single gradient contributions: entry-wise equality is not defined against this reference).  TEACHER-FORCED fp64
    modules (the device's recorded arg-max codes and gates imposed on the fp64 forward, `_teacher_forced_forward`): EVERY entry of
    EVERY gradient within 5e-3 -- the proof that the entries the free-running comparison cannot hold are routing flips and
    nothing else."""
    import copy
    import encoder as crw_encoder
    torch.manual_seed(3)
    enc = crw_encoder.Resnet(pos_embed).cuda()
    with torch.no_grad():  # move the BatchNorm parameters off their 1 / 0 initial values
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.6, 1.4)
                m.bias.uniform_(-0.2, 0.2)
    ref = copy.deepcopy(enc).double()
    ref.hip_convs = None
    forced = copy.deepcopy(ref)
    probe = copy.deepcopy(enc)
    probe.hip_convs = "stepwise"
    enc.hip_convs = path
    x = torch.randn(P, 2 if pos_embed else 1, *hw).cuda()
    gy = torch.randn(P, 128).cuda()
    ref.train()
    y_ref = ref(x.double())
    y_ref.backward(gy.double())

    enc.train()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _no_library_convs(monkeypatch)
        y = enc(x)
        y.backward(gy)
        dec = _device_decisions(probe.train(), x)
    monkeypatch.undo()
    torch.testing.assert_close(y.double(), y_ref.detach(), rtol=2e-3, atol=2e-3 * y_ref.abs().max().item())
    forced.train()
    y_tf, flips = _teacher_forced_forward(forced, x.double(), dec)
    y_tf.backward(gy.double())
    # imposing the device's choices moves the fp64 forward by no more than the flips' own margins
    torch.testing.assert_close(y_tf.detach(), y_ref.detach(), rtol=1e-3, atol=1e-3 * y_ref.abs().max().item())
    print(f"routing decisions where the device and fp64 differ (P = {P}, {hw[0]}x{hw[1]}, {path}): {flips}")
    for (k, p), (_, q), (_, t) in zip(enc.named_parameters(), ref.named_parameters(), forced.named_parameters()):
        assert p.grad is not None, k
        if k == "fc0.bias":  # true gradient is zero (it feeds a BatchNorm); both sides hold rounding noise
            assert p.grad.abs().max().item() <= 1e-4 * max(1.0, enc.bn0.weight.grad.abs().max().item())
            continue
        a, b_, c_ = p.grad.double().flatten(), q.grad.flatten(), t.grad.flatten()
        # free-running reference: direction and norm (one flipped routing decision moves the 3-element gradients of the stem,
        # sums over everything, by up to ~1 %)
        cos = float(torch.dot(a, b_) / (a.norm() * b_.norm() + 1e-30))
        below_pool = k in ("fc0.weight", "bn0.weight", "bn0.bias", "model.conv1.weight", "model.bn1.weight", "model.bn1.bias")
        assert cos > 0.999 and abs(float(a.norm() / b_.norm()) - 1) < (3e-2 if below_pool else 1e-2), (k, cos, float(a.norm()), float(b_.norm()))
        # teacher-forced reference: every entry.  fc0.weight with ONE input channel survives only through BatchNorm's eps (the
        # difference of sums ~1e5 times larger, test_rn_stem_matches_torch): held to that kernel test's 2e-2
        tol = 2e-2 if (k == "fc0.weight" and not pos_embed) else 5e-3
        scale = max(c_.abs().max().item(), 1e-6)
        bad = (a - c_).abs() > tol * scale + tol * c_.abs()
        assert not bad.any(), (k, int(bad.sum()), a.numel(), float(((a - c_).abs() / (scale + c_.abs())).max()))
    for (k, b), (_, c) in zip(enc.named_buffers(), ref.named_buffers()):
        if b.is_floating_point():
            torch.testing.assert_close(b.double(), c, rtol=1e-3, atol=1e-5, msg=lambda m: f"{k}: {m}")
        else:
            assert int(b) == int(c) == 1, k


def test_resnet_step_at_bench_batch_matches_fp64(hip, monkeypatch):
    """One step of the native pass at the batch bench.py times (`--model 1`: P = 8 * 32 * 63 = 16128 patches = 126 tiles of 128,
    every patch slice and both streams in play) against the same modules in float64 on the GPU: features within 1e-4 of the
    feature scale, running statistics, every gradient's norm within 1 % and direction (cosine) -- entry-wise equality against a
    free-running reference is not defined (see test_resnet_hip_matches_pytorch_modules), so the teacher-forced reference is held
    beside it: every entry of every gradient within 5e-3 at this size too."""
    import copy
    import encoder as crw_encoder
    P = 8 * 32 * 63
    torch.manual_seed(16128)
    enc = crw_encoder.Resnet(False).cuda()
    ref = copy.deepcopy(enc).double()
    ref.hip_convs = None
    forced = copy.deepcopy(ref)
    probe = copy.deepcopy(enc)
    probe.hip_convs = "stepwise"
    g = torch.Generator(device="cuda").manual_seed(7)
    # radargram-like patches: a smooth layered term under the noise, so that features are not pure noise
    rows = torch.arange(16, device="cuda").float()[None, None, :, None]
    x = torch.randn(P, 1, 16, 16, generator=g, device="cuda") + torch.sin(rows * 0.4 + torch.rand(P, 1, 1, 1, generator=g, device="cuda") * 6.28)
    gy = torch.randn(P, 128, generator=g, device="cuda") / P
    y_ref = ref.train()(x.double())
    y_ref.backward(gy.double())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _no_library_convs(monkeypatch)
        y = enc.train()(x)
        y.backward(gy)
        dec = _device_decisions(probe.train(), x)
    monkeypatch.undo()
    fscale = y_ref.detach().abs().max().item()
    err = (y.double() - y_ref.detach()).abs().max().item()
    assert err <= 1e-4 * fscale, (err, fscale)
    y_tf, flips = _teacher_forced_forward(forced.train(), x.double(), dec)
    y_tf.backward(gy.double())
    print(f"P = {P}: feature error {err / fscale:.2e} of scale; routing decisions where the device and fp64 differ: {flips}")
    for (k, p), (_, q), (_, t) in zip(enc.named_parameters(), ref.named_parameters(), forced.named_parameters()):
        if k == "fc0.bias":
            continue
        a, b_, c_ = p.grad.double().flatten(), q.grad.flatten(), t.grad.flatten()
        cos = float(torch.dot(a, b_) / (a.norm() * b_.norm() + 1e-30))
        # fc0.weight with ONE input channel survives only through BatchNorm's eps (a difference of sums ~1e5 times larger,
        # test_rn_stem_matches_torch): 3 % there, 1 % everywhere else
        assert cos > 0.9999 and abs(float(a.norm() / b_.norm()) - 1) < (3e-2 if k == "fc0.weight" else 1e-2), (k, cos, float(a.norm()), float(b_.norm()))
        tol = 3e-2 if k == "fc0.weight" else 5e-3
        scale = max(c_.abs().max().item(), 1e-30)
        bad = (a - c_).abs() > tol * scale + tol * c_.abs()
        assert not bad.any(), (k, int(bad.sum()), a.numel(), float(((a - c_).abs() / (scale + c_.abs())).max()))
    for (k, b), (_, c) in zip(enc.named_buffers(), ref.named_buffers()):
        if b.is_floating_point():
            torch.testing.assert_close(b.double(), c, rtol=1e-4, atol=1e-6, msg=lambda m: f"{k}: {m}")


def test_resnet_native_and_stepwise_paths_agree(hip):
    """crw_rn_train_fwd / _bwd against the Python-driven schedule of the same kernels: the forward is the same sequence of
    launches (features and running statistics bit for bit); the native backward takes the BatchNorm-backward sums in the
    epilogues of the backward-data products and adds the second gradient of a junction there, i.e. other summation orders:
    gradients equal to fp32 rounding."""
    import copy
    import encoder as crw_encoder
    torch.manual_seed(9)
    a = crw_encoder.Resnet(False).cuda()
    b = copy.deepcopy(a)
    b.hip_convs = "stepwise"
    x = torch.randn(200, 1, 16, 16).cuda()
    gy = torch.randn(200, 128).cuda()
    ya, yb = a(x), b(x)
    ya.backward(gy)
    yb.backward(gy)
    assert torch.equal(ya, yb)
    for (k, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(p, q), k
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        if k == "fc0.bias":  # rounding noise around a true zero on both sides
            continue
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-3, atol=1e-4 * max(1e-6, q.grad.abs().max().item()), msg=lambda m: f"{k}: {m}")


@pytest.mark.parametrize("hw,ov", [((16, 16), 8), ((32, 32), 24)])
@pytest.mark.parametrize("train_mode", [True, False])
def test_resnet_inference_through_propagate(hip, monkeypatch, hw, ov, train_mode):
    """Inference as the reference runs it with its default encoder, under `torch.no_grad()`: never `.eval()`'d in
    scripts/test/test_all.py / test_mc1.py (32x32 patches, overlap 24: test_mc1.py:19,21) -- there the forward is bit for bit the
    forward of a training step, batch statistics and running-statistics update included --, `encoder.train(False)` in
    scripts/test/test.py:42 -- BatchNorm on the running statistics, nothing updated.  Both on the hand-written kernels (every
    PyTorch convolution / batch-norm entry point disabled), through `utils.propagate`; the label map against the oracle's label
    propagation on the device's features (teacher-forced fp64 audit: every disagreement must be a floating-point near-tie)."""
    import copy
    import encoder as crw_encoder
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    from oracle import crw_oracle as orc
    torch.manual_seed(5)
    T, N, M = 6, 20, 4
    h, w = hw
    a = crw_encoder.Resnet(False).cuda()
    g = torch.Generator().manual_seed(hw[0])
    rows = N * (h - ov) + ov
    rg = torch.sin(torch.arange(rows)[:, None] / 9.0 + 0.01 * torch.arange(T * w)[None, :]) + 0.5 * torch.randn(rows, T * w, generator=g)
    seq = torch.stack([torch.stack([rg[n * (h - ov):n * (h - ov) + h, t * w:(t + 1) * w] for n in range(N)]) for t in range(T)]).cuda()
    x = seq.reshape(T * N, 1, h, w)
    a(x).sum().backward()  # one training step's worth of running statistics
    a.train(train_mode)
    b = copy.deepcopy(a)
    cfg = dict(CXT_SIZE=4, RADIUS=5, TEMP=0.1, KNN=5)
    seg = (torch.arange(rows)[:, None] * M // rows).float().repeat(1, w).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _no_library_convs(monkeypatch)
        if train_mode:
            ya = a(x)
        with torch.no_grad():
            yb = b(x)
        stats = [v.clone() for v in b.buffers()]
        pred, xent, _ = crw_utils.propagate(seq, seg, b, LabelPropVOS_CRW(cfg), M, False, False)
    monkeypatch.undo()
    assert not yb.requires_grad
    if train_mode:
        assert torch.equal(ya.detach(), yb)
        for (k, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
            assert not torch.equal(p, q) or not p.is_floating_point(), k  # propagate() ran the forward once more: statistics moved on
    else:
        ref = copy.deepcopy(a).double()
        ref.hip_convs = None
        with torch.no_grad():
            y64 = ref(x.double())
        torch.testing.assert_close(yb.double(), y64, rtol=1e-3, atol=1e-4 * y64.abs().max().item())
        for u, v in zip(stats, b.buffers()):
            assert torch.equal(u, v)  # eval mode updates nothing
    assert pred.shape == (N, T) and xent.shape == (N, T - 1)
    assert torch.equal(pred[:, 0], crw_utils.seed_labels(seg, N))
    feats = hip.normalize(yb.reshape(T, N, -1).float().contiguous())
    if train_mode:  # propagate's own forward saw the same batch: the same features
        pred2, L = LabelPropVOS_CRW(cfg).propagate_all(feats, crw_utils.seed_labels(seg, N), M)
        assert torch.equal(pred, pred2)
        audit = orc.labelprop_tie_audit(feats.cpu().numpy(), L.cpu().numpy(), pred.cpu().numpy(), cfg["CXT_SIZE"], cfg["RADIUS"],
                                        cfg["TEMP"], cfg["KNN"], eps=1e-5)
        assert audit["not_ties"] == 0 and audit["max_soft_err"] <= 1e-4, audit


def test_resnet_single_patch_batch_raises_like_batchnorm(hip):
    """One 16x16 patch leaves layer4's BatchNorm one value per channel: nn.BatchNorm2d raises ValueError in training mode, and so
    does the HIP path (before any launch) instead of normalising by sqrt(eps)."""
    import copy
    import encoder as crw_encoder
    a = crw_encoder.Resnet(False).cuda()
    b = copy.deepcopy(a)
    b.hip_convs = None
    x = torch.randn(1, 1, 16, 16).cuda()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        b(x)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        a(x)
    assert torch.isfinite(a(torch.randn(2, 1, 16, 16).cuda())).all()


@pytest.mark.parametrize("P,runs", [(700, 5), (16128, 4)])
def test_resnet_native_pass_is_reproducible(hip, P, runs):
    """Side stream, last-block merges (tickets handed over by release / acquire) and split slabs must not make the result depend on
    the schedule: the same step run several times (fresh module copies, same input) gives bit-identical features, running statistics
    and gradients -- at a small batch and at the bench batch (126 patch tiles, every CU busy, the side stream active throughout),
    there with another stream's kernels competing for the chip."""
    import copy
    import encoder as crw_encoder
    torch.manual_seed(21)
    base = crw_encoder.Resnet(False).cuda()
    x = torch.randn(P, 1, 16, 16).cuda()
    gy = torch.randn(P, 128).cuda()
    ref = None
    noise_stream = torch.cuda.Stream()
    junk = torch.randn(2048, 2048, device="cuda")
    for run in range(runs):
        if P > 1000 and run % 2 == 1:  # every other run shares the chip with an unrelated stream
            with torch.cuda.stream(noise_stream):
                for _ in range(8):
                    junk = torch.tanh(junk @ junk * 1e-3)
        m = copy.deepcopy(base)
        y = m(x)
        y.backward(gy)
        torch.cuda.synchronize()
        got = [y.detach()] + [b.detach().clone() for b in m.buffers()] + [p.grad for p in m.parameters()]
        if ref is None:
            ref = got
        else:
            for k, (a, b) in enumerate(zip(ref, got)):
                assert torch.equal(a, b), f"tensor {k} differs between two runs of the same step"


@pytest.mark.parametrize("name", ["resnet_train_B2T4N5", "resnet_train_32x32_B2T4N5", "resnet_train_20x27_B2T4N5"])
def test_resnet_hip_training_step_matches_reference(hip, monkeypatch, name):
    """SURVEY section 8 row a8 on the hand-written kernels: CRW.forward + backward with the reference's DEFAULT encoder against
    the reference's own CPU run (fixtures resnet_train_*: 16x16 patches; 32x32 with overlap 24, scripts/test/test_mc1.py:19,21;
    20x27), with every PyTorch convolution / batch-norm entry point disabled.  Where the fixture holds them: the encoder switched
    to eval mode AFTER the step (scripts/test/test.py:42) -- BatchNorm on the running statistics this step has just updated --
    against the reference's eval-mode features, and every running statistic."""
    import model as crw_model
    import encoder as crw_encoder
    g = load_golden(name)
    torch.manual_seed(int(g["seed"]))
    enc = crw_encoder.Resnet(False)
    net = crw_model.CRW(enc, float(g["tau"]), False).cuda()
    net.train(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _no_library_convs(monkeypatch)
        loss, A = net(torch.as_tensor(g["seq"]).cuda())
        loss.backward()
    monkeypatch.undo()
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    np.testing.assert_allclose(A.detach().cpu().numpy(), g["A"], rtol=1e-3, atol=5e-3)
    np.testing.assert_allclose(enc.bn0.running_mean.cpu().numpy(), g["bn0.running_mean"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(enc.bn0.running_var.cpu().numpy(), g["bn0.running_var"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(enc.model.bn1.running_mean.cpu().numpy(), g["model.bn1.running_mean"], rtol=1e-3, atol=1e-5)
    names = [k for k, _ in enc.named_parameters()]
    assert names == list(g["grad_names"])
    # Gradients, two ways.  (1) End to end -- HIP walk + HIP encoder against the reference's fp32 run: every gradient's norm.
    # (2) The encoder alone: the reference's OWN dLoss/dEmb (fixture `demb`) pushed through the HIP backward, entry by entry above the
    # max-pool; below it -- and for (1) -- a FREE-RUNNING comparison is limited by routing decisions (the reference's fp32 forward
    # picks its own arg-max pixels / ReLU gates; with the 40 patches of these fixtures one flip moves the sums below the pool by a
    # few per cent): direction + norm there.  Entry-by-entry equality below the pool is what test_resnet_hip_matches_pytorch_modules
    # holds against the teacher-forced reference at the same patch sizes.
    below_pool = ("fc0.weight", "bn0.weight", "bn0.bias", "model.conv1.weight", "model.bn1.weight", "model.bn1.bias")
    for (k, p_), ref_norm in zip(enc.named_parameters(), g["grad_norms"]):
        tol = 5e-2 if k in below_pool else 2e-2
        got = float(p_.grad.double().norm())
        assert abs(got - ref_norm) <= tol * ref_norm + 1e-4, (k, got, ref_norm)
    torch.manual_seed(int(g["seed"]))
    enc2 = crw_encoder.Resnet(False).cuda().train(True)
    seq_d = torch.as_tensor(g["seq"]).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _no_library_convs(monkeypatch)
        emb2 = enc2(seq_d.reshape(-1, 1, *seq_d.shape[-2:]))
        emb2.backward(torch.as_tensor(g["demb"]).cuda())
    monkeypatch.undo()
    np.testing.assert_allclose(emb2.detach().cpu().numpy(), g["emb"], rtol=1e-3, atol=1e-4 * np.abs(g["emb"]).max())
    for k, p_ in enc2.named_parameters():
        if "grad." + k not in g:
            continue
        ref = g["grad." + k]
        a_, b_ = p_.grad.double().flatten().cpu(), torch.as_tensor(ref).double().flatten()
        cos = float(torch.dot(a_, b_) / (a_.norm() * b_.norm() + 1e-30))
        if k in below_pool:
            assert cos > 0.995 and abs(float(a_.norm() / b_.norm()) - 1) < 5e-2, (k, cos, float(a_.norm() / b_.norm()))
        else:
            # every entry within 2 % of the gradient's scale.  (Not tighter: at this initialisation -- BatchNorm bias 0, so the
            # ReLU inputs are centred on their gates -- relative noise of 1e-6 on the input patches moves these gradients by 2-3e-3
            # in float64 already, tools/r04_rn_fixture_diag.py / profiles/r04_rn_fixture_diag.log: a gate-flip random walk, ~ the
            # square root of the forward noise; PyTorch-ROCm's own fp32 modules sit 2.5e-3 from float64 on this fixture, the
            # hi/lo-pair kernels 7.6e-3.)
            # -- and a single flipped gate moves single entries by one element's contribution (a BatchNorm bias gradient is a plain
            # sum of gated gradients): at most 0.5 % of a tensor's entries may leave the band, direction > 0.9995
            bad = np.abs(p_.grad.cpu().numpy() - ref) > 2e-2 * np.abs(ref) + 2e-2 * np.abs(ref).max()
            assert bad.mean() <= 5e-3, (k, int(bad.sum()), bad.size)
            assert cos > 0.9995, (k, cos)
    if "emb_eval" in g:
        for k, b in enc.named_buffers():
            if b.is_floating_point():
                np.testing.assert_allclose(b.cpu().numpy(), g["buffer." + k], rtol=1e-3, atol=1e-5, err_msg=k)
        seq = torch.as_tensor(g["seq"]).cuda()
        enc.train(False)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _no_library_convs(monkeypatch)
            with torch.no_grad():
                emb_eval = enc(seq.reshape(-1, 1, *seq.shape[-2:]))
        monkeypatch.undo()
        scale = np.abs(g["emb_eval"]).max()
        np.testing.assert_allclose(emb_eval.cpu().numpy(), g["emb_eval"], rtol=1e-3, atol=1e-4 * scale)
