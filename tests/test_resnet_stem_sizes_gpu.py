"""The Resnet stem at patch sizes other than 16 x 16, kernel by kernel, and the helpers no test named: crw_rn_stem_band_fwd (and
its geometry rule crw_rn_stem_band_ok), crw_rn_bn_stats_rows, crw_rn_colsum; the fallback route crw_rn_stem_fwd + crw_rn_conv
mode 2; the backward kernels crw_rn_pack_stem / crw_rn_wgrad mode 2 / crw_rn_conv mode 3 / crw_rn_stem_bwd across the widths
where crw_rn_stem_cols(w) passes a multiple of 64 (19 | 20, 40 | 41).

Reference: the fp64 `_Stem` module of test_resnet_hip.py in train mode with the same parameters, exactly as in
test_rn_stem_matches_torch.  Tolerances: that test's and test_rn_batchnorm_kernels_match_torch's, none new --
    Z1 rtol 2e-4, atol 5e-5 of the output scale;  partial sums rtol 1e-4, atol 1e-6 P H1 W1 scale (scale^2 for the squares);
    dw1 rtol 2e-4, atol 5e-5 of its maximum;  bn0 gradients rtol 1e-3, atol 1e-4 max(1, scale);  fc0.weight rtol 2e-2, atol
    2e-3 max(1, scale);  |fc0.bias| <= 1e-3 max(1, |dgamma|max);  running statistics and coefficients rtol 1e-5, atol 1e-6.

The reference's 7x7 weight holds the values the kernels read, `wvals(conv1.weight)` = the bf16 hi + lo pair of every weight (the
suite's convention: "the same operand values", test_resnet_hip.py).  Z1 and the gradients meet their bars with the raw fp32 weight
too; the batch statistics do not: a weight's representation error (up to 2^-17 relative) is the same for every sample, so it does
not average out of a channel mean -- measured against the raw weight, `shift` sat at up to 5.9e-6 where the bar is 1e-6 + 1e-5
|shift| (32x32: 2.0 x the bar, 20x27: 2.3 x, 9x12: 1.3 x), `scale` inside it.

The band kernel's accepted set is not monotone in the width (csrc/resnet_stem.hip stem_band_geometry: the LDS bound
(2 RB + 5) ((w + 9) & ~1) <= 832 with RB = min(H1, 96 / W1) output rows per band): at h = 16, w = 84 is accepted, 85 ... 94
refused, 95 ... 110 accepted again (one output row per band), 111 refused."""
import pytest
import torch

from test_resnet_hip import _Stem, nhwc, planes, wvals

pytestmark = pytest.mark.gpu

MOM = 0.1


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    return crw_hip


def _geo(h, w):
    H0, W0 = h + 2, w + 2
    H1, W1 = (H0 - 1) // 2 + 1, (W0 - 1) // 2 + 1
    return H0, W0, H1, W1, max(H0 + 6, 2 * H1 + 6), max(W0 + 6, 2 * W1 + 6)


def _nets(cin, seed):
    torch.manual_seed(seed)
    net = _Stem(cin).cuda()
    with torch.no_grad():
        net.bn0.weight.copy_(torch.tensor([0.8, -1.2, 1.5]))
        net.bn0.bias.copy_(torch.tensor([0.3, 0.1, -0.2]))
    ref = _Stem(cin).cuda().double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in net.state_dict().items()})
    with torch.no_grad():
        ref.conv1.weight.copy_(wvals(net.conv1.weight.detach()))  # the operand values the kernels read (see the module docstring)
    return net, ref.train()


def _close(what, got, ref, rtol, atol):
    got, ref = got.detach(), ref.detach()
    err = (got.double() - ref).abs()
    worst = float((err / (atol + rtol * ref.abs())).max())
    print(f"    {what}: worst error / bar = {worst:.3f} (max |err| {float(err.max()):.3e}, rtol {rtol:g}, atol {atol:.3e})")
    torch.testing.assert_close(got.double(), ref, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


FORWARD = [  # h, w, cin, P, accepted by the band kernel
    (32, 32, 1, 130, True), (20, 27, 2, 70, True), (9, 12, 1, 5, True),   # 9 x 12: one band
    (40, 16, 1, 5, True),                                                  # three bands, the last short
    (16, 84, 1, 5, True), (16, 85, 1, 5, False), (16, 95, 2, 5, True), (16, 110, 1, 3, True), (16, 111, 1, 3, False)]


@pytest.mark.parametrize("h,w,cin,P,band", FORWARD)
def test_rn_stem_forward_any_size(hip, h, w, cin, P, band):
    """crw_rn_stem_band_ok against the hand-derived rule; crw_rn_stem_stats; where accepted crw_rn_stem_band_fwd (Z1, its partial
    rows, crw_rn_bn_stats_rows on them: coefficients and running statistics); for every size crw_rn_stem_fwd + crw_rn_conv mode 2;
    where both routes exist their Z1 agree within the same bar."""
    assert hip.rn_stem_band_ok(h, w) == band, "the band kernel's geometry rule changed (csrc/resnet_stem.hip stem_band_geometry)"
    H0, W0, H1, W1, Hm, Wm = _geo(h, w)
    net, ref = _nets(cin, 5 + cin + h + w)
    x = torch.randn(P, cin, h, w).cuda() * 1.5 + 0.3
    with torch.no_grad():
        y_ref = ref(x.double())
    scale = y_ref.abs().max().item()
    print(f"\n  stem forward {h}x{w} cin {cin} P {P}: Z1 {H1}x{W1}, output scale {scale:.3f}, band kernel {'accepted' if band else 'refused'}")

    stem = hip.rn_stem_stats(x, net.fc0, net.bn0, MOM)
    _close("bn0.running_mean", net.bn0.running_mean, ref.bn0.running_mean, 1e-5, 1e-6)
    _close("bn0.running_var", net.bn0.running_var, ref.bn0.running_var, 1e-5, 1e-6)

    Zband = None
    if band:
        wf, _ = hip.rn_pack_stem16(net.conv1.weight)
        Zband, part = hip.rn_stem_band_fwd(x, stem, wf, H1, W1)
        _close("band Z1", nhwc(Zband, P, H1, W1, 64), y_ref, 2e-4, 5e-5 * scale)
        assert not Zband[P:].any()
        n = P * H1 * W1
        pt = part.double().sum(0)
        _close("band partial sums", pt[:, 0], y_ref.sum((0, 2, 3)), 1e-4, 1e-6 * n * scale)
        _close("band partial sums of squares", pt[:, 1], (y_ref ** 2).sum((0, 2, 3)), 1e-4, 1e-6 * n * scale * scale)
        # crw_rn_bn_stats_rows on those rows against fp64 batch statistics of the reference output
        g = torch.Generator().manual_seed(h * w)
        bn1 = torch.nn.BatchNorm2d(64).cuda()
        with torch.no_grad():
            bn1.weight.copy_(torch.rand(64, generator=g) + 0.5)
            bn1.bias.copy_(torch.randn(64, generator=g) * 0.3)
            bn1.running_mean.copy_(torch.randn(64, generator=g) * 0.1)
            bn1.running_var.copy_(torch.rand(64, generator=g) + 0.5)
        rm0, rv0 = bn1.running_mean.double().clone(), bn1.running_var.double().clone()
        coef = hip.rn_bn_stats_rows(part, n, bn1, MOM)
        mean, var = y_ref.mean((0, 2, 3)), y_ref.var((0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + bn1.eps)
        sc = bn1.weight.double() * invstd
        for name, got, want in (("scale", coef[0], sc), ("shift", coef[1], bn1.bias.double() - mean * sc), ("mean", coef[2], mean),
                                ("invstd", coef[3], invstd), ("bn1.running_mean", bn1.running_mean, (1 - MOM) * rm0 + MOM * mean),
                                ("bn1.running_var", bn1.running_var, (1 - MOM) * rv0 + MOM * var * n / (n - 1))):
            _close("rows " + name, got, want, 1e-5, 1e-6)

    # the fallback route, at every size: the map planes in HBM and the gathered product
    wstem = hip.rn_pack_stem(net.conv1.weight, h, w)
    xmap, stem2 = hip.rn_stem_fwd(x, net.fc0, net.bn0, Hm, Wm, MOM, update_running=False)
    torch.testing.assert_close(stem2[:21], stem[:21], rtol=1e-6, atol=1e-7)
    Z1, part = hip.rn_conv(hip.RN_STEM_FWD, P, (Hm, Wm, 4), (H1, W1), 64, (7, 7), 2, 3, xmap, wstem[:2], stats=True)
    _close("mode 2 Z1", nhwc(Z1, P, H1, W1, 64), y_ref, 2e-4, 5e-5 * scale)
    assert not Z1[P:].any()
    pt = part.reshape(-1, H1 * W1, 64, 2).double().sum((0, 1))
    _close("mode 2 partial sums", pt[:, 0], y_ref.sum((0, 2, 3)), 1e-4, 1e-6 * P * H1 * W1 * scale)
    _close("mode 2 partial sums of squares", pt[:, 1], (y_ref ** 2).sum((0, 2, 3)), 1e-4, 1e-6 * P * H1 * W1 * scale * scale)
    if Zband is not None:
        _close("band Z1 against mode 2 Z1", Zband[:P], Z1[:P].double(), 2e-4, 5e-5 * scale)


@pytest.mark.parametrize("h,w,cin", [(20, 27, 2), (9, 19, 1), (12, 20, 1), (16, 40, 1), (16, 41, 2)])
def test_rn_stem_backward_any_size(hip, h, w, cin):
    """crw_rn_pack_stem(h, w), crw_rn_wgrad mode 2, crw_rn_conv mode 3 (the Toeplitz product; crw_rn_stem_cols(w) = 64 | 128 at
    w = 19 | 20, 128 | 192 at 40 | 41), crw_rn_stem_bwd against the fp64 gradients"""
    P = 130
    H0, W0, H1, W1, Hm, Wm = _geo(h, w)
    net, ref = _nets(cin, 7 + cin + h + w)
    x = torch.randn(P, cin, h, w).cuda() * 1.5 + 0.3
    dy = torch.randn(P, 64, H1, W1).cuda()
    y_ref = ref(x.double())
    y_ref.backward(dy.double())
    cols = hip.rn_stem_cols(w)
    assert cols == -(-3 * (w + 2) // 64) * 64
    print(f"\n  stem backward {h}x{w} cin {cin} P {P}: Z1 {H1}x{W1}, {cols} Toeplitz columns")

    wstem = hip.rn_pack_stem(net.conv1.weight, h, w)
    xmap, stem = hip.rn_stem_fwd(x, net.fc0, net.bn0, Hm, Wm, MOM)
    dp, _ = planes(hip, dy)
    dw1 = hip.rn_wgrad(hip.RN_STEM_FWD, P, (Hm, Wm, 4), (H1, W1, 64), (7, 7), 2, 3, xmap, dp)
    gw = ref.conv1.weight.grad
    _close("conv1.weight", dw1, gw, 2e-4, 5e-5 * gw.abs().max().item())

    dX0, _ = hip.rn_conv(hip.RN_STEM_BWD, P, (H1, W1, 64), (H0, 1), cols, (7, 7), 2, 3, dp, wstem[2:])
    assert not dX0[P:].any()
    dw0, db0, dg, db = hip.rn_stem_bwd(dX0, x, stem, net.fc0.weight.detach(), net.fc0.bias.detach())
    for name, got, want in (("bn0.weight", dg, ref.bn0.weight.grad), ("bn0.bias", db, ref.bn0.bias.grad)):
        _close(name, got, want, 1e-3, 1e-4 * max(1.0, want.abs().max().item()))
    want = ref.fc0.weight.grad
    _close("fc0.weight", dw0, want, 2e-2, 2e-3 * max(1.0, want.abs().max().item()))
    noise, bar = db0.abs().max().item(), 1e-3 * max(1.0, dg.abs().max().item())
    print(f"    fc0.bias: |gradient| max {noise:.3e} (true value 0), bar {bar:.3e}")
    assert noise <= bar


@pytest.mark.parametrize("nrows,C", [(1, 128), (200, 128), (16128, 128), (130, 3)])
def test_rn_colsum_matches_fp64(hip, nrows, C):
    """The kernels add in double and round once (rn_rows_reduce_kernel, rn_colsum_finalize_kernel): per column
    |got - ref| <= 2^-23 |ref| + 2^-40 sum |x|  (the one fp32 rounding of the result, and the sum carried in double)."""
    g = torch.Generator().manual_seed(nrows + C)
    x = (torch.randn(nrows, C, generator=g) * 3 + 0.25).cuda()
    got = hip.rn_colsum(x).double()
    ref = x.double().sum(0)
    bound = 2.0 ** -23 * ref.abs() + 2.0 ** -40 * x.double().abs().sum(0)
    worst = float(((got - ref).abs() / bound).max())
    print(f"\n  colsum {nrows} x {C}: worst |got - ref| / bound = {worst:.3f}")
    assert got.shape == (C,) and bool(((got - ref).abs() <= bound).all()), worst
