"""Do the encoder's entry points (CNN and Resnet kernels) read memory they did not write?  Every case calls the C ABI through
crw_hip.lib() with this test's own buffers -- workspaces exactly as long as the crw_*_bytes queries ask, at the allocator's
addresses -- once with every workspace and output filled with 0xFF (NaN as fp32 / bf16 / fp64, 0xFFFFFFFF as a ticket) and once
with 0x00 (tests/stale_ref.py; its proof on planted defects: tests/test_stale.py).  Held per case: every region the header
documents as written is finite and bit-identical between the two runs; every other byte still holds its fill; rows the header
promises zero (P .. Ppad-1 of planes and of raw convolution outputs, tickets "left zeroed") are zero.  Inputs are random and the
comparison is between two runs of the same code: no tolerance, no reference.

Every case of the table runs a second time between guard bands (`run_banded` of tests/stale_ref.py): the builders pass every device
input -- the planes and weight packs that another entry point produced included -- through `home`, which puts each of them, like
every output and workspace, in the middle of a larger allocation whose surroundings are NaN in one run and zero in the other.  A
kernel that fetches a halo, a padding row or a partial tile from in front of or behind an operand, or stores past an output's end,
is reported with the operand and the distance.

Read before anything ran (csrc/): the only words of a workspace that steer control flow are the block tickets of
rn_sums_tail_kernel (resnet_bn.hip), zeroed by every entry point that owns a set (rn_zero_tickets in crw_rn_bn_stats[_rows],
crw_rn_bn_bwd, crw_rn_pool_bwd, and forward_pass / crw_rn_train_bwd of resnet_net.hip); everything else a workspace holds is
floating-point partials, activations, packed weights and code bytes that a kernel of the same call (or, for crw_rn_train_bwd and
the front end's `saved`, the documented forward call) writes first.

Coverage = the crw_*_bytes queries of include/crw_hip.h:
  crw_enc_wgrad_ws_bytes ....... crw_enc_conv3x3_wgrad, crw_enc_conv3x3_wgrad_map          (cases enc_wgrad*, enc_wgrad_map)
  crw_enc_front_saved_bytes .... crw_enc_front_fwd -> crw_enc_front_bwd                    (enc_front*; the record is opaque: only
  crw_enc_front_ws_bytes ....... crw_enc_front_bwd, crw_enc_front_bwd_map                   what the backward makes of it is held)
  crw_linear128_wgrad_ws_bytes . crw_linear128_wgrad
  crw_rn_conv_part_floats ...... crw_rn_conv with `part`                                   (rn_conv_wgrad, rn_stem_any)
  crw_rn_wgrad_ws_bytes ........ crw_rn_wgrad
  crw_rn_bn_stats_ws_bytes ..... crw_rn_bn_stats, crw_rn_bn_stats_rows
  crw_rn_bn_bwd_ws_bytes / crw_rn_pool_bwd_ws_bytes
  crw_rn_stem_ws_bytes ......... crw_rn_stem_fwd, crw_rn_stem_bwd, crw_rn_stem_stats
  crw_rn_stem16_ws_bytes ....... crw_rn_stem16_wgrad, crw_rn_stem16_bwd (+ crw_rn_stem16_fwd, crw_rn_stem_band_fwd: no workspace,
                                 partial rows that idle waves must still write)
  crw_rn_colsum_ws_bytes, crw_rn_train_ws_bytes (train_fwd + train_bwd, train_fwd_nograd, eval_fwd), crw_gemm_bf16_ws_bytes,
  crw_confusion_ws_bytes, crw_calibration_ws_bytes
Not here, covered elsewhere: crw_walk_state_bytes / crw_walk_scratch_bytes / crw_affinity_ws_bytes (test_walk_routes_gpu.py
test_walk_ignores_stale_workspace), crw_horizons_ws_bytes (test_horizons.py), crw_labelmap_ordered_workspace /
crw_labelmap_posterior_workspace (test_ordered.py, test_posterior.py).  The outputs-only CNN forward / backward-data kernels
(crw_enc_conv3x3[_map]) take no workspace and are here for their outputs."""
import ctypes

import pytest
import torch

import stale_ref as sr
from stale_ref import Buf, Case, rows

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
MOM, EPS = 0.1, 1e-5


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    return crw_hip


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(name, status):
    assert status == 0, (name, "status", status)


def _nb(t):
    return t.numel() * t.element_size()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).cuda()


def _case(entry, inputs, bufs, run, home):
    def synced(inp, t):
        run(inp, t)
        torch.cuda.synchronize()
    return Case(entry, inputs, bufs, synced, device="cuda", home=home)


def _tickets(nbytes, ticket_bytes=128):
    """the ticket set at the end of a workspace (RN_TICKET_BLOCKS counters): left zeroed"""
    return [(nbytes - ticket_bytes, nbytes)]


# ================================================================================================ CNN encoder
def enc_wgrad(hip, cin, cout, P, split, dgap, home=sr.PLAIN):
    """P = 5: fewer patches than slices; P = 200: two patches per slice, with the final flush step of the streamed kernel"""
    lib, g = hip.lib(), _gen(cin + P + split)
    xh, xl = hip.enc_pack_input(_randn(g, P, cin, 10, 10), split)
    dyh, dyl = hip.enc_pack_input(torch.relu(_randn(g, P, cout, 10, 10)), split)   # (with dgap: the forward activation plane)
    dg = _randn(g, P, cout) if dgap else None
    if dgap:
        dyl = None                                                                  # "dy_lo ignored"
    xh, xl, dyh, dyl, dg = home.many(x_hi=xh, x_lo=xl, dy_hi=dyh, dy_lo=dyl, dgap=dg)
    nws = lib.crw_enc_wgrad_ws_bytes(P, cin, cout, split)
    bufs = dict(dw=Buf(cout * cin * 9 * 4, step=cin * 9 * 4), db=Buf(cout * 4), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_enc_conv3x3_wgrad", lib.crw_enc_conv3x3_wgrad(split, P, cin, cout, _p(dyh), _p(dyl), _p(xh), _p(xl), _p(dg), _p(t["dw"]),
                                                               _p(t["db"]), _p(t["ws"]), nws, _stream()))
    return _case("crw_enc_conv3x3_wgrad", None, bufs, run, home)


def enc_wgrad_map(hip, cin, cout, H, W, P, split, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(H * W + split)
    xh, xl = hip.enc_pack_input_map(_randn(g, P, cin, H, W), split)
    dyh, dyl = hip.enc_pack_input_map(_randn(g, P, cout, H, W), split)
    xh, xl, dyh, dyl = home.many(x_hi=xh, x_lo=xl, dy_hi=dyh, dy_lo=dyl)
    nws = lib.crw_enc_wgrad_ws_bytes(P * ((H + 9) // 10) * ((W + 9) // 10), cin, cout, split)
    bufs = dict(dw=Buf(cout * cin * 9 * 4, step=cin * 9 * 4), db=Buf(cout * 4), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_enc_conv3x3_wgrad_map", lib.crw_enc_conv3x3_wgrad_map(split, P, H, W, cin, cout, _p(dyh), _p(dyl), _p(xh), _p(xl),
                                                                       _p(t["dw"]), _p(t["db"]), _p(t["ws"]), nws, _stream()))
    return _case("crw_enc_conv3x3_wgrad_map", None, bufs, run, home)


def _front_inputs(hip, g, P, cin, split, home, hw=(16, 16), dy_pix=100):
    x = _randn(g, P, cin, *hw)
    w1, b1 = _randn(g, 8, cin, 5, 5, scale=0.2), _randn(g, 8, scale=0.1)
    w2, b2 = _randn(g, 32, 8, 5, 5, scale=0.07), _randn(g, 32, scale=0.1)
    fh, fl, bh, bl = hip.enc_front_pack(w2, split)
    dy = _randn(g, P, dy_pix, 32)
    x, w1, b1, b2, dy = home.many(x=x, w1=w1, b1=b1, b2=b2, dy=dy)
    return x, w1, b1, home.many(w2_hi=fh, w2_lo=fl, w2b_hi=bh, w2b_lo=bl), b2, dy


def enc_front(hip, cin, P, split, use_saved, home=sr.PLAIN):
    """crw_enc_front_fwd (with `saved`) then crw_enc_front_bwd from the record, or both without it (the backward recomputes).
    P = 257: 256 slices of 2 patches, slices 129 .. 255 hold none and must write zero partial sums.  y_lo is absent at split 1."""
    lib, g = hip.lib(), _gen(cin * 1000 + P + split)
    x, w1, b1, (fh, fl, bh, bl), b2, dy = _front_inputs(hip, g, P, cin, split, home)
    nws, nsv = lib.crw_enc_front_ws_bytes(P, cin), lib.crw_enc_front_saved_bytes(P)
    bufs = dict(y_hi=Buf(P * 100 * 32 * 2, BF16, step=100 * 32 * 2), dw1=Buf(8 * cin * 25 * 4), db1=Buf(8 * 4), dw2=Buf(32 * 8 * 25 * 4), db2=Buf(32 * 4),
                ws=Buf(nws, ws=True))
    if split == 3:
        bufs["y_lo"] = Buf(P * 100 * 32 * 2, BF16, step=100 * 32 * 2)
    if use_saved:
        bufs["saved"] = Buf(nsv, None, ws=True)        # an opaque record (code bytes, padded): held through what the backward reads

    def run(_, t):
        sv = _p(t["saved"]) if use_saved else None
        _ok("crw_enc_front_fwd", lib.crw_enc_front_fwd(split, _p(x), P, cin, _p(w1), _p(b1), _p(fh), _p(fl), _p(b2), _p(t["y_hi"]),
                                                       _p(t.get("y_lo")), sv, _stream()))
        _ok("crw_enc_front_bwd", lib.crw_enc_front_bwd(split, _p(x), P, cin, _p(w1), _p(b1), _p(fh), _p(fl), _p(b2), _p(bh), _p(bl), _p(dy),
                                                       sv, _p(t["dw1"]), _p(t["db1"]), _p(t["dw2"]), _p(t["db2"]), _p(t["ws"]), nws,
                                                       _stream()))
    return _case("crw_enc_front_fwd + crw_enc_front_bwd" + (" (saved)" if use_saved else " (recompute)"), None, bufs, run, home)


def enc_front_bwd_map(hip, cin, H, W, P, split, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(H * W + cin + split)
    x, w1, b1, (fh, fl, bh, bl), b2, dy = _front_inputs(hip, g, P, cin, split, home, (H, W), (H - 6) * (W - 6))
    nws = lib.crw_enc_front_ws_bytes(P * ((H - 6 + 9) // 10) * ((W - 6 + 9) // 10), cin)
    bufs = dict(dw1=Buf(8 * cin * 25 * 4), db1=Buf(8 * 4), dw2=Buf(32 * 8 * 25 * 4), db2=Buf(32 * 4), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_enc_front_bwd_map", lib.crw_enc_front_bwd_map(split, _p(x), P, cin, H, W, _p(w1), _p(b1), _p(fh), _p(fl), _p(b2), _p(bh),
                                                               _p(bl), _p(dy), _p(t["dw1"]), _p(t["db1"]), _p(t["dw2"]), _p(t["db2"]),
                                                               _p(t["ws"]), nws, _stream()))
    return _case("crw_enc_front_bwd_map", None, bufs, run, home)


def linear128_wgrad(hip, P, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(P)
    dy, x = home.many(dy=_randn(g, P, 128), x=_randn(g, P, 128))
    nws = lib.crw_linear128_wgrad_ws_bytes(P)
    bufs = dict(dw=Buf(128 * 128 * 4), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_linear128_wgrad", lib.crw_linear128_wgrad(_p(dy), _p(x), _p(t["dw"]), P, _p(t["ws"]), nws, _stream()))
    return _case("crw_linear128_wgrad", None, bufs, run, home)


def enc_conv(hip, mode, cin, cout, P, split, dgap=False, home=sr.PLAIN):
    """outputs only.  mode 0 with `gap`; mode 1 with mask_hi, and with dgap (x_hi then the forward activation plane, x_lo ignored)"""
    lib, g = hip.lib(), _gen(mode * 7 + cin + split + dgap)
    w = _randn(g, *((cout, cin) if mode == 0 else (cin, cout)), 3, 3, scale=0.05)
    fh, fl, bh, bl = hip.enc_pack_weights(w, split)
    wh, wl = (fh, fl) if mode == 0 else (bh, bl)
    xh, xl = hip.enc_pack_input(torch.relu(_randn(g, P, cin, 10, 10)), split)
    bias = _randn(g, cout, scale=0.1) if mode == 0 else None
    mask = hip.enc_pack_input(torch.relu(_randn(g, P, cout, 10, 10)), 1)[0] if mode == 1 else None
    dg = _randn(g, P, cin) if dgap else None
    if dgap:
        xl = None
    xh, xl, wh, wl, bias, mask, dg = home.many(x_hi=xh, x_lo=xl, w_hi=wh, w_lo=wl, bias=bias, mask_hi=mask, dgap=dg)
    plane = P * 100 * cout
    bufs = dict(y_hi=Buf(plane * 2, BF16), y_f32=Buf(plane * 4))
    if split == 3:
        bufs["y_lo"] = Buf(plane * 2, BF16)
    if mode == 0:
        bufs["gap"] = Buf(P * cout * 4)

    def run(_, t):
        _ok("crw_enc_conv3x3", lib.crw_enc_conv3x3(mode, split, P, cin, cout, _p(xh), _p(xl), _p(wh), _p(wl), _p(bias), _p(mask),
                                                   _p(t["y_hi"]), _p(t.get("y_lo")), _p(t["y_f32"]), _p(t.get("gap")), _p(dg), _stream()))
    return _case(f"crw_enc_conv3x3 mode {mode}", None, bufs, run, home)


def enc_conv_map(hip, cin, cout, H, W, P, split, home=sr.PLAIN):
    """mode 0 with gap_part: 14 x 21 = 2 x 3 tiles, partial in both directions"""
    lib, g = hip.lib(), _gen(H + W + split)
    fh, fl, _, _ = hip.enc_pack_weights(_randn(g, cout, cin, 3, 3, scale=0.05), split)
    xh, xl = hip.enc_pack_input_map(_randn(g, P, cin, H, W), split)
    bias = _randn(g, cout, scale=0.1)
    xh, xl, fh, fl, bias = home.many(x_hi=xh, x_lo=xl, w_hi=fh, w_lo=fl, bias=bias)
    ntile = ((H + 9) // 10) * ((W + 9) // 10)
    bufs = dict(y_hi=Buf(P * H * W * cout * 2, BF16), gap_part=Buf(P * ntile * cout * 4))
    if split == 3:
        bufs["y_lo"] = Buf(P * H * W * cout * 2, BF16)

    def run(_, t):
        _ok("crw_enc_conv3x3_map", lib.crw_enc_conv3x3_map(0, split, P, H, W, cin, cout, _p(xh), _p(xl), _p(fh), _p(fl), _p(bias), None,
                                                           _p(t["y_hi"]), _p(t.get("y_lo")), None, _p(t["gap_part"]), _stream()))
    return _case("crw_enc_conv3x3_map mode 0", None, bufs, run, home)


# ================================================================================================ Resnet building blocks
def _padrows(t, Ppad):
    out = torch.zeros(Ppad, t[0].numel(), device="cuda")
    out[:t.shape[0]] = t.reshape(t.shape[0], -1)
    return out


def _split(hip, t, P):
    """fp32 [P, ...] -> (hi, lo) planes [Ppad, n] with zero padding rows"""
    flat = t.reshape(P, -1).contiguous()
    return hip.rn_split(flat, P, flat.shape[1])


def _part_of(Z, Ppad, npix, C):
    """what a convolution epilogue hands crw_rn_bn_stats: per (64-row tile half, pixel) column sums and sums of squares"""
    zp = Z.reshape(Ppad // 64, 64, npix, C)
    return torch.stack([zp.sum(1), (zp * zp).sum(1)], -1).contiguous().reshape(-1)


def _bn_params(g, C):
    return (torch.rand(C, generator=g) + 0.5).cuda(), _randn(g, C, scale=0.3), _randn(g, C, scale=0.1), (torch.rand(C, generator=g) + 0.5).cuda()


def rn_conv_wgrad(hip, P=200, H=5, C=64, home=sr.PLAIN):
    """crw_rn_conv mode 0 with `part`, and crw_rn_wgrad: 5x5, 64 -> 64"""
    lib, g = hip.lib(), _gen(P)
    Ppad = hip.rn_padded(P)
    xh, xl = _split(hip, _randn(g, P, H * H, C), P)
    dh, dl = _split(hip, _randn(g, P, H * H, C), P)
    fh, fl, _, _ = hip.rn_pack_conv(_randn(g, C, C, 3, 3, scale=0.04))
    xh, xl, dh, dl, fh, fl = home.many(x_hi=xh, x_lo=xl, d_hi=dh, d_lo=dl, w_hi=fh, w_lo=fl)
    geo = (0, P, H, H, C, H, H, C, 3, 3, 1, 1)
    nws, row = lib.crw_rn_wgrad_ws_bytes(*geo), H * H * C * 4
    assert nws > 0
    bufs = dict(out=Buf(Ppad * row, zero=[rows(P, Ppad, row)], step=row), part=Buf(lib.crw_rn_conv_part_floats(P, H * H, C) * 4),
                dw=Buf(C * C * 9 * 4), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_rn_conv", lib.crw_rn_conv(*geo, _p(xh), _p(xl), _p(fh), _p(fl), None, _p(t["out"]), _p(t["part"]), _stream()))
        _ok("crw_rn_wgrad", lib.crw_rn_wgrad(*geo, _p(xh), _p(xl), _p(dh), _p(dl), _p(t["dw"]), _p(t["ws"]), nws, _stream()))
    return _case("crw_rn_conv mode 0 + crw_rn_wgrad", None, bufs, run, home)


def rn_bn_stats(hip, C=64, npix=25, P=200, by_rows=False, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(C + npix + by_rows)
    Ppad = hip.rn_padded(P)
    gamma, beta, rm, rv = _bn_params(g, C)
    if by_rows:                                        # the stem's partial rows [rows][C][2] over `count` samples per channel
        nrows = lib.crw_rn_stem16_rows()
        z = _randn(g, nrows, 5, C, scale=2.0, shift=0.5)
        part, count = torch.stack([z.sum(1), (z * z).sum(1)], -1).contiguous(), float(nrows * 5)
    else:
        part = _part_of(_padrows(_randn(g, P, npix, C, scale=2.0, shift=0.5), Ppad), Ppad, npix, C)
    part, gamma, beta = home.many(part=part, gamma=gamma, beta=beta)
    nws = lib.crw_rn_bn_stats_ws_bytes(C)
    bufs = dict(coef=Buf(4 * C * 4), run_mean=Buf(C * 4, init=rm), run_var=Buf(C * 4, init=rv), ws=Buf(nws, ws=True, zero=_tickets(nws)))

    def run(_, t):
        tail = (C, _p(gamma), _p(beta), _p(t["run_mean"]), _p(t["run_var"]), MOM, EPS, _p(t["coef"]), _p(t["ws"]), nws, _stream())
        if by_rows:
            _ok("crw_rn_bn_stats_rows", lib.crw_rn_bn_stats_rows(_p(part), nrows, count, *tail))
        else:
            _ok("crw_rn_bn_stats", lib.crw_rn_bn_stats(_p(part), P, npix, *tail))
    return _case("crw_rn_bn_stats_rows" if by_rows else "crw_rn_bn_stats", None, bufs, run, home)


class _BN:
    """the few attributes of nn.BatchNorm2d the crw_hip wrappers read (inputs are built through them)"""

    def __init__(self, g, C):
        self.weight, self.bias, self.running_mean, self.running_var = _bn_params(g, C)
        self.eps = EPS


def rn_bn_bwd(hip, C=128, npix=9, P=130, home=sr.PLAIN):
    """the shortcut form: y = relu(bn(Z) + bn_d(Zd))"""
    lib, g = hip.lib(), _gen(C + npix)
    Ppad = hip.rn_padded(P)
    Z, Zd = _padrows(_randn(g, P, npix, C, scale=2.0, shift=0.5), Ppad), _padrows(_randn(g, P, npix, C, scale=0.7, shift=-0.2), Ppad)
    g1, g2 = _padrows(_randn(g, P, npix, C), Ppad), _padrows(_randn(g, P, npix, C), Ppad)
    coef = hip.rn_bn_stats(_part_of(Z, Ppad, npix, C), P, npix, _BN(g, C), MOM)
    coefd = hip.rn_bn_stats(_part_of(Zd, Ppad, npix, C), P, npix, _BN(g, C), MOM)
    mask, _ = hip.rn_bn_apply(Z, coef, P, npix, C, Zd=Zd, coef_d=coefd)
    g1, g2, mask, Z, coef, Zd, coefd = home.many(g1=g1, g2=g2, mask_hi=mask, Z=Z, coef=coef, Zd=Zd, coef_d=coefd)
    nws, row = lib.crw_rn_bn_bwd_ws_bytes(P, npix, C), npix * C * 2
    pl = lambda: Buf(Ppad * row, BF16, zero=[rows(P, Ppad, row)], step=row)
    bufs = dict(dz_hi=pl(), dz_lo=pl(), dzd_hi=pl(), dzd_lo=pl(), dgamma=Buf(C * 4), dbeta=Buf(C * 4), dgamma_d=Buf(C * 4),
                dbeta_d=Buf(C * 4), ws=Buf(nws, ws=True, zero=_tickets(nws)))

    def run(_, t):
        _ok("crw_rn_bn_bwd", lib.crw_rn_bn_bwd(_p(g1), _p(g2), _p(mask), _p(Z), _p(coef), _p(Zd), _p(coefd), P, npix, C, _p(t["dz_hi"]),
                                               _p(t["dz_lo"]), _p(t["dzd_hi"]), _p(t["dzd_lo"]), None, _p(t["dgamma"]), _p(t["dbeta"]),
                                               _p(t["dgamma_d"]), _p(t["dbeta_d"]), _p(t["ws"]), nws, _stream()))
    return _case("crw_rn_bn_bwd", None, bufs, run, home)


def rn_pool_bwd(hip, P=70, H=7, W=6, C=64, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(P + H)
    Ppad = hip.rn_padded(P)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Z = _padrows(_randn(g, P, H * W, C, scale=1.5), Ppad)
    d1, d2 = _padrows(_randn(g, P, Ho * Wo, C), Ppad), _padrows(_randn(g, P, Ho * Wo, C), Ppad)
    bn = _BN(g, C)
    bn.weight = _randn(g, C)                           # negative scales too
    coef = hip.rn_bn_stats(_part_of(Z, Ppad, H * W, C), P, H * W, bn, MOM)
    _, amax = hip.rn_bn_pool(Z, coef, P, H, W, C)
    d1, d2, amax, Z, coef = home.many(d1=d1, d2=d2, amax=amax, Z=Z, coef=coef)
    nws, row = lib.crw_rn_pool_bwd_ws_bytes(P, H, W, C), H * W * C * 2
    pl = lambda: Buf(Ppad * row, BF16, zero=[rows(P, Ppad, row)], step=row)
    bufs = dict(dz_hi=pl(), dz_lo=pl(), dgamma=Buf(C * 4), dbeta=Buf(C * 4), ws=Buf(nws, ws=True, zero=_tickets(nws)))

    def run(_, t):
        _ok("crw_rn_pool_bwd", lib.crw_rn_pool_bwd(_p(d1), _p(d2), _p(amax), _p(Z), _p(coef), P, H, W, C, _p(t["dz_hi"]), _p(t["dz_lo"]),
                                                   _p(t["dgamma"]), _p(t["dbeta"]), _p(t["ws"]), nws, _stream()))
    return _case("crw_rn_pool_bwd", None, bufs, run, home)


STEM_RECORD = 27 * 4       # csrc/resnet_bn.hip rn_stem_finalize_kernel: floats 0 .. 26 of the 32 are the record, the rest is spare


def _stem_params(g, cin):
    w0, b0 = _randn(g, 3, cin, scale=0.6), _randn(g, 3, scale=0.2)
    gamma, beta = torch.tensor([0.8, -1.2, 1.5]).cuda(), torch.tensor([0.3, 0.1, -0.2]).cuda()
    return w0, b0, gamma, beta, _randn(g, 3, scale=0.1), (torch.rand(3, generator=g) + 0.5).cuda()


def _stem_geo(h, w):
    H0, W0 = h + 2, w + 2
    H1, W1 = (H0 - 1) // 2 + 1, (W0 - 1) // 2 + 1
    return H0, W0, H1, W1, max(H0 + 6, 2 * H1 + 6), max(W0 + 6, 2 * W1 + 6)


def rn_stem_any(hip, h=20, w=27, cin=2, P=130, home=sr.PLAIN):
    """crw_rn_stem_fwd -> crw_rn_conv mode 2 (+ part) -> [dz] -> crw_rn_wgrad mode 2, crw_rn_conv mode 3 -> crw_rn_stem_bwd"""
    lib, g = hip.lib(), _gen(h * w + cin)
    Ppad = hip.rn_padded(P)
    H0, W0, H1, W1, Hm, Wm = _stem_geo(h, w)
    x = _randn(g, P, cin, h, w, scale=1.5, shift=0.3)
    w0, b0, gamma, beta, rm, rv = _stem_params(g, cin)
    fh, fl, th, tl = hip.rn_pack_stem(_randn(g, 64, 3, 7, 7, scale=0.08), h, w)
    dh, dl = _split(hip, _randn(g, P, H1 * W1, 64), P)
    x, w0, b0, gamma, beta = home.many(x=x, w0=w0, b0=b0, gamma=gamma, beta=beta)
    fh, fl, th, tl, dh, dl = home.many(w_hi=fh, w_lo=fl, toep_hi=th, toep_lo=tl, d_hi=dh, d_lo=dl)
    cols = lib.crw_rn_stem_cols(w)
    fgeo, bgeo = (2, P, Hm, Wm, 4, H1, W1, 64, 7, 7, 2, 3), (3, P, H1, W1, 64, H0, 1, cols, 7, 7, 2, 3)
    nstem, nwg = lib.crw_rn_stem_ws_bytes(), lib.crw_rn_wgrad_ws_bytes(*fgeo)
    assert nwg > 0
    mrow, zrow, xrow = Hm * Wm * 4 * 2, H1 * W1 * 64 * 4, H0 * cols * 4
    bufs = dict(map_hi=Buf(Ppad * mrow, BF16, zero=[rows(P, Ppad, mrow)], step=mrow),
                map_lo=Buf(Ppad * mrow, BF16, zero=[rows(P, Ppad, mrow)], step=mrow),
                stem=Buf(32 * 4, written=[(0, STEM_RECORD)]), run_mean=Buf(12, init=rm), run_var=Buf(12, init=rv),
                Z1=Buf(Ppad * zrow, zero=[rows(P, Ppad, zrow)], step=zrow),
                part=Buf(lib.crw_rn_conv_part_floats(P, H1 * W1, 64) * 4, step=H1 * W1 * 64 * 2 * 4),     # [tile half][pixel][C][2]
                dw1=Buf(64 * 3 * 49 * 4), dX0=Buf(Ppad * xrow, zero=[rows(P, Ppad, xrow)], step=xrow), dw0=Buf(3 * cin * 4), db0=Buf(12),
                dgamma=Buf(12), dbeta=Buf(12), ws_fwd=Buf(nstem, ws=True), ws_wgrad=Buf(nwg, ws=True), ws_bwd=Buf(nstem, ws=True))

    def run(_, t):
        _ok("crw_rn_stem_fwd", lib.crw_rn_stem_fwd(_p(x), P, cin, h, w, Hm, Wm, _p(w0), _p(b0), _p(gamma), _p(beta), _p(t["run_mean"]),
                                                   _p(t["run_var"]), MOM, EPS, _p(t["map_hi"]), _p(t["map_lo"]), _p(t["stem"]),
                                                   _p(t["ws_fwd"]), nstem, _stream()))
        _ok("crw_rn_conv mode 2", lib.crw_rn_conv(*fgeo, _p(t["map_hi"]), _p(t["map_lo"]), _p(fh), _p(fl), None, _p(t["Z1"]), _p(t["part"]),
                                                  _stream()))
        _ok("crw_rn_wgrad mode 2", lib.crw_rn_wgrad(*fgeo, _p(t["map_hi"]), _p(t["map_lo"]), _p(dh), _p(dl), _p(t["dw1"]), _p(t["ws_wgrad"]),
                                                    nwg, _stream()))
        _ok("crw_rn_conv mode 3", lib.crw_rn_conv(*bgeo, _p(dh), _p(dl), _p(th), _p(tl), None, _p(t["dX0"]), None, _stream()))
        _ok("crw_rn_stem_bwd", lib.crw_rn_stem_bwd(_p(t["dX0"]), _p(x), _p(t["stem"]), _p(w0), _p(b0), P, cin, h, w, _p(t["dw0"]), _p(t["db0"]),
                                                   _p(t["dgamma"]), _p(t["dbeta"]), _p(t["ws_bwd"]), nstem, _stream()))
    return _case("crw_rn_stem_fwd / crw_rn_conv modes 2, 3 / crw_rn_wgrad mode 2 / crw_rn_stem_bwd", None, bufs, run, home)


def rn_stem16(hip, cin=1, P=200, home=sr.PLAIN):
    """crw_rn_stem_stats -> crw_rn_stem16_fwd -> crw_rn_stem16_wgrad, crw_rn_stem16_bwd.  Header: Z1 is [P][81][64] -- rows of
    patches beyond P are not written (the binding zeroes them itself)"""
    lib, g = hip.lib(), _gen(16 + cin)
    Ppad = hip.rn_padded(P)
    x = _randn(g, P, cin, 16, 16, scale=1.5, shift=0.3)
    w0, b0, gamma, beta, rm, rv = _stem_params(g, cin)
    wf, wt = hip.rn_pack_stem16(_randn(g, 64, 3, 7, 7, scale=0.08))
    dh, dl = _split(hip, _randn(g, P, 81, 64), P)
    x, w0, b0, gamma, beta, wf, wt, dh, dl = home.many(x=x, w0=w0, b0=b0, gamma=gamma, beta=beta, wf=wf, wt=wt, dz_hi=dh, dz_lo=dl)
    nstem, n16, nrows, zrow = lib.crw_rn_stem_ws_bytes(), lib.crw_rn_stem16_ws_bytes(), lib.crw_rn_stem16_rows(), 81 * 64 * 4
    bufs = dict(stem=Buf(32 * 4, written=[(0, STEM_RECORD)]), run_mean=Buf(12, init=rm), run_var=Buf(12, init=rv),
                Z1=Buf(Ppad * zrow, written=[rows(0, P, zrow)], step=zrow), part=Buf(nrows * 64 * 2 * 4, step=64 * 2 * 4),
                dw1=Buf(64 * 3 * 49 * 4),
                dw0=Buf(3 * cin * 4), db0=Buf(12), dgamma=Buf(12), dbeta=Buf(12), ws_stats=Buf(nstem, ws=True),
                ws_wgrad=Buf(n16, ws=True), ws_bwd=Buf(n16, ws=True))

    def run(_, t):
        _ok("crw_rn_stem_stats", lib.crw_rn_stem_stats(_p(x), P, cin, 16, 16, _p(w0), _p(b0), _p(gamma), _p(beta), _p(t["run_mean"]),
                                                       _p(t["run_var"]), MOM, EPS, _p(t["stem"]), _p(t["ws_stats"]), nstem, _stream()))
        _ok("crw_rn_stem16_fwd", lib.crw_rn_stem16_fwd(_p(x), P, cin, _p(t["stem"]), _p(wf), _p(t["Z1"]), _p(t["part"]), _stream()))
        _ok("crw_rn_stem16_wgrad", lib.crw_rn_stem16_wgrad(_p(x), P, cin, _p(t["stem"]), _p(dh), _p(dl), _p(t["dw1"]), _p(t["ws_wgrad"]), n16,
                                                           _stream()))
        _ok("crw_rn_stem16_bwd", lib.crw_rn_stem16_bwd(_p(x), P, cin, _p(t["stem"]), _p(w0), _p(b0), _p(wt), _p(dh), _p(dl), _p(t["dw0"]),
                                                       _p(t["db0"]), _p(t["dgamma"]), _p(t["dbeta"]), _p(t["ws_bwd"]), n16, _stream()))
    return _case("crw_rn_stem_stats / crw_rn_stem16_fwd / _wgrad / _bwd", None, bufs, run, home)


def rn_stem_band(hip, h=32, w=32, cin=1, P=3, home=sr.PLAIN):
    """P = 3: most of the waves hold no patch and must still leave correct (zero) partial rows"""
    lib, g = hip.lib(), _gen(h + w)
    assert lib.crw_rn_stem_band_ok(h, w) == 1
    Ppad = hip.rn_padded(P)
    _, _, H1, W1, _, _ = _stem_geo(h, w)
    x = _randn(g, P, cin, h, w, scale=1.5, shift=0.3)
    w0, b0, gamma, beta, rm, rv = _stem_params(g, cin)
    wf, _ = hip.rn_pack_stem16(_randn(g, 64, 3, 7, 7, scale=0.08))
    x, w0, b0, gamma, beta, wf = home.many(x=x, w0=w0, b0=b0, gamma=gamma, beta=beta, wf=wf)
    nstem, nrows, zrow = lib.crw_rn_stem_ws_bytes(), lib.crw_rn_stem16_rows(), H1 * W1 * 64 * 4
    bufs = dict(stem=Buf(32 * 4, written=[(0, STEM_RECORD)]), run_mean=Buf(12, init=rm), run_var=Buf(12, init=rv),
                Z1=Buf(Ppad * zrow, written=[rows(0, P, zrow)], step=zrow), part=Buf(nrows * 64 * 2 * 4, step=64 * 2 * 4),
                ws_stats=Buf(nstem, ws=True))

    def run(_, t):
        _ok("crw_rn_stem_stats", lib.crw_rn_stem_stats(_p(x), P, cin, h, w, _p(w0), _p(b0), _p(gamma), _p(beta), _p(t["run_mean"]),
                                                       _p(t["run_var"]), MOM, EPS, _p(t["stem"]), _p(t["ws_stats"]), nstem, _stream()))
        _ok("crw_rn_stem_band_fwd", lib.crw_rn_stem_band_fwd(_p(x), P, cin, h, w, _p(t["stem"]), _p(wf), _p(t["Z1"]), _p(t["part"]), _stream()))
    return _case("crw_rn_stem_stats / crw_rn_stem_band_fwd", None, bufs, run, home)


def rn_colsum(hip, nrows=200, C=128, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(nrows)
    x = home(_randn(g, nrows, C), "x")
    nws = lib.crw_rn_colsum_ws_bytes(C)
    bufs = dict(out=Buf(C * 4), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_rn_colsum", lib.crw_rn_colsum(_p(x), nrows, C, _p(t["out"]), _p(t["ws"]), nws, _stream()))
    return _case("crw_rn_colsum", None, bufs, run, home)


# ================================================================================================ the whole Resnet pass
def _resnet(cin, seed):
    import encoder as crw_encoder
    torch.manual_seed(seed)
    net = crw_encoder.Resnet(cin == 2).cuda()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.6, 1.4)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    prm = [p.detach().contiguous() for p in net.parameters()]
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(prm) == 42 and len(bns) == 13
    return prm, bns, [k for k, _ in net.named_parameters()]


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def rn_pass(hip, kind, P, h, w, cin, home=sr.PLAIN):
    """kind "train": crw_rn_train_fwd then crw_rn_train_bwd -- out, all 26 running statistics (each run starts from its own copy)
    and all 42 gradients; "nograd" / "eval": the forward alone (eval updates nothing: the statistics must come back as they went in).
    inputs = (x, dout): run_reused hands in a second batch."""
    lib, g = hip.lib(), _gen(P + h + w)
    prm, bns, names = _resnet(cin, P)
    prm = [home(p, "prm " + k) for k, p in zip(names, prm)]
    nws = lib.crw_rn_train_ws_bytes(P, cin, h, w)
    assert nws > 0
    bufs = dict(out=Buf(P * 128 * 4), ws=Buf(nws, ws=True))
    for i, m in enumerate(bns):
        bufs[f"run_mean[{i}]"] = Buf(_nb(m.running_mean), init=m.running_mean.clone())
        bufs[f"run_var[{i}]"] = Buf(_nb(m.running_var), init=m.running_var.clone())
    if kind == "train":
        for k, p in zip(names, prm):
            bufs["grad " + k] = Buf(_nb(p), step=sr.largest_step(p))

    def run(inp, t):
        x, dout = inp
        pp = _ptrs(prm)                                # (built here: the closure keeps the parameter tensors alive)
        rm, rv = _ptrs([t[f"run_mean[{i}]"] for i in range(13)]), _ptrs([t[f"run_var[{i}]"] for i in range(13)])
        if kind == "eval":
            _ok("crw_rn_eval_fwd", lib.crw_rn_eval_fwd(_p(x), P, cin, h, w, pp, rm, rv, EPS, _p(t["out"]), _p(t["ws"]), nws, _stream()))
            return
        fwd = lib.crw_rn_train_fwd if kind == "train" else lib.crw_rn_train_fwd_nograd
        _ok("crw_rn_train_fwd", fwd(_p(x), P, cin, h, w, pp, rm, rv, MOM, EPS, _p(t["out"]), _p(t["ws"]), nws, _stream()))
        if kind == "train":
            gp = _ptrs([t["grad " + k] for k in names])
            _ok("crw_rn_train_bwd", lib.crw_rn_train_bwd(_p(dout), _p(x), P, cin, h, w, pp, gp, _p(t["ws"]), nws, _stream()))
    entry = {"train": "crw_rn_train_fwd + crw_rn_train_bwd", "nograd": "crw_rn_train_fwd_nograd", "eval": "crw_rn_eval_fwd"}[kind]
    return _case(entry, home.many(x=_randn(g, P, cin, h, w), dout=_randn(g, P, 128)), bufs, run, home)


# ================================================================================================ others with a workspace
def gemm_bf16(hip, n=128, batch=2, split=3, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(n)
    A, B = home.many(A=_randn(g, batch, n, n), B=_randn(g, batch, n, n))
    nws = lib.crw_gemm_bf16_ws_bytes(n, batch, split)
    bufs = dict(C=Buf(batch * n * n * 4), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_gemm_bf16", lib.crw_gemm_bf16(_p(A), _p(B), _p(t["C"]), n, batch, 0, 0, 0, split, _p(t["ws"]), nws, 1, _stream()))
    return _case("crw_gemm_bf16", None, bufs, run, home)


def _label_maps(g, P, K):
    gt = torch.randint(0, K, (P,), generator=g).float().cuda()
    pred = torch.randint(0, K, (P,), generator=g).float().cuda()
    return gt, pred


def confusion(hip, P=5000, K=5, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(P)
    gt, pred = _label_maps(g, P, K)
    gt, pred = home.many(gt=gt, pred=pred)
    nws = lib.crw_confusion_ws_bytes(P, K)
    bufs = dict(counts=Buf(K * K * 8, None), dropped=Buf(2 * 8, None), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_confusion", lib.crw_confusion(_p(gt), 0, _p(pred), 0, None, 0, P, K, 0, -1, -1, _p(t["counts"]), _p(t["dropped"]),
                                               _p(t["ws"]), nws, _stream()))
    return _case("crw_confusion", None, bufs, run, home)


def calibration(hip, P=5000, K=5, bins=10, home=sr.PLAIN):
    lib, g = hip.lib(), _gen(P + bins)
    gt, pred = _label_maps(g, P, K)
    gt, pred, conf = home.many(gt=gt, pred=pred, conf=torch.rand(P, generator=g).cuda())
    nws = lib.crw_calibration_ws_bytes(P, K, bins)
    bufs = dict(counts=Buf(bins * 2 * 8, None), conf_sum=Buf(bins * 8, F64), dropped=Buf(3 * 8, None), ws=Buf(nws, ws=True))

    def run(_, t):
        _ok("crw_calibration", lib.crw_calibration(_p(gt), 0, _p(pred), 0, _p(conf), None, 0, P, K, bins, 0, -1, -1, _p(t["counts"]),
                                                   _p(t["conf_sum"]), _p(t["dropped"]), _p(t["ws"]), nws, _stream()))
    return _case("crw_calibration", None, bufs, run, home)


# ================================================================================================ the table
def _both(name, fn, *a, **k):
    return [(f"{name}-split{s}", fn, a + (s,), k) for s in (3, 1)]


TABLE = (
    _both("enc_wgrad-128x128-P5", enc_wgrad, 128, 128, 5, dgap=False)
    + _both("enc_wgrad-128x128-P5-dgap", enc_wgrad, 128, 128, 5, dgap=True)
    + _both("enc_wgrad-128x128-P200", enc_wgrad, 128, 128, 200, dgap=False)
    + _both("enc_wgrad_map-64x128-14x21-P3", enc_wgrad_map, 64, 128, 14, 21, 3)
    + _both("enc_front-cin2-P7-saved", enc_front, 2, 7, use_saved=True)
    + _both("enc_front-cin2-P7-recompute", enc_front, 2, 7, use_saved=False)
    + _both("enc_front-cin2-P257-saved", enc_front, 2, 257, use_saved=True)
    + _both("enc_front-cin2-P257-recompute", enc_front, 2, 257, use_saved=False)
    + _both("enc_front_bwd_map-cin1-20x27-P5", enc_front_bwd_map, 1, 20, 27, 5)
    + _both("enc_conv-mode0-64x128-P5-gap", enc_conv, 0, 64, 128, 5)
    + _both("enc_conv-mode1-128x128-P5-mask", enc_conv, 1, 128, 128, 5)
    + _both("enc_conv-mode1-128x128-P5-dgap", enc_conv, 1, 128, 128, 5, dgap=True)
    + _both("enc_conv_map-mode0-64x128-14x21-P3", enc_conv_map, 64, 128, 14, 21, 3)
    + [("linear128_wgrad-P256", linear128_wgrad, (256,), {}),
       ("rn_conv_wgrad-5x5-64-P200", rn_conv_wgrad, (), {}),
       ("rn_bn_stats-C64-npix25-P200", rn_bn_stats, (), {}),
       ("rn_bn_stats_rows-C64", rn_bn_stats, (), dict(by_rows=True)),
       ("rn_bn_bwd-shortcut-C128-npix9-P130", rn_bn_bwd, (), {}),
       ("rn_pool_bwd-P70-7x6", rn_pool_bwd, (), {}),
       ("rn_stem_any-20x27-cin2-P130", rn_stem_any, (), {}),
       ("rn_stem16-cin1-P200", rn_stem16, (), {}),
       ("rn_stem_band-32x32-P3", rn_stem_band, (), {}),
       ("rn_colsum-200x128", rn_colsum, (), {}),
       ("rn_train-P130-16x16-cin1", rn_pass, ("train", 130, 16, 16, 1), {}),
       ("rn_train-P40-32x32-cin2", rn_pass, ("train", 40, 32, 32, 2), {}),
       ("rn_nograd-P70-20x27", rn_pass, ("nograd", 70, 20, 27, 1), {}),
       ("rn_eval-P70-20x27", rn_pass, ("eval", 70, 20, 27, 1), {}),
       ("gemm_bf16-n128-b2-split3", gemm_bf16, (), {}),
       ("confusion-P5000-K5", confusion, (), {}),
       ("calibration-P5000-K5-bins10", calibration, (), {})])


@pytest.mark.parametrize("build,args,kwargs", [pytest.param(f, a, k, id=i) for i, f, a, k in TABLE])
def test_encoder_ignores_stale_memory(hip, build, args, kwargs):
    case = build(hip, *args, **kwargs)
    out = sr.run_twice(case)
    live = [k for k, b in case.bufs.items() if not b.ws and b.init is None and out[k][:b.nbytes].any()]
    assert live, (case.entry, "every output is all zeros: the case computes nothing")


@pytest.mark.parametrize("build,args,kwargs", [pytest.param(f, a, k, id=i) for i, f, a, k in TABLE])
def test_encoder_stays_inside_its_operands(hip, build, args, kwargs):
    """the same case with every input, output and workspace between guard bands: nothing read from them reaches a result, no
    byte of them is written"""
    case = build(hip, *args, home=sr.Home("cuda"), **kwargs)
    assert case.home.operands, (case.entry, "no input went through `home`")
    out = sr.run_banded(case)
    live = [k for k, b in case.bufs.items() if not b.ws and b.init is None and out[k][:b.nbytes].any()]
    assert live, (case.entry, "every output is all zeros: the case computes nothing")


@pytest.mark.parametrize("mapped", [False, True], ids=["10x10", "14x21"])
def test_pooled_output_without_a_kernel_is_refused(hip, mapped):
    """Found by the table's map case when it ran at (cin, cout) = (32, 64): with 64 output channels on the 8-wave kernel (split 3) the row tiles are split over
    waves and no wave holds a channel's whole pixel sum, so nothing wrote `gap` / `gap_part` -- and the call returned CRW_OK.  It
    is refused now, before anything is launched: every output still holds its fill.  (Split 1 runs 4 waves: served, see below.)"""
    lib, g, P, cin, cout = hip.lib(), _gen(64), 3, 32, 64
    H, W = (14, 21) if mapped else (10, 10)
    fh, fl, _, _ = hip.enc_pack_weights(_randn(g, cout, cin, 3, 3, scale=0.05), 3)
    xh, xl = hip.enc_pack_input_map(_randn(g, P, cin, H, W), 3)
    bias = _randn(g, cout, scale=0.1)
    ntile = ((H + 9) // 10) * ((W + 9) // 10) if mapped else 1
    y, gap = sr.filled(P * H * W * cout * 2, 0xFF, "cuda"), sr.filled(P * ntile * cout * 4, 0xFF, "cuda")

    def call(split, xl_, fl_):
        if mapped:
            return lib.crw_enc_conv3x3_map(0, split, P, H, W, cin, cout, _p(xh), _p(xl_), _p(fh), _p(fl_), _p(bias), None, _p(y), None, None,
                                           _p(gap), _stream())
        return lib.crw_enc_conv3x3(0, split, P, cin, cout, _p(xh), _p(xl_), _p(fh), _p(fl_), _p(bias), None, _p(y), None, None, _p(gap), None,
                                   _stream())
    assert call(3, xl, fl) == hip.CRW_EINVAL
    torch.cuda.synchronize()
    assert bool((y == 0xFF).all()) and bool((gap == 0xFF).all()), "a refused call wrote something"
    assert call(1, None, None) == hip.CRW_OK                        # 4 waves, one per 16 channels: the sums exist
    torch.cuda.synchronize()
    assert torch.isfinite(gap.view(F32)).all() and gap.view(F32).abs().sum() > 0


def test_resnet_pass_carries_nothing_between_calls(hip):
    """crw_rn_train_fwd + _bwd at 16 x 16 on one batch, then on a second batch of other values in the SAME workspace and outputs,
    un-refilled: bit for bit what the second batch gives on freshly zero-filled ones (tickets left zeroed, no slab of the previous
    step added in)."""
    case = rn_pass(hip, "train", 130, 16, 16, 1)
    g = _gen(99)
    sr.run_reused(case, (_randn(g, 130, 1, 16, 16, scale=1.3, shift=-0.2), _randn(g, 130, 128)))
