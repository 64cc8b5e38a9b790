"""The conv-trunk chain kernel (csrc/encoder_conv.hip, `crw_enc_conv_fwd_chain`): conv3 -> conv4 -> conv5 of a patch in one workgroup,
the activations handed from layer to layer in LDS.  It runs the per-layer kernel's own k-loops and epilogues, so every output must
equal, bit for bit, what three `crw_enc_conv3x3` launches write -- there is no tolerance anywhere in this file.

  * bitwise: P in {1, 2, 5, 513} (513 > the 512 workgroups resident at once: a second round on LDS that a chain has used), post-ReLU
    inputs with exact zeros; and one case whose activations are strictly positive in every layer, so that a halo left from the
    previous layer's image (another row stride) would change every border pixel of the next layer;
  * stale memory and guard bands: the entry point under `run_twice` and `run_banded` of tests/stale_ref.py;
  * whole model: `_HipEncoder` forward and backward with the chain against CRW_CONV_CHAIN=0 -- pooled features and every gradient
    bit-equal -- and the per-layer route while bench.py's kernel events are collected."""
import ctypes

import pytest
import torch

import stale_ref as sr
from stale_ref import Buf, Case

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LAYERS = ((32, 64), (64, 128), (128, 128))  # (cin, cout) of conv3, conv4, conv5
OUTPUTS = ("y3_hi", "y3_lo", "y4_hi", "y4_lo", "y5_hi", "gap")


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    assert crw_hip.has_conv_chain(), "the library was built without crw_enc_conv_fwd_chain"
    return crw_hip


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _planes(x):
    """fp32 [P,100,C] -> (hi, lo) bf16 planes, x = hi + lo to fp32 grade; an exact zero stays zero in both"""
    hi = x.to(BF16)
    return hi, (x - hi.float()).to(BF16)


def _inputs(hip, P, positive, seed):
    """x3 planes, packed forward weights and biases of the three layers.  positive: inputs, weights and biases all > 0, so every
    activation of every layer is > 0 (asserted by the caller on the reference)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, 100, 32, generator=g)
    x = (x.abs() + 0.25) if positive else torch.relu(x)          # relu: about half the entries are exact zeros
    xh, xl = _planes(x.cuda())
    packed, biases = [], []
    for cin, cout in LAYERS:
        w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        if positive:
            w, b = w.abs() * 0.1, b.abs() + 0.01
        packed.append(hip.enc_pack_weights(w.cuda(), 3))
        biases.append(b.cuda())
    return xh, xl, packed, biases


def _per_layer(hip, xh, xl, packed, biases):
    y3h, y3l, _, _ = hip.enc_conv3x3(0, 3, xh, xl, packed[0][0], packed[0][1], 64, bias=biases[0])
    y4h, y4l, _, _ = hip.enc_conv3x3(0, 3, y3h, y3l, packed[1][0], packed[1][1], 128, bias=biases[1])
    y5h, _, _, gap = hip.enc_conv3x3(0, 3, y4h, y4l, packed[2][0], packed[2][1], 128, bias=biases[2], gap=True, lo_plane=False)
    return dict(zip(OUTPUTS, (y3h, y3l, y4h, y4l, y5h, gap)))


_REFERENCE = {}


def _reference(hip, P, positive=False):
    """inputs and per-layer result of one (P, kind), computed once for the module and never written to"""
    key = (P, positive)
    if key not in _REFERENCE:
        inp = _inputs(hip, P, positive, seed=100 + P + 7 * positive)
        _REFERENCE[key] = (inp, _per_layer(hip, *inp))
        torch.cuda.synchronize()
    return _REFERENCE[key]


def _assert_equal(got, ref):
    for name in OUTPUTS:
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape, name
        same = got[name].view(torch.int16 if got[name].dtype == BF16 else torch.int32) == \
            ref[name].view(torch.int16 if ref[name].dtype == BF16 else torch.int32)
        assert bool(same.all()), (name, "entries that differ:", int((~same).sum()), "of", same.numel(),
                                  "first at", (~same).nonzero()[0].tolist())
        assert torch.equal(got[name], ref[name]), name


@pytest.mark.parametrize("P", [1, 2, 5, 513])
def test_forward_chain_is_bitwise_the_three_layers(hip, P):
    (xh, xl, packed, biases), ref = _reference(hip, P)
    assert float((xh.float() == 0).float().mean()) > 0.3                     # exact zeros, like a post-ReLU plane
    assert float(ref["y5_hi"].float().abs().max()) > 0 and float(ref["gap"].abs().max()) > 0
    got = dict(zip(OUTPUTS, hip.enc_conv_fwd_chain(xh, xl, packed, biases)))
    _assert_equal(got, ref)


def test_forward_chain_rezeroes_the_halo_between_layers(hip):
    """every activation > 0: the halo pixels of a layer's image overlap interior pixels of the previous one"""
    (xh, xl, packed, biases), ref = _reference(hip, 5, positive=True)
    for name in ("y3_hi", "y4_hi", "y5_hi"):
        assert bool((ref[name].float() > 0).all()), name
    got = dict(zip(OUTPUTS, hip.enc_conv_fwd_chain(xh, xl, packed, biases)))
    _assert_equal(got, ref)


def _chain_case(hip, P, home):
    lib = hip.lib()
    xh, xl, packed, biases = _reference(hip, P)[0]
    ops = home.many(x_hi=xh, x_lo=xl, w3_hi=packed[0][0], w3_lo=packed[0][1], b3=biases[0], w4_hi=packed[1][0], w4_lo=packed[1][1],
                    b4=biases[1], w5_hi=packed[2][0], w5_lo=packed[2][1], b5=biases[2])
    bufs = dict(y3_hi=Buf(P * 100 * 64 * 2, BF16), y3_lo=Buf(P * 100 * 64 * 2, BF16), y4_hi=Buf(P * 100 * 128 * 2, BF16),
                y4_lo=Buf(P * 100 * 128 * 2, BF16), y5_hi=Buf(P * 100 * 128 * 2, BF16), gap=Buf(P * 128 * 4))

    def run(_, t):
        status = lib.crw_enc_conv_fwd_chain(3, P, *[_p(o) for o in ops], *[_p(t[k]) for k in OUTPUTS], _stream())
        assert status == 0, ("crw_enc_conv_fwd_chain", "status", status)
        torch.cuda.synchronize()
    return Case("crw_enc_conv_fwd_chain", None, bufs, run, device="cuda", home=home)


def _assert_bytes_equal(out, ref):
    for name in OUTPUTS:
        assert torch.equal(out[name], ref[name].reshape(-1).view(torch.uint8)), name


def test_forward_chain_ignores_stale_memory(hip):
    """outputs poisoned with 0xFF and with 0x00: finite, bit-identical, and the per-layer result"""
    out = sr.run_twice(_chain_case(hip, 5, sr.PLAIN))
    _assert_bytes_equal(out, _reference(hip, 5)[1])


def test_forward_chain_stays_inside_its_operands(hip):
    """every operand between guard bands of 0xFF and of 0x00: nothing read from them, nothing written to them"""
    out = sr.run_banded(_chain_case(hip, 5, sr.Home("cuda")))
    _assert_bytes_equal(out, _reference(hip, 5)[1])


def test_forward_chain_refuses_what_it_does_not_run(hip):
    lib = hip.lib()
    (xh, xl, packed, biases), ref = _reference(hip, 1)
    outs = [torch.empty_like(ref[k]) for k in OUTPUTS]
    w = [_p(a) for pk, b in zip(packed, biases) for a in (pk[0], pk[1], b)]
    call = lambda split, P, x_lo, y4_lo: lib.crw_enc_conv_fwd_chain(split, P, _p(xh), x_lo, *w, _p(outs[0]), _p(outs[1]), _p(outs[2]), y4_lo,
                                                                    _p(outs[4]), _p(outs[5]), _stream())
    assert call(1, 1, _p(xl), _p(outs[3])) == hip.CRW_EINVAL        # plain bf16 stays per-layer
    assert call(3, 0, _p(xl), _p(outs[3])) == hip.CRW_EINVAL
    assert call(3, 1, None, _p(outs[3])) == hip.CRW_EINVAL
    assert call(3, 1, _p(xl), None) == hip.CRW_EINVAL               # the next layer reads the lo plane: not optional
    assert call(3, 1, _p(xl), _p(outs[3])) == 0
    torch.cuda.synchronize()


def _encoder_step(hip, enc, x, r):
    import encoder
    params = [p for i in range(1, 6) for p in (getattr(enc, f"conv{i}").weight, getattr(enc, f"conv{i}").bias)]
    for p in params:
        p.grad = None
    gap = encoder._HipEncoder.apply(x, *params, 3, None)
    (gap * r).sum().backward()
    torch.cuda.synchronize()
    return gap.detach().clone(), [p.grad.detach().clone() for p in params]


def test_whole_encoder_with_and_without_the_chain(hip, monkeypatch):
    """B = 1, T = 2, N = 3: P = 6 patches through `_HipEncoder`, forward and backward"""
    import encoder
    torch.manual_seed(5)
    enc = encoder.CNN(False).cuda()
    x = torch.randn(6, 1, 16, 16).cuda()
    r = torch.randn(6, 128).cuda()
    calls = []
    chain = hip.enc_conv_fwd_chain
    monkeypatch.setattr(hip, "enc_conv_fwd_chain", lambda *a: (calls.append(1), chain(*a))[1])

    monkeypatch.delenv("CRW_CONV_CHAIN", raising=False)
    gap1, grads1 = _encoder_step(hip, enc, x, r)
    assert len(calls) == 1                                                  # the chain ran
    monkeypatch.setenv("CRW_CONV_CHAIN", "0")                               # read per call
    gap0, grads0 = _encoder_step(hip, enc, x, r)
    assert len(calls) == 1                                                  # ... and here it did not
    assert float(gap0.abs().max()) > 0 and torch.equal(gap1, gap0)
    assert len(grads0) == 10
    for i, (a, b) in enumerate(zip(grads1, grads0)):
        assert float(b.abs().max()) > 0 and torch.equal(a, b), ("gradient of parameter", i)

    monkeypatch.delenv("CRW_CONV_CHAIN")
    monkeypatch.setattr(hip, "KERNEL_EVENTS", {})                           # bench.py's roofline names per-layer kernels
    gap2, _ = _encoder_step(hip, enc, x, r)
    assert len(calls) == 1 and torch.equal(gap2, gap0)
    assert {("fwd", 32, 64), ("fwd", 64, 128), ("fwd", 128, 128)} <= set(hip.KERNEL_EVENTS)
