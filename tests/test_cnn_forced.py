"""CPU proof of tests/cnn_forced_ref.py, the gate-forced fp64 reference that tests/test_cnn_forced_gpu.py holds the `CNN`
training step to: forced with its own gates it IS the oracle, bit for bit; forced with other gates it moves by what those gates are
worth and no more; the audit reports a gate outside its margin; the spy reads the planes in the layout the kernels write."""
import types

import pytest
import torch

import cnn_forced_ref as fr
from conftest import load_golden
from oracle import crw_oracle as orc


def _case(name):
    """-> (seq [B,T,N,h,w] fp32, state dict fp32, tau, pos_embed)"""
    if name == "cnn_cfg1_B2T8N7":
        g, w = load_golden(name), load_golden("cnn_weights_seed11")
        return torch.tensor(g["seq"]), {k: torch.tensor(v) for k, v in w.items()}, float(g["tau"]), bool(g["pos_embed"])
    import dataset as crw_dataset
    import encoder as crw_encoder
    T, (h, w), ov = 4, (20, 27), (10, 0)
    ds = crw_dataset.RGDataset.synthetic(ov[0] + 5 * (h - ov[0]), 2 * T * w, T, (h, w), ov, seed=13)
    torch.manual_seed(11)
    sd = {k: v.detach().clone() for k, v in crw_encoder.CNN(False).state_dict().items()}
    return ds[0][None].contiguous(), sd, 0.05, False


CASES = ["cnn_cfg1_B2T8N7", "item_20x27"]


def _leaves(sd, dtype):
    return {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd.items()}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", CASES)
def test_forced_with_own_gates_is_the_oracle_bit_for_bit(name, dtype):
    """`z * (z > 0)` is `relu(z)` and passes the gradient where relu does: loss, logits, features and every parameter gradient of
    the helper forced with the gates of its own forward equal `oracle.crw_forward_torch` bit for bit (so does the helper left
    free-running).  A helper that restated a layer, a padding or the head differently could not."""
    seq, sd0, tau, pe = _case(name)
    seq = seq.to(dtype)
    sd = _leaves(sd0, dtype)
    loss, A, emb = orc.crw_forward_torch(seq, sd, tau, use_pos_embed=pe)
    loss.backward()
    free = fr.crw_forward_forced(seq, _leaves(sd0, dtype), tau, pe)
    for gates in (None, fr.own_gates(free.z)):
        sd2 = _leaves(sd0, dtype)
        out = fr.crw_forward_forced(seq, sd2, tau, pe, gates=gates)
        out.loss.backward()
        assert torch.equal(out.loss, loss) and torch.equal(out.A, A) and torch.equal(out.emb, emb)
        for k in sd:
            assert torch.equal(sd2[k].grad, sd[k].grad), k
        assert out.x3.grad is not None and out.x3.grad.shape == out.x3.shape and out.x3.grad.abs().max() > 0
        for z, z0 in zip(out.z, free.z):
            assert torch.equal(z, z0) and not z.requires_grad


@pytest.mark.parametrize("name", CASES)
def test_flipped_gates_move_the_features_within_the_sum_of_their_margins(name):
    """Every gate whose pre-activation lies within the format bound, |z| <= e, turned over: exactly the freedom the audit leaves
    the device.  Turning a gate moves its activation by |z|, so the features move by at most
        |fc.weight| mean_pixels(d5),   d3 = |z3| f3,   d_{l+1} = conv(d_l, |w_{l+1}|) + |z_{l+1}| f_{l+1}     (f: turned or not)
    (`flip_feature_bound`).  Held for both bounds: each layer's own arithmetic (carry=False), where the turned gates are worth less
    than the forward's own 1e-4 of the feature scale -- forcing such gates moves the forward by rounding -- and the bound with the lower layers'
    errors carried through |w| (carry=True), which by conv5 covers nearly every pre-activation: the inequality still holds, and the
    figures printed here are why the GPU tests also audit every layer on the device's own input (`layer_audit`)."""
    seq, sd0, tau, pe = _case(name)
    sd = {k: v.double() for k, v in sd0.items()}
    with torch.no_grad():
        free = fr.crw_forward_forced(seq.double(), sd, tau, pe)
        scale = free.emb.abs().max().item()
        seen = {}
        for carry in (False, True):
            es = fr.format_bounds(free.x, sd, carry=carry)
            assert all(e.shape == z.shape and (e > 0).all() for e, z in zip(es, free.z))
            gates, flips = fr.flipped_gates(free.z, es)
            n = [int(f.sum()) for f in flips]
            out = fr.crw_forward_forced(seq.double(), sd, tau, pe, gates=gates)
            moved = (out.emb - free.emb).abs().reshape(-1, free.emb.shape[-1])
            bound = fr.flip_feature_bound(free.z, flips, sd)
            assert (moved <= bound * (1 + 1e-9) + 1e-15 * scale).all(), (carry, n, float((moved - bound).max()))
            seen[carry] = (n, moved.max().item() / scale, bound.max().item() / scale)
            # what the audit says about these gates: every difference inside the margin they were turned at, none outside
            for (cnt, outside, worst), k in zip(fr.gate_audit(gates, free.z, es, 1.0), n):
                assert cnt == k and outside == 0 and worst <= 1.0
        print(f"{name}: carry -> (gates turned per layer, features moved, bound; of the feature scale): {seen}")
        assert all(k > 0 for k in seen[False][0]) and 0 < seen[False][1] < 1e-4   # (measured 2e-6; worst case through |w| 2e-4)
        assert all(a >= b for a, b in zip(seen[True][0], seen[False][0])) and seen[True][1] > seen[False][1]
        # the sharp audit on the reference's own activations finds nothing to report, and sees a gate closed far from zero
        acts = [free.x3] + [torch.relu(z) for z in free.z[:2]]
        own = list(fr.own_gates(free.z))
        assert fr.layer_audit(acts, own, sd) == [(0, 0, 0.0)] * 3
        i = free.z[1].flatten().argmax()
        own[1] = own[1].clone()
        own[1].view(-1)[i] = False
        assert [r[:2] for r in fr.layer_audit(acts, own, sd)] == [(0, 0), (1, 1), (0, 0)]


def test_gate_audit_reports_a_gate_outside_the_margin():
    """One open gate closed where z is far from zero, one inside the margin: the audit counts both and puts one outside."""
    g = torch.Generator().manual_seed(0)
    z = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    e = torch.full_like(z, 1e-3)
    z[0, 0, 0, 0], z[1, 2, 3, 4] = 0.5, 1.5e-3
    gates = z > 0
    assert fr.gate_audit([gates], [z], [e]) == [(0, 0, 0.0)]
    gates[0, 0, 0, 0] = False
    gates[1, 2, 3, 4] = False
    (cnt, outside, worst), = fr.gate_audit([gates], [z], [e])
    assert (cnt, outside) == (2, 1) and abs(worst - 500.0) < 1e-9


def test_bar_is_four_times_the_worst_rounded_up_to_one_digit():
    for worst, bar in ((2.2e-6, 9e-6), (2.5e-6, 1e-5), (2.6e-6, 2e-5), (1e-7, 4e-7), (7.4e-4, 3e-3), (0.0, 0.0)):
        assert abs(fr.bar_from(worst) - bar) <= 1e-12 * max(bar, 1e-30), (worst, fr.bar_from(worst), bar)
        assert fr.bar_from(worst) >= 4 * worst


def test_bar_tables_are_consistent():
    """Every bar is `bar_from` of its recorded worst value; the four-case bars are never looser than the five-case ones; "mixed"
    runs the default's forward and head, so it carries the default's bars there; the loss keeps 1e-4."""
    keys = set(fr.WORST["bf16x3"]) | {"loss"}
    for arith, bars in fr.BARS.items():
        assert set(bars) == keys and bars["loss"] == 1e-4
        for k, (v, case) in fr.WORST[arith].items():
            assert bars[k] == fr.bar_from(v) and 4 * v <= bars[k] < 10 * v and case in "abcde"
    assert all(fr.BARS_ACDE[k] <= fr.BARS["bf16x3"][k] for k in keys) and set(fr.BARS_ACDE) == keys
    assert all(case != "b" for _, case in fr.WORST_ACDE.values())
    for k in ("x3", "features", "A", "fc.weight", "fc.bias"):
        assert fr.BARS["mixed"][k] == fr.BARS["bf16x3"][k]
    assert fr.bars_for("bf16x3", "b_posembed_B1T4N3") is fr.BARS["bf16x3"] and fr.bars_for("bf16x3", "P2016") is fr.BARS_ACDE
    assert fr.bars_for("mixed", "a_cfg1_B2T8N7") is fr.BARS["mixed"]


def test_spy_records_planes_gates_and_the_front_backward(monkeypatch):
    """The spy on a stand-in module with the bindings' signatures: calls go through unchanged, mode-1 calls leave no gate, planes
    [P, H*W, C] come back as [P, C, H, W], the front backward's dy and return are kept, and the originals return on exit."""
    P, H, W = 2, 3, 4
    hi = torch.arange(P * H * W * 5, dtype=torch.float32).reshape(P, H * W, 5).bfloat16()
    lo = torch.full_like(hi, 2.0 ** -10)
    ret5 = (torch.ones(8, 1, 5, 5), torch.ones(8), torch.ones(32, 8, 5, 5), torch.ones(32))

    def enc_front_fwd(split, x, w1, b1, w2f, b2, save=False):
        return hi, lo, None

    def enc_front_fwd_map(split, x, w1, b1, w2f, b2):
        return hi, None

    def enc_conv3x3(mode, split, xh, xl, wh, wl, cout, bias=None, mask=None, planes=True, f32=False, gap=False, dgap=None,
                    lo_plane=True):
        return xh, xl, None, None

    def enc_conv3x3_map(split, xh, xl, wh, wl, cout, H, W, bias=None, planes=True, gap=False, lo_plane=True, mode=0, mask=None,
                        f32=False):
        return xh, xl, None

    def enc_front_bwd(split, x, w1, b1, w2f, b2, w2b, dy, saved=None):
        return ret5

    def enc_front_bwd_map(split, x, w1, b1, w2f, b2, w2b, dy):
        return ret5

    mod = types.SimpleNamespace(**{f.__name__: f for f in (enc_front_fwd, enc_front_fwd_map, enc_conv3x3, enc_conv3x3_map,
                                                            enc_front_bwd, enc_front_bwd_map)})
    x = torch.zeros(P, 1, H + 6, W + 6)
    with fr.spy(monkeypatch, mod) as rec:
        assert mod.enc_front_fwd_map(3, x, None, None, None, None)[0] is hi
        mod.enc_conv3x3_map(3, hi, lo, None, None, 5, H, W)
        mod.enc_conv3x3_map(3, hi, lo, None, None, 5, H, W, mode=1)
        dy = torch.randn(P, H * W, 32)
        assert mod.enc_front_bwd_map(3, x, None, None, None, None, None, dy) is ret5
        dy0 = dy.clone()
        dy.zero_()  # the record holds a copy
    assert mod.enc_conv3x3_map is enc_conv3x3_map and mod.enc_front_bwd_map is enc_front_bwd_map
    assert rec.hw == (H, W) and len(rec.x3) == 1 and torch.equal(rec.x3[0], hi.double())
    assert len(rec.gates) == 1 and rec.gates[0].shape == (P, 5, H, W)
    assert torch.equal(rec.gates[0][1, 2], hi[1, :, 2].reshape(H, W) != 0) and not rec.gates[0][0, 0, 0, 0]
    assert torch.equal(rec.dx3[0], dy0) and all(a is b for a, b in zip(rec.front_grads[0], ret5)) and rec.front_call[0][0] == "enc_front_bwd_map"
    assert rec.calls["enc_conv3x3_map"] == 2 and rec.calls["enc_front_bwd"] == 0
    x16 = torch.zeros(P, 1, 16, 16)
    h16 = torch.ones(P, 100, 4).bfloat16()
    with fr.spy(monkeypatch, mod) as rec:
        mod.enc_front_fwd(3, x16, None, None, None, None, save=True)
        mod.enc_conv3x3(0, 3, h16, None, None, None, 4)
        mod.enc_conv3x3(1, 3, h16, None, None, None, 4)
    assert rec.hw == (10, 10) and torch.equal(rec.x3[0], hi.double() + lo.double())
    assert len(rec.gates) == 1 and rec.gates[0].shape == (P, 4, 10, 10) and rec.gates[0].all()
