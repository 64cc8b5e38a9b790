"""Gate-forced fp64 reference of the `CNN` training step, format-derived bounds on its pre-activations, and a spy on the encoder's
kernel calls.  TEST INFRASTRUCTURE ONLY; no GPU code, importable on the CPU.  Proved by tests/test_cnn_forced.py (CPU), used by
tests/test_cnn_forced_gpu.py and test_hip_parity.test_full_model_at_baseline_shape_vs_oracle.

Why forced.  An fp32-grade forward and an fp64 forward may open a ReLU differently where a pre-activation is within ~1e-5 of
zero, and one flipped gate moves a whole gradient term: against a free-running reference the weight gradients can only be held to
per cent.  Here the device's own gates of conv3..conv5 (its activation planes are non-zero exactly where the gate is open) are
imposed on the fp64 forward, `relu(z)` becoming `z * gate`; both sides then differentiate the SAME piecewise-linear function and
every gradient entry is comparable.  `gate_audit` keeps the forcing honest: a device gate may differ from `z > 0` only where
`|z| <= 2 e`, `e` being what the kernels' number formats can add to `z` (`format_bounds`), so a wrong gate cannot hide behind it.

The front end (conv1-ReLU-pool-conv2-ReLU-pool) stays free-running: its pooling record is opaque.  The gradient that crosses into
it, `dx3`, is a plain fp32 argument of `crw_hip.enc_front_bwd[_map]`; the spy records it and `x3.grad` is its reference."""
import contextlib
import inspect
import types

import torch
import torch.nn.functional as TF

from oracle import crw_oracle as orc

U24, U18 = 2.0 ** -24, 2.0 ** -18
LAYERS = ("conv3", "conv4", "conv5")


# ------------------------------------------------------------------------------------------------ format-derived bounds
def fp32_conv_bound(x_abs, w, b, K):
    """What fp32 FMA arithmetic can add to conv(x, w) + b: at most K roundings of 2^-24 on the sum of absolute products."""
    return K * U24 * TF.conv2d(x_abs, w.abs(), b.abs(), padding=1)


def split_conv_bound(a_abs, w, b, K, e_in):
    """What a convolution on bf16 hi/lo operand pairs with fp32 accumulation can add to conv(a, w) + b.  8-bit significands:
    |lo| <= 2^-9 |hi|, the lo.lo product is dropped and each lo is itself rounded -- 3 * 2^-18 on the sum of absolute products;
    the accumulation K * 2^-24 on the same sum (K the reduction length); plus the bound `e_in` of the layer below carried through
    |w|."""
    return (3 * U18 + K * U24) * TF.conv2d(a_abs, w.abs(), b.abs(), padding=1) + TF.conv2d(e_in, w.abs(), None, padding=1)


def front_bounds(xd, w1, b1, w2, b2):
    """fp64 front end up to conv2's pre-activations with the bounds of both layers: conv1 is fp32 FMA (at most 64 roundings),
    conv2 runs on hi/lo pairs with fp32 accumulation over 256 products, plus conv1's bound carried through the pool (a maximum
    moves by no more than its candidates do).  -> namespace(pre1, e1, a1, pre2, e2)."""
    pre1 = TF.conv2d(xd, w1, b1, padding=1)
    e1 = fp32_conv_bound(xd.abs(), w1, b1, 64)
    a1 = TF.max_pool2d(TF.relu(pre1), 2, 1)
    pre2 = TF.conv2d(a1, w2, b2, padding=1)
    e2 = split_conv_bound(a1, w2, b2, 256, TF.max_pool2d(e1, 2, 1))
    return types.SimpleNamespace(pre1=pre1, e1=e1, a1=a1, pre2=pre2, e2=e2)


def format_bounds(x, sd, carry=True):
    """(e3, e4, e5) [P,C,H,W] fp64: per-element bounds on what the default arithmetic (hi/lo pairs, fp32 accumulation) can add to
    the pre-activations z3..z5, from the free-running fp64 reference alone: x [P,cin,h,w] the patches (after pos_embed), sd the
    parameters.  ReLU and max-pool are 1-Lipschitz per element / per window, so a layer's bound passes through them unchanged.

    carry=True: the bound of the layer below is carried through |w| -- a worst case in which every error below has the sign of its
    weight.  It is rigorous and it grows ~10x per layer (|w| sums to ~8.5 per output while the signal, with mixed signs, shrinks):
    at the golden weights it covers 0.5 % of conv3's pre-activations, 15 % of conv4's and practically all of conv5's.
    carry=False: each layer's own arithmetic alone, on exact inputs (2e-4 .. 9e-4 of the pre-activations lie inside it); the bound
    `layer_audit` holds a layer to when its input is the device's own."""
    with torch.no_grad():
        p = {k: v.detach().to(x.device, torch.float64) for k, v in sd.items()}
        f = front_bounds(x.double(), p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"])
        a = TF.max_pool2d(TF.relu(f.pre2), 2, 1)
        e = TF.max_pool2d(f.e2, 2, 1)
        out = []
        for name in LAYERS:
            w, b = p[name + ".weight"], p[name + ".bias"]
            e = split_conv_bound(a, w, b, 9 * w.shape[1], e if carry else torch.zeros_like(a))
            out.append(e)
            a = TF.relu(TF.conv2d(a, w, b, padding=1))
    return tuple(out)


def layer_audit(inputs, gates, sd, margin=2.0):
    """The sharp form of the gate audit, layer by layer on the DEVICE's own inputs: inputs[l] [P,C,H,W] fp64 is what the device fed
    to conv3 / conv4 / conv5 (hi + lo of its planes, exact), so fp64 z = conv(input, w) + b differs from the device's
    pre-activation by that one layer's arithmetic only, bounded by `split_conv_bound` with nothing carried.  Per layer: (gates that
    differ from z > 0, how many of them lie outside |z| <= margin * e, the largest |z| / e among them)."""
    out = []
    with torch.no_grad():
        for name, a, g in zip(LAYERS, inputs, gates):
            w, b = (sd[name + k].detach().to(a.device, torch.float64) for k in (".weight", ".bias"))
            z = TF.conv2d(a, w, b, padding=1)
            e = split_conv_bound(a.abs(), w, b, 9 * w.shape[1], torch.zeros_like(a))
            out.append(gate_audit([g], [z], [e], margin)[0])
    return out


# ------------------------------------------------------------------------------------------------ the forced model
def cnn_forward_forced(x, sd, gates=None):
    """`oracle.cnn_forward` with optional gates: conv1-ReLU-pool-conv2-ReLU-pool free-running, then conv3..conv5 with
    `z * gate` in place of `relu(z)` where gates = (g3, g4, g5), bool [P,C,H,W]; average pool and head as the oracle's.
    -> (features, x3 (retain_grad when it carries one), [z3, z4, z5] detached)."""
    x = TF.max_pool2d(TF.relu(TF.conv2d(x, sd["conv1.weight"], sd["conv1.bias"], padding=1)), 2, 1)
    x = TF.max_pool2d(TF.relu(TF.conv2d(x, sd["conv2.weight"], sd["conv2.bias"], padding=1)), 2, 1)
    x3 = x
    if x3.requires_grad:
        x3.retain_grad()
    zs = []
    for i, name in enumerate(LAYERS):
        z = TF.conv2d(x, sd[name + ".weight"], sd[name + ".bias"], padding=1)
        zs.append(z.detach())
        x = TF.relu(z) if gates is None else z * gates[i].to(z.dtype)
    x = x.mean((2, 3))
    return TF.linear(x, sd["fc.weight"], sd["fc.bias"]), x3, zs


def crw_forward_forced(seq, sd, tau, use_pos_embed=False, gates=None):
    """`oracle.crw_forward_torch` on `cnn_forward_forced`, in seq's dtype on seq's device.
    -> namespace(loss, A, emb [B,T,N,C], x3, z=[z3,z4,z5], x (the patches that entered conv1))."""
    B, T, N, h, w = seq.shape
    x = seq.reshape(-1, h, w).unsqueeze(1)
    if use_pos_embed:  # the oracle builds the ramp in fp32 on the CPU, as the model does: the same values in any dtype
        x = orc.pos_embed(x.cpu()).to(seq.device)
    feats, x3, zs = cnn_forward_forced(x, sd, gates)
    emb = feats.reshape(B, T, N, -1)
    loss, A = orc.walk_loss_torch(emb, tau)
    return types.SimpleNamespace(loss=loss, A=A, emb=emb, x3=x3, z=zs, x=x)


def own_gates(zs):
    return tuple(z > 0 for z in zs)


def gate_audit(gates, zs, es, margin=2.0):
    """Per layer: (number of positions where the device's gate differs from `z_ref > 0`, how many of them lie OUTSIDE
    `|z_ref| <= margin * e`, the largest |z_ref| / e among them).  The second number must be zero."""
    out = []
    for g, z, e in zip(gates, zs, es):
        diff = g.to(z.device) != (z > 0)
        ratio = (z.abs() / e)[diff]
        out.append((int(diff.sum()), int((ratio > margin).sum()), float(ratio.max()) if ratio.numel() else 0.0))
    return out


def flipped_gates(zs, es, margin=1.0):
    """The free-running gates with every decision inside `|z| <= margin * e` turned over -> (gates, flips per layer)."""
    gates, flips = [], []
    for z, e in zip(zs, es):
        near = z.abs() <= margin * e
        gates.append((z > 0) ^ near)
        flips.append(near)
    return tuple(gates), flips


def flip_feature_bound(zs, flips, sd):
    """How far turning over the gates at `flips` can move the features [P,128], per entry.  A turned gate puts 0 where relu(z) = z
    was, or z <= 0 where 0 was: it moves that activation by exactly |z|.  Through the layers: with d_l the bound on a layer's activations,
        d3 = |z3| f3,    d_{l+1} = conv(d_l, |w_{l+1}|) + |z_{l+1}| f_{l+1}
    (a forced layer is linear where its gate is held, so what arrives from below passes with |w| and the gate <= 1; where the
    gate itself is turned, |z_{l+1}| of the UNperturbed forward is added), then the average pool and |fc.weight|."""
    d = None
    for name, z, f in zip(LAYERS, zs, flips):
        own = z.abs() * f.to(z.dtype)
        d = own if d is None else TF.conv2d(d, sd[name + ".weight"].detach().abs(), None, padding=1) + own
    return d.mean((2, 3)) @ sd["fc.weight"].detach().abs().t()


# ------------------------------------------------------------------------------------------------ measures
def rel_err(got, ref):
    """Largest entry-wise error relative to the reference tensor's largest entry."""
    ref = ref.detach().double()
    return float((got.detach().double().to(ref.device) - ref).abs().max() / ref.abs().max())


def planes_value(hi, lo):
    """hi + lo in fp64 (exact: the pair spans at most the 24 bits of the fp32 value it was split from)."""
    return hi.double() + (lo.double() if lo is not None else 0)


def planes_nchw(t, H, W):
    """channels-last planes / maps [P, H*W, C] -> [P, C, H, W]."""
    P, _, C = t.shape
    return t.reshape(P, H, W, C).permute(0, 3, 1, 2)


def bar_from(worst):
    """4 x the worst measured value, rounded UP to one significant digit."""
    import math
    v = 4.0 * worst
    if v <= 0:
        return 0.0
    q = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / q - 1e-9) * q


# ------------------------------------------------------------------------------------------------ the bars
# The worst error of every asserted quantity over the five cases of tests/test_cnn_forced_gpu.py, as first measured on an MI355X
# (profiles/cnn_forced_tests.log), with the case it comes from.  Entry-wise maximum relative to the reference tensor's largest
# entry; A relative to 1 / tau.  The bar is 4 x that value rounded up to one significant digit (`bar_from`): the kernels are
# bit-reproducible, so the margin is for other seeds and compiler versions, not for run-to-run noise.  The loss keeps the
# north_star's 1e-4 relative in every arithmetic.  (b), 12 patches with two input channels, is the worst-conditioned case in
# every arithmetic -- its bias gradients nearly cancel -- and sets most backward bars; on the other four the default stays below
# 1.8e-5 on dx3 and below 1.1e-5 on every parameter gradient.
WORST = {
    "bf16x3": {"x3": (8.045e-06, "a"), "features": (1.303e-06, "c"), "A": (6.021e-07, "c"),                  # bars 4e-5, 6e-6, 3e-6
               "dx3": (1.764e-05, "a"),                                                                      # 8e-5
               "conv3.weight": (1.027e-05, "b"), "conv3.bias": (1.060e-05, "b"),                             # 5e-5, 5e-5
               "conv4.weight": (2.502e-05, "b"), "conv4.bias": (2.736e-05, "b"),                             # 2e-4, 2e-4
               "conv5.weight": (3.000e-05, "b"), "conv5.bias": (6.945e-05, "b"),                             # 2e-4, 3e-4
               "fc.weight": (1.845e-05, "b"), "fc.bias": (1.238e-04, "b")},                                  # 8e-5, 5e-4
    # the default's forward bit for bit (so its forward and fc figures); the backward on the hi planes alone; 16x16 cases (a)-(c)
    "mixed": {"x3": (8.045e-06, "a"), "features": (1.303e-06, "c"), "A": (6.021e-07, "c"),                   # 4e-5, 6e-6, 3e-6
              "dx3": (4.600e-03, "a"),                                                                       # 2e-2
              "conv3.weight": (5.173e-03, "b"), "conv3.bias": (7.723e-03, "b"),                              # 3e-2, 4e-2
              "conv4.weight": (1.122e-02, "b"), "conv4.bias": (1.180e-02, "b"),                              # 5e-2, 5e-2
              "conv5.weight": (2.309e-02, "b"), "conv5.bias": (5.020e-02, "b"),                              # 1e-1, 3e-1
              "fc.weight": (1.845e-05, "b"), "fc.bias": (1.238e-04, "b")},                                   # 8e-5, 5e-4
    "bf16": {"x3": (5.870e-03, "a"), "features": (1.021e-03, "e"), "A": (1.207e-05, "c"),                    # 3e-2, 5e-3, 5e-5
             "dx3": (7.633e-03, "b"),                                                                        # 4e-2
             "conv3.weight": (8.899e-03, "b"), "conv3.bias": (9.062e-03, "b"),                               # 4e-2, 4e-2
             "conv4.weight": (2.014e-02, "b"), "conv4.bias": (2.195e-02, "b"),                               # 9e-2, 9e-2
             "conv5.weight": (2.084e-02, "b"), "conv5.bias": (5.095e-02, "b"),                               # 9e-2, 3e-1
             "fc.weight": (8.686e-03, "b"), "fc.bias": (3.533e-03, "b")},                                    # 4e-2, 2e-2
}
BARS = {arith: dict({k: bar_from(v) for k, (v, _) in worst.items()}, loss=1e-4) for arith, worst in WORST.items()}
# What that costs: with conv4's weight gradient reading a zero lo plane of y3 (a deliberate local edit), conv4.weight is 1.3e-4 off
# on (a) and 7.5e-5 on (c) -- 22 x and 11 x the default's own error there, and still under the 2e-4 that (b) sets.  So the default
# arithmetic is ALSO held, on every case but (b) and on the P = 2016 item of test_hip_parity.py, to the bars of those four cases:
WORST_ACDE = {"conv3.weight": (6.361e-06, "d"), "conv3.bias": (6.015e-06, "d"),                              # 3e-5, 3e-5
              "conv4.weight": (6.936e-06, "c"), "conv4.bias": (5.272e-06, "d"),                              # 3e-5, 3e-5
              "conv5.weight": (4.356e-06, "a"), "conv5.bias": (3.850e-06, "e"),                              # 2e-5, 2e-5
              "fc.weight": (1.016e-05, "a"), "fc.bias": (9.874e-06, "a")}                                    # 5e-5, 4e-5
BARS_ACDE = dict(BARS["bf16x3"], **{k: bar_from(v) for k, (v, _) in WORST_ACDE.items()})


def bars_for(arith, case):
    """The bars a case is held to: `BARS[arith]`; the default arithmetic on any case but (b): the sharper `BARS_ACDE`."""
    return BARS_ACDE if arith == "bf16x3" and not case.startswith("b") else BARS[arith]


# ------------------------------------------------------------------------------------------------ the spy
SPIED = ("enc_front_fwd", "enc_front_fwd_map", "enc_conv3x3", "enc_conv3x3_map", "enc_front_bwd", "enc_front_bwd_map")


class Record:
    """What one forward + backward of `CNN` handed to / got from the six spied functions (all calls go through unchanged)."""

    def __init__(self):
        self.x3 = []           # per front-end forward: hi + lo, fp64 [P, H*W, 32]
        self.hw = None         # (H, W) of the conv3..conv5 feature map
        self.gates = []        # per mode-0 conv call: bool [P, C, H, W]
        self.planes = []       # per mode-0 conv call: the returned (hi, lo | None) planes themselves
        self.dx3 = []          # per front-end backward: the dy argument (a copy)
        self.front_grads = []  # per front-end backward: the returned (dw1, db1, dw2, db2)
        self.front_call = []   # per front-end backward: (function name, args, kwargs)
        self.calls = {k: 0 for k in SPIED}


@contextlib.contextmanager
def spy(monkeypatch, module):
    """Wrap `module`'s (crw_hip's) front-end and 3x3 entry points for the duration of the block; `encoder.py` resolves them at
    call time, so patching the module attributes is enough.  Yields a `Record`; the originals are restored on exit."""
    rec = Record()

    def wrap(name):
        orig = getattr(module, name)
        sig = inspect.signature(orig)

        def wrapped(*args, **kwargs):
            ret = orig(*args, **kwargs)
            ba = sig.bind(*args, **kwargs)
            ba.apply_defaults()
            a = ba.arguments
            rec.calls[name] += 1
            if name.startswith("enc_front_fwd"):
                yh, yl = ret[0], ret[1]
                rec.x3.append(planes_value(yh, yl))
                h, w = a["x"].shape[-2:]
                rec.hw = (h - 6, w - 6)
            elif name.startswith("enc_conv3x3"):
                if a["mode"] == 0:
                    H, W = (a["H"], a["W"]) if name.endswith("_map") else (10, 10)
                    rec.gates.append(planes_nchw(ret[0] != 0, H, W))
                    rec.planes.append((ret[0], ret[1]))
            else:
                rec.dx3.append(a["dy"].detach().clone())
                rec.front_grads.append(tuple(ret))
                rec.front_call.append((name, args, kwargs))
            return ret
        return wrapped

    with monkeypatch.context() as m:
        for n in SPIED:
            m.setattr(module, n, wrap(n))
        yield rec
