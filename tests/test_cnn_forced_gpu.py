"""The `CNN` training step as `encoder.py` wires it -- `_HipEncoder` / `_HipMapEncoder`, the head, `model.affinity` and the walk --
held entry by entry to the gate-forced fp64 reference of tests/cnn_forced_ref.py (proved on the CPU by tests/test_cnn_forced.py).

The free-running 2e-2 checks of test_hip_parity.py cannot tell the default arithmetic (hi/lo bf16 pairs, three products per MAC)
from a build that lost a lo plane somewhere in the backward hand-off.  Here the device's own ReLU gates of conv3..conv5 are imposed
on an fp64 forward on the device (PyTorch ops), after an audit that the gates are the reference's wherever the number formats
leave no doubt; every entry of x3, the features, the logits, dx3 and the gradients of conv3..conv5 and fc is then held to
`cnn_forced_ref.BARS` (4 x the worst value measured over the five cases, one significant digit).  The opt-in arithmetics are the
mutants that prove the bars have teeth: "mixed" (backward on the hi planes alone) and "bf16" must EXCEED the default's bars.

The gradients of conv1 / conv2 come out of the front end's backward, whose pooling record is opaque: they are checked for wiring
(autograd hands on exactly what the kernel returned for the recorded dx3, and a direct call reproduces it); their accuracy stays
with the well-posed kernel tests and the free-running checks of test_hip_parity.py."""
import types
import warnings

import pytest
import torch

import cnn_forced_ref as fr
from conftest import load_golden

pytestmark = pytest.mark.gpu

# name -> what it is; [B,T,N] items, P = B*T*N patches
CASES = {
    "a_cfg1_B2T8N7": "golden cnn_cfg1_B2T8N7 + cnn_weights_seed11: P = 112, 16x16",
    "b_posembed_B1T4N3": "golden cnn_posembed_B1T4N3 + its weights: cin = 2, P = 12",
    "c_B1T5N63": "[1,5,63] at 16x16 / (8,0): P = 315, more than one patch per weight-gradient slice",
    "d_B2T4N5_20x27": "[2,4,5] at 20x27 / (10,0): map path, 14x21 map = 2x3 tiles, partial in both directions",
    "e_B2T4N5_32x32": "[2,4,5] at 32x32 / (24,0): map path, 26x26 map = 3x3 tiles",
}
FORWARD = ("x3", "features", "A", "loss")
BACKWARD = ("dx3",) + tuple(f"{l}.{p}" for l in fr.LAYERS for p in ("weight", "bias")) + ("fc.weight", "fc.bias")
TEETH = ("conv3.weight", "conv4.weight", "conv5.weight")


def _case(name):
    """-> namespace(seq [B,T,N,h,w] fp32 (CPU), sd, tau, pos_embed, is_map)"""
    import dataset as crw_dataset
    import encoder as crw_encoder
    if name[0] in "ab":
        g = load_golden("cnn_cfg1_B2T8N7" if name[0] == "a" else "cnn_posembed_B1T4N3")
        w = load_golden("cnn_weights_seed11" if name[0] == "a" else "cnn_weights_posembed_seed21")
        return types.SimpleNamespace(seq=torch.tensor(g["seq"]), sd={k: torch.tensor(v) for k, v in w.items()}, tau=float(g["tau"]),
                                     pe=bool(g["pos_embed"]), is_map=False)
    if name[0] == "c":
        seq = crw_dataset.RGDataset.synthetic(512, 160, 5, (16, 16), (8, 0), seed=17)[0][None].contiguous()
        assert seq.shape == (1, 5, 63, 16, 16)
    else:
        T = 4
        (h, w), ov = ((20, 27), (10, 0)) if name[0] == "d" else ((32, 32), (24, 0))
        ds = crw_dataset.RGDataset.synthetic(ov[0] + 5 * (h - ov[0]), 2 * T * w, T, (h, w), ov, seed=13)
        seq = torch.stack([ds[0], ds[T]])
        assert seq.shape == (2, 4, 5, h, w)
    torch.manual_seed(11)
    sd = {k: v.detach().clone() for k, v in crw_encoder.CNN(False).state_dict().items()}
    return types.SimpleNamespace(seq=seq, sd=sd, tau=0.05, pe=False, is_map=name[0] in "de")


def device_step(hip, mp, c, convs, steps=1):
    """`steps` times forward + backward of CRW(CNN) on the HIP path under the spy, the PyTorch fallback an error.
    -> list of namespace(loss, A, feats [P,128], grads {name: tensor}, rec (the spy's record))."""
    import encoder as crw_encoder
    import model as crw_model
    enc = crw_encoder.CNN(c.pe)
    enc.hip_convs = convs
    enc.load_state_dict(c.sd)
    net = crw_model.CRW(enc, c.tau, c.pe).cuda()
    feats = []
    enc.register_forward_hook(lambda m, i, o: feats.append(o.detach()))
    seq = c.seq.cuda()
    out = []
    for _ in range(steps):
        net.zero_grad(set_to_none=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            mp.setattr(crw_encoder.CNN, "_warned_fallback", False)  # the fallback warns once per process: make it able to
            with fr.spy(mp, hip) as rec:
                loss, A = net(seq)
                loss.backward()
        torch.cuda.synchronize()
        m = "_map" if c.is_map else ""
        # the kernels ran as wired: one front end, conv3..conv5 forward and their three backward-data calls, one front backward
        assert (rec.calls["enc_front_fwd" + m], rec.calls["enc_conv3x3" + m], rec.calls["enc_front_bwd" + m]) == (1, 6, 1), rec.calls
        assert sum(rec.calls.values()) == 8 and len(rec.gates) == 3
        out.append(types.SimpleNamespace(loss=loss.detach(), A=A.detach(), feats=feats.pop(), rec=rec,
                                         grads={k: p.grad.detach().clone() for k, p in enc.named_parameters()}))
    return out


def forced_reference(c, gates):
    """The fp64 reference on the device with `gates` imposed (None: free-running), differentiated.
    -> (namespace of crw_forward_forced, {name: gradient})"""
    sd = {k: v.detach().double().cuda().requires_grad_(True) for k, v in c.sd.items()}
    ref = fr.crw_forward_forced(c.seq.cuda().double(), sd, c.tau, c.pe, gates=gates)
    ref.loss.backward()
    return ref, {k: v.grad for k, v in sd.items()}


def measure(c, run, ref, gref):
    """Every asserted quantity's error: entry-wise maximum relative to the reference tensor's largest entry (A: to 1 / tau;
    the loss: relative)."""
    H, W = run.rec.hw
    err = {"x3": fr.rel_err(fr.planes_nchw(run.rec.x3[0], H, W), ref.x3),
           "features": fr.rel_err(run.feats, ref.emb.reshape(run.feats.shape)),
           "A": float((run.A.double() - ref.A.detach()).abs().max()) * c.tau,
           "loss": abs(run.loss.item() - ref.loss.item()) / abs(ref.loss.item()),
           "dx3": fr.rel_err(fr.planes_nchw(run.rec.dx3[0], H, W), ref.x3.grad)}
    for k in BACKWARD[1:]:
        err[k] = fr.rel_err(run.grads[k], gref[k])
    return err


def report(tag, convs, err, keys):
    bars = fr.bars_for(convs, tag)
    for k in keys:
        print(f"  {tag} {convs:7s} {k:13s} error {err[k]:.3e}   bar {bars[k]:.0e}   {'ok' if err[k] <= bars[k] else 'OVER'}")


@pytest.fixture(scope="module")
def runs():
    """Every (case, arithmetic) is run once and shared by the tests below: device steps (two for the default, for the
    reproducibility test), the forced reference at the device's gates, and the measured errors.  Nothing here is modified later."""
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    cache = {}
    with pytest.MonkeyPatch.context() as mp:
        def get(name, convs):
            if (name, convs) not in cache:
                c = _case(name)
                steps = device_step(crw_hip, mp, c, convs, steps=2 if convs == "bf16x3" else 1)
                gates = steps[0].rec.gates
                if convs == "mixed":  # the default's forward: the same gates (asserted in the teeth test), the same reference
                    ref, gref = get(name, "bf16x3").ref, get(name, "bf16x3").gref
                else:
                    ref, gref = forced_reference(c, gates)
                cache[name, convs] = types.SimpleNamespace(c=c, steps=steps, run=steps[0], ref=ref, gref=gref,
                                                           err=measure(c, steps[0], ref, gref), hip=crw_hip)
            return cache[name, convs]
        yield get


@pytest.mark.parametrize("name", CASES)
def test_gate_audit(runs, name):
    """Forcing must not hide a gate bug.  (1) Against the free-running fp64 forward: every position where a device gate differs
    from `z_ref > 0` has |z_ref| <= 2 e of its layer, e the format bound with the lower layers' bounds carried through |w|
    (`format_bounds`).  That worst case grows ~10x per layer and by conv5 it allows nearly anything (tests/test_cnn_forced.py
    prints what it covers), so (2) every layer is also audited on the device's OWN input planes, where fp64 and the device differ
    by that one layer's arithmetic: |z| <= 2 e with nothing carried (`layer_audit`).  One gate outside either margin fails."""
    r = runs(name, "bf16x3")
    free = fr.crw_forward_forced(r.c.seq.cuda().double(), {k: v.double().cuda() for k, v in r.c.sd.items()}, r.c.tau, r.c.pe)
    es = fr.format_bounds(free.x, r.c.sd)
    carried = fr.gate_audit(r.run.rec.gates, free.z, es)
    H, W = r.run.rec.hw
    inputs = [fr.planes_nchw(r.run.rec.x3[0], H, W)] + [fr.planes_nchw(fr.planes_value(*p), H, W) for p in r.run.rec.planes[:2]]
    local = fr.layer_audit(inputs, r.run.rec.gates, r.c.sd)
    for layer, g, a, b in zip(fr.LAYERS, r.run.rec.gates, carried, local):
        print(f"  {name} {layer}: {g.numel()} gates, {int(g.sum())} open; differ from free-running fp64: {a[0]} (outside 2 e: {a[1]}, "
              f"worst |z| / e {a[2]:.3f}); differ from fp64 on the device's own input: {b[0]} (outside 2 e: {b[1]}, worst {b[2]:.3f})")
    assert all(a[1] == 0 for a in carried), carried
    assert all(b[1] == 0 for b in local), local
    assert all(0 < int(g.sum()) < g.numel() for g in r.run.rec.gates)


@pytest.mark.parametrize("name", CASES)
def test_forward_against_forced_reference(runs, name):
    """x3 as the front end wrote it (hi + lo), the features, the logits (error relative to 1 / tau) and the loss (the
    north_star's 1e-4 relative) against the fp64 forward forced with the device's gates."""
    r = runs(name, "bf16x3")
    report(name, "bf16x3", r.err, FORWARD)
    for k in FORWARD:
        assert r.err[k] <= fr.bars_for("bf16x3", name)[k], (k, r.err[k])


@pytest.mark.parametrize("name", CASES)
def test_backward_every_entry_against_forced_reference(runs, name):
    """dx3 (the gradient that crosses from the trunk into the front end, as `enc_front_bwd[_map]` received it) against `x3.grad`,
    and every entry of the gradients of conv3..conv5 and fc, each relative to its reference tensor's largest entry.  (b) is held
    to the bars over all five cases, which it sets; the other four to the sharper bars they set (`cnn_forced_ref.bars_for`)."""
    r = runs(name, "bf16x3")
    report(name, "bf16x3", r.err, BACKWARD)
    for k in BACKWARD:
        assert r.err[k] <= fr.bars_for("bf16x3", name)[k], (k, r.err[k])


@pytest.mark.parametrize("name", CASES)
def test_front_end_wiring(runs, name):
    """What autograd hands to conv1.* / conv2.* is bit for bit what the front end's backward returned for the recorded dx3, and
    a direct call of `crw_hip.enc_front_bwd[_map]` on the recorded arguments reproduces it.  (Their accuracy: the well-posed kernel
    tests and the free-running checks of test_hip_parity.py; the front end's pooling record is not decoded here.)"""
    r = runs(name, "bf16x3")
    rec = r.run.rec
    fname, args, kwargs = rec.front_call[0]
    assert fname == ("enc_front_bwd_map" if r.c.is_map else "enc_front_bwd")
    again = getattr(r.hip, fname)(*args, **kwargs)
    for k, got, once in zip(("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"), rec.front_grads[0], again):
        assert torch.equal(r.run.grads[k], got), k
        assert torch.equal(once, got), k
        assert torch.isfinite(got).all() and got.abs().max() > 0, k


@pytest.mark.parametrize("name", CASES)
def test_second_step_is_bit_identical(runs, name):
    """A second forward and backward of the same step: the same loss, logits, gates and gradients, bit for bit."""
    a, b = runs(name, "bf16x3").steps
    assert torch.equal(a.loss, b.loss) and torch.equal(a.A, b.A) and torch.equal(a.feats, b.feats)
    assert all(torch.equal(x, y) for x, y in zip(a.rec.gates, b.rec.gates)) and torch.equal(a.rec.dx3[0], b.rec.dx3[0])
    for k in a.grads:
        assert torch.equal(a.grads[k], b.grads[k]), k


@pytest.mark.parametrize("name", [n for n in CASES if n[0] in "abc"])
def test_mixed_keeps_the_forward_and_misses_the_default_bars(runs, name):
    """hip_convs = "mixed" (16x16 patches only: `_HipMapEncoder` takes no `bwd_split`, on the map path "mixed" IS "bf16x3" and there
    is no difference to assert) runs the default's forward -- x3, gates, features, logits and loss bit for bit -- and its backward on
    the hi planes alone.  It holds its own bars and, on (a) and (c), EXCEEDS the default's on the weight gradients of conv3..conv5:
    a backward that lost its lo planes cannot pass test_backward_every_entry_against_forced_reference."""
    d, m = runs(name, "bf16x3"), runs(name, "mixed")
    assert torch.equal(m.run.loss, d.run.loss) and torch.equal(m.run.A, d.run.A) and torch.equal(m.run.feats, d.run.feats)
    assert torch.equal(m.run.rec.x3[0], d.run.rec.x3[0]) and all(torch.equal(x, y) for x, y in zip(m.run.rec.gates, d.run.rec.gates))
    report(name, "mixed", m.err, BACKWARD)
    for k in BACKWARD:
        assert m.err[k] <= fr.BARS["mixed"][k], (k, m.err[k])
    if name[0] in "ac":
        for k in TEETH:
            print(f"  {name} teeth: mixed {k} {m.err[k]:.3e} = {m.err[k] / fr.BARS['bf16x3'][k]:.1f} x the default's bar "
                  f"({m.err[k] / d.err[k]:.0f} x the default's error)")
            assert m.err[k] > fr.BARS["bf16x3"][k], k


@pytest.mark.parametrize("name", CASES)
def test_plain_bf16_holds_its_own_bars_and_misses_the_default_ones(runs, name):
    """hip_convs = "bf16" (plain bf16 operands both ways) against the fp64 forward forced with ITS gates: inside its own bars on
    every case and, on (a), (c) and (d), OVER the default's bars on the features and on the weight gradients of conv3..conv5 -- the
    map path's only mutant."""
    d, b = runs(name, "bf16x3"), runs(name, "bf16")
    report(name, "bf16", b.err, FORWARD + BACKWARD)
    for k in FORWARD + BACKWARD:
        assert b.err[k] <= fr.BARS["bf16"][k], (k, b.err[k])
    if name[0] in "acd":
        for k in ("features",) + TEETH:
            print(f"  {name} teeth: bf16 {k} {b.err[k]:.3e} = {b.err[k] / fr.BARS['bf16x3'][k]:.1f} x the default's bar "
                  f"({b.err[k] / d.err[k]:.0f} x the default's error)")
            assert b.err[k] > fr.BARS["bf16x3"][k], k
