"""Cases, inputs, the fp64 reference and its mutants for the two forward-only passes of the `Resnet` (crw_rn_eval_fwd: BatchNorm
on the running statistics; crw_rn_train_fwd_nograd: train-mode BatchNorm under `torch.no_grad()`), on a state that looks like a
trained checkpoint.  Used by test_resnet_infer.py (host) and test_resnet_infer_gpu.py (MI355X); nothing here touches a GPU.

The state (`trained_like`): gamma = +-U(0.3, 1.7), about a quarter of the channels negative, one channel per BatchNorm exactly 0;
beta ~ N(0, 0.3); every running mean / variance = the fp64 batch statistic of a STATISTICS batch (64 patches, 1.5 noise + 0.4 + a
layered sine, the recipe of test_resnet_step_at_bench_batch_matches_fp64); convolution and linear weights at their seeded initial
values.  The TEST batch comes from another distribution (unit noise, no shift, the sine at another frequency and phase), so the
running statistics are visibly not the test batch's own: eval-mode and train-mode features differ by far more than any bar.

The reference (`reference`): `copy.deepcopy(net).double()` with `hip_convs = None` -- PyTorch's own modules on the raw fp32
parameters widened to fp64 -- in eval mode, or in train mode under no_grad (features + the updated buffers).  With `taps=True` it
also returns the fp64 activations after the stem, the pool and every block: what a failing device case is bisected against.

The mutants are one-line changes of that reference of the kind a kernel could make; test_resnet_infer.py shows that each one moves
the features (or the buffers) by more than 100 x the device bar on this state."""
import copy
import functools
import zlib

import torch
import torch.nn.functional as TF

FEATURE_BAR = 1e-4                   # max |y - y64| <= FEATURE_BAR * max |y64|: test_resnet_step_at_bench_batch_matches_fp64's bar
BUFFER_RTOL, BUFFER_ATOL = 1e-3, 1e-5  # running statistics after a no-grad pass: test_resnet_hip_matches_pytorch_modules's bar

PPW, BAND, GATHERED = "rn_stem.patch_per_wave", "rn_stem.band", "rn_stem.gathered"

# (h, w, cin, [P ...], stem route to expect; None = whatever crw_rn_stem_band_ok(h, w) says)
CASES = [
    (16, 16, 1, [1, 127, 128, 129, 257], PPW),
    (16, 16, 2, [70], PPW),
    (20, 27, 2, [5, 130], BAND),
    (32, 32, 1, [1, 129], BAND),          # 2x2 final map
    (40, 64, 1, [30], None),              # 2x3 final map
    (16, 85, 1, [5, 129], GATHERED),      # the band kernel refuses w = 85 ... 94 at h = 16 (test_resnet_stem_sizes_gpu.py)
    (16, 111, 2, [3], GATHERED),
]

# Train-mode BatchNorm needs more than one value per channel: the no-grad cases replace P = 1 by the smallest P that nn.BatchNorm2d
# accepts AND at which the comparison is well posed (test_resnet_infer.py::test_conditioning: PyTorch's own fp32 modules within a
# tenth of the device bars of the fp64 reference).  16x16: layer4's map is 1x1, so its BatchNorms see P values per channel; with two
# values per channel fp32 modules sit at 1.0e-5 of the feature scale, on the limit itself, with three at 3e-6.  32x32: four values
# per patch, so P = 1 is legal, and well posed (9e-7).
NOGRAD_SMALLEST_P = {(16, 16, 1): 3, (32, 32, 1): 1}

MODES = ("eval", "nograd")


def cases(mode):
    """[(h, w, cin, P, route)] of one mode, one entry per (case, P)"""
    out = []
    for h, w, cin, Ps, route in CASES:
        for P in Ps:
            if mode == "nograd" and P == 1:
                P = NOGRAD_SMALLEST_P[(h, w, cin)]
            out.append((h, w, cin, P, route))
    return out


def case_id(c):
    return f"{c[0]}x{c[1]}-cin{c[2]}-P{c[3]}"


# The seed of a case fixes its weights, its BatchNorm state and its batches.  Default: a hash of the case.  16x16 / cin 1 takes a seed
# (the first of 0 ... 39 with this property) whose fc0 draws a weight of -0.004: that channel of bn0 then has a running variance of
# 4e-5, of eps's own order, as a thin lifting layer can have after training -- the one place where a forgotten eps is visible in
# the features (mutant b: 0.5 of the scale there, 2e-3 on the other cases).  The case stays well posed (test_conditioning).
SEEDS = {(16, 16, 1): 36}


def case_seed(h, w, cin):
    return SEEDS.get((h, w, cin), zlib.crc32(f"resnet-infer-{h}x{w}-{cin}".encode()) % 100003)


def _rows(h):
    return torch.arange(h, dtype=torch.float32)[None, None, :, None]


def _with_position(sig):
    """cin = 2: the row position r / H - 0.5 in channel 0, the signal in channel 1 (`utils.pos_embed`)"""
    P, _, h, w = sig.shape
    pe = (torch.arange(h, dtype=torch.float32) / h - 0.5).view(1, 1, h, 1).expand(P, 1, h, w)
    return torch.cat([pe, sig], 1).contiguous()


def stats_batch(h, w, cin, seed):
    """the 64 patches whose fp64 batch statistics become the running statistics"""
    g = torch.Generator().manual_seed(seed * 2 + 1)
    sig = 1.5 * torch.randn(64, 1, h, w, generator=g) + 0.4 + torch.sin(_rows(h) * 0.4 + torch.rand(64, 1, 1, 1, generator=g) * 6.28)
    return sig if cin == 1 else _with_position(sig)


def input_batch(h, w, cin, P, seed):
    """the P patches a case runs: unit noise, no shift, the layered term at another frequency and phase"""
    g = torch.Generator().manual_seed(seed * 2 + 1000 * P)
    sig = torch.randn(P, 1, h, w, generator=g) + torch.sin(_rows(h) * 0.7 + 2.0 + torch.rand(P, 1, 1, 1, generator=g))
    return sig if cin == 1 else _with_position(sig)


def batchnorms(net):
    return [(k, m) for k, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]


def make_net(cin, seed):
    import encoder as crw_encoder
    torch.manual_seed(seed)
    return crw_encoder.Resnet(cin == 2)


def trained_like(net, seed, hw=(16, 16)):
    """Moves `net` (on the CPU, fp32) off its initial state the way training does; deterministic from the seed.  Returns net."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, m in batchnorms(net):
            C = m.num_features
            gamma = torch.rand(C, generator=g) * 1.4 + 0.3
            gamma = torch.where(torch.rand(C, generator=g) < 0.25, -gamma, gamma)
            gamma[int(torch.randint(C, (1,), generator=g))] = 0.0
            m.weight.copy_(gamma)
            m.bias.copy_(torch.randn(C, generator=g) * 0.3)
    ref = _widen(net).train()
    for _, m in batchnorms(ref):
        m.momentum = 1.0  # running statistic := this batch's statistic
    with torch.no_grad():
        ref(stats_batch(hw[0], hw[1], net.fc0.in_channels, seed).double())
        for (_, m), (_, r) in zip(batchnorms(net), batchnorms(ref)):
            m.running_mean.copy_(r.running_mean)
            m.running_var.copy_(r.running_var)
            m.num_batches_tracked.fill_(100)
    return net


def one_step_from_init(net, x):
    """the state the older eval-mode tests run on: ONE training step's worth of running statistics on the initial gamma = 1,
    beta = 0 (test_resnet_inference_through_propagate)"""
    was = net.hip_convs
    net.hip_convs = None
    with torch.no_grad():
        net.train()(x)
    net.hip_convs = was
    return net


def _widen(net):
    ref = copy.deepcopy(net).double()
    ref.hip_convs = None
    return ref


# ---- the reference and its mutants ------------------------------------------------------------------------------------------------
MUTANTS = {
    "a": (("eval",), "batch statistics where the running ones belong"),
    "b": (("eval", "nograd"), "eps left out"),
    "c": (("eval", "nograd"), "the variance where its square root belongs"),
    "d": (("eval",), "running statistics of layer1[0].bn1 and layer1[0].bn2 swapped"),
    "e": (("eval",), "layer2's downsample BatchNorm reading the main branch's bn2 statistics"),
    "f": (("nograd",), "running_var updated with the biased variance"),
    "g": (("eval", "nograd"), "bn0's shift and relu0 left off the one-pixel border of fc0's padding"),
}


def _bn(ref, m, z, train, mutant):
    """one BatchNorm of the reference: the module itself, or the module with ONE line changed"""
    if mutant is None:
        return m(z)
    body = ref.model
    mean, var, eps, use_batch = m.running_mean, m.running_var, m.eps, train
    if mutant == "a":
        use_batch = True
    if mutant == "b":
        eps = 0.0
    if mutant == "d" and m is body.layer1[0].bn1:
        mean, var = body.layer1[0].bn2.running_mean, body.layer1[0].bn2.running_var
    if mutant == "d" and m is body.layer1[0].bn2:
        mean, var = body.layer1[0].bn1.running_mean, body.layer1[0].bn1.running_var
    if mutant == "e" and m is body.layer2[0].downsample[1]:
        mean, var = body.layer2[0].bn2.running_mean, body.layer2[0].bn2.running_var
    if train:
        old = m.running_var.clone()
        y = m(z)  # the module's own output and its running-statistics update (unbiased variance) ...
        if mutant == "f":  # ... replaced by the biased one
            m.running_var.copy_((1 - m.momentum) * old + m.momentum * z.var((0, 2, 3), unbiased=False))
        if mutant not in ("b", "c"):
            return y
    if use_batch:
        mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    inv = 1.0 / (var + eps) if mutant == "c" else 1.0 / torch.sqrt(var + eps)
    sc = m.weight * inv
    return z * sc[None, :, None, None] + (m.bias - mean * sc)[None, :, None, None]


def _forward(ref, x, train, mutant, taps):
    """Resnet.forward on PyTorch ops, written out so that every BatchNorm passes through `_bn` and the activations can be kept"""
    body = ref.model
    a = torch.relu(_bn(ref, ref.bn0, ref.fc0(x), train, mutant))
    if mutant == "g":
        a = TF.pad(a[:, :, 1:-1, 1:-1], (1, 1, 1, 1))
    taps["stem"] = a
    z1 = body.conv1(a)
    taps["conv1"] = z1
    a = body.maxpool(torch.relu(_bn(ref, body.bn1, z1, train, mutant)))
    taps["pool"] = a
    for i in range(1, 5):
        m = getattr(body, f"layer{i}")[0]
        y = _bn(ref, m.bn2, m.conv2(torch.relu(_bn(ref, m.bn1, m.conv1(a), train, mutant))), train, mutant)
        s = a if m.downsample is None else _bn(ref, m.downsample[1], m.downsample[0](a), train, mutant)
        a = torch.relu(y + s)
        taps[f"layer{i}"] = a
    return body.fc(torch.flatten(body.avgpool(a), 1))


def reference(net, x, mode, mutant=None, taps=False, buffers=None):
    """fp64 PyTorch modules on net's raw fp32 parameters and buffers.  mode 'eval': BatchNorm on the running statistics, nothing
    updated -> y [P,128];  mode 'nograd': train-mode BatchNorm under no_grad -> (y, {buffer name: value after the pass}).
    mutant: None (the modules themselves) or a key of MUTANTS.  buffers: return the reference's buffers after the pass (default:
    in mode 'nograd' only).  taps=True appends {name: fp64 activation} (stem, conv1, pool, layer1 ... layer4) to what is returned."""
    assert mode in MODES and (mutant is None or mode in MUTANTS[mutant][0])
    ref = _widen(net).train(mode == "nograd")
    kept = {}
    with torch.no_grad():
        if mutant is None and not taps:
            y = ref(x.double())
        else:
            y = _forward(ref, x.double(), mode == "nograd", mutant, kept)
    out = (y, {k: v.clone() for k, v in ref.named_buffers()}) if (mode == "nograd" if buffers is None else buffers) else (y,)
    if taps:
        out += (kept,)
    return out[0] if len(out) == 1 else out


# ---- what a case runs (shared by the host and the GPU tests: built once per process) -------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_net(h, w, cin):
    """the trained-like fp32 module of a case, on the CPU; callers deepcopy it"""
    seed = case_seed(h, w, cin)
    return trained_like(make_net(cin, seed), seed, (h, w))


@functools.lru_cache(maxsize=None)
def case_input(h, w, cin, P):
    return input_batch(h, w, cin, P, case_seed(h, w, cin))


@functools.lru_cache(maxsize=None)
def case_reference(h, w, cin, P, mode):
    """reference(...) of a case; computed once, shared, never written to"""
    return reference(case_net(h, w, cin), case_input(h, w, cin, P), mode)


def feature_error(y, y64):
    """(max |y - y64| / max |y64|, max |y64|)"""
    scale = y64.abs().max().item()
    return (y.double().cpu() - y64).abs().max().item() / scale, scale


def buffer_error(got, want, rtol=BUFFER_RTOL, atol=BUFFER_ATOL):
    """worst |got - want| / (atol + rtol |want|) over the floating-point buffers, and the buffer it occurs in"""
    worst, where = 0.0, None
    for k, v in want.items():
        if not v.is_floating_point():
            continue
        e = float(((got[k].double().cpu() - v).abs() / (atol + rtol * v.abs())).max())
        if e > worst:
            worst, where = e, k
    return worst, where
