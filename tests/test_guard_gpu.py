"""crw_adam_step_guarded (include/crw_hip_guard.h) on the device, and a training run that survives its data.

The kernel: every case is a short sequence of calls on this test's own buffers, run by `run_twice` (the workspace filled with 0xFF,
then with 0x00: stale memory) and by `run_banded` (every operand between poisoned guard bands) of tests/stale_ref.py, and then held
against crw_adam_step itself on copies -- bit for bit wherever the header promises bits -- and against tests/guard_ref.py for the
norm, the coefficient and the counters.  The sizes: 1, 3, 4, 5 (a lone scalar tail, one float4, one float4 and a tail), 1023 / 1024 /
1025 (around one 256-thread round of float4), and 3 * 4096 + 3 (four reduction blocks, the last one a ragged tail).

End to end: scripts/train.py on a 64 x 256 radargram with two NaN columns, as it is today (the witness that the fixture bites), with
--skip_nonfinite and with --nodata skip; and checkpoint / resume through optim.FlatAdam, bit for bit."""
import ctypes
import importlib.util
import math
import os
import struct

import numpy as np
import pytest
import torch

import guard_ref as gr
import stale_ref as sr
from conftest import PKG
from stale_ref import Buf, Case
from test_encoder_stale_gpu import _gen, _ok, _p, _randn, _stream

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 3 * 4096 + 3)
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
EINVAL, EWORKSPACE = 1, 2
BADS = (float("nan"), float("inf"), -float("inf"))


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_guard()
    return crw_hip


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _plain(lib, p, g, m, v, step):
    _ok("crw_adam_step", lib.crw_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], step, _stream()))


def _guarded(lib, p, g, m, v, step, max_norm, ctl, ws):
    return lib.crw_adam_step_guarded(_p(p), _p(g), _p(m), _p(v), p.numel(), HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], step, max_norm,
                                     _p(ctl), _p(ws), ws.numel(), _stream())


def _start(n, seed):
    """a state in the middle of a run: parameters of order 1, moments that are not zero"""
    g = _gen(seed)
    return _randn(g, n), _randn(g, n, scale=0.05), torch.rand(n, generator=g).cuda() * 0.01 + 1e-6


def _grad(n, seed, scale=1.0):
    return _randn(_gen(1000 + seed), n, scale=scale)


class Sequence:
    """calls = [(g, max_norm), ...] run as steps 1 .. len(calls) on one set of buffers; after every call a snapshot (p, m, v clones
    and the control block's fields) is kept for the test to read.  `case()` wraps it for tests/stale_ref.py: p, m, v and ctl are
    in/out operands that start from the same bytes in every run, ws is a workspace of exactly the size the library asks for."""

    def __init__(self, hip, n, calls, seed=5):
        self.hip, self.lib, self.n = hip, hip.lib(), n
        self.home = sr.Home("cuda")
        self.calls = [(self.home(g, f"g{i}"), mx) for i, (g, mx) in enumerate(calls)]
        self.p0, self.m0, self.v0 = _start(n, seed)
        self.snaps = []

    def case(self):
        n, nws = self.n, self.lib.crw_adam_guard_ws_bytes(self.n)
        assert nws == -(-n // gr.BLOCK_ELEMS) * 8 + 16
        f = lambda t: Buf(4 * n, torch.float32, init=t)
        bufs = dict(p=f(self.p0), m=f(self.m0), v=f(self.v0), ctl=Buf(gr.CTL_BYTES, None, init=torch.zeros(gr.CTL_BYTES, dtype=torch.uint8)),
                    ws=Buf(nws, None, ws=True))

        def run(_, t):
            p, m, v = (t[k][:4 * n].view(torch.float32) for k in "pmv")
            ctl, ws = t["ctl"][:gr.CTL_BYTES], t["ws"][:nws]
            del self.snaps[:]
            for step, (g, mx) in enumerate(self.calls, 1):
                _ok("crw_adam_step_guarded", _guarded(self.lib, p, g, m, v, step, mx, ctl, ws))
                torch.cuda.synchronize()
                self.snaps.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), raw=bytes(ctl.cpu().tolist()), **self.hip.guard_ctl_unpack(ctl)))
            torch.cuda.synchronize()
        return Case("crw_adam_step_guarded", None, bufs, run, device="cuda", home=self.home)

    def held(self):
        """over stale workspaces and between guard bands; both harness runs end in the same bytes -> the snapshots of the last run"""
        case = self.case()
        a = sr.run_twice(case)
        first = [dict(s) for s in self.snaps]
        b = sr.run_banded(case)
        for k in ("p", "m", "v", "ctl"):
            assert torch.equal(a[k], b[k]), k
        for s, t in zip(first, self.snaps):
            assert s["raw"] == t["raw"] and all(_same(s[k], t[k]) for k in "pmv")
        assert all(s["raw"][32:] == bytes(32) for s in self.snaps)                         # the reserved half stays as it was zeroed
        return self.snaps

    def plain(self, upto, grads=None, steps=None):
        """crw_adam_step on copies of the starting state: the calls [0, upto) (or `grads` at `steps`) -> p, m, v"""
        p, m, v = self.p0.clone(), self.m0.clone(), self.v0.clone()
        grads = [g for g, _ in self.calls[:upto]] if grads is None else grads
        for step, g in zip(steps or range(1, len(grads) + 1), grads):
            _plain(self.lib, p, g, m, v, step)
        torch.cuda.synchronize()
        return p, m, v


# ================================================================================================ (a) finite, no bound
@pytest.mark.parametrize("n", SIZES)
def test_finite_gradients_without_a_bound_are_crw_adam_step(hip, n):
    """steps 1 .. 5, max_norm = 0: p, m and v are crw_adam_step's bits after every step, applied == step, and the norm is the fp64
    norm within n * 2^-52 * norm (the device sums per block, the reference in index order)"""
    seq = Sequence(hip, n, [(_grad(n, s, 10.0 ** (s - 2)), 0.0) for s in range(5)])
    snaps = seq.held()
    for step, s in enumerate(snaps, 1):
        p, m, v = seq.plain(step)
        assert _same(s["p"], p) and _same(s["m"], m) and _same(s["v"], v), step
        assert (s["applied"], s["skipped"], s["last_applied"], s["scale"]) == (step, 0, 1, 1.0)
        _, want = gr.sum_squares(seq.calls[step - 1][0].cpu().numpy())
        assert abs(s["norm"] - want) <= n * 2.0 ** -52 * want, (step, s["norm"], want)
    assert not _same(snaps[-1]["p"], seq.p0)


# ================================================================================================ (b) one non-finite value
def _poison_cases():
    out = []
    for j, n in enumerate(SIZES):
        where = {0, n - 1}
        if n % 4:
            where.add(n - n % 4)                                   # the first element of the ragged tail
        for k, idx in enumerate(sorted(where)):
            out.append((n, idx, BADS[(j + k) % 3]))
    n = SIZES[-1]                                                  # four blocks: every value in a block other than the first and in the tail
    out += [(n, idx, bad) for idx in (gr.BLOCK_ELEMS + 17, 3 * gr.BLOCK_ELEMS + 1) for bad in BADS if (n, idx, bad) not in out]
    return out


@pytest.mark.parametrize("n,idx,bad", _poison_cases())
def test_one_non_finite_value_refuses_the_step(hip, n, idx, bad):
    """calls: finite, POISONED, finite (the last two under a bound the gradients never reach).  The poisoned call leaves p, m and v
    with the bits they had; skipped == 1, last_applied == 0, scale == 0 and the norm is not finite.  The third call is step
    t = applied + 1 = 2 with coefficients recomputed on the device: m and v are crw_adam_step's bits at step 2, and every update
    u = p_new - p_old lies within 2^-21 |u_ref| + 2^-23 |p| of crw_adam_step's"""
    g1, g2, g3 = _grad(n, 1), _grad(n, 2), _grad(n, 3)
    g2[idx] = bad
    seq = Sequence(hip, n, [(g1, 0.0), (g2, 1e6), (g3, 1e6)])
    a, b, c = seq.held()
    assert (a["applied"], a["skipped"]) == (1, 0)
    assert _same(b["p"], a["p"]) and _same(b["m"], a["m"]) and _same(b["v"], a["v"])
    assert (b["applied"], b["skipped"], b["last_applied"], b["scale"]) == (1, 1, 0, 0.0)
    assert not math.isfinite(b["norm"]) and (math.isnan(b["norm"]) if math.isnan(bad) else b["norm"] == math.inf)
    assert (c["applied"], c["skipped"], c["last_applied"], c["scale"]) == (2, 1, 1, 1.0)
    p, m, v = seq.plain(0, grads=[g1, g3], steps=[1, 2])          # what a run that never saw the poisoned call computes
    assert _same(c["m"], m) and _same(c["v"], v)
    u, u_ref = c["p"].double() - b["p"].double(), p.double() - b["p"].double()
    bound = 2.0 ** -21 * u_ref.abs() + 2.0 ** -23 * b["p"].double().abs()
    equal = int((_bits(c["p"]) == _bits(p)).sum())
    print(f"n={n} idx={idx} bad={bad}: {equal} of {n} entries of p bit-equal, worst |u - u_ref| / bound = {float(((u - u_ref).abs() / bound).max()):.3f}")
    assert bool(((u - u_ref).abs() <= bound).all())
    assert torch.isfinite(c["p"]).all() and not _same(c["p"], b["p"])
    assert _same(seq.calls[1][0], g2)                              # g is never written


# ================================================================================================ (c) the bound
@pytest.mark.parametrize("n", SIZES)
def test_a_gradient_ten_times_the_bound_is_scaled(hip, n):
    """calls: norm = 10 x max_norm, norm = max_norm / 2, norm = 10 x max_norm again.  ctl.scale is fp32(min(1, max_norm / (ctl.norm +
    1e-6))) recomputed on the host from the device's own norm; p, m and v are crw_adam_step's bits on fl32(g * scale); below the bound
    the scale is 1 and the bits are those of the unbounded call"""
    max_norm = 0.75
    grads = []
    for s, factor in enumerate((10.0, 0.5, 10.0)):
        g = _grad(n, 10 + s)
        grads.append(g * (factor * max_norm / float(g.double().norm())))
    seq = Sequence(hip, n, [(g, max_norm) for g in grads])
    snaps = seq.held()
    used = []
    for s, g, factor in zip(snaps, grads, (10.0, 0.5, 10.0)):
        want = np.float32(min(1.0, float(np.float32(max_norm)) / (s["norm"] + 1e-6)))
        assert s["scale"] == float(want) and s["last_applied"] == 1
        assert (s["scale"] == 1.0) is (factor < 1) and abs(s["norm"] - factor * max_norm) < 1e-5 * max_norm
        assert float(gr.clip_coef(s["norm"], max_norm)) == s["scale"]
        used.append(g if factor < 1 else g * torch.tensor(s["scale"], dtype=torch.float32, device="cuda"))       # one fp32 rounding
        p, m, v = seq.plain(0, grads=used)
        assert _same(s["p"], p) and _same(s["m"], m) and _same(s["v"], v)
    assert abs(snaps[0]["scale"] - 0.1) < 1e-6 and snaps[-1]["applied"] == 3 and snaps[-1]["skipped"] == 0
    assert all(_same(held, g) for (held, _), g in zip(seq.calls, grads))                                          # g is never written


# ================================================================================================ (d) twice the same bits
@pytest.mark.parametrize("n", (1025, 3 * 4096 + 3))
def test_two_runs_give_the_same_bits_whatever_the_workspace_held(hip, n):
    """(c)'s calls on two sets of buffers whose workspaces start from different garbage: identical control blocks after every call,
    identical p, m and v -- no atomics, a summation order that n alone fixes"""
    lib, max_norm = hip.lib(), 0.75
    grads = [_grad(n, 20 + s, 3.0 ** s) for s in range(3)]
    runs = []
    for fill in (0xA5, 0x3C):
        p, m, v = _start(n, 8)
        ctl = torch.zeros(gr.CTL_BYTES, dtype=torch.uint8, device="cuda")
        ws = torch.full((lib.crw_adam_guard_ws_bytes(n),), fill, dtype=torch.uint8, device="cuda")
        raws = []
        for step, g in enumerate(grads, 1):
            _ok("crw_adam_step_guarded", _guarded(lib, p, g, m, v, step, max_norm, ctl, ws))
            raws.append(bytes(ctl.cpu().tolist()))
        runs.append((p, m, v, raws))
    (p1, m1, v1, r1), (p2, m2, v2, r2) = runs
    assert r1 == r2 and _same(p1, p2) and _same(m1, m2) and _same(v1, v2)
    assert struct.unpack_from(gr.CTL_FORMAT, r1[-1])[0] == 3


# ================================================================================================ (e) refusals
def test_refusals_leave_everything_as_it_was(hip):
    lib, n = hip.lib(), 1025
    p, m, v = _start(n, 2)
    g = _grad(n, 2)
    keep = [t.clone() for t in (p, m, v)]
    ctl = torch.zeros(gr.CTL_BYTES, dtype=torch.uint8, device="cuda")
    need = lib.crw_adam_guard_ws_bytes(n)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    call = lambda **kw: lib.crw_adam_step_guarded(_p(kw.get("p", p)), _p(kw.get("g", g)), _p(m), _p(v), kw.get("n", n), HP["lr"], kw.get("b1", 0.9),
                                                  kw.get("b2", 0.999), HP["eps"], kw.get("step", 1), kw.get("max_norm", 0.0),
                                                  kw.get("ctl", _p(ctl)), kw.get("ws", _p(ws)), kw.get("nbytes", need), _stream())
    assert call(n=0) == EINVAL and call(step=0) == EINVAL and call(b1=1.0) == EINVAL and call(b2=1.5) == EINVAL
    assert call(p=p[1:]) == EINVAL and call(g=g[2:]) == EINVAL                                  # not 16-byte aligned
    assert call(max_norm=-0.5) == EINVAL and call(max_norm=float("nan")) == EINVAL
    assert call(ctl=None) == EINVAL and call(ctl=ctypes.c_void_p(ctl.data_ptr() + 4)) == EINVAL
    assert call(ws=None) == EINVAL and call(ws=ctypes.c_void_p(ws.data_ptr() + 4)) == EINVAL
    assert call(nbytes=need - 1) == EWORKSPACE and call(nbytes=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(keep, (p, m, v))) and not ctl.any() and not ws.any()
    assert call(max_norm=float("inf")) == 0 and call(ws=ctypes.c_void_p(ws.data_ptr() + 8), step=2) == 0      # no bound; 8-byte aligned ws
    torch.cuda.synchronize()
    assert hip.guard_ctl_unpack(ctl)["applied"] == 2 and not _same(p, keep[0])


# ================================================================================================ FlatAdam
def _train():
    spec = importlib.util.spec_from_file_location("crw_train_guard_gpu", os.path.join(PKG, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _module():
    torch.manual_seed(5)
    return torch.nn.Sequential(torch.nn.Conv2d(1, 3, 3), torch.nn.Linear(7, 5), torch.nn.Linear(5, 130)).cuda()


def _flat_adam(**kw):
    import dist as crw_dist
    import optim as crw_optim
    net = _module()
    return net, crw_optim.FlatAdam(crw_dist.FlatGradBucket(net.parameters(), lazy=False), lr=1e-2, **kw)


def _drive(net, opt, steps, poison_at=()):
    for s in steps:
        g = torch.Generator(device="cuda").manual_seed(40 + s)
        for q in net.parameters():
            q.grad.copy_(torch.randn(q.shape, device="cuda", generator=g) * 10.0 ** (s % 3 - 1))
        if s in poison_at:
            next(iter(net.parameters())).grad.view(-1)[1] = float("inf")
        opt.step()


def test_flat_adam_unguarded_is_unchanged_and_guarded_counts(hip):
    """both options off: `step()` is crw_adam_step and the state dict has the keys it had; either on: the guarded entry point, whose
    bits are the plain step's while nothing is refused or clipped, and `stats()` is one 64-byte copy"""
    a, plain = _flat_adam()
    b, guarded = _flat_adam(skip_nonfinite=True)
    assert plain.guarded is False and plain.ctl is None and set(plain.state_dict()) == {"m", "v", "t", "lr", "betas", "eps"}
    with pytest.raises(RuntimeError, match="not guarded"):
        plain.stats()
    _drive(a, plain, range(4))
    _drive(b, guarded, range(4))
    assert _same(plain.flat, guarded.flat) and _same(plain.m, guarded.m) and _same(plain.v, guarded.v)
    st = guarded.stats()
    assert set(st) == {"applied", "skipped", "last_norm", "last_scale", "last_applied"}
    assert (st["applied"], st["skipped"], st["last_scale"], st["last_applied"]) == (4, 0, 1.0, 1)
    assert abs(st["last_norm"] - float(guarded.bucket.flat.double().norm())) <= 1e-12 * st["last_norm"]
    c, clipped = _flat_adam(max_grad_norm=0.01)                    # a clip implies the skip
    assert clipped.guarded and clipped.skip_nonfinite is False
    _drive(c, clipped, range(2), poison_at=(1,))
    st = clipped.stats()
    assert (st["applied"], st["skipped"], st["last_applied"]) == (1, 1, 0) and torch.isfinite(clipped.flat).all()
    with pytest.raises(ValueError, match="max_grad_norm"):
        _flat_adam(max_grad_norm=-1.0)


def test_resume_through_flat_adam_is_bit_equal(hip, tmp_path):
    """6 steps in one go against 3 steps, a checkpoint file (scripts/train.py's), fresh objects, and 3 more; a refused step among
    the first three and a bound that bites: p, m, v and the control block are the same bytes"""
    train = _train()
    kw = dict(max_grad_norm=0.5, skip_nonfinite=True)
    whole, opt = _flat_adam(**kw)
    _drive(whole, opt, range(6), poison_at=(1,))
    first, opt1 = _flat_adam(**kw)
    _drive(first, opt1, range(3), poison_at=(1,))
    path = str(tmp_path / "enc.pt.ckpt")
    train.save_checkpoint(path, first, opt1, epoch=0, step_in_epoch=3, total_step=3)
    second, opt2 = _flat_adam(**kw)
    with torch.no_grad():
        opt2.flat.add_(1.0)
    assert train.load_checkpoint(path, second, opt2, "cuda") == (0, 3, 3)
    opt2._check_views()                                            # the parameters are still views of the flat buffer
    assert opt2.t == 3 and opt2.stats()["skipped"] == 1 and opt2.stats()["applied"] == 2
    _drive(second, opt2, range(3, 6))
    assert _same(opt.flat, opt2.flat) and _same(opt.m, opt2.m) and _same(opt.v, opt2.v)
    assert bytes(opt.ctl.cpu().tolist()) == bytes(opt2.ctl.cpu().tolist())
    st = opt2.stats()
    assert (st["applied"], st["skipped"]) == (5, 1) and 0 < st["last_scale"] < 1
    for qa, qb in zip(whole.parameters(), second.parameters()):
        assert _same(qa.data, qb.data)


# ================================================================================================ end to end
NAN_COLUMNS = (40, 200)


@pytest.fixture(scope="module")
def radargram(tmp_path_factory):
    import dataset as crw_dataset
    rg = crw_dataset.synthetic_radargram(64, 256, seed=7)
    for c in NAN_COLUMNS:
        rg[:, c] = float("nan")
    path = tmp_path_factory.mktemp("guard") / "rg_nan.pt"
    torch.save(rg, str(path))
    return str(path), rg


def _arm(train, radargram, tmp_path, name, *flags):
    ckpt = str(tmp_path / f"{name}.pt")
    args = train.get_args_parser().parse_args(["--model", "0", "--data_path", radargram[0], "--patch_size", "16", "16", "--seq_length", "4",
                                               "--batch_size", "2", "--epochs", "1", "--save", ckpt, *flags])
    args.overlap = tuple(args.overlap)
    losses = []
    torch.manual_seed(11)                                           # what the module does at import
    train.main(args, on_step=lambda i, l: losses.append(l))
    return [float(l) for l in losses], torch.load(ckpt), train.main.optimizer, ckpt


def test_training_survives_two_nan_columns(hip, radargram, tmp_path, capsys):
    import dataset as crw_dataset
    train = _train()
    ds = crw_dataset.RGDataset.from_tensor(radargram[1], 4, (16, 16), (8, 0))
    finite = ds.finite_items()
    assert len(ds) == 13 and finite.tolist() == gr.finite_items_ref(radargram[1].numpy(), ds.pxh, ds.pxw, 16, 13) and int(finite.sum()) == 6
    # (i) as today: the witness that the fixture bites
    losses, saved, _, _ = _arm(train, radargram, tmp_path, "today")
    out = capsys.readouterr().out
    assert len(losses) == 6 and any(math.isnan(l) for l in losses) and "skipped:" not in out and "nodata" not in out
    assert all(not torch.isfinite(t).all() for t in saved.values() if t.is_floating_point())
    # (ii) refused steps
    losses, saved, opt, ckpt = _arm(train, radargram, tmp_path, "skip", "--skip_nonfinite", "--save_every", "2")
    out = capsys.readouterr().out
    bad = sum(not math.isfinite(l) for l in losses)
    st = opt.stats()
    print(f"--skip_nonfinite: losses {losses}, stats {st}")
    assert len(losses) == 6 and 0 < bad < 6 and st["skipped"] == bad and st["applied"] == 6 - bad
    assert all(torch.isfinite(t).all() for t in saved.values() if t.is_floating_point())
    assert f"skipped: {bad}  grad norm:" in out
    ck = torch.load(ckpt + ".ckpt")
    assert set(ck) == {"encoder", "optimizer", "epoch", "step_in_epoch", "total_step"} and (ck["epoch"], ck["step_in_epoch"], ck["total_step"]) == (0, 6, 6)
    assert "ctl" in ck["optimizer"] and ck["optimizer"]["t"] == 6
    # (iii) the bad items left out: nothing to refuse
    losses, saved, opt, _ = _arm(train, radargram, tmp_path, "nodata", "--nodata", "skip", "--skip_nonfinite")
    out = capsys.readouterr().out
    st = opt.stats()
    assert len(losses) == int(finite.sum()) // 2 == 3 and all(math.isfinite(l) for l in losses)
    assert (st["applied"], st["skipped"]) == (3, 0)
    assert out.count("--nodata skip: 7 of 13 items hold a NaN or an infinity; 7 items are left out of every epoch") == 1
    assert all(torch.isfinite(t).all() for t in saved.values() if t.is_floating_point())


def test_resumed_run_steps_over_the_consumed_batches(hip, radargram, tmp_path, capsys):
    """--save_every 2 --steps 2, then --resume: the resumed run takes the epoch's remaining four batches, in the epoch's order"""
    train = _train()
    seen = []
    real = train.epoch_items
    _, _, _, ckpt = _arm(train, radargram, tmp_path, "part", "--skip_nonfinite", "--save_every", "2", "--steps", "2")
    losses_a, _, opt_a, _ = _arm(train, radargram, tmp_path, "whole", "--skip_nonfinite")
    train.epoch_items = lambda *a, **kw: seen.append(real(*a, **kw)[0]) or real(*a, **kw)
    losses_b, _, opt_b, _ = _arm(train, radargram, tmp_path, "rest", "--skip_nonfinite", "--resume", ckpt + ".ckpt")
    out = capsys.readouterr().out
    assert "Resumed" in out and "epoch 0, 2 steps into it, 2 steps in all" in out
    assert len(losses_a) == 6 and len(losses_b) == 4 and seen == [real(13, 0, 2, None)[0]]
    assert [math.isfinite(l) for l in losses_b] == [math.isfinite(l) for l in losses_a[2:]]             # the same batches, in order
    sa, sb = opt_a.stats(), opt_b.stats()
    assert (sa["applied"], sa["skipped"]) == (sb["applied"], sb["skipped"]) and opt_b.t == 6
