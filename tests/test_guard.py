"""Keeping a training run alive, the parts that need no GPU: the guarded Adam step's definition (tests/guard_ref.py, plain loops)
against torch.optim.Adam and torch.nn.utils.clip_grad_norm_; `RGDataset.finite_items()` against a plain loop over the items; the
flags of scripts/train.py, what they refuse, what `--nodata skip` leaves of an epoch; and checkpoint / resume on the CPU optimizer
path (`GuardedTorchAdam`), bit for bit."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import guard_ref as gr
from conftest import PKG, load_golden

N, STEPS = 37, 20


def _train():
    spec = importlib.util.spec_from_file_location("crw_train_guard", os.path.join(PKG, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def train():
    return _train()


def _grads(seed=3, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(N, generator=g)
    return p0, [torch.randn(N, generator=g) * scale * 10.0 ** ((t % 6) - 3) for t in range(STEPS)]


# ================================================================================================ the definition against torch
def test_definition_without_a_clip_is_torch_adam_bit_for_bit():
    """20 steps at n = 37, gradients over six orders of magnitude: m, v and p of the plain loops are the bits of an fp32
    torch.optim.Adam (defaults, lr 1e-3), the norm is the fp64 norm, and every step counts as applied with scale 1"""
    p0, grads = _grads()
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=1e-3)
    ref = gr.GuardRef(p0.numpy())
    for t, g in enumerate(grads, 1):
        q.grad = g.clone()
        opt.step()
        assert ref.step(g.numpy(), max_norm=None) is True
        st = opt.state[q]
        assert np.array_equal(st["exp_avg"].numpy(), ref.m) and np.array_equal(st["exp_avg_sq"].numpy(), ref.v), t
        assert np.array_equal(q.detach().numpy(), ref.p), t
        want = float(g.double().norm())
        assert abs(ref.ctl["norm"] - want) <= N * 2.0 ** -52 * want
        assert (ref.ctl["applied"], ref.ctl["skipped"], ref.ctl["last_applied"], float(ref.ctl["scale"])) == (t, 0, 1, 1.0)
    for max_norm in (0, 0.0, math.inf):                          # no bound
        assert float(gr.clip_coef(3.0, max_norm)) == 1.0


def test_definition_with_a_clip_against_fp64_torch():
    """the same 20 steps with max_norm = a tenth of the typical norm (so most steps are clipped and some are not) against
    torch.optim.Adam + clip_grad_norm_ on fp64 copies: every update u = p_new - p_old within
    2^-21 |u_ref| + 2^-23 |p| (the bound tests/test_guard_gpu.py puts on a recomputed step), the coefficient within fp32 rounding"""
    p0, grads = _grads()
    max_norm = 0.5
    q = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([q], lr=1e-3)
    ref = gr.GuardRef(p0.numpy())
    clipped = 0
    for t, g in enumerate(grads, 1):
        q.grad = g.double().clone()
        total = torch.nn.utils.clip_grad_norm_([q], max_norm)
        before64, before32 = q.detach().clone(), ref.p.copy()
        opt.step()
        ref.step(g.numpy(), max_norm=max_norm)
        coef = min(1.0, max_norm / (float(total) + 1e-6))
        assert float(ref.ctl["scale"]) == float(np.float32(coef)), t
        clipped += coef < 1.0
        u_ref = (q.detach() - before64).numpy()
        u = ref.p.astype(np.float64) - before32.astype(np.float64)
        bound = 2.0 ** -21 * np.abs(u_ref) + 2.0 ** -23 * np.abs(before64.numpy())
        worst = float(np.max(np.abs(u - u_ref) / bound))
        print(f"step {t}: coef {coef:.6g}, worst |u - u_ref| / bound = {worst:.3f}")
        assert np.all(np.abs(u - u_ref) <= bound), (t, worst)
    assert 0 < clipped < STEPS                                    # both sides of the bound were taken


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_poisoned_step_changes_nothing_and_does_not_count(bad):
    p0, grads = _grads()
    ref, twin = gr.GuardRef(p0.numpy()), gr.GuardRef(p0.numpy())
    for g in grads[:3]:
        ref.step(g.numpy())
        twin.step(g.numpy())
    poisoned = grads[3].numpy().copy()
    poisoned[N // 2] = bad
    before = (ref.p.copy(), ref.m.copy(), ref.v.copy())
    assert ref.step(poisoned, max_norm=1.0) is False
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, (ref.p, ref.m, ref.v)))
    c = ref.ctl
    assert (c["applied"], c["skipped"], c["last_applied"], float(c["scale"])) == (3, 1, 0, 0.0) and not math.isfinite(c["norm"])
    # the next step is step t = applied + 1 = 4 although it is the fifth call: the twin that never saw the poison takes the same one
    ref.step(grads[4].numpy())
    twin.step(grads[4].numpy())
    assert ref.calls == 5 and twin.calls == 4 and ref.ctl["applied"] == twin.ctl["applied"] == 4
    assert np.array_equal(ref.p, twin.p) and np.array_equal(ref.m, twin.m) and np.array_equal(ref.v, twin.v)
    assert len(ref.ctl_bytes()) == gr.CTL_BYTES


# ================================================================================================ finite_items
def _dataset(name):
    import dataset as crw_dataset
    g = load_golden(name)
    dim, ov, L = tuple(int(x) for x in g["dim"]), tuple(int(x) for x in g["overlap"]), int(g["length"])
    return (lambda rg: crw_dataset.RGDataset.from_tensor(rg, L, dim, ov)), torch.tensor(g["rg"]).clone()


def _hold(ds):
    want = gr.finite_items_ref(ds.T.numpy(), ds.pxh, ds.pxw, ds.w - ds.ow, len(ds))
    got = ds.finite_items()
    assert got.dtype == torch.bool and tuple(got.shape) == (len(ds),)
    assert got.tolist() == want
    return want


@pytest.mark.parametrize("name", ["dataset_64x256", "dataset_50x200_ow"])
def test_finite_items_against_a_loop_over_items(name, capsys):
    """the two dataset fixtures' geometries (the second overlaps in W): a poisoned column at an item's first column, at its last
    column and one column past it, a NaN, an infinity, a poisoned pixel below the rows the items span, and a clean radargram"""
    make, rg = _dataset(name)
    ds = make(rg.clone())
    assert all(_hold(ds))                                          # clean: every item is finite
    sw, pxw, pxh, n = ds.w - ds.ow, ds.pxw, ds.pxh, len(ds)
    i = n // 2
    for col, hit in ((sw * i, True), (sw * i + pxw - 1, True), (sw * i + pxw, False)):
        for bad in (float("nan"), float("inf"), -float("inf")):
            t = rg.clone()
            t[pxh // 2, col] = bad
            want = _hold(make(t))
            assert col < t.shape[1] and want[i] is (not hit)
            if ds.ow == 0 and col == sw * i + pxw and i + 1 < n:
                assert want[i + 1] is False                        # without overlap the column past an item is the next item's first
    if pxh < rg.shape[0]:                                          # rows the items do not span are not looked at
        t = rg.clone()
        t[pxh:, :] = float("nan")
        assert all(_hold(make(t)))
    t = rg.clone()                                                 # two poisoned columns, first and last row
    t[0, 3] = float("nan")
    t[pxh - 1, rg.shape[1] - 1] = float("inf")
    want = _hold(make(t))
    assert want[0] is False and (want[-1] is False or sw * (n - 1) + pxw < rg.shape[1])
    capsys.readouterr()


def test_finite_items_under_shared_encode_batches(train):
    """--shared_encode: batch b = items [b * B, (b + 1) * B) is kept only when all of them are finite; the ordinary order drops the
    items themselves, before the batches are cut, and both are functions of the epoch number alone"""
    make, rg = _dataset("dataset_50x200_ow")
    t = rg.clone()
    ds0 = make(rg.clone())
    t[1, (ds0.w - ds0.ow) * 2] = float("nan")                       # the first column of item 2: items 0 .. 2 at most hold it
    ds = make(t)
    finite = train.finite_mask(ds)
    assert finite == gr.finite_items_ref(t.numpy(), ds.pxh, ds.pxw, ds.w - ds.ow, len(ds)) and not all(finite) and any(finite)
    B = 2
    for epoch in (0, 1):
        order, g = train.epoch_items(len(ds), epoch, B, finite)
        plain, g0 = train.epoch_items(len(ds), epoch, B, None)
        assert [i for i in plain if finite[i]][:len(order)] == order and len(order) % B == 0 and all(finite[i] for i in order)
        assert len(order) == sum(finite) // B * B
        assert train.epoch_items(len(ds), epoch, B, finite)[0] == order                       # the same on every rank, and on resume
        kept = train.shared_batches(len(ds), B, g, finite)
        every = train.shared_batches(len(ds), B, g0, None)
        assert sorted(every) == list(range(len(ds) // B))
        assert kept == [b for b in every if all(finite[b * B:(b + 1) * B])] and len(kept) < len(every)
    sub = torch.utils.data.Subset(ds, range(0, len(ds), 3))
    assert train.finite_mask(sub) == [finite[i] for i in range(0, len(ds), 3)]


# ================================================================================================ the flags
def test_flags_parse_default_to_today_and_refuse(train, tmp_path):
    parse = train.get_args_parser().parse_args
    a = parse([])
    assert (a.nodata, a.clip_grad_norm, a.skip_nonfinite, a.save_every, a.resume) == ("keep", None, False, 0, "")
    assert train.check_flags(a) is False
    assert not any(k in str(train.printable(a)) for k in train.SURVIVAL_DEFAULTS)             # the printed line is what it was
    assert "model=1" in str(train.printable(a)) and "save=''" in str(train.printable(a))
    b = parse(["--nodata", "skip", "--clip_grad_norm", "2.5", "--skip_nonfinite", "--save_every", "10"])
    assert (b.nodata, b.clip_grad_norm, b.skip_nonfinite, b.save_every) == ("skip", 2.5, True, 10) and train.check_flags(b) is True
    assert all(k in str(train.printable(b)) for k in ("nodata='skip'", "clip_grad_norm=2.5", "skip_nonfinite=True", "save_every=10"))
    assert train.check_flags(parse(["--clip_grad_norm", "1"])) is True and train.check_flags(parse(["--skip_nonfinite"])) is True
    with pytest.raises(SystemExit):
        parse(["--nodata", "drop"])                               # argparse: keep and skip are the choices
    for argv, msg in ((["--clip_grad_norm", "0"], "clip_grad_norm must be a finite number > 0"),
                      (["--clip_grad_norm", "-1"], "clip_grad_norm"), (["--clip_grad_norm", "nan"], "clip_grad_norm"),
                      (["--clip_grad_norm", "inf"], "clip_grad_norm"), (["--save_every", "-3"], "save_every must be >= 0"),
                      (["--resume", str(tmp_path / "none.ckpt")], "no such checkpoint")):
        with pytest.raises(SystemExit, match=msg):
            train.check_flags(parse(argv))
    old = parse([])
    for k in train.SURVIVAL_DEFAULTS:                              # an args object built before the flags existed
        delattr(old, k)
    assert train.check_flags(old) is False and old.nodata == "keep"
    assert train.save_path(parse(["--save", "x/y.pt"])) == "x/y.pt" and train.save_path(a).endswith("models/sharad16_3.pt")


# ================================================================================================ the CPU optimizer path
def _net():
    torch.manual_seed(4)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def _batch(step, poison=False):
    g = torch.Generator().manual_seed(100 + step)
    x = torch.randn(4, 6, generator=g)
    if poison:
        x[0, 0] = float("nan")
    return x, torch.randn(4, 3, generator=g)


def _run(train, net, opt, steps, poison_at=()):
    for s in steps:
        x, y = _batch(s, s in poison_at)
        for p in net.parameters():
            p.grad = None
        ((net(x) - y) ** 2).mean().backward()
        opt.step()


def test_cpu_fallback_clips_and_skips_like_torch(train):
    net, twin = _net(), _net()
    opt = train.GuardedTorchAdam(net.parameters(), 1e-2, max_grad_norm=0.05, skip_nonfinite=False)
    ref = torch.optim.Adam(twin.parameters(), lr=1e-2)
    before = None
    for s in range(5):
        if s == 2:                                                 # a poisoned batch: refused, nothing moves (a clip implies the skip)
            before = [p.detach().clone() for p in net.parameters()]
            _run(train, net, opt, [s], poison_at=(s,))
            assert all(torch.equal(a, b) for a, b in zip(before, net.parameters()))
            assert opt.stats()["skipped"] == 1 and opt.stats()["last_applied"] == 0 and not math.isfinite(opt.stats()["last_norm"])
            continue
        _run(train, net, opt, [s])
        x, y = _batch(s)
        ref.zero_grad()
        ((twin(x) - y) ** 2).mean().backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.05)
        ref.step()
        assert all(torch.equal(a, b) for a, b in zip(net.parameters(), twin.parameters())), s
    st = opt.stats()
    assert (st["applied"], st["skipped"], st["last_applied"]) == (4, 1, 1) and 0 < st["last_scale"] < 1 and st["last_norm"] > 0.05
    plain = train.GuardedTorchAdam(_net().parameters(), 1e-2)
    assert plain.guarded is False


def test_resume_on_the_cpu_optimizer_path_is_bit_equal(train, tmp_path):
    """6 steps in one go against 3 steps, a checkpoint, a fresh process' worth of objects, and 3 more -- with a refused step among
    the first three, so that the applied count (not the call count) is what the resumed optimizer must carry"""
    kw = dict(max_grad_norm=0.05, skip_nonfinite=True)
    whole = _net()
    opt = train.GuardedTorchAdam(whole.parameters(), 1e-2, **kw)
    _run(train, whole, opt, range(6), poison_at=(1,))
    first = _net()
    opt1 = train.GuardedTorchAdam(first.parameters(), 1e-2, **kw)
    _run(train, first, opt1, range(3), poison_at=(1,))
    path = str(tmp_path / "run.pt.ckpt")
    train.save_checkpoint(path, first, opt1, epoch=1, step_in_epoch=3, total_step=3)
    assert not os.path.exists(path + ".tmp")
    second = _net()
    with torch.no_grad():
        for p in second.parameters():
            p.add_(1.0)                                            # not the checkpoint's values until it is loaded
    opt2 = train.GuardedTorchAdam(second.parameters(), 1e-2, **kw)
    assert train.load_checkpoint(path, second, opt2) == (1, 3, 3)
    _run(train, second, opt2, range(3, 6))
    for a, b in zip(whole.parameters(), second.parameters()):
        assert torch.equal(a, b)
    assert opt2.stats() == opt.stats() and opt.stats()["skipped"] == 1 and opt.stats()["applied"] == 5
    for (ka, sa), (kb, sb) in zip(opt.opt.state_dict()["state"].items(), opt2.opt.state_dict()["state"].items()):
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and sa["step"] == sb["step"]
