"""What the reference side does with NaN and infinite values -- the PyTorch-op route of encoder.CNN / encoder.Resnet, the numpy oracle
of the walk, torch.optim.Adam, all on the CPU -- pinned as assertions, so that a PyTorch whose relu / max_pool2d / softmax stop
propagating them shows up here and not as a riddle in tests/test_nonfinite_gpu.py; and the rule functions of tests/nonfinite_ref.py
on hand-made masks, the ones they must reject included.  No GPU."""
import numpy as np
import pytest
import torch

import encoder
import nonfinite_ref as nf

P, BAD = 6, 2                        # six patches, one pixel of patch 2 poisoned
REST = nf.others(P, [BAD])
WHERE = ("corner", "centre", "last")


# ------------------------------------------------------------------------------------------------ the rules on hand-made masks
def test_rules_accept_and_reject():
    nan, inf = float("nan"), float("inf")
    ref = torch.tensor([1.0, nan, 3.0, -inf])
    assert nf.nonfinite(ref).tolist() == [False, True, False, True]
    assert nf.nonfinite(np.float64(nan)).item() and not nf.nonfinite(0.5).item()
    # NaN and inf are not told apart; a superset passes the superset rule and fails the equality rule
    assert nf.superset_misses(ref, torch.tensor([1.0, inf, 3.0, nan])) == 0
    assert nf.mask_differences(ref, torch.tensor([1.0, inf, 3.0, nan])) == 0
    assert nf.superset_misses(ref, torch.tensor([nan, nan, 3.0, nan])) == 0
    assert nf.mask_differences(ref, torch.tensor([nan, nan, 3.0, nan])) == 1          # a spurious NaN
    # laundering: the reference's NaN came out as 0 -- both rules reject
    assert nf.superset_misses(ref, torch.tensor([1.0, 0.0, 3.0, -inf])) == 1
    assert nf.mask_differences(ref, torch.tensor([1.0, 0.0, 3.0, -inf])) == 1
    assert nf.superset_misses(ref, torch.zeros(4)) == 2
    with pytest.raises(AssertionError):
        nf.superset_misses(ref, torch.zeros(5))
    # bits: -0.0 is not 0.0, a NaN equals itself, rows outside `keep` do not count
    clean = torch.tensor([[0.0, 1.0], [2.0, nan], [4.0, 5.0]])
    run = torch.tensor([[-0.0, 1.0], [2.0, nan], [nan, 5.0]])
    assert nf.changed_bits(clean, clean.clone()) == 0
    assert nf.changed_bits(run, clean) == 2 and nf.changed_bits(run, clean, [1]) == 0 and nf.changed_bits(run, clean, [0, 1]) == 1
    assert nf.changed_bits(run.double(), clean.double(), [2]) == 1
    with pytest.raises(AssertionError):
        nf.changed_bits(run, clean.double())
    assert nf.others(5, [1, 3]) == [0, 2, 4]
    assert nf.nonfinite(nf.as_values(torch.tensor([True, False]))).tolist() == [True, False]


def test_poison_builders():
    for n, want in ((5, [0, 1, 2, 4]), (29, [0, 1, 13, 14, 28]), (130, [0, 1, 127, 128, 129]), (70, [0, 1, 34, 35, 69])):
        ps = nf.patch_poisons(n)
        assert nf.poisoned_patches(ps) == want and ps[0] == (0, "corner", "nan") and ps[-1][2] == "nan"
        assert {v for _, _, v in ps} == set(nf.VALUES)
    x = torch.zeros(5, 2, 20, 27)
    xp = nf.poison_patches(x, nf.patch_poisons(5))
    assert int(nf.nonfinite(xp).sum()) == 4 and int(nf.nonfinite(xp[:, 0]).sum()) == 0 and int(nf.nonfinite(x).sum()) == 0
    assert torch.isnan(xp[0, 1, 0, 0]) and xp[1, 1, 10, 13] == float("inf") and xp[2, 1, 19, 26] == float("-inf")
    e = nf.poison_entry(torch.zeros(2, 3), (1, 2), "-inf")
    assert e[1, 2] == float("-inf") and int(nf.nonfinite(e).sum()) == 1


# ------------------------------------------------------------------------------------------------ CNN
@pytest.fixture(scope="module")
def cnn():
    torch.manual_seed(3)
    return encoder.CNN(False)


@pytest.mark.parametrize("hw", [(16, 16), (20, 27)], ids=["16x16", "20x27"])
def test_cnn_reference_is_patch_local_and_propagates(cnn, hw):
    """one poisoned pixel: all 128 features of its patch non-finite, the other five patches bit-equal to the clean run, fp32 and fp64
    masks alike.  Gradients under a finite gy: every bias finite (no activation enters it); conv3 / conv4 / conv5 / fc weights
    entirely non-finite; conv1.weight: the taps that ever meet the pixel -- 4 of 25 at a corner (padding 1), all at the centre;
    conv2.weight in between at a corner (18 .. 36 % non-finite), all at the centre."""
    h, w = hw
    g = torch.Generator().manual_seed(h * w)
    x, gy = torch.randn(P, 1, h, w, generator=g), torch.randn(P, 128, generator=g)
    y0, g0, _ = nf.module_reference(cnn, x, gy)
    assert int(nf.nonfinite(y0).sum()) == 0 and all(int(nf.nonfinite(t).sum()) == 0 for t in g0.values())
    for where in WHERE:
        for v in nf.VALUES:
            xp = nf.poison_patches(x, [(BAD, where, v)])
            y, gr, _ = nf.module_reference(cnn, xp, gy)
            y64, gr64, _ = nf.module_reference(cnn, xp, gy, torch.float64)
            tag = (hw, where, v)
            assert int(nf.nonfinite(y[BAD]).sum()) == 128 and int(nf.nonfinite(y[REST]).sum()) == 0, tag
            assert nf.changed_bits(y, y0, REST) == 0, tag
            assert nf.mask_differences(y, y64) == 0 and all(nf.mask_differences(gr[k], gr64[k]) == 0 for k in gr), tag
            bad = {k: int(nf.nonfinite(t).sum()) for k, t in gr.items()}
            size = {k: t.numel() for k, t in gr.items()}
            assert all(bad[k] == 0 for k in bad if k.endswith(".bias")), (tag, bad)
            assert all(bad[k] == size[k] for k in ("conv3.weight", "conv4.weight", "conv5.weight", "fc.weight")), (tag, bad)
            if where == "centre":
                assert bad["conv1.weight"] == size["conv1.weight"] and bad["conv2.weight"] == size["conv2.weight"], (tag, bad)
            else:
                assert bad["conv1.weight"] * 25 == 4 * size["conv1.weight"], (tag, bad)
                assert 18 * size["conv2.weight"] <= 100 * bad["conv2.weight"] <= 36 * size["conv2.weight"], (tag, bad)


@pytest.mark.parametrize("name", ["conv3.weight", "conv1.bias"])
def test_cnn_reference_poisoned_weight(cnn, name):
    """one NaN in a weight or a bias: every feature of every patch non-finite"""
    net = nf.cpu_module(cnn)
    with torch.no_grad():
        dict(net.named_parameters())[name].view(-1)[1] = float("nan")
    y, _, _ = nf.module_reference(net, torch.randn(P, 1, 16, 16, generator=torch.Generator().manual_seed(1)))
    assert int(nf.nonfinite(y).sum()) == y.numel()


# ------------------------------------------------------------------------------------------------ Resnet
def test_resnet_reference_train_spreads_eval_is_patch_local():
    torch.manual_seed(4)
    rn = encoder.Resnet(False)
    g = torch.Generator().manual_seed(5)
    x, gy = torch.randn(P, 1, 16, 16, generator=g), torch.randn(P, 128, generator=g)
    for v in nf.VALUES:
        xp = nf.poison_patches(x, [(BAD, "corner", v)])
        rn.train(True)                                  # batch statistics: the poison reaches every patch and stays in the buffers
        y, gr, bufs = nf.module_reference(rn, xp, gy)
        assert int(nf.nonfinite(y).sum()) == y.numel() == P * 128, v
        assert int(nf.nonfinite(bufs["bn0.running_mean"]).sum()) == 3 and int(nf.nonfinite(bufs["bn0.running_var"]).sum()) == 3, v
        assert int(nf.nonfinite(gr["model.fc.bias"]).sum()) == 0                      # the sum of gy
        assert all(int(nf.nonfinite(gr[k]).sum()) == gr[k].numel() for k in ("fc0.weight", "bn0.weight", "model.conv1.weight", "model.fc.weight")), v
        rn.train(False)                                 # running statistics: patch-local
        y0, _, _ = nf.module_reference(rn, x)
        y, _, _ = nf.module_reference(rn, xp)
        assert int(nf.nonfinite(y[BAD]).sum()) == 128 and int(nf.nonfinite(y[REST]).sum()) == 0, v
        assert nf.changed_bits(y, y0, REST) == 0, v


# ------------------------------------------------------------------------------------------------ the walk's oracle
def _emb(B, T, N, C):
    g = torch.Generator().manual_seed(N + C)
    return (torch.randn(1, 1, N, C, generator=g) + 0.6 * torch.randn(B, T, N, C, generator=g)).float()


def test_oracle_masks_by_poisoned_frame():
    """B=3, T=4, N=7, C=8, one entry of emb[1, t, 3] poisoned.  t = 0, 1: loss NaN; t = T-1: the last logit matrix feeds no cycle --
    the loss is the clean run's, to the bit.  Items 0 and 2 bit-equal to the clean run throughout."""
    B, T, N, C, tau = 3, 4, 7, 8, 0.07
    emb = _emb(B, T, N, C)
    clean = nf.oracle_run(emb.numpy(), tau)
    assert all(int(nf.nonfinite(clean[k]).sum()) == 0 for k in clean)
    # frame -> non-finite entries of (A[1] of 147, At[1] of 98, demb[1] of 224)
    want = {0: (7, 98, 168), 1: (14, 56, 168), T - 1: (7, 0, 112)}
    for t, counts in want.items():
        for v in nf.VALUES:
            o = nf.oracle_run(nf.poison_entry(emb, (1, t, 3, 5), v).numpy(), tau)
            got = tuple(int(nf.nonfinite(o[k][1]).sum()) for k in ("A", "At", "demb"))
            assert got == counts, (t, v, got)
            if t == T - 1:
                assert float(o["loss"]) == float(clean["loss"]), (v, float(o["loss"]))
            else:
                assert np.isnan(o["loss"]), (t, v)
            assert int(nf.nonfinite(o["norm"]).sum()) == 1 and nf.nonfinite(o["norm"])[1, t, 3].item()
            assert int(nf.nonfinite(o["ehat"][1, t, 3]).sum()) >= 1 and int(nf.nonfinite(o["ehat"]).sum()) <= C
            for k in ("A", "At", "dA", "demb"):
                assert nf.changed_bits(torch.as_tensor(o[k]), torch.as_tensor(clean[k]), [0, 2]) == 0, (t, v, k)


def test_oracle_zero_row_is_finite():
    emb = _emb(3, 4, 7, 8)
    emb[1, 1, 3] = 0.0
    o = nf.oracle_run(emb.numpy(), 0.07)
    assert all(int(nf.nonfinite(o[k]).sum()) == 0 for k in o)


# ------------------------------------------------------------------------------------------------ Adam
def test_adam_reference_is_elementwise():
    n = 4 * 256 + 3
    g = torch.Generator().manual_seed(9)
    p, g1, g2 = (torch.randn(n, generator=g) for _ in range(3))
    bad = {0: "nan", 4 * 256 - 2: "+inf", n - 2: "nan"}     # float4 body, its last quad, the scalar tail
    g1p = g1.clone()
    for i, v in bad.items():
        g1p[i] = nf.VALUES[v]
    clean = nf.adam_reference(p, [g1, g2])
    run = nf.adam_reference(p, [g1p, g2])               # the poison arrives once; the moments keep it
    for a, b in zip(run, clean):
        assert sorted(torch.nonzero(nf.nonfinite(a)).flatten().tolist()) == sorted(bad)
        assert nf.changed_bits(a, b, nf.others(n, bad)) == 0
