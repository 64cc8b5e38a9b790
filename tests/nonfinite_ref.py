"""Non-finite values (NaN, +inf, -inf) on the training path: poison builders, the mask rules of the contract (include/crw_hip.h,
"Non-finite values") and the reference runs they are held against -- the PyTorch-op route of encoder.CNN / encoder.Resnet
on the CPU, the numpy oracle of the walk, torch.optim.Adam on the CPU.  tests/test_nonfinite.py pins what the references do and
tries the rules on hand-made masks; tests/test_nonfinite_gpu.py applies them to the kernels.

The rules ("non-finite" = NaN or +-inf, never told apart: the hi/lo bf16 split turns inf into NaN on its own):
    no laundering     where the reference is non-finite, we are             superset_misses(ref, ours) == 0
                      features, A, loss: the masks are EQUAL                mask_differences(ref, ours) == 0
    no contamination  what the reference keeps bit-equal to its clean run, we keep bit-equal to OUR clean run
                                                                            changed_bits(ours, ours_clean, keep) == 0
No tolerance appears anywhere: masks and bits only."""
import copy

import numpy as np
import torch

VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


# ------------------------------------------------------------------------------------------------ the rules
def nonfinite(t):
    """boolean mask (torch, on the CPU) of the NaN / inf entries of a tensor, an array or a number"""
    t = torch.as_tensor(np.asarray(t)) if not torch.is_tensor(t) else t.detach().cpu()
    return ~torch.isfinite(t)


def as_values(mask):
    """a boolean mask as a tensor the rules take: NaN where it is set, 0 elsewhere"""
    mask = torch.as_tensor(np.asarray(mask)) if not torch.is_tensor(mask) else mask
    assert mask.dtype == torch.bool
    return torch.where(mask, float("nan"), 0.0)


def _masks(ref, ours):
    ref, ours = nonfinite(ref), nonfinite(ours)
    assert ref.shape == ours.shape, ("the masks describe different tensors", tuple(ref.shape), tuple(ours.shape))
    return ref, ours


def superset_misses(ref, ours):
    """entries where the reference is non-finite and we are finite (laundered); 0 = the rule holds"""
    ref, ours = _masks(ref, ours)
    return int((ref & ~ours).sum())


def mask_differences(ref, ours):
    """entries non-finite on one side only: laundered ones and spurious ones; 0 = the masks are equal"""
    ref, ours = _masks(ref, ours)
    return int((ref ^ ours).sum())


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])


def changed_bits(run, clean, keep=None):
    """entries of run[keep] whose BITS differ from clean[keep] (keep: index along dimension 0, all of it when None) -- -0.0 against
    0.0 and one NaN payload against another count; 0 = not contaminated"""
    assert run.shape == clean.shape and run.dtype == clean.dtype, (run.shape, clean.shape, run.dtype, clean.dtype)
    a, b = _bits(run), _bits(clean)
    if keep is not None:
        keep = torch.as_tensor(keep, dtype=torch.long)
        a, b = a[keep], b[keep]
    return int((a != b).sum())


def others(n, poisoned):
    """the indices 0 .. n-1 that are not poisoned"""
    gone = set(int(i) for i in poisoned)
    return [i for i in range(n) if i not in gone]


# ------------------------------------------------------------------------------------------------ poison builders
def pixel(h, w, where):
    return {"corner": (0, 0), "centre": (h // 2, w // 2), "last": (h - 1, w - 1)}[where]


def patch_poisons(P, tile=128):
    """several poisons for one run (the no-contamination rule keeps them apart): NaN at the corner pixel of patch 0 (it reaches ONE
    candidate of a pooling window), +inf at the centre of patch 1, -inf at the last pixel of the patch on either side of a boundary
    -- of the 128-patch tile when P crosses one, else of the middle -- and NaN in patch P - 1.  -> [(patch, where, value name)]"""
    edge = tile if P > tile else P // 2
    got = [(0, "corner", "nan"), (1, "centre", "+inf"), (edge - 1, "last", "-inf"), (edge, "last", "-inf"), (P - 1, "centre", "nan")]
    seen, out = set(), []
    for p, where, v in got:
        if 0 <= p < P and p not in seen:
            seen.add(p)
            out.append((p, where, v))
    assert len(out) < P, "no clean patch left"
    return out


def poison_patches(x, poisons, channel=-1):
    """x [P,cin,h,w] -> a copy with the poisons of patch_poisons() written (into the last channel: the image, not the position code)"""
    x = x.clone()
    h, w = x.shape[-2:]
    for p, where, v in poisons:
        y, xx = pixel(h, w, where)
        x[p, channel, y, xx] = VALUES[v]
    return x


def poisoned_patches(poisons):
    return sorted(p for p, _, _ in poisons)


def poison_entry(t, index, value):
    """a copy of t with t[index] = VALUES[value]"""
    t = t.clone()
    t[index] = VALUES[value]
    return t


# ------------------------------------------------------------------------------------------------ reference runs
def _step(net, x, gy):
    """features and parameter gradients of net(x) under the output gradient gy (None: forward only)"""
    net.zero_grad(set_to_none=True)
    if gy is None:
        with torch.no_grad():
            return net(x).detach(), {}
    y = net(x)
    y.backward(gy)
    return y.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def cpu_module(net, dtype=torch.float32):
    """a copy of the module on the CPU: CPU tensors take the PyTorch-op route (encoder.py), whatever hip_convs says"""
    return copy.deepcopy(net).to("cpu", dtype)


def module_reference(net, x, gy=None, dtype=torch.float32):
    """the PyTorch-op route on the CPU -> (features, {parameter: gradient}, {buffer: value after the call}); net is not touched"""
    ref = cpu_module(net, dtype)
    y, grads = _step(ref, x.detach().cpu().to(dtype), None if gy is None else gy.detach().cpu().to(dtype))
    return y, grads, {k: b.detach().clone() for k, b in ref.named_buffers()}


def oracle_run(emb, tau):
    """the numpy oracle in float64 on raw features emb [B,T,N,C] -> dict(loss, A, At, dA, demb, ehat, norm)"""
    from oracle import crw_oracle as orc
    e = np.asarray(emb, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = orc.crw_from_features(e, tau)
        nrm = np.sqrt((e * e).sum(-1))
        out["norm"] = np.maximum(nrm, orc.EPS_NORM)
        out["ehat"] = e / out["norm"][..., None]
    return out


def adam_reference(p, grads, lr=1e-3):
    """torch.optim.Adam (defaults) on the CPU, one step per gradient in `grads` -> (p, m, v) after the last"""
    q = torch.nn.Parameter(p.detach().cpu().clone())
    opt = torch.optim.Adam([q], lr=lr)
    for g in grads:
        q.grad = g.detach().cpu().clone()
        opt.step()
    st = opt.state[q]
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]
