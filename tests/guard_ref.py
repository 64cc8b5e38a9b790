"""The guarded Adam step of include/crw_hip_guard.h as plain loops (no GPU, no library): the definition that tests/test_guard.py holds
against torch.optim.Adam + torch.nn.utils.clip_grad_norm_ and that tests/test_guard_gpu.py uses for the norm, the coefficient and the
counters.  fp64 norm, fp32 update, one element at a time.

The roundings of the update are those of torch's CPU kernels, which is what lets the CPU test ask for bits: the first moment is one
fused multiply-add (lerp), the second moment is v * b2 rounded, then one fused multiply-add of (w2 * g) and g onto it (addcmul),
everything else rounds after every operation.  The device fuses the second moment the other way round (v * b2 is the fused product),
so on the GPU the bits are held against crw_adam_step itself, never against this file."""
import math
import struct

import numpy as np

f32 = np.float32

CTL_BYTES = 64
CTL_FORMAT = "<qqdfi"                  # int64 applied; int64 skipped; double norm; float scale; int32 last_applied; reserved
CTL_OFFSETS = {"applied": 0, "skipped": 8, "norm": 16, "scale": 24, "last_applied": 28, "reserved": 32}
BLOCK_ELEMS = 4096                     # elements per reduction block (CRW_GUARD_BLOCK_ELEMS)


def fma32(a, b, c):
    """fl32(a * b + c) with one rounding"""
    if hasattr(math, "fma"):
        return f32(math.fma(float(a), float(b), float(c)))
    return f32(np.float64(a) * np.float64(b) + np.float64(c))      # the product is exact in fp64


def sum_squares(g):
    """ss = sum of (double)g[i]^2 in index order, and sqrt(ss); the device's order differs (per-block partials), so the two agree
    within n * 2^-52 * norm, and exactly on whether ss is finite"""
    ss = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for x in np.asarray(g, dtype=np.float32):
            ss = ss + float(x) * float(x)
    return ss, math.sqrt(ss) if ss >= 0 and not math.isnan(ss) else float("nan")


def clip_coef(norm, max_norm):
    """c = fp32(min(1, max_norm / (norm + 1e-6))) when 0 < max_norm < inf, else 1"""
    if max_norm is None or not (0 < max_norm < math.inf):
        return f32(1.0)
    return f32(min(1.0, float(f32(max_norm)) / (norm + 1e-6)))


def bias_coefficients(lr, beta1, beta2, t):
    """(-lr / (1 - beta1^t), sqrt(1 - beta2^t)): in double from the Python floats like the host code of torch.optim, each rounded
    once.  (The C ABI is handed fp32 betas and widens those: its coefficients can sit one fp32 ulp away.)"""
    return f32(-lr / (1.0 - beta1 ** t)), f32(math.sqrt(1.0 - beta2 ** t))


def adam_update(p, g, m, v, neg_step, bc2_sqrt, beta1, beta2, eps):
    """crw_adam_step's arithmetic on fp32 arrays in place, element by element"""
    w1, w2, b2, eps = f32(1.0 - beta1), f32(1.0 - beta2), f32(beta2), f32(eps)      # the weights rounded from double, like torch's
    with np.errstate(all="ignore"):
        for i in range(len(p)):
            gg = f32(g[i])
            m[i] = fma32(w1, f32(gg - m[i]), m[i])
            v[i] = fma32(f32(w2 * gg), gg, f32(v[i] * b2))
            denom = f32(f32(np.sqrt(v[i])) / bc2_sqrt) + eps
            p[i] = f32(p[i] + f32(neg_step * f32(m[i] / f32(denom))))


class GuardRef:
    """p, m, v (fp32 numpy arrays, updated in place) and the control block as a dict; step(g, max_norm) is one call."""

    def __init__(self, p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.p = np.array(p, dtype=np.float32)
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)
        self.lr, self.betas, self.eps = lr, betas, eps
        self.calls = 0
        self.ctl = dict(applied=0, skipped=0, norm=0.0, scale=f32(0), last_applied=0)

    def step(self, g, max_norm=None):
        self.calls += 1
        ss, norm = sum_squares(g)
        c = self.ctl
        if not math.isfinite(ss):                                       # p, m, v keep their bits
            c.update(skipped=c["skipped"] + 1, last_applied=0, norm=norm, scale=f32(0))
            return False
        t = self.calls - c["skipped"]
        assert t == c["applied"] + 1
        coef = clip_coef(norm, max_norm)
        with np.errstate(all="ignore"):
            scaled = np.array([f32(f32(x) * coef) for x in g], dtype=np.float32)      # g itself is never written
        neg_step, bc2_sqrt = bias_coefficients(self.lr, self.betas[0], self.betas[1], t)
        adam_update(self.p, scaled, self.m, self.v, neg_step, bc2_sqrt, self.betas[0], self.betas[1], self.eps)
        c.update(applied=c["applied"] + 1, last_applied=1, norm=norm, scale=coef)
        return True

    def ctl_bytes(self):
        c = self.ctl
        return struct.pack(CTL_FORMAT, c["applied"], c["skipped"], c["norm"], float(c["scale"]), c["last_applied"]).ljust(CTL_BYTES, b"\0")


def finite_items_ref(T, pxh, pxw, stride, count):
    """item i is finite when rows [0, pxh) x columns [stride * i, stride * i + pxw) of the radargram T hold no NaN or infinity:
    a plain loop over the items"""
    out = []
    for i in range(count):
        block = np.asarray(T[:pxh, stride * i:stride * i + pxw], dtype=np.float64)
        out.append(bool(np.isfinite(block).all()))
    return out
