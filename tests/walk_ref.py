"""float64 references for the walk's logit gradient dA, slice by slice.  TEST INFRASTRUCTURE ONLY (no GPU needed).

`oracle.walk_backward` is the formula; this module adds what the route tests (test_walk_routes.py on the CPU,
test_walk_routes_gpu.py on the device) share:

  inputs ........ seeded fp32 logits of five kinds (see KINDS)
  embeddings .... the fp32 embeddings behind the `peaked` kinds (the GPU tests feed them to crw_affinity_fwd)
  stats_fp64 .... the four softmax statistics of A in float64, cast to fp32, in crw_affinity_fwd's [4,B,T-1,N] layout
  walk_fp64_torch the prefix form of `oracle.walk_loss_torch` started from A instead of the embeddings, differentiated by
                  autograd in float64 on A's device: (loss, At, dA)
  dA_fp64 ....... `oracle.walk_backward` on float64 A (numpy in) / the autograd version (torch tensor in, any device)
  dA_rounded .... the same formulas in float64 with a rounding q on every matrix the bf16 chains keep only as bf16 images
                  -- the arithmetic's inherent error, from the reference and the number format, never from a kernel --
                  and, for the tests of the bars themselves, one planted defect
  const_closed_form  loss and dA of constant logits
  slice_report .. per (b, t): max|got - ref| / max|ref|
  audit ......... the slices that miss the entrywise bound |got - ref| <= bar[b,t] * max|ref[b,t]|
  global_bar_misses  the same question put to the bar the suite had before (one scale for the whole tensor)

numpy arrays and torch tensors are both accepted where it says so; reports are numpy.
"""
import numpy as np

from oracle import crw_oracle as orc

KINDS = ("randn3", "peaked", "peaked01", "shift", "const")
PEAKED_C = 32
PEAKED_TAU = {"peaked": 0.05, "peaked01": 0.01}

# planted defects `dA_rounded(defect=...)` / `plant` know (test_walk_routes.py::test_planted_defects)
LO_FAMILIES = ("F", "Gt", "Lt", "R", "dAt", "dLt", "dR")
FORMULA_DEFECTS = ("coldot_over_rows", "dGt0_omitted", "gloss_ignored")
RESULT_DEFECTS = ("edge_column_zeroed", "slices_swapped", "last_slice_nonzero")


# ---------------------------------------------------------------------------------------------- the routes and their cases
# (route, chains, [(B, T, N), ...], kinds).  The route is decided by the chain arithmetic and the padded node count Np
# (fp32 chain: walk.hip `small` = Np <= 64 -> the persistent LDS kernel, else the grouped fp32 GEMMs; bf16 chains: 128-tiles, or
# 256-tiles when the batch fills the chip, `big` in launch_gemm_group_bf16), and by N % 4 / the address of A (vector or scalar
# softmax kernels).  T = 3 is K = 1: no recurrence and no dGt / dF product.
ROUTE_TABLE = (
    ("persistent", (0,), ((3, 4, 1), (2, 3, 5), (2, 7, 31), (1, 5, 32), (2, 7, 33), (1, 4, 63), (1, 4, 64)), ("randn3", "shift")),
    ("persistent", (0,), ((2, 7, 31), (1, 5, 32), (2, 7, 33), (1, 4, 63), (1, 4, 64)), ("peaked",)),
    ("gemm_f32", (0,), ((2, 5, 65), (1, 3, 96), (1, 4, 97), (1, 4, 128), (1, 6, 130), (1, 4, 132), (1, 9, 257)), ("randn3", "peaked")),
    ("gemm_f32", (0,), ((1, 6, 130),), ("peaked01",)),
    ("bf16_128", (1, 2), ((2, 3, 5), (2, 7, 33), (1, 3, 96), (1, 4, 127), (1, 4, 128), (2, 5, 129), (1, 9, 250)), ("randn3", "peaked")),
    ("bf16_256", (1, 2), ((8, 10, 500),), ("peaked",)),
)
# the library's names (include/crw_hip_routes.h) for the rows' routes: what a case of the row must take,
# and what it must not
ROUTE_NAMES = {
    "persistent": (("walk.fwd_persistent", "walk.bwd_persistent"), ("walk.fwd_gemm", "walk.bwd_gemm", "gemm_bf16.t128", "gemm_bf16.t256_stagger")),
    "gemm_f32": (("walk.fwd_gemm", "walk.bwd_gemm"), ("walk.fwd_persistent", "walk.bwd_persistent", "gemm_bf16.t128", "gemm_bf16.t256_stagger")),
    "bf16_128": (("walk.fwd_gemm", "walk.bwd_gemm", "gemm_bf16.t128"), ("walk.fwd_persistent", "gemm_bf16.t256_stagger", "gemm_f32.t32", "gemm_f32.t64", "gemm_f32.t128")),
    # (the chain steps of the one large case are 2 x 2 x 8 x 2 = 64 tiles of 256: they stay on 128-tiles; its batched products fill the chip)
    "bf16_256": (("walk.fwd_gemm", "walk.bwd_gemm", "gemm_bf16.t256_stagger"), ("walk.fwd_persistent", "gemm_f32.t32", "gemm_f32.t64", "gemm_f32.t128")),
}
CHAIN_MODE = {0: "none", 1: "bf16", 2: "bf16x3"}
GLOSS = 0.7
# peaked cases whose default seed misses the admission condition of test_walk_routes.py (the fp32 oracle itself is then no
# better than 1e-4 of some slice): another seed, never another bar
_SEED = {("peaked", 2, 3, 5): 38, ("peaked", 2, 7, 31): 19}


def case_seed(kind, B, T, N):
    base = "peaked" if kind == "peaked01" else ("randn3" if kind == "shift" else kind)
    return _SEED.get((base, B, T, N), 1000 * B + 10 * N + T)


def route_cases(with_chain=True):
    """Every (route, chain, kind, B, T, N) of ROUTE_TABLE; without the chain: the distinct (kind, B, T, N)."""
    out = []
    for route, chains, shapes, kinds in ROUTE_TABLE:
        for chain in chains:
            for kind in kinds:
                for B, T, N in shapes:
                    item = (route, chain, kind, B, T, N) if with_chain else (kind, B, T, N)
                    if item not in out:
                        out.append(item)
    return out


def per_slice(kind):
    """peaked01 slices vanish to 1e-17 of the largest and fp32 cannot follow them: those cases are judged on the tensor's
    maximum (the bar the suite had before) and are in the table for the forward and the zero structure."""
    return kind != "peaked01"


# ---------------------------------------------------------------------------------------------- inputs
def embeddings(B, T, N, seed, C=PEAKED_C):
    """fp32 embeddings [B,T,N,C]: one base per node shared by every frame and item + half as much noise (peaked transitions)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((1, 1, N, C))
    return (base + 0.5 * rng.standard_normal((B, T, N, C))).astype(np.float32)


def inputs(kind, B, T, N, seed, c=None):
    """fp32 logits A [B,T-1,N,N].
      randn3 .... 3 * randn
      peaked .... oracle.affinity(l2_normalize(embeddings), tau = 0.05), C = 32
      peaked01 .. the same at tau = 0.01: logits to +-100, softmax rows with exact zeros
      shift ..... randn3 + 1000 (both softmaxes are invariant to it; one ulp of the logits is then 6e-5)
      const ..... every logit `c`"""
    if kind == "randn3" or kind == "shift":
        A = 3.0 * np.random.default_rng(seed).standard_normal((B, T - 1, N, N))
        return (A.astype(np.float32) + np.float32(1000.0 if kind == "shift" else 0.0)).astype(np.float32)
    if kind in PEAKED_TAU:
        eh = orc.l2_normalize(embeddings(B, T, N, seed), np.float64)
        return orc.affinity(eh, PEAKED_TAU[kind]).astype(np.float32)
    if kind == "const":
        return np.full((B, T - 1, N, N), c, np.float32)
    raise ValueError(kind)


def stats_fp64(A):
    """Row max / row sum exp / column max / column sum exp of every A[b,t] in float64 -> fp32 [4,B,T-1,N]."""
    A = np.asarray(A, np.float64)
    rmax, cmax = A.max(-1), A.max(-2)
    rsum = np.exp(A - rmax[..., None]).sum(-1)
    csum = np.exp(A - cmax[..., None, :]).sum(-2)
    return np.stack([rmax, rsum, cmax, csum]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- fp64 references
def walk_fp64_torch(A, gloss=1.0):
    """A: torch tensor [B,T-1,N,N] on any device -> (loss float, At [B,T-2,N,N] float64, dA float64), the recurrences of
    `oracle.walk_loss_torch` (its lines after the affinity) on float64 A, the gradient by autograd."""
    import torch
    A = A.detach().double().requires_grad_(True)
    B, Tm1, N, _ = A.shape
    T = Tm1 + 1
    if T < 3:
        return 0.0, A.new_zeros((B, 0, N, N)), torch.zeros_like(A)
    F = torch.softmax(A, -1)
    Gt = torch.softmax(A, -2)
    eye = torch.eye(N, dtype=A.dtype, device=A.device)
    loss = A.new_zeros(())
    Lt = R = None
    Ats = []
    for k in range(1, T - 1):
        if k == 1:
            Lt, R = Gt[:, 0], eye.expand(B, N, N)
        else:
            Lt, R = Gt[:, k - 1] @ Lt, F[:, k - 1] @ R
        At = Lt.transpose(1, 2) @ R
        Ats.append(At.detach())
        lse = torch.logsumexp(At, -1)
        loss = loss - (torch.diagonal(At, dim1=1, dim2=2) - lse).sum() / (B * N)
    loss = loss / N
    (loss * gloss).backward()
    return loss.item(), torch.stack(Ats, 1), A.grad


def dA_fp64(A, gloss=1.0):
    """numpy A -> `oracle.walk_backward` on float64 (numpy out); torch A -> autograd on A's device (torch out)."""
    if _is_torch(A):
        return walk_fp64_torch(A, gloss)[2]
    return orc.walk_backward(np.asarray(A, np.float64), gloss)


def const_closed_form(B, T, N, gloss=1.0):
    """Constant logits: F = Gt = 1/N, every Lt_k, R_k (k > 1) and At_k is 1/N, so loss = (T-2) ln N / N; dAt_k has zero row
    sums, which kills every term except dGt_0 = dLt_1 = R_1 dAt_1^T = coef (1/N - I): dA[:,0] = gloss / (B N^3) (1/N - I),
    every other slice 0."""
    dA = np.zeros((B, T - 1, N, N))
    if T >= 3:
        dA[:, 0] = gloss / (B * N ** 3) * (1.0 / N - np.eye(N))
    return (T - 2) * np.log(N) / N if T >= 3 else 0.0, dA


# ---------------------------------------------------------------------------------------------- bf16 image emulation
def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _bf16(x):
    """float64 -> nearest-even bf16 of its fp32 value -> float64"""
    if _is_torch(x):
        return x.float().bfloat16().double()
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def _f32(x):
    return x.float().double() if _is_torch(x) else np.asarray(x, np.float32).astype(np.float64)


def rounding(mode):
    """q of `dA_rounded`: 'none' identity; 'bf16' one image; 'bf16x3' hi + lo images (x32 = the fp32 value the kernel rounds)."""
    if mode == "none":
        return lambda x: x
    if mode == "bf16":
        return _bf16
    if mode == "bf16x3":
        def q(x):
            hi = _bf16(x)
            return hi + _bf16(_f32(x) - hi)
        return q
    raise ValueError(mode)


def _exp(x):
    return x.exp() if _is_torch(x) else np.exp(x)


def _softmax(x, axis):  # oracle._softmax, for either array type
    if _is_torch(x):
        m = x.amax(axis, keepdim=True)
        e = (x - m).exp()
        return e / e.sum(axis, keepdim=True)
    return orc._softmax(x, axis)


def _sum(x, axis):
    return x.sum(axis, keepdim=True) if _is_torch(x) else x.sum(axis, keepdims=True)


def _t(x):
    return x.transpose(1, 2) if _is_torch(x) else x.transpose(0, 2, 1)


def _eye(N, like):
    if _is_torch(like):
        import torch
        return torch.eye(N, dtype=like.dtype, device=like.device)
    return np.eye(N, dtype=like.dtype)


def dA_rounded(A, gloss=1.0, mode="none", defect=None):
    """`oracle.walk_prefix_form` + `oracle.walk_backward`, statement for statement, in float64 (numpy or torch A), with the
    rounding q(mode) applied to every matrix the bf16 chains keep only as bf16 images (walk.hip: layout_state /
    layout_scratch): F and Gt as chain operands, every Lt_k and R_k after its product, dAt, and dLt / dR where they are GEMM
    operands (their fp32 planes accumulate unrounded; dGt_0 = dLt_1 copies the fp32 plane).  At_k, dF, dGt are fp32 planes only
    and the softmax backward recomputes F / Gt from A: not rounded.  mode 'none' reproduces `oracle.walk_backward` bit for bit.

    defect: None, 'lo_dropped:<family>' (family in LO_FAMILIES: that family's images are plain bf16 whatever the mode), or
    one of FORMULA_DEFECTS."""
    if not _is_torch(A):
        A = np.asarray(A, np.float64)
    else:
        A = A.double()
    q = rounding(mode)
    dropped = defect[len("lo_dropped:"):] if defect and defect.startswith("lo_dropped:") else None
    if dropped is not None and dropped not in LO_FAMILIES:
        raise ValueError(defect)
    if defect is not None and dropped is None and defect not in FORMULA_DEFECTS:
        raise ValueError(defect)
    qf = {fam: (_bf16 if fam == dropped else q) for fam in LO_FAMILIES}
    if defect == "gloss_ignored":
        gloss = 1.0

    B, Tm1, N, _ = A.shape
    T = Tm1 + 1
    K = T - 2
    if K < 1:
        return A * 0
    F, Gt = _softmax(A, -1), _softmax(A, -2)
    Fq, Gtq = qf["F"](F), qf["Gt"](Gt)
    eye = _eye(N, A)
    Lt, R, Ats = [], [], []
    for k in range(1, T - 1):
        if k == 1:
            Lt.append(Gtq[:, 0] + 0)          # Lt_1 = Gt_0: the images are copied
            R.append(eye.expand(B, N, N) + 0 if _is_torch(A) else np.broadcast_to(eye, (B, N, N)).copy())
        else:
            Lt.append(qf["Lt"](Gtq[:, k - 1] @ Lt[-1]))
            R.append(qf["R"](Fq[:, k - 1] @ R[-1]))
        Ats.append(_t(Lt[-1]) @ R[-1])

    dF, dGt = A * 0, A * 0
    coef = gloss / (N * B * N)
    dLt_next = dR_next = None
    for k in range(K, 0, -1):
        dAt = qf["dAt"](coef * (_softmax(Ats[k - 1], -1) - eye))
        dLt = R[k - 1] @ _t(dAt)
        dR = Lt[k - 1] @ dAt
        if k < K:
            dLt_op, dR_op = qf["dLt"](dLt_next), qf["dR"](dR_next)
            dLt = dLt + _t(Gtq[:, k]) @ dLt_op
            dGt[:, k] = dLt_op @ _t(Lt[k - 1])
            dR = dR + _t(Fq[:, k]) @ dR_op
            dF[:, k] = dR_op @ _t(R[k - 1])
        dLt_next, dR_next = dLt, dR
    if defect != "dGt0_omitted":
        dGt[:, 0] = dLt_next
    cdot = _sum(dGt * Gt, -1) if defect == "coldot_over_rows" else _sum(dGt * Gt, -2)
    return F * (dF - _sum(dF * F, -1)) + Gt * (dGt - cdot)


def plant(dA, defect):
    """A defect of RESULT_DEFECTS planted into a copy of a (numpy, float64) result:
      edge_column_zeroed .. column N-1 (the padded edge) of the last slice that enters the loss, item 0
      slices_swapped ...... the adjacent pair (t, t+1) of non-zero slices with the smallest larger maximum, every item
      last_slice_nonzero .. one entry of dA[:, -1], which never enters the loss, at 1e-3 of the smallest non-zero slice"""
    out = np.array(dA, np.float64)
    B, Tm1, N, _ = out.shape
    scale = np.abs(out).max((-1, -2))                   # [B, T-1]
    live = Tm1 - 1                                       # slices 0 .. T-3 enter the loss
    if defect == "edge_column_zeroed":
        out[0, live - 1, :, N - 1] = 0
    elif defect == "slices_swapped":
        if live < 2:
            raise ValueError("needs two slices that enter the loss (T >= 4)")
        pair = np.maximum(scale[:, :live - 1], scale[:, 1:live]).max(0)
        t = int(pair.argmin())
        out[:, [t, t + 1]] = out[:, [t + 1, t]]
    elif defect == "last_slice_nonzero":
        out[0, -1, N // 2, 0] = 1e-3 * scale[:, :live][scale[:, :live] > 0].min()
    else:
        raise ValueError(defect)
    return out


# ---------------------------------------------------------------------------------------------- reports
def as_f64(x, dev=None):
    import torch
    if torch.is_tensor(x):
        return x.detach().double() if dev is None else x.detach().to(dev, torch.float64)
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))
    return t if dev is None else t.to(dev)


def _pair(got, ref):
    import torch
    dev = got.device if torch.is_tensor(got) else (ref.device if torch.is_tensor(ref) else None)
    g, r = as_f64(got, dev), as_f64(ref, dev)
    if g.shape != r.shape or g.dim() != 4:
        raise ValueError((tuple(g.shape), tuple(r.shape)))
    return g, r


def slice_report(got, ref):
    """Per (b, t): ratio = max|got - ref| / max|ref| of that slice.  Slices whose reference is identically zero are reported
    apart: ratio is 0 there, `zero_ref` marks them and `zero_bad` those of them where `got` is not all zeros (NaN included).
    -> dict(ratio [B,T-1], scale [B,T-1] = max|ref|, zero_ref, zero_bad), numpy."""
    g, r = _pair(got, ref)
    scale = r.abs().amax((-1, -2))
    err = (g - r).abs().amax((-1, -2))
    err = err.masked_fill(~((g - r).abs() >= 0).all(-1).all(-1), float("inf"))      # a NaN anywhere in the slice
    zero_ref = scale == 0
    ratio = (err / scale.masked_fill(zero_ref, 1.0)).masked_fill(zero_ref, 0.0)
    zero_bad = zero_ref & ~(g == 0).all(-1).all(-1)
    return dict(ratio=ratio.cpu().numpy(), scale=scale.cpu().numpy(), zero_ref=zero_ref.cpu().numpy(),
                zero_bad=zero_bad.cpu().numpy())


def audit(got, ref, bar):
    """The slices of `got` that miss the entrywise bound |got - ref| <= bar[b,t] * max|ref[b,t]| (bar: a number or [B,T-1]);
    where the reference slice is identically zero, `got` must be all zeros.  -> list of dict(b, t, index=(row, col) of the worst
    entry, got, ref, err, bound, ratio = err / max|ref[b,t]|, bar), empty when everything holds.  A NaN is an offence."""
    import torch
    g, r = _pair(got, ref)
    B, Tm1, N, _ = r.shape
    bar_t = torch.as_tensor(np.broadcast_to(np.asarray(bar, np.float64), (B, Tm1)).copy(), device=r.device)
    scale = r.abs().amax((-1, -2))
    bound = bar_t * scale
    err = (g - r).abs()
    err = torch.where(err >= 0, err, torch.full_like(err, float("inf")))            # NaN -> inf
    bad = ~(err <= bound[..., None, None])
    out = []
    for b, t in bad.any(-1).any(-1).nonzero().tolist():
        flat = int(err[b, t].argmax())
        i, j = divmod(flat, N)
        sc = float(scale[b, t])
        out.append(dict(b=b, t=t, index=(i, j), got=float(g[b, t, i, j]), ref=float(r[b, t, i, j]), err=float(err[b, t, i, j]),
                        bound=float(bound[b, t]), ratio=float(err[b, t, i, j]) / sc if sc > 0 else float("inf"),
                        bar=float(bar_t[b, t])))
    return out


def global_bar_misses(got, ref, rtol=1e-3, afrac=1e-4):
    """The bar of test_walk_backward_dA_matches_oracle: |got - ref| <= rtol |ref| + afrac max|ref| with ONE maximum for the
    whole tensor.  -> number of entries that miss it (0 = that bar lets `got` through)."""
    g, r = _pair(got, ref)
    return int((~((g - r).abs() <= rtol * r.abs() + afrac * r.abs().max())).sum())
