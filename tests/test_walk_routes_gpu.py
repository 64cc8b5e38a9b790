"""The walk's dA (crw_walk_fwd / crw_walk_bwd) slice by slice against float64 on every chain route, the batch split of
walk.hip:launch_group, and whether any walk kernel reads workspace it did not write.

References, bars and the case table: tests/walk_ref.py; their CPU proof (admission of every case, the emulated rounding
errors E, planted defects): tests/test_walk_routes.py.  Per-slice bars, as fractions of max|dA_ref[b,t]|:
    fp32 chain 1e-3;   bf16x3 chain 1e-3 + 4 E_x3[b,t];   bf16 chain 1e-3 + 4 E_bf16[b,t]
E is computed here from the reference (the formulas in float64 with the chain's bf16 images emulated), never from the kernel.
At and the loss keep the tolerances the suite already had for them (test_hip_parity.py)."""
import ctypes

import numpy as np
import pytest
import torch

import walk_ref as wr
from oracle import crw_oracle as orc

pytestmark = pytest.mark.gpu

# (At rtol, At atol, |loss - fp64|) per chain arithmetic: the tolerances of test_hip_parity.py
FWD_TOL = {0: (1e-4, 1e-6, 1e-4), 2: (2e-4, 2e-6, 1e-4), 1: (3e-2, 2e-3, 5e-3)}
GPU_REF_FROM = 256      # node count from which the float64 reference is evaluated on the device


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    return crw_hip


def _gloss(v=wr.GLOSS):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def _walk(hip, A, chain, stats, gloss=None):
    loss, state, At = hip.walk_fwd(A, chain=chain, want_At=True, stats=stats)
    dA = hip.walk_bwd(_gloss() if gloss is None else gloss, A, state, chain=chain)
    torch.cuda.synchronize()
    return loss.item(), At, dA


_REFS = {}


def _reference(hip, kind, B, T, N):
    """Logits on the device, the statistics to import, and the float64 loss / At / dA of those very logits -- once per case.
    `peaked` logits come from embeddings: they are crw_affinity_fwd's own output (held to the host logits first) and the
    imported statistics are the ones its epilogue delivers; otherwise the statistics are float64 ones cast to fp32."""
    key = (kind, B, T, N)
    if key in _REFS:
        return _REFS[key]
    seed = wr.case_seed(kind, B, T, N)
    A_host = wr.inputs(kind, B, T, N, seed)
    if kind in wr.PEAKED_TAU:
        emb = torch.from_numpy(wr.embeddings(B, T, N, seed)).cuda()
        A, _, _, stats = hip.affinity_fwd(emb, wr.PEAKED_TAU[kind])
        torch.cuda.synchronize()
        np.testing.assert_allclose(A.cpu().numpy(), A_host, rtol=1e-4, atol=1e-4)
        A_host = A.cpu().numpy()
    else:
        A = torch.from_numpy(A_host).cuda()
        stats = torch.from_numpy(wr.stats_fp64(A_host)).cuda()
    if N >= GPU_REF_FROM:
        loss, At, dA = wr.walk_fp64_torch(A, wr.GLOSS)
        src = A
    else:
        loss, At = orc.walk_prefix_form(A_host.astype(np.float64))
        dA = wr.dA_fp64(A_host, wr.GLOSS)
        src = A_host
        if wr.per_slice(kind) and kind in wr.PEAKED_TAU:  # the device's own logits, not the host's: admission again
            adm = wr.slice_report(orc.walk_backward(A_host, np.float32(wr.GLOSS)), dA)["ratio"].max()
            assert adm <= 1e-4, ("not admissible per slice", adm)
    _REFS[key] = dict(A=A, stats=stats, loss=float(loss), At=At, dA=dA, src=src, E={})
    return _REFS[key]


def _bar(ref, chain):
    """[B,T-1] per-slice bar of the chain; E from the reference's own emulation, cached per case"""
    if chain == 0:
        return 1e-3, 0.0
    mode = wr.CHAIN_MODE[chain]
    if mode not in ref["E"]:
        ref["E"][mode] = wr.slice_report(wr.dA_rounded(ref["src"], wr.GLOSS, mode), ref["dA"])["ratio"]
    return 1e-3 + 4 * ref["E"][mode], float(ref["E"][mode].max())


def _check_forward(chain, loss, At, ref):
    rtol, atol, ltol = FWD_TOL[chain]
    At_ref = wr.as_f64(ref["At"], At.device)
    err = (At.double() - At_ref).abs()
    worst = float((err - rtol * At_ref.abs()).max()) if err.numel() else 0.0
    assert worst <= atol, ("At", worst, atol)
    assert abs(loss - ref["loss"]) <= ltol, (loss, ref["loss"])


def _check_dA(tag, chain, kind, dA, ref):
    """dA through `audit` at the chain's per-slice bar (peaked01: the tensor-wide bar, see walk_ref.per_slice); dA[:, -1] all
    zeros.  -> worst slice ratio"""
    assert torch.count_nonzero(dA[:, -1]).item() == 0, "A_{T-2} never enters the loss"
    rep = wr.slice_report(dA, ref["dA"])
    assert not rep["zero_bad"].any()
    bar, Emax = _bar(ref, chain)
    if wr.per_slice(kind):
        bad = wr.audit(dA, ref["dA"], bar)
        what = f"worst slice ratio {rep['ratio'].max():.3e} (bar 1e-3 + 4 E, max E {Emax:.2e})"
    else:
        assert chain == 0                                             # rtol 1e-3, atol 1e-4 max|dA| is the fp32 chain's bar
        bad = wr.global_bar_misses(dA, ref["dA"], rtol=1e-3, afrac=1e-4)
        live = ~rep["zero_ref"]
        what = (f"tensor-wide bar; worst slice ratio {rep['ratio'].max():.3e}, slice maxima "
                f"{rep['scale'][live].min():.1e} .. {rep['scale'].max():.1e}")
    print(f"{tag}: {what}")
    assert not bad, (tag, bad[:4] if isinstance(bad, list) else bad)
    return float(rep["ratio"].max())


@pytest.mark.parametrize("route,chain,kind,B,T,N", wr.route_cases())
def test_walk_dA_per_slice(hip, route, chain, kind, B, T, N):
    """Every case of walk_ref.ROUTE_TABLE, with the walk's own statistics and with imported ones: At and the loss against
    float64 at the tolerances the suite had, dA through `audit` at the per-slice bar of the chain, dA[:, -1] all zeros.  Both
    runs must pass the same bar.  The T = 3 rows are K = 1: no recurrence, no dGt / dF product."""
    ref = _reference(hip, kind, B, T, N)
    must, must_not = wr.ROUTE_NAMES[route]
    for name, stats in (("own statistics", None), ("imported statistics", ref["stats"])):
        with hip.routes() as hit:
            loss, At, dA = _walk(hip, ref["A"], chain, stats)
        # the case runs the route its row is named for (the library's own account, not the shape's promise)
        assert set(must) <= set(hit) and not set(must_not) & set(hit), (route, sorted(hit))
        assert ("softmax.stats_import" in hit) == (stats is not None), sorted(hit)
        _check_forward(chain, loss, At, ref)
        _check_dA(f"{route} chain {chain} {kind} {(B, T, N)} {name}", chain, kind, dA, ref)
    if route == "bf16_256" and chain == 2:
        del _REFS[(kind, B, T, N)]                                    # (the last user of the one large reference)


@pytest.mark.parametrize("B,T,N", [(1, 4, 64), (1, 4, 128)])
def test_walk_dA_logits_not_16_byte_aligned(hip, B, T, N):
    """N % 4 == 0 but A starts one float into its buffer: `vec` is false by address, so the scalar softmax kernels run at a
    node count that otherwise always takes the vector ones (persistent kernel at 64, fp32 GEMMs at 128)."""
    ref = _reference(hip, "randn3", B, T, N)
    n = ref["A"].numel()
    buf = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    A = buf[1:1 + n].view(B, T - 1, N, N)
    A.copy_(ref["A"])
    assert A.is_contiguous() and A.data_ptr() % 16 == 4 and ref["A"].data_ptr() % 16 == 0
    for name, stats in (("own statistics", None), ("imported statistics", ref["stats"])):
        with hip.routes() as hit:
            loss, At, dA = _walk(hip, A, 0, stats)
        assert {"softmax.fwd_scalar", "softmax.bwd_scalar"} <= set(hit) and not {"softmax.fwd_vec", "softmax.bwd_vec"} & set(hit), sorted(hit)
        assert ("walk.fwd_persistent" in hit) == (N == 64) and ("walk.fwd_gemm" in hit) == (N == 128), sorted(hit)
        _check_forward(0, loss, At, ref)
        _check_dA(f"unaligned logits {(B, T, N)} {name}", 0, "randn3", dA, ref)


@pytest.mark.parametrize("chain,B,T,N", [(0, 2, 5, 33), (1, 2, 5, 129), (2, 2, 5, 129)])
def test_walk_gloss_zero(hip, chain, B, T, N):
    """gloss = 0: dA is all zeros, none NaN (0 * the softmaxes, not 0 * something unwritten)."""
    A = torch.from_numpy(wr.inputs("randn3", B, T, N, 7)).cuda()
    _, _, dA = _walk(hip, A, chain, None, gloss=_gloss(0.0))
    assert not torch.isnan(dA).any() and torch.count_nonzero(dA).item() == 0


@pytest.mark.parametrize("B,T,N", [(2, 5, 7), (1, 3, 33), (1, 4, 130)])
@pytest.mark.parametrize("c", [3.25, -100.0, 1000.0])
def test_walk_const_logits_closed_form(hip, B, T, N, c):
    """Constant logits (walk_ref.const_closed_form): loss = (T-2) ln N / N to 1e-6 relative; dA[:,0] = gloss / (B N^3) (1/N - I)
    at the fp32 per-slice bar.  Every other slice has a zero reference, where `audit` would demand exact zeros; fp32 leaves
    rounding residue of the terms that cancel there, so those slices are bounded by the fp32 bar times max|dA[:,0]| instead --
    except dA[:, -1], which no term reaches and which stays exactly zero."""
    A = torch.from_numpy(wr.inputs("const", B, T, N, 0, c=c)).cuda()
    loss_ref, dA_ref = wr.const_closed_form(B, T, N, wr.GLOSS)
    for name, stats in (("own statistics", None), ("imported statistics", torch.from_numpy(wr.stats_fp64(A.cpu().numpy())).cuda())):
        loss, _, dA = _walk(hip, A, 0, stats)
        print(f"const {c} {(B, T, N)} {name}: loss rel {abs(loss - loss_ref) / loss_ref:.2e}, slice 0 ratio "
              f"{wr.slice_report(dA[:, :1], dA_ref[:, :1])['ratio'].max():.2e}, other slices / max|dA[:,0]| "
              f"{(dA[:, 1:].abs().max().item() if T > 3 else 0.0) / np.abs(dA_ref[:, 0]).max():.2e}")
        assert abs(loss - loss_ref) <= 1e-6 * loss_ref
        assert not wr.audit(dA[:, :1], dA_ref[:, :1], 1e-3)
        assert torch.count_nonzero(dA[:, -1]).item() == 0
        rest = dA[:, 1:].double().abs()
        assert bool((rest <= 1e-3 * np.abs(dA_ref[:, 0]).max()).all())


# ------------------------------------------------------------------------------------------------ batch split
SPLIT_B, SPLIT_T, SPLIT_N = 10923, 5, 5                 # K * B = 3 * 10923 = 32769 = MAXB + 1


def _split_case(hip, chain):
    """K * B = 32769 batched products: walk.hip:launch_group issues 32768 and then 1, with every operand image and result
    pointer advanced by hand.  Batch index k * B + b: the split falls between (k = 2, b = 10921) and (k = 2, b = 10922), the
    last cycle product of the last two items.  The float64 reference runs on the device."""
    B, T, N = SPLIT_B, SPLIT_T, SPLIT_N
    lib = hip.lib()
    assert (T - 2) * B == 32768 + 1
    need = lib.crw_walk_state_bytes(B, T, N, chain) + lib.crw_walk_scratch_bytes(B, T, N, chain)
    A = torch.from_numpy(wr.inputs("randn3", B, T, N, 32769)).cuda()
    loss_ref, At_ref, dA_ref = wr.walk_fp64_torch(A, wr.GLOSS)
    ref = dict(loss=loss_ref, At=At_ref, dA=dA_ref, src=A, E={})
    loss, At, dA = _walk(hip, A, chain, None)
    _check_forward(chain, loss, At, ref)
    rep = wr.slice_report(dA, dA_ref)
    bar, Emax = _bar(ref, chain)
    looked = (0, 10921, 10922)                          # first item, and the two items either side of the split (10922 = last)
    rtol, atol, _ = FWD_TOL[chain]
    for b in looked:
        e = (At[b].double() - At_ref[b]).abs()
        assert float((e - rtol * At_ref[b].abs()).max()) <= atol, ("At", b)
        assert not wr.audit(dA[b:b + 1], dA_ref[b:b + 1], bar if chain == 0 else bar[b:b + 1]), ("dA", b)
    print(f"batch split chain {chain}: {need / 2 ** 30:.2f} GiB of state + scratch; per-slice ratios of b = 0 / 10921 / 10922: "
          + " / ".join(f"{rep['ratio'][b].max():.2e}" for b in looked) + f"; worst of all {B} items {rep['ratio'].max():.2e} "
          f"(max E {Emax:.2e})")
    bad = wr.audit(dA, dA_ref, bar)                     # and every other item
    assert not bad, bad[:4]
    assert torch.count_nonzero(dA[:, -1]).item() == 0


def test_walk_batch_split_f32(hip):
    """Chain 0, Np = 32: about 1.5 GiB of state + scratch."""
    _split_case(hip, 0)


def test_walk_batch_split_bf16(hip):
    """Chain 1, Np = 128: about 20 GB of state + scratch, so only where 40 GB are free."""
    free = torch.cuda.mem_get_info()[0]
    if free < 40e9:
        pytest.skip(f"needs 40 GB of free device memory for about 20 GB of workspace ({free / 1e9:.0f} GB free)")
    _split_case(hip, 1)


# ------------------------------------------------------------------------------------------------ stale workspace
def _filled(nbytes, byte):
    t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    return t.fill_(byte)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _raw_run(hip, emb, tau, chain, imported, byte):
    """crw_affinity_fwd -> crw_walk_fwd -> crw_walk_bwd through the C ABI with this test's own buffers: ws, state and scratch
    are exactly as long as the library asks and filled with `byte`, and so is every output, so that a part nobody writes shows
    too.  -> dict of the outputs as byte tensors."""
    lib = hip.lib()
    B, T, N, C = emb.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nws = lib.crw_affinity_ws_bytes(B, T, N)
    nstate, nscratch = lib.crw_walk_state_bytes(B, T, N, chain), lib.crw_walk_scratch_bytes(B, T, N, chain)
    ws, state, scratch = _filled(nws, byte), _filled(nstate, byte), _filled(nscratch, byte)
    f = 4
    out = dict(ehat=_filled(emb.numel() * f, byte), norm=_filled(B * T * N * f, byte), A=_filled(B * (T - 1) * N * N * f, byte),
               stats=_filled(4 * B * (T - 1) * N * f, byte), At=_filled(B * (T - 2) * N * N * f, byte), loss=_filled(f, byte),
               dA=_filled(B * (T - 1) * N * N * f, byte))
    g = _gloss()
    st = lib.crw_affinity_fwd(_p(emb), B, T, N, C, float(tau), _p(out["ehat"]), _p(out["norm"]), _p(out["A"]), _p(out["stats"]),
                              _p(ws), nws, stream)
    assert st == 0, ("crw_affinity_fwd", st)
    st = lib.crw_walk_fwd(_p(out["A"]), _p(out["stats"]) if imported else None, B, T, N, chain, _p(state), nstate, _p(out["At"]),
                          _p(out["loss"]), stream)
    assert st == 0, ("crw_walk_fwd", st)
    st = lib.crw_walk_bwd(_p(g), _p(out["A"]), B, T, N, chain, _p(state), nstate, _p(scratch), nscratch, _p(out["dA"]), stream)
    assert st == 0, ("crw_walk_bwd", st)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("imported", [False, True], ids=["own", "imported"])
@pytest.mark.parametrize("chain,B,T,N", [(0, 2, 5, 5), (0, 2, 5, 33), (0, 1, 4, 130), (1, 2, 5, 129), (2, 2, 5, 129)])
def test_walk_ignores_stale_workspace(hip, chain, B, T, N, imported):
    """Forward + backward once with ws / state / scratch filled with byte 0xFF (NaN as fp32 and as bf16) and once with 0x00:
    A, stats, loss, At and dA are finite and bit-identical between the two, i.e. no kernel consumes memory it did not write
    (state and scratch come from torch.empty in crw_hip; softmax.hip loads statistics quads and dF / dGt quads that reach past
    N and relies on its guards and on exact zeros in the padding).  The buffers have exactly the byte counts the library asks
    for, at the allocator's (256-byte aligned) addresses: this checks what is read, not where."""
    emb = torch.from_numpy(wr.embeddings(B, T, N, 77 + N)).cuda()
    runs = [_raw_run(hip, emb, 0.05, chain, imported, byte) for byte in (0xFF, 0x00)]
    for name in ("ehat", "norm", "A", "stats", "loss", "At", "dA"):
        a, b = runs[0][name], runs[1][name]
        assert torch.isfinite(a.view(torch.float32)).all(), (name, "not finite with the workspace filled with 0xFF")
        assert torch.isfinite(b.view(torch.float32)).all(), (name, "not finite with the workspace filled with 0x00")
        assert torch.equal(a, b), (name, "depends on what the workspace held before the call")
    assert torch.count_nonzero(runs[0]["dA"].view(torch.float32).view(B, T - 1, N, N)[:, :-1]).item() > 0
