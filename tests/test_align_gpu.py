"""GPU side of aligning a memory bank to its item: the entry points of include/crw_hip_align.h through the C ABI, held to the
definitions of tests/align_ref.py (whose checkers tests/test_align.py proves on planted defects).
  * crw_center_normalize: every entry within `align_ref.center_bound` of the fp64 definition, the worst fraction
    printed; segments of unequal length, a ONE-ROW segment -- by convention the all-zero row, +0 in every channel, as F.normalize
    leaves a zero vector -- and an empty one; the offsets by value and on the device, device offsets that are out of order; the
    means bit-equal across calls and workspace contents; all-zero means give crw_normalize's bits; operands at odd addresses;
  * crw_labelprop_topk_long_bias: every slot of every list against fp64 (`align_ref.biased_lists_audit`, the checker of
    tests/test_labelprop_lists_gpu.py with its bound widened by the one rounded add) on plain and on twin frames (exact ties), on the
    vector route and on the matrix cores; a zero bias gives crw_labelprop_topk_long's bits;
  * both over stale memory and between guard bands;
  * the [30, 13] counts of tests/test_align.py through `propagate_all` and `utils.propagate`.
Nothing here provokes a fault: offsets a kernel reads from the device are clamped by the kernel, which is what the planted ones show."""
import ctypes

import numpy as np
import pytest
import torch

import align_ref as ar
import longmem_ref as lm
import sliding_ref as slr
import stale_ref as sr
from test_labelprop_lists import twin_frames

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32
EINVAL = 1
BIAS = 0.1


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_align() and crw_hip.has_long_memory() and crw_hip.has_routes()
    return crw_hip


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def eq_bits(a, b):
    return torch.equal(a.view(I32), b.view(I32))


def center(lib, emb, bounds, on_device, ws=None, ehat=None, mean=None, want=0):
    """crw_center_normalize on emb [rows, C]; bounds: a list of S + 1 offsets, given by value or as a device array"""
    rows, C = emb.shape
    S = len(bounds) - 1
    nbytes = lib.crw_center_normalize_ws_bytes(rows, C, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda") if ws is None else ws
    ehat = torch.empty_like(emb) if ehat is None else ehat
    mean = torch.empty(S, C, dtype=F64, device="cuda") if mean is None else mean
    dev = torch.tensor(bounds, dtype=I32, device="cuda") if on_device else None
    host = None if on_device else (ctypes.c_int32 * (S + 1))(*bounds)
    st = lib.crw_center_normalize(_p(emb), rows, C, _p(dev), host, S, _p(ws), ws.numel(), _p(ehat), _p(mean), _stream())
    assert st == want, ("crw_center_normalize", st)
    return ehat, mean


def topk_bias(lib, ehat, cxt, K, radius, temp, k, first, raw, route, bias, out=None, want=0):
    T, N, C = ehat.shape
    WV, I = out or (torch.empty(T - first, k, N, device="cuda"), torch.empty(T - first, k, N, device="cuda", dtype=I32))
    st = lib.crw_labelprop_topk_long_bias(_p(ehat), T, N, C, cxt, K, radius, temp, k, first, _p(WV), _p(I), raw, route, bias, _stream())
    assert st == want, ("crw_labelprop_topk_long_bias", st)
    return WV, I


def topk_long(lib, ehat, cxt, K, radius, temp, k, first, raw, route):
    T, N, C = ehat.shape
    WV, I = torch.empty(T - first, k, N, device="cuda"), torch.empty(T - first, k, N, device="cuda", dtype=I32)
    assert lib.crw_labelprop_topk_long(_p(ehat), T, N, C, cxt, K, radius, temp, k, first, _p(WV), _p(I), raw, route, _stream()) == 0
    return WV, I


def raw_features(rows, C, seed, offset=3.0):
    """rows whose common offset is larger than their spread, as a bank's and an item's are at start = 1.0"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, C)) + offset * rng.standard_normal(C)).astype(np.float32)


# ================================================================================================ crw_center_normalize
# (rows, C, offsets): the [30, 13] item behind a bank of four (442 rows; 14 slabs of 32) with a one-row segment; the [40, 24] item
# behind five with a one-row and an empty segment; 64 slabs of 33 rows, the slab bound (2 100 > 64 * 32), C = 128, a segment edge
# inside a slab and inside a workgroup's 64 rows; C = 300 > 256: two passes over the channels in launch 1, a one-row segment FIRST;
# C = 7: 32 row sub-sums per channel; one row, one segment
CENTER_CASES = [(442, 8, [0, 52, 53, 442]), (1080, 16, [0, 120, 121, 121, 1080]), (2100, 128, [0, 1000, 2100]), (333, 300, [0, 1, 333]),
                (97, 7, [0, 64, 65, 97]), (1, 5, [0, 1])]


@pytest.mark.parametrize("rows,C,bounds", CENTER_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_center_normalize_is_the_definition(hip, rows, C, bounds):
    lib = hip.lib()
    emb_np = raw_features(rows, C, rows + C)
    emb = torch.from_numpy(emb_np).cuda()
    S = len(bounds) - 1
    nbytes = lib.crw_center_normalize_ws_bytes(rows, C, S)
    outs = []
    for on_device in (False, True):
        for fill in (0xFF, 0x00):                                   # what the workspace held must not matter
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
            outs.append(center(lib, emb, bounds, on_device, ws=ws))
    ehat, mean = outs[0]
    assert all(eq_bits(e, ehat) and torch.equal(m.view(torch.int64), mean.view(torch.int64)) for e, m in outs[1:])
    v = ar.center_violations(emb_np, bounds, ehat.cpu().numpy(), mean.cpu().numpy())
    print(f"crw_center_normalize rows {rows} C {C} offsets {bounds}: worst |ehat - fp64| / bound {v['worst']:.3g}")
    assert v["outside"] == 0 and v["mean"] == 0 and v["worst"] <= 1, v
    for s, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        if hi - lo == 1:                                            # a one-row segment: the all-zero row, +0 in every channel
            assert not ehat[lo].any() and not torch.signbit(ehat[lo]).any()
            assert torch.equal(mean[s], emb[lo].double())           # ... and it is its own mean, exactly
        if hi == lo:
            assert not mean[s].any()                                # an empty segment: nothing of ehat, a zero row of mean
    # through the binding, both kinds of offsets, and in place
    via, vmean = hip.center_normalize(emb, bounds, return_mean=True)
    assert eq_bits(via, ehat) and torch.equal(vmean, mean)
    assert eq_bits(hip.center_normalize(emb.reshape(1, rows, C), torch.tensor(bounds, dtype=I32, device="cuda")).reshape(rows, C), ehat)
    inplace = emb.clone()
    center(lib, inplace, bounds, False, ehat=inplace)
    assert eq_bits(inplace, ehat)


def test_center_normalize_clamps_the_offsets_it_reads_from_the_device(hip):
    """b_0 reads as 0, b_S as rows, every other offset as min(rows, max(the one before, what the array holds))"""
    lib = hip.lib()
    rows, C = 97, 8
    emb = torch.from_numpy(raw_features(rows, C, 3)).cuda()
    want = center(lib, emb, [0, 50, 50, 97], False)
    got = center(lib, emb, [99, 50, 20, -4], True)
    assert eq_bits(got[0], want[0]) and torch.equal(got[1], want[1])
    want = center(lib, emb, [0, 97, 97, 97], False)
    got = center(lib, emb, [0, 2 ** 31 - 1, -2 ** 31, 5], True)
    assert eq_bits(got[0], want[0]) and torch.equal(got[1], want[1])


def test_center_normalize_at_odd_addresses(hip):
    """fp32 operands at 4-byte, the workspace at 1-byte alignment: the same bits as at the allocator's"""
    lib = hip.lib()
    rows, C, bounds = 130, 12, [0, 31, 130]
    emb = torch.from_numpy(raw_features(rows, C, 9)).cuda()
    want, wmean = center(lib, emb, bounds, True)
    nbytes = lib.crw_center_normalize_ws_bytes(rows, C, 2)
    for shift in (1, 3):
        src = torch.zeros(rows * C + 4, device="cuda")
        dst = torch.full((rows * C + 4,), float("nan"), device="cuda")
        src[shift:shift + rows * C] = emb.reshape(-1)
        e_in, e_out = src[shift:shift + rows * C].view(rows, C), dst[shift:shift + rows * C].view(rows, C)
        assert e_in.data_ptr() % 16 == 4 * shift
        ws = torch.full((nbytes + 8,), 0xFF, dtype=torch.uint8, device="cuda")[shift:shift + nbytes]
        got, gmean = center(lib, e_in, bounds, True, ws=ws, ehat=e_out)
        assert eq_bits(got, want) and torch.equal(gmean, wmean)
        assert torch.isnan(dst[:shift]).all() and torch.isnan(dst[shift + rows * C:]).all()


@pytest.mark.parametrize("C", (8, 16, 128, 7, 300))
def test_with_all_means_zero_the_bits_are_crw_normalize_s(hip, C):
    """every segment is [X; -X] with X on a grid of 2^-8: its fp64 sums are exact and cancel, every mean is 0, y = x"""
    lib = hip.lib()
    rng = np.random.default_rng(C)
    halves = (40, 3, 517)
    parts, bounds = [], [0]
    for h in halves:
        x = np.round(rng.standard_normal((h, C)) * 256) / 256
        parts += [x, -x]
        bounds.append(bounds[-1] + 2 * h)
    emb = torch.from_numpy(np.concatenate(parts).astype(np.float32)).cuda()
    rows = emb.shape[0]
    plain = torch.empty_like(emb)
    assert lib.crw_normalize(_p(emb), rows, C, _p(plain), None, _stream()) == 0
    for on_device in (False, True):
        ehat, mean = center(lib, emb, bounds, on_device)
        assert not mean.any()
        assert eq_bits(ehat, plain)


def test_center_normalize_argument_checks(hip):
    lib = hip.lib()
    emb = torch.zeros(10, 4, device="cuda")
    out = torch.zeros(10, 4, device="cuda")
    ws = torch.zeros(lib.crw_center_normalize_ws_bytes(10, 4, 2), dtype=torch.uint8, device="cuda")
    center(lib, emb, [0, 10], False, ws=ws[:8], ehat=out, want=2)                   # CRW_EWORKSPACE
    for bad in ([1, 10], [0, 9], [0, 7, 5, 10]):
        center(lib, emb, bad, False, ehat=out, want=EINVAL)
    assert lib.crw_center_normalize(_p(emb), 10, 4, None, None, 1, _p(ws), ws.numel(), _p(out), None, _stream()) == EINVAL
    assert lib.crw_center_normalize(_p(emb), 10, 4, None, (ctypes.c_int32 * 1)(0), 0, _p(ws), ws.numel(), _p(out), None, _stream()) == EINVAL   # S < 1
    assert not out.any()


# ================================================================================================ crw_labelprop_topk_long_bias
# (T, N, C, M, cxt, radius, temp, knn, amp), K, route: the vector route at [30, 13]; the matrix cores at [40, 24] -- they take 64, 128
# or 256 channels (C = 16 has no matrix-core form: asserted below), so the item is made with C = 64 there --; [40, 24] with its own
# C = 16 on the vector route.  first_frame = 1: the frames n <= K, K < n <= K + cxt and n > K + cxt are all in the call.
V30, M40, V40 = slr.DRIFT_SHAPES[0], (40, 24, 64, 3, 6, 4, 0.05, 5, 8), slr.DRIFT_SHAPES[1]
BIAS_CASES = [(V30, 2, 1), (V30, 5, 1), (M40, 5, 2), (V40, 5, 1)]
ROUTE_NAME = {1: "labelprop.topk_valu", 2: "labelprop.topk_mfma_chunks1"}


def bank_item(hip, shape, K):
    """the virtual item [K - 1 traces of a labelled item, an emerging target] at start = 1.0, centred and normalised by the device"""
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    ea, _ = lm.campaign_item(7, 100, T, N, C, M, 0.6 * amp, True, False, 0.5, 1.0)
    et, _ = lm.campaign_item(7, 0, T, N, C, M, amp, True, True, 0.0, 1.0)
    B = K - 1
    frames = list(np.linspace(0, T - 1, B).astype(int))
    emb = torch.from_numpy(np.concatenate([ea[frames], et])).cuda()
    return hip.center_normalize(emb, [0, B * N, (B + T) * N])


@pytest.mark.parametrize("shape,K,route", BIAS_CASES, ids=lambda v: "x".join(map(str, v[:3])) if isinstance(v, tuple) else str(v))
def test_biased_lists_against_fp64(hip, shape, K, route):
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    lib = hip.lib()
    feats = bank_item(hip, shape, K)
    F = feats.shape[0]
    assert F > K + cxt + 1
    for name, f in (("plain", feats), ("twin frames", twin_frames(feats).contiguous())):
        for bias in (BIAS, -0.05):
            with hip.routes() as hit:
                W, I = topk_bias(lib, f, cxt, K, radius, temp, knn, 1, 0, route, bias)
                V, Iv = topk_bias(lib, f, cxt, K, radius, temp, knn, 1, 1, route, bias)
            assert set(hit) == {ROUTE_NAME[route]}, hit
            assert torch.equal(I, Iv), "the scores mode selects other candidates than the weights mode"
            res = ar.biased_lists_audit(f, K, cxt, radius, temp, knn, 1, W, I, V, bias)
            print(f"{shape[:3]} K {K} route {route} bias {bias} {name}: worst error / bound "
                  + ", ".join(f"{k} {v:.3g}" for k, v in res["worst"].items()))
            assert not any(res["violations"].values()), (name, bias, res)
            assert all(v <= 1 for v in res["worst"].values()), (name, bias, res)
            if name == "twin frames":   # the tie rule is exercised: neighbouring slots with the same logit bit for bit
                full = V[:, 1:] != -float("inf")
                assert bool(((V[:, :-1] == V[:, 1:]) & full).any())
            W0, I0 = topk_long(lib, f, cxt, K, radius, temp, knn, 1, 0, route)
            assert not torch.equal(I0, I)                           # the bias is live: it changes which keys are chosen
            Wa, Ia = topk_bias(lib, f, cxt, K, radius, temp, knn, 1, 0, 0, bias)     # the route the call takes unasked
            assert torch.equal(Ia, I) and eq_bits(Wa, W)
            via = hip.labelprop_topk(f, cxt, radius, temp, knn, first_frame=1, n_long=K, route="auto", long_bias=bias)
            assert torch.equal(via[1], I) and eq_bits(via[0], W)
    if C == 16:
        topk_bias(lib, feats, cxt, K, radius, temp, knn, 1, 0, 2, BIAS, want=EINVAL)   # no matrix-core form of 16 channels


@pytest.mark.parametrize("shape,K,route", BIAS_CASES, ids=lambda v: "x".join(map(str, v[:3])) if isinstance(v, tuple) else str(v))
def test_a_zero_bias_is_topk_long_bit_for_bit(hip, shape, K, route):
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    lib = hip.lib()
    feats = bank_item(hip, shape, K)
    for first in (1, K, K + cxt + 2):
        for raw in (0, 1):
            want = topk_long(lib, feats, cxt, K, radius, temp, knn, first, raw, route)
            for zero in (0.0, -0.0):
                with hip.routes() as hit:
                    got = topk_bias(lib, feats, cxt, K, radius, temp, knn, first, raw, route, zero)
                assert set(hit) == {ROUTE_NAME[route]}, hit
                assert torch.equal(got[1], want[1]) and eq_bits(got[0], want[0]), (first, raw, zero)


def test_bias_argument_checks(hip):
    lib = hip.lib()
    T, N, C, cxt, knn = 8, 10, 8, 3, 4
    feats = hip.normalize(torch.from_numpy(raw_features(T * N, C, 1, 0.0)).cuda().view(T, N, C))
    W, I = torch.zeros(T - 2, knn, N, device="cuda"), torch.zeros(T - 2, knn, N, device="cuda", dtype=I32)
    for bad in (float("nan"), float("inf"), -float("inf")):
        topk_bias(lib, feats, cxt, 2, 3, 0.1, knn, 2, 0, 0, bad, out=(W, I), want=EINVAL)
    for K, first, route in ((0, 2, 0), (T, 2, 0), (2, 0, 0), (2, T, 0), (2, 2, 3), (2, 2, 2)):
        topk_bias(lib, feats, cxt, K, 3, 0.1, knn, first, 0, route, BIAS, out=(W, I), want=EINVAL)
    assert not W.any() and not I.any()


# ================================================================================================ stale memory and guard bands
def _out(*shape, dtype=F32):
    like = torch.empty(shape, dtype=dtype, device="meta")
    return sr.Buf(like.numel() * like.element_size(), dtype if dtype.is_floating_point else None, step=sr.largest_step(like))


def _as(t, name, dtype, *shape):
    like = torch.empty(shape, dtype=dtype, device="meta")
    return t[name][:like.numel() * like.element_size()].view(dtype).view(shape)


def banded_case(hip, home, shape, K, route, on_device):
    """both entry points on one virtual item: the raw features of a bank of K - 1 traces, a one-row segment and the item are centred
    and normalised into `ehat`, whose lists (weights and logits) are then made under the bias"""
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    lib = hip.lib()
    F = K - 1 + T
    emb_np = raw_features(F * N, C, 31)
    bounds = [0, (K - 1) * N - 1, (K - 1) * N, F * N]
    S, n = 3, F - K
    nbytes = lib.crw_center_normalize_ws_bytes(F * N, C, S)
    emb, seg = home.many(emb=torch.from_numpy(emb_np).cuda(), seg=torch.tensor(bounds, dtype=I32, device="cuda"))
    host = (ctypes.c_int32 * (S + 1))(*bounds)
    bufs = dict(ws=sr.Buf(nbytes, None, ws=True), ehat=_out(F, N, C), mean=_out(S, C, dtype=F64), Wo=_out(n, knn, N),
                Io=_out(n, knn, N, dtype=I32), Vo=sr.Buf(n * knn * N * 4, None, step=knn * N * 4), Ivo=_out(n, knn, N, dtype=I32))

    def run(_, t):
        ehat = _as(t, "ehat", F32, F, N, C)
        st = lib.crw_center_normalize(_p(emb), F * N, C, _p(seg) if on_device else None, None if on_device else host, S, _p(t["ws"]), nbytes,
                                      _p(ehat), _p(t["mean"]), _stream())
        assert st == 0, st
        for raw, (w, i) in enumerate((("Wo", "Io"), ("Vo", "Ivo"))):
            st = lib.crw_labelprop_topk_long_bias(_p(ehat), F, N, C, cxt, K, radius, temp, knn, K, _p(t[w]), _p(t[i]), raw, route, BIAS, _stream())
            assert st == 0, st
        torch.cuda.synchronize()

    case = sr.Case(f"crw_center_normalize / crw_labelprop_topk_long_bias (route {route})", None, bufs, run, device="cuda", home=home)

    def check(t):
        ehat = _as(t, "ehat", F32, F * N, C)
        v = ar.center_violations(emb_np, bounds, ehat.cpu().numpy(), _as(t, "mean", F64, S, C).cpu().numpy())
        assert v["outside"] == 0 and v["mean"] == 0, v
        assert torch.allclose(_as(t, "Wo", F32, n, knn, N).sum(1), torch.ones(n, N, device="cuda"), atol=1e-5)
        assert torch.equal(_as(t, "Io", I32, n, knn, N), _as(t, "Ivo", I32, n, knn, N))
        return ehat, _as(t, "Wo", F32, n, knn, N)
    return case, check


@pytest.mark.parametrize("shape,K,route,on_device", [(V30, 2, 1, True), (V30, 5, 1, False), (M40, 5, 2, True)],
                         ids=lambda v: "x".join(map(str, v[:3])) if isinstance(v, tuple) else str(v))
def test_entry_points_over_stale_memory_and_between_guard_bands(hip, shape, K, route, on_device):
    case, check = banded_case(hip, sr.Home("cuda"), shape, K, route, on_device)
    assert case.home.operands
    a = check(sr.run_banded(case))
    b = check(sr.run_twice(case))
    assert eq_bits(a[0], b[0]) and eq_bits(a[1], b[1])


# ================================================================================================ the tables, the host path
def test_the_device_reproduces_the_counts_of_the_smallest_shape(hip):
    """the [30, 13] cells that tests/test_align.py asserts, through `LabelPropVOS_CRW.propagate_all(memory=, memory_bias=)` on features
    from `crw_hip.center_normalize` / `normalize`: centred, no seed (the cost: 23 / 13 / 9 and 19 / 23 / 12 of 390) and emerging (0);
    the bias 0.1 uncentred, emerging at start 1.0 (24 / 0 / 0 and 20 / 0 / 0) and at start 0 (0)"""
    from imported.labelprop import LabelPropVOS_CRW
    from test_align import BIASED_START_1, CENTRED_30_13
    shape = slr.DRIFT_SHAPES[0]
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=cxt, RADIUS=radius, TEMP=temp, KNN=knn, CONTEXT="sliding"))
    cells = [((B, 1.0, False, "center", 0.0), CENTRED_30_13[B]) for B in (4, 8)]
    cells += [((B, st, True, "center", 0.0), (0, 0, 0)) for B in (1, 4, 8) for st in (0.0, 1.0)]
    cells += [((B, 1.0, True, None, BIAS), BIASED_START_1[B][0]) for B in (4, 8)]
    cells += [((B, 0.0, True, None, BIAS), (0, 0, 0)) for B in (1, 4, 8)]
    for (B, start, emerging, align, bias), want in cells:
        got = []
        for s in range(3):
            emb, cls, K, ff, f0 = lm.bank_case(shape, s, B, start, emerging)
            e = torch.from_numpy(emb).cuda()
            feats = hip.center_normalize(e, [0, B * N, (B + T) * N]) if align else hip.normalize(e)
            memory = (feats[:B].contiguous(), torch.from_numpy(cls[:B]).to(torch.int8).cuda())
            seed = torch.from_numpy(cls[B]).float().cuda() if emerging else None
            pred, L = lp.propagate_all(feats[B:].contiguous(), seed, M, memory=memory, memory_bias=bias)
            assert pred.shape == (N, T) and L.shape == (T * N, M)
            got.append(int((pred.cpu().numpy().T[f0 - B:] != cls[f0:]).sum()))
        print(f"B = {B}, start = {start}, {'emerging' if emerging else 'no seed'}, align {align}, bias {bias}: {got} (CPU fp64 {list(want)})")
        assert tuple(got) == tuple(want), (B, start, emerging, align, bias)


def test_propagate_with_the_two_options_on_the_device(hip):
    """`utils.propagate(memory=, memory_align=, memory_bias=)` with an encoder that hands its patches on as features: the labels are
    `propagate_all`'s on the centred features; None and 0.0 give the bits of the call without the options"""
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    from test_align import CENTRED_30_13
    from test_confidence import Flatten
    shape = slr.DRIFT_SHAPES[0]
    T, N, C, M, cxt, radius, temp, knn, amp = shape
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=cxt, RADIUS=radius, TEMP=temp, KNN=knn, CONTEXT="sliding"))
    B = 4
    emb, cls, K, ff, f0 = lm.bank_case(shape, 0, B, 1.0, False)
    patches = torch.from_numpy(emb).reshape(B + T, N, 2, C // 2)
    bank = crw_utils.memory_bank(patches[:B], torch.from_numpy(cls[:B]).to(torch.int8))
    seq = patches[B:].cuda()
    run = lambda **kw: crw_utils.propagate(seq, None, Flatten(), lp, M, False, False, memory=bank, soft=True, **kw)
    pred, _, _, L = run(memory_align="center")
    assert int((pred.cpu().numpy().T != cls[B:]).sum()) == CENTRED_30_13[B][0]
    feats = hip.center_normalize(torch.from_numpy(emb).cuda(), [0, B * N, (B + T) * N])
    want = lp.propagate_all(feats[B:].contiguous(), None, M, memory=(feats[:B].contiguous(), bank.labels.cuda()))
    assert torch.equal(pred, want[0]) and eq_bits(L, want[1])
    both = run(memory_align="center", memory_bias=BIAS)
    want = lp.propagate_all(feats[B:].contiguous(), None, M, memory=(feats[:B].contiguous(), bank.labels.cuda()), memory_bias=BIAS)
    assert torch.equal(both[0], want[0]) and eq_bits(both[3], want[1])
    plain, off = run(), run(memory_align=None, memory_bias=0.0)
    assert torch.equal(plain[0], off[0]) and eq_bits(plain[3], off[3]) and not torch.equal(plain[0], pred)
