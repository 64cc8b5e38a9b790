"""GPU side of the ordered maps' posterior: the kernel of csrc/labelmap_dense.hip (crw_labelmap_ordered_posterior,
crw_labelmap_ordered_joint_posterior) against the fp64 reference of posterior_ref.py within the derived bound rho and against the
CPU route within 2 rho, over the shapes of dense_ref.py and the geometry cases of joint_ref.py; the exact properties -- equal bits
across label dtype, window placement and what the workspace held before, the joint call on one source twice against the single
call, nothing written outside the windows, post in [0, 1] and 0 outside the order, every refusal before a launch --, the quality
figures' first cases, and `segment(..., posterior=True)` against the direct calls.  Nothing here provokes a fault."""
import ctypes

import pytest
import torch

import dense_ref as dr
import joint_ref as jr
import posterior_ref as pr
from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case, forced_propagate
from test_posterior import CASE_IDS, SHAPE_IDS, joint_quality, orders, single_quality

pytestmark = pytest.mark.gpu

bits = lambda t: t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_posterior()
    return crw_hip


def windowed(hip, call, labels, rows, cols, S, off, poison):
    """`call(labels=, out=, out_hz=, workspace=)` into windows of wider sentinel-filled tensors at column offset `off`, over a
    workspace filled with `poison` -> (post window, hz window) after checking that nothing outside them changed."""
    need = hip.labelmap_posterior_workspace(rows, cols, S)
    ws = torch.full((need + 64,), poison, dtype=torch.uint8, device="cuda")
    wide_lab = torch.full((rows, cols + 7), -7, dtype=labels.dtype, device="cuda")
    wide_lab[:, off:off + cols] = labels
    before = wide_lab.clone()
    wide, wide_hz = torch.full((rows, cols + 7), -7.0, device="cuda"), torch.full((3, S - 1, cols + 9), -7.0, device="cuda")
    out, out_hz = call(labels=wide_lab[:, off:off + cols], out=wide[:, off:off + cols], out_hz=wide_hz[:, :, off + 2:off + 2 + cols],
                       workspace=ws)
    assert out.data_ptr() == wide[:, off:].data_ptr() and out_hz.data_ptr() == wide_hz[:, :, off + 2:].data_ptr()
    assert (wide[:, :off] == -7).all() and (wide[:, off + cols:] == -7).all()
    assert (wide_hz[:, :, :off + 2] == -7).all() and (wide_hz[:, :, off + 2 + cols:] == -7).all()
    assert torch.equal(wide_lab, before) and (ws[need:] == poison).all()  # the labels are read, nothing behind the workspace's size is written
    return out, out_hz


# ---- 1. the kernel against the reference and the CPU route ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.SHAPES, ids=SHAPE_IDS)
def test_kernel_against_the_reference(hip, shape):
    T, N, M, rows, cols = shape
    L, ref = dr.reference(shape)
    Ld = L.cuda()
    worst = 0.0
    for order in orders(M):
        S = len(order)
        for flip in (False, True):
            probs = ref.probs[:, :, ::-1] if flip else ref.probs
            lab8 = hip.labelmap_ordered(Ld, T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)[0]
            call = lambda labels, **kw: hip.labelmap_ordered_posterior(Ld, T, N, M, rows, cols, order, labels, flip=flip, **kw)
            post, hz = call(lab8)
            assert post.is_cuda and post.shape == (rows, cols) and hz.shape == (3, S - 1, cols)
            what = f"gpu {shape} {order} flip={flip}"
            worst = max(worst, pr.check(probs, order, lab8.cpu().numpy(), post.cpu().numpy(), hz.cpu().numpy(), what=what))
            cpu = hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, lab8.cpu(), flip=flip)
            pr.check(probs, order, lab8.cpu().numpy(), post.cpu().numpy(), hz.cpu().numpy(), what=what + " against the CPU route", slack=2.0,
                     against=(cpu[0].numpy(), cpu[1].numpy()))
            # equal bits: fp32 labels, windows at odd offsets in wider maps, a 0xFF- and a 0x00-filled workspace
            for labels, off, poison in ((lab8.float(), 0, 0xFF), (lab8, 1, 0x00), (lab8.float(), 3, 0x00), (lab8, 5, 0xFF)):
                out, out_hz = windowed(hip, call, labels, rows, cols, S, off, poison)
                assert torch.equal(bits(out), bits(post)) and torch.equal(bits(out_hz), bits(hz)), (what, labels.dtype, off, poison)
    print(f"{shape}: worst error / tolerance over the orders and flips {worst:.3e}")


@pytest.mark.parametrize("index", range(len(jr.CASES)), ids=CASE_IDS)
def test_joint_kernel_against_the_reference(hip, index):
    c = jr.case(index)
    N, M, rows, ncols, order = c.shared
    S = len(order)
    kind = dr.KINDS[index % 3]
    Ls = [L.cuda() for L in c.L]
    a, b = c.source(0, Ls[0]), c.source(1, Ls[1])
    lab = hip.labelmap_ordered_joint(a, b, *c.shared, confidence=kind, dtype=torch.int8)[0]
    call = lambda labels, **kw: hip.labelmap_ordered_joint_posterior(a, b, *c.shared, labels, confidence=kind, **kw)
    post, hz = call(lab)
    ca, cb = (jr.dense_confidence(hip, src, N, M, rows, ncols, kind) for src in (a, b))
    probs = jr.selected((cb > ca).cpu().numpy(), *c.probs)  # teacher-forced on the kernel's own took
    what = f"gpu joint {CASE_IDS[index]} {kind}"
    pr.check(probs, order, lab.cpu().numpy(), post.cpu().numpy(), hz.cpu().numpy(), what=what)
    for labels, off, poison in ((lab.float(), 0, 0x00), (lab, 3, 0xFF)):
        out, out_hz = windowed(hip, call, labels, rows, ncols, S, off, poison)
        assert torch.equal(bits(out), bits(post)) and torch.equal(bits(out_hz), bits(hz)), (what, labels.dtype, off)
    for src in (a, b):  # the same source twice: a tie keeps a, the evidence is the single call's, and so is every bit
        L, T, cols, col0, flip = src
        lab1 = hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)[0]
        one, one_hz = hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, lab1, flip=flip)
        two, two_hz = hip.labelmap_ordered_joint_posterior(src, src, *c.shared, lab1[:, col0:col0 + ncols], confidence=kind)
        assert torch.equal(bits(two), bits(one[:, col0:col0 + ncols])) and torch.equal(bits(two_hz), bits(one_hz[:, :, col0:col0 + ncols])), what


# ---- 2. any labels ---------------------------------------------------------------------------------------------------------------------
def test_labels_outside_the_order_and_the_range_of_post(hip):
    shape = dr.SHAPES[3]
    T, N, M, rows, cols = shape
    L, ref = dr.reference(shape)
    order = (4, 0, 2)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(-2, M + 1, (rows, cols), generator=g).to(torch.int8)  # any labels, -2 ... M: columns that step back too
    post, hz = hip.labelmap_ordered_posterior(L.cuda(), T, N, M, rows, cols, order, labels.cuda())
    outside = ~torch.isin(labels, torch.tensor(order, dtype=torch.int8))
    post, hz = post.cpu(), hz.cpu()
    assert outside.any() and (post[outside] == 0).all() and (post[~outside] > 0).all() and post.max() <= 1
    pr.check(ref.probs, order, labels.numpy(), post.numpy(), hz.numpy(), what="gpu, any labels")
    half = labels.float()
    half[0, 0] = 0.5  # a label that is no integer is outside every order
    post2 = hip.labelmap_ordered_posterior(L.cuda(), T, N, M, rows, cols, order, half.cuda())[0].cpu()
    assert post2[0, 0] == 0 and torch.equal(post2[1:], post[1:])


def test_one_hot_evidence_against_the_order_stays_finite(hip):
    """Seed-like one-hot rows whose classes run AGAINST the order down the column, 64 rows deep: the floor keeps every path alive
    in the definition; where fp32 cannot hold a row's normaliser the kernel writes 0, never a NaN."""
    T, N, M, rows, cols = 2, 8, 4, 64, 70
    classes = (M - 1 - torch.arange(N) * M // N).repeat(T)
    L = torch.nn.functional.one_hot(classes, M).float().cuda()
    order = (0, 1, 2, 3)
    lab = hip.labelmap_ordered(L, T, N, M, rows, cols, order, dtype=torch.int8)[0]
    for floor in (2.0 ** -20, 1e-4, 0.25):
        post, hz = hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, lab, floor=floor)
        assert torch.isfinite(post).all() and torch.isfinite(hz).all() and post.min() >= 0 and post.max() <= 1
        assert (hz[1] >= 0).all() and (hz[1] <= rows * (1 + 1e-5)).all() and (hz[2] >= 0).all()


# ---- 3. status codes -------------------------------------------------------------------------------------------------------------------
def test_kernel_argument_errors_launch_nothing(hip):
    lib = hip.lib()
    La, Lb = torch.full((16, 4), 0.25, device="cuda"), torch.full((16, 4), 0.25, device="cuda")
    labels = torch.zeros(8, 8, device="cuda")
    post, hz = torch.full((8, 8), -7.0, device="cuda"), torch.full((3, 1, 8), -7.0, device="cuda")
    need = lib.crw_labelmap_posterior_workspace(8, 8, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    order = (ctypes.c_int * 2)(0, 1)

    def call(joint, floor=1e-4, post_ptr=post.data_ptr(), hz_ptr=hz.data_ptr(), hz_ld=8, ws_ptr=ws.data_ptr(), ws_bytes=need, kind=0, S=2,
             col0_b=8):
        tail = (floor, labels.data_ptr(), 0, 8, post_ptr, hz_ptr, hz_ld, ws_ptr, ws_bytes, None)
        if joint:
            return lib.crw_labelmap_ordered_joint_posterior(La.data_ptr(), 4, 8, 0, 0, Lb.data_ptr(), 4, 16, col0_b, 1, 4, 4, 8, 8, order, S, kind,
                                                            *tail)
        return lib.crw_labelmap_ordered_posterior(La.data_ptr(), 4, 4, 4, 8, 8, 0, order, S, *tail)

    for joint in (False, True):
        for kw in (dict(floor=0.0), dict(floor=2.0 ** -21), dict(floor=0.3), dict(floor=float("nan")), dict(post_ptr=None, hz_ptr=None),
                   dict(hz_ld=7), dict(ws_ptr=None), dict(S=1), dict(S=5)):
            assert call(joint, **kw) == hip.CRW_EINVAL, (joint, kw)
        assert call(joint, ws_bytes=need - 1) == hip.CRW_EWORKSPACE
    for kw in (dict(kind=-1), dict(kind=3), dict(col0_b=9), dict(col0_b=-1)):
        assert call(True, **kw) == hip.CRW_EINVAL, kw
    with pytest.raises(hip.CrwError) as e:
        hip.labelmap_ordered_posterior(La, 4, 4, 4, 8, 8, (0, 1), labels, out=post, out_hz=hz, workspace=ws[:need - 4])
    assert e.value.status == hip.CRW_EWORKSPACE
    torch.cuda.synchronize()
    assert (post == -7).all() and (hz == -7).all() and not ws.any()
    assert call(False, hz_ptr=None) == hip.CRW_OK  # either output may be null
    torch.cuda.synchronize()
    assert (hz == -7).all() and (post != -7).all()
    first = post.clone()
    post.fill_(-7.0)
    assert call(True, post_ptr=None) == hip.CRW_OK
    torch.cuda.synchronize()
    assert (post == -7).all() and (hz != -7).all()
    assert call(True) == hip.CRW_OK
    torch.cuda.synchronize()
    # uniform rows: every monotone path weighs the same; label 0 at row r is state 0 there: (rows - r) of the rows + 1 paths
    want = (8 - torch.arange(8.0, device="cuda")) / 9
    assert torch.allclose(post, want[:, None].expand(8, 8), rtol=1e-5) and torch.equal(bits(post), bits(first))
    assert (hz[0] == 8).all() and torch.allclose(hz[1], torch.full((1, 8), 4.0, device="cuda"), rtol=1e-5)  # B uniform on 0 ... 8


# ---- 4. quality: the first case of each kind -------------------------------------------------------------------------------------------
def test_quality_on_the_first_layered_items_on_the_device(hip):
    single_quality(hip, 0, "cuda")
    joint_quality(hip, 0, "cuda")


# ---- 5. segment ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_last", [False, True], ids=["forward", "use_last"])
def test_segment_posterior_against_the_direct_calls(hip, monkeypatch, use_last):
    import inference as crw_inference
    import utils as crw_utils
    enc, fresh, seg, lp, N = e2e_case(0, n_rg=2, H=100)
    forced = [6, None]
    order = (0, 1, 2, 3, 4)
    T, W = T_E2E, PATCH[1]
    rg_len, rows, rg_h = T * W, seg.shape[0], N * 8 + 8
    kind = "maxprob"
    kw = dict(correction=True, use_last=use_last, dataset_id=2, confidence=kind, upsample="bilinear", decode="ordered", order=order,
              merge="ordered" if use_last else "rule")

    def segment(**extra):
        monkeypatch.setattr(crw_inference, "propagate", forced_propagate(forced))
        return crw_inference.segment(fresh(), seg, enc, lp, M_E2E, T, PATCH, OVERLAP, **kw, **extra)

    plain, out = segment(), segment(posterior=True)
    assert set(out) == set(plain) | {"post", "horizon", "floor"} and out["floor"] == 1e-4 and out["change_idx"] == forced
    for k in ("pred", "forward", "conf", "forward_conf"):
        assert torch.equal(bits(out[k]), bits(plain[k])), k
    width = out["pred"].shape[1]
    assert out["post"].shape == (rows, width) and out["horizon"].shape == (3, len(order) - 1, width)
    assert out["post"].min() >= 0 and out["post"].max() <= 1 and torch.isfinite(out["horizon"]).all()
    ds, segd = fresh(), seg.cuda()
    soft = lambda seq, ref, last: crw_utils.propagate(seq.cuda(), ref, enc, lp, M_E2E, False, last, soft=True)[-1]
    fwd = [soft(ds[t * T], segd[:rg_h, rg_len * t:rg_len * t + W], False) for t in range(2)]
    px = (T - 6) * W
    tail = soft(ds.get_smaller_item(0, T - 6), segd[:, rg_len - px:rg_len - px + W], False)
    for t in range(2):
        a, b = rg_len * t, rg_len * (t + 1)
        cut = px if t == 0 else 0
        windows = []
        if use_last:
            seq = ds[t * T]  # (the reverse pass runs on the items the correction shortened)
            rev = (soft(seq, torch.flip(segd[:, a:b], (-1,))[:, :W], True), seq.shape[0], rg_len)
            joint = lambda x, y, lo, hi: hip.labelmap_ordered_joint_posterior(x, y, N, M_E2E, rows, hi - lo, order, out["pred"][:, lo:hi],
                                                                               confidence=kind)
            windows.append((a, b - cut, joint((fwd[t], T, rg_len, 0, False), (*rev, 0, True), a, b - cut)))
            if cut:
                windows.append((b - cut, b, joint((tail, T - 6, px, 0, False), (*rev, rg_len - px, True), b - cut, b)))
        else:
            lab = hip.labelmap_ordered(fwd[t], T, N, M_E2E, rows, rg_len, order)[0]
            whole = hip.labelmap_ordered_posterior(fwd[t], T, N, M_E2E, rows, rg_len, order, lab)
            windows.append((a, b - cut, tuple(m[..., :rg_len - cut] for m in whole)))
            if cut:
                windows.append((b - cut, b, hip.labelmap_ordered_posterior(tail, T - 6, N, M_E2E, rows, px, order, out["pred"][:, b - cut:b])))
        for lo, hi, (post, hz) in windows:
            assert torch.equal(bits(out["post"][:, lo:hi]), bits(post)), (t, lo, hi)
            assert torch.equal(bits(out["horizon"][:, :, lo:hi]), bits(hz)), (t, lo, hi)
    cal = crw_inference.calibration(out["pred"], out["post"], seg, 3, remove_unc=False, nclasses=M_E2E)
    bars = crw_inference.horizon_bars(out["horizon"], seg, order)
    print(f"use_last={use_last}: ECE of post {cal.ece:.4f}, invalid confidences {cal.dropped[2]}\n{bars}")
    assert cal.dropped[2] == 0 and bars.n.shape == (len(order) - 1,)
