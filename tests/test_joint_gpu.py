"""GPU side of the order-preserving merge: the kernel of csrc/labelmap_dense.hip (crw_labelmap_ordered_joint[_batch]) against its
definition (joint_ref.py) -- the same source twice is `labelmap_ordered`, conf is the confidence merge's bit for bit, the labels
teacher-forced on `took` against the fp64 decode of the selected rows -- over the geometry cases, both label dtypes, the three
confidence kinds and soft labels off their 16-byte alignment; column windows, stale workspaces, the batch, the status codes, the
quality claim's first case, and `segment(..., merge='ordered')` / `segment_sweep` against merge='confidence' and against the joint
calls assembled by hand.  The reference is never another call of the code under test; nothing here provokes a fault."""
import ctypes
import itertools

import pytest
import torch

import dense_ref as dr
import joint_ref as jr
import ordered_ref as od
from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case, forced_propagate
from test_joint import CASE_IDS, monotone

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.int8)


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_joint()
    return crw_hip


def on_device(L, misalign):
    """L on the device; `misalign`: 4 bytes behind an allocation's start, so no 8- or 16-byte load of a row is possible."""
    if not misalign:
        return L.cuda()
    buf = torch.empty(L.numel() + 1, device="cuda")
    out = buf[1:].view(L.shape)
    out.copy_(L)
    assert out.data_ptr() % 8 == 4
    return out


# ---- 1. the kernel against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(jr.CASES)), ids=CASE_IDS)
def test_kernel_against_the_definition(hip, index):
    c = jr.case(index)
    N, M, rows, ncols, order = c.shared
    for i, (kind, dtype) in enumerate(itertools.product(dr.KINDS, DTYPES)):
        Ls = [on_device(L, misalign=i % 2 == 1) for L in c.L]
        a, b = c.source(0, Ls[0]), c.source(1, Ls[1])
        for src in (a, b):  # the same source twice: a tie keeps a, the map is labelmap_ordered's window
            L, T, cols, col0, flip = src
            lab, conf = hip.labelmap_ordered_joint(src, src, N, M, rows, ncols, order, confidence=kind, dtype=dtype)
            want, wantc = hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence=kind, flip=flip, dtype=dtype)
            assert lab.is_cuda and lab.shape == (rows, ncols) and lab.dtype == dtype
            assert torch.equal(lab, want[:, col0:col0 + ncols]), (kind, dtype)
            assert torch.equal(conf.view(torch.int32), wantc[:, col0:col0 + ncols].contiguous().view(torch.int32)), (kind, dtype)
        lab, conf = hip.labelmap_ordered_joint(a, b, N, M, rows, ncols, order, confidence=kind, dtype=dtype)
        jr.check_against_the_definition(hip, c, lab, conf, kind, *Ls, what=f"gpu {CASE_IDS[index]} {kind} {dtype}")


# ---- 2. windows, 3. stale workspaces --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("index", [0, 2, 3], ids=[CASE_IDS[i] for i in (0, 2, 3)])
def test_column_windows_of_wider_maps_over_stale_workspaces(hip, index, dtype):
    c = jr.case(index)
    N, M, rows, ncols, order = c.shared
    a, b = (c.source(k, c.L[k].cuda()) for k in (0, 1))
    need = hip.labelmap_ordered_workspace(1, rows, ncols)
    lab, conf = hip.labelmap_ordered_joint(a, b, *c.shared, confidence="margin", dtype=dtype)
    for off, poison in ((0, 0xFF), (1, 0x00), (3, 0xFF), (5, 0x00)):
        ws = torch.full((need + 64,), poison, dtype=torch.uint8, device="cuda")
        wide = torch.full((rows, ncols + 7), -7, dtype=dtype, device="cuda")
        widec = torch.full((rows, ncols + 7), -7.0, device="cuda")
        out, outc = hip.labelmap_ordered_joint(a, b, *c.shared, confidence="margin", dtype=dtype, out=wide[:, off:off + ncols],
                                               out_conf=widec[:, off:off + ncols], workspace=ws)
        assert out.data_ptr() == wide[:, off:].data_ptr() and outc.data_ptr() == widec[:, off:].data_ptr()
        for m, want in ((wide, lab), (widec, conf)):  # a 0xFF- and a 0x00-filled workspace give the bits of a fresh one
            assert torch.equal(m[:, off:off + ncols], want)
            assert (m[:, :off] == -7).all() and (m[:, off + ncols:] == -7).all()
        assert (ws[need:] == poison).all()  # nothing behind the workspace's size is written
    with pytest.raises(ValueError):
        hip.labelmap_ordered_joint(a, b, *c.shared, confidence="margin", out=torch.zeros(rows, 2 * ncols, device="cuda")[:, ::2])


# ---- 4. batch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [1, 2, 5], ids=[CASE_IDS[i] for i in (1, 2, 5)])
def test_batch_kernel_equals_the_one_map_kernel_per_configuration(hip, index):
    c = jr.case(index)
    N, M, rows, ncols, order = c.shared
    G = 3
    Ls = [torch.stack([dr.dirichlet_rows(T, N, M, seed=70 + 5 * g + k) for g in range(G)]).cuda() for k, (T, _, _, _) in enumerate(c.geo)]
    for dtype in DTYPES:
        lab, conf = hip.labelmap_ordered_joint_batch(c.source(0, Ls[0]), c.source(1, Ls[1]), G, *c.shared, confidence="entropy", dtype=dtype)
        assert lab.shape == (G, rows, ncols) and lab.dtype == dtype
        for g in range(G):
            one, onec = hip.labelmap_ordered_joint(c.source(0, Ls[0][g]), c.source(1, Ls[1][g]), *c.shared, confidence="entropy", dtype=dtype)
            assert torch.equal(lab[g], one) and torch.equal(conf[g].view(torch.int32), onec.view(torch.int32))
    wide = torch.full((G, rows, ncols + 5), -7, dtype=torch.int8, device="cuda")
    widec = torch.full((G, rows, ncols + 5), -7.0, device="cuda")
    hip.labelmap_ordered_joint_batch(c.source(0, Ls[0]), c.source(1, Ls[1]), G, *c.shared, confidence="entropy", out=wide[:, :, 3:3 + ncols],
                                     out_conf=widec[:, :, 3:3 + ncols])
    want, wantc = hip.labelmap_ordered_joint_batch(c.source(0, Ls[0]), c.source(1, Ls[1]), G, *c.shared, confidence="entropy")
    for m, w in ((wide, want), (widec, wantc)):
        assert torch.equal(m[:, :, 3:3 + ncols], w) and (m[:, :, :3] == -7).all() and (m[:, :, 3 + ncols:] == -7).all()


# ---- 5. status codes ------------------------------------------------------------------------------------------------------------------
def test_kernel_argument_errors_launch_nothing(hip):
    lib = hip.lib()
    La, Lb = torch.full((16, 4), 0.25, device="cuda"), torch.full((16, 4), 0.25, device="cuda")  # dyadic weights: every value exact
    out, outc = torch.zeros(8, 8, device="cuda"), torch.zeros(8, 8, device="cuda")
    need = lib.crw_labelmap_ordered_workspace(1, 8, 8)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    order = (ctypes.c_int * 2)(0, 1)

    def call(col0_b=8, kind=0, conf=outc.data_ptr(), ws_ptr=ws.data_ptr(), ws_bytes=need, Lb_ptr=Lb.data_ptr()):
        return lib.crw_labelmap_ordered_joint(La.data_ptr(), 4, 8, 0, 0, Lb_ptr, 4, 16, col0_b, 1, 4, 4, 8, 8, order, 2, kind, out.data_ptr(), 0,
                                              conf, 8, ws_ptr, ws_bytes, None)

    for kw in (dict(col0_b=9), dict(col0_b=-1), dict(kind=-1), dict(kind=-1, conf=None), dict(kind=3), dict(ws_ptr=None), dict(Lb_ptr=None)):
        assert call(**kw) == hip.CRW_EINVAL, kw
    assert call(ws_bytes=need - 1) == hip.CRW_EWORKSPACE
    with pytest.raises(hip.CrwError) as e:
        hip.labelmap_ordered_joint((La, 4, 8, 0, False), (Lb, 4, 16, 8, True), 4, 4, 8, 8, (0, 1), confidence="maxprob", out=out,
                                   out_conf=outc, workspace=ws[:need - 2])
    assert e.value.status == hip.CRW_EWORKSPACE
    torch.cuda.synchronize()
    assert not out.any() and not outc.any() and not ws.any()
    assert call(conf=None) == hip.CRW_OK  # conf may be null: the labels alone
    torch.cuda.synchronize()
    assert not outc.any()
    assert call() == hip.CRW_OK
    torch.cuda.synchronize()
    assert (outc == 0.25).all() and (out == 0).all()  # uniform rows: every state ties, the lowest is kept


# ---- 6. the quality claim, first case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(od.SEEDS)), ids=[f"seed{s}" for s in od.SEEDS])
def test_joint_map_on_paired_layered_items_on_the_device(hip, index):
    assert jr.PAIRS[index][0] == od.QUALITY[0]
    jr.check_quality(jr.quality_counts(hip, index, "cuda"))


# ---- 7. segment / segment_sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("correction", [False, True], ids=["", "correction"])
def test_segment_merge_ordered_against_merge_confidence(hip, monkeypatch, correction):
    import inference as crw_inference
    import utils as crw_utils
    enc, fresh, seg, lp, N = e2e_case(0, n_rg=2, H=100)
    forced = [6, None]
    order = (0, 1, 2, 3, 4)
    T, W = T_E2E, PATCH[1]
    rg_len, rows, rg_h = T * W, seg.shape[0], N * 8 + 8
    kw = dict(correction=correction, use_last=True, dataset_id=2, confidence="maxprob", upsample="bilinear", decode="ordered", order=order)

    def segment(merge):
        monkeypatch.setattr(crw_inference, "propagate", forced_propagate(forced))
        return crw_inference.segment(fresh(), seg, enc, lp, M_E2E, T, PATCH, OVERLAP, merge=merge, **kw)

    plain, out = segment("confidence"), segment("ordered")
    assert set(out) == set(plain) and out["change_idx"] == forced
    for k in ("conf", "forward", "forward_conf"):
        assert torch.equal(out[k].view(torch.int32), plain[k].view(torch.int32)), k
    assert monotone(out["pred"], order) and out["pred"].shape == plain["pred"].shape and out["pred"].dtype == torch.float32
    print(f"correction={correction}: merge='confidence' steps back in {jr.steps_back(plain['pred'].cpu().numpy(), order)} columns, "
          f"merge='ordered' differs from it at {int((out['pred'] != plain['pred']).sum())} of {out['pred'].numel()} pixels")
    if correction:
        return
    ds, segd = fresh(), seg.cuda()
    soft = lambda seq, ref, last: crw_utils.propagate(seq.cuda(), ref, enc, lp, M_E2E, False, last, soft=True)[-1]
    for t in range(2):  # every radargram's window is the joint map of its two passes' soft labels
        seq = ds[t * T]
        Lf = soft(seq, segd[:rg_h, rg_len * t:rg_len * t + W], False)
        Lr = soft(seq, torch.flip(segd[:, rg_len * t:rg_len * (t + 1)], (-1,))[:, :W], True)
        lab, conf = hip.labelmap_ordered_joint((Lf, T, rg_len, 0, False), (Lr, T, rg_len, 0, True), N, M_E2E, rows, rg_len, order,
                                               confidence="maxprob")
        assert torch.equal(out["pred"][:, rg_len * t:rg_len * (t + 1)], lab)
        assert torch.equal(out["conf"][:, rg_len * t:rg_len * (t + 1)].contiguous().view(torch.int32), conf.view(torch.int32))


def test_segment_sweep_merge_ordered_equals_segment_per_configuration(hip, monkeypatch):
    from imported.labelprop import LabelPropSweep
    from test_sweep_dense_gpu import sweep_against_segment
    enc, fresh, seg, _, _ = e2e_case(0, n_rg=2, H=100)
    sweep = LabelPropSweep(6, [6, 4], [0.1], [8, 5])
    order = (0, 1, 2, 4)
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cuda", confidence="margin", merge="ordered", upsample="bilinear",
              decode="ordered", order=order)
    out = sweep_against_segment(monkeypatch, fresh, (seg, enc, M_E2E, T_E2E, PATCH, OVERLAP), sweep, kw, [6, None])
    assert out["change_idx"] == [6, None] and not (out["pred"] == 3).any()
    assert all(monotone(m, order) for m in out["pred"]) and len({m.cpu().numpy().tobytes() for m in out["pred"]}) > 1
