"""GPU side of the dense label map: the kernel of csrc/labelmap_dense.hip against the fp64 helper on the host (dense_ref.py) under
the bound B of DESIGN.md section 3, the exact dyadic cases and their ties, column windows of wider maps at every 16-byte phase,
`segment(..., upsample='bilinear')` against the same maps assembled by hand, and the command line.  The reference is never another
call of the code under test; nothing here provokes a fault."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_ref as dr
from conftest import PKG
from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case, forced_propagate

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.int8)


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_dense()
    return crw_hip


# ---- 1. the kernel against the fp64 helper ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (None,) + dr.KINDS, ids=str)
@pytest.mark.parametrize("shape", dr.SHAPES + dr.EXACT[:1] + [dr.SLAB], ids=str)
def test_kernel_against_the_fp64_helper(hip, shape, kind):
    T, N, M, rows, cols = shape
    L, ref = dr.reference(shape)
    Ld = L.cuda()
    for dtype in DTYPES:
        for flip in (False, True):
            lab, conf = hip.labelmap_dense(Ld, T, N, M, rows, cols, confidence=kind, flip=flip, dtype=dtype)
            assert lab.is_cuda and lab.shape == (rows, cols) and lab.dtype == dtype and (conf is None) == (kind is None)
            lab, conf = lab.cpu(), (None if conf is None else conf.cpu())
            if flip:
                lab, conf = torch.flip(lab, (1,)), (None if conf is None else torch.flip(conf, (1,)))
            dr.check_outputs(ref, lab.numpy(), None if conf is None else conf.numpy(), kind,
                             f"gpu {shape} {kind} {dtype} flip={flip}")


def test_rows_that_start_off_a_16_byte_boundary(hip):
    """L one float into a buffer (M = 4 and 6: the 16- and 8-byte loads fall back): bitwise the aligned call."""
    for shape in ((8, 8, 4, 5, 3), (9, 12, 6, 50, 61)):
        T, N, M, rows, cols = shape
        L = dr.reference(shape)[0].cuda()
        buf = torch.zeros(L.numel() + 1, device="cuda")
        buf[1:] = L.view(-1)
        a = hip.labelmap_dense(L, T, N, M, rows, cols, confidence="entropy")
        b = hip.labelmap_dense(buf[1:].view(T * N, M), T, N, M, rows, cols, confidence="entropy")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 2. exact cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.EXACT, ids=str)
def test_exact_dyadic_case_and_ties_on_the_device(hip, shape):
    T, N, M, rows, cols = shape
    L = dr.exact_rows(T, N, M)
    ref = dr.Ref(L.numpy(), T, N, M, rows, cols)
    ties = ref.gap == 0
    assert ties.any() and (ref.labels[ties] == M - 2).all()
    for dtype in DTYPES:
        for flip in (False, True):
            lab, conf = hip.labelmap_dense(L.cuda(), T, N, M, rows, cols, confidence="maxprob", flip=flip, dtype=dtype)
            lab, conf = (torch.flip(t.cpu(), (1,)) if flip else t.cpu() for t in (lab, conf))
            assert np.array_equal(lab.numpy().astype(np.int64), ref.labels)  # outright, the exact ties included
            assert np.array_equal(conf.numpy().astype(np.float64), ref.conf["maxprob"])


# ---- 3. windows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cols", [29, 61])
def test_column_windows_of_a_wider_map(hip, cols, dtype):
    T, N, M, rows = 9, 12, 6, 50
    L = dr.dirichlet_rows(T, N, M, seed=3).cuda()
    for flip in (False, True):
        lab, conf = hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin", dtype=dtype, flip=flip)
        if flip:
            plain = hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin", dtype=dtype)
            assert torch.equal(lab, torch.flip(plain[0], (1,))) and torch.equal(conf, torch.flip(plain[1], (1,)))
        only, _ = hip.labelmap_dense(L, T, N, M, rows, cols, dtype=dtype, flip=flip)
        assert torch.equal(only, lab)
        for a in (0, 1, 3, 5):
            wide = torch.full((rows, cols + 7), -7, dtype=dtype, device="cuda")
            widec = torch.full((rows, cols + 7), -7.0, device="cuda")
            out, outc = hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin", dtype=dtype, flip=flip,
                                           out=wide[:, a:a + cols], out_conf=widec[:, a:a + cols])
            assert out.data_ptr() == wide[:, a:].data_ptr() and outc.data_ptr() == widec[:, a:].data_ptr()
            for m, want in ((wide, lab), (widec, conf)):
                assert torch.equal(m[:, a:a + cols], want)
                assert (m[:, :a] == -7).all() and (m[:, a + cols:] == -7).all()
            # labels alone, and a pitch that moves the 16-byte phase from row to row
            odd = torch.full((rows, cols + 6), -7, dtype=dtype, device="cuda")
            hip.labelmap_dense(L, T, N, M, rows, cols, dtype=dtype, flip=flip, out=odd[:, a:a + cols])
            assert torch.equal(odd[:, a:a + cols], lab) and (odd[:, :a] == -7).all() and (odd[:, a + cols:] == -7).all()
    # a confidence map whose 16-byte phase is not the labels': single stores, the same values
    wide = torch.full((rows, cols + 8), -7, dtype=dtype, device="cuda")
    widec = torch.full((rows, cols + 8), -7.0, device="cuda")
    lab, conf = hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin", dtype=dtype)
    hip.labelmap_dense(L, T, N, M, rows, cols, confidence="margin", dtype=dtype, out=wide[:, 4:4 + cols], out_conf=widec[:, 1:1 + cols])
    assert torch.equal(wide[:, 4:4 + cols], lab) and torch.equal(widec[:, 1:1 + cols], conf)
    assert (widec[:, :1] == -7).all() and (widec[:, 1 + cols:] == -7).all() and (wide[:, :4] == -7).all() and (wide[:, 4 + cols:] == -7).all()
    with pytest.raises(ValueError):
        hip.labelmap_dense(L, T, N, M, rows, cols, out=torch.zeros(rows, 2 * cols, device="cuda")[:, ::2])


def test_kernel_argument_errors(hip):
    lib = hip.lib()
    L = torch.full((12, 3), 1 / 3, device="cuda")
    out = torch.zeros(8, 8, device="cuda")
    for T, M, rows, cols, kind, ld in ((0, 3, 8, 8, -1, 8), (4, 1, 8, 8, -1, 8), (4, 17, 8, 8, -1, 8), (4, 3, 0, 8, -1, 8),
                                       (4, 3, 8, (1 << 22) + 1, -1, 1 << 23), (4, 3, 8, 8, 0, 8), (4, 3, 8, 8, 3, 8), (4, 3, 8, 8, -1, 7)):
        assert lib.crw_labelmap_dense(L.data_ptr(), T, 3, M, rows, cols, 0, kind, out.data_ptr(), 0, None, ld, None) == hip.CRW_EINVAL
    assert not out.any()


# ---- 4. segment(upsample='bilinear') ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", ["rule", "confidence"])
def test_segment_bilinear_is_the_hand_assembled_map(hip, monkeypatch, merge):
    import inference as crw_inference
    import utils as crw_utils
    enc, fresh, seg, lp, N = e2e_case(0, n_rg=2, H=100)
    forced = [6, None]
    T, W = T_E2E, PATCH[1]
    rg_len, rows, rg_h = T * W, seg.shape[0], N * 8 + 8
    args = (seg, enc, lp, M_E2E, T, PATCH, OVERLAP)
    kw = dict(correction=True, use_last=True, dataset_id=3, confidence="maxprob", merge=merge)

    def segment(**more):
        monkeypatch.setattr(crw_inference, "propagate", forced_propagate(forced))
        return crw_inference.segment(fresh(), *args, **kw, **more)

    plain, near, out = segment(), segment(upsample="nearest"), segment(upsample="bilinear")
    for k in ("pred", "forward", "conf", "forward_conf"):
        assert torch.equal(plain[k], near[k])
    assert out["change_idx"] == forced and set(out) == set(plain)
    assert all(out[k].shape == plain[k].shape and out[k].dtype == torch.float32 for k in ("pred", "forward", "conf", "forward_conf"))

    # by hand: propagate(soft=True), contiguous unflipped labelmap_dense calls, cat / flip / slicing
    ds, segd = fresh(), seg.cuda()
    soft = lambda seq, ref, last: crw_utils.propagate(seq.cuda(), ref, enc, lp, M_E2E, False, last, soft=True)[-1]
    dense = lambda L, frames, cols: hip.labelmap_dense(L, frames, N, M_E2E, rows, cols, confidence="maxprob")
    fl, fc = [], []
    for t in range(2):
        L = soft(ds[t * T], segd[:rg_h, rg_len * t:rg_len * t + W], False)
        assert L.shape == (T * N, M_E2E) and L.is_cuda and L.dtype == torch.float32
        lab, conf = dense(L, T, rg_len)
        fl.append(lab)
        fc.append(conf)
    small = T - forced[0]
    px = small * W
    tail = dense(soft(ds.get_smaller_item(0, small), segd[:, rg_len - px:rg_len - px + W], False), small, px)
    fl[0][:, rg_len - px:], fc[0][:, rg_len - px:] = tail
    fwd, fconf = torch.cat(fl, 1), torch.cat(fc, 1)
    assert torch.equal(out["forward"], fwd) and torch.equal(out["forward_conf"], fconf)
    rl, rc = [], []
    for t in range(2):  # after the correction: the shortened items, stretched to rg_len
        seq = ds[t * T]
        L = soft(seq, torch.flip(segd[:, rg_len * t:rg_len * (t + 1)], (-1,))[:, :W], True)
        lab, conf = dense(L, seq.shape[0], rg_len)
        rl.append(torch.flip(lab, (-1,)))
        rc.append(torch.flip(conf, (-1,)))
    rev, rconf = torch.cat(rl, 1), torch.cat(rc, 1)
    take = rconf > fconf if merge == "confidence" else crw_inference._reverse_rule_mask(fwd, rev, 3).view_as(fwd)
    assert torch.equal(out["pred"], torch.where(take, rev, fwd)) and torch.equal(out["conf"], torch.where(take, rconf, fconf))
    assert float(fconf.min()) >= 1 / M_E2E - 1e-6 and float(fconf.max()) <= 1 and not torch.equal(out["forward"], plain["forward"])


def test_propagate_soft_is_the_propagation_s_L(hip):
    """The soft labels `propagate` hands out are the rows its labels and its confidence come from, for `propagate_all` and for a
    foreign `lp` that only offers `predict`."""
    import utils as crw_utils
    from conftest import load_golden
    from imported.labelprop import LabelPropVOS_CRW
    from test_hip_parity import _Flatten
    g = load_golden("labelprop_trunc_T14N10")
    T, N, C = g["emb"].shape
    M = int(g["nclasses"])
    cfg = dict(CXT_SIZE=int(g["cxt_size"]), RADIUS=int(g["radius"]), TEMP=float(g["temp"]), KNN=int(g["knn"]))
    seq, seg_ref = torch.tensor(g["emb"]).cuda().reshape(T, N, C // 4, 4), torch.tensor(g["seg_ref"]).cuda()

    class PredictOnly:
        def __init__(self, inner):
            self.inner = inner

        def predict(self, feats, masks, curr_feat):
            return self.inner.predict(feats, masks, curr_feat)

    run = lambda lp, **kw: crw_utils.propagate(seq, seg_ref, _Flatten(), lp, M, False, False, **kw)
    three, four, five = run(LabelPropVOS_CRW(cfg)), run(LabelPropVOS_CRW(cfg), soft=True), run(LabelPropVOS_CRW(cfg), confidence="margin", soft=True)
    assert len(three) == 3 and len(four) == 4 and len(five) == 5 and torch.equal(three[0], four[0])
    L = four[3]
    assert L.shape == (T * N, M) and L.is_cuda and L.dtype == torch.float32 and torch.equal(L, five[4])
    assert torch.equal(L.view(T, N, M).argmax(-1).t().float(), three[0])
    assert torch.equal(hip.labelprop_confidence(L, T, N, M, "margin"), five[3])
    foreign = run(PredictOnly(LabelPropVOS_CRW(cfg)), soft=True)
    assert len(foreign) == 4 and torch.equal(foreign[3], L)
    one = crw_utils.propagate(seq[:1], seg_ref, _Flatten(), LabelPropVOS_CRW(cfg), M, False, False, soft=True)
    assert len(one) == 4 and one[3].shape == (N, M) and one[3].is_cuda and torch.equal(one[3].argmax(-1).float(), one[0][:, 0])


# ---- 5. driver --------------------------------------------------------------------------------------------------------------------
def test_cli_with_upsample_in_a_child_process(hip, tmp_path):
    H, W, T = 100, 2 * 16 * 10, 10
    js = tmp_path / "report.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_all.py"), "--synthetic", str(H), str(W), "--dataset", "0",
                        "--model", "0", "--seq_length", str(T), "-c", "6", "-r", "6", "-k", "8", "--use_last", "true", "--output_folder",
                        str(tmp_path / "out") + "/", "--report_json", str(js), "--confidence", "maxprob", "--upsample", "bilinear"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(js.read_text())
    assert d["upsample"] == "bilinear" and d["calibration"]["kind"] == "maxprob"
    assert "upsample='bilinear'" in r.stdout
    saved = torch.load(tmp_path / "out" / "predicted_map.pt", map_location="cpu")
    assert saved.dtype == torch.int8 and list(saved.shape) == d["map_shape"]
