"""GPU side of the depth-ordered label map: the kernel of csrc/labelmap_dense.hip (crw_labelmap_ordered[_batch]) against the
definition in fp64 (ordered_ref.py: feasibility, optimality gap, sanity), the exact dyadic cases, a confidence that is
`labelmap_dense`'s bit for bit, column windows at odd offsets and pitches over a poisoned workspace, the batch, the status codes, the
quality claim, `segment(..., decode='ordered')` against the same maps assembled by hand, `segment_sweep`, and the command line.  The
reference is never another call of the code under test; nothing here provokes a fault."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_ref as dr
import ordered_ref as od
from conftest import PKG
from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case, forced_propagate
from test_ordered import ORDERS, WIDE, unflip

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.int8)


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_ordered()
    return crw_hip


# ---- 1. the kernel against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.SHAPES + [dr.SLAB], ids=str)
def test_kernel_against_the_definition(hip, shape):
    T, N, M, rows, cols = shape
    order = tuple(range(M))
    L, ref, _, score = od.reference(shape, order)
    Ld = L.cuda()
    for dtype, flip in ((torch.float32, False), (torch.int8, True)):
        lab, conf = hip.labelmap_ordered(Ld, T, N, M, rows, cols, order, flip=flip, dtype=dtype)
        assert lab.is_cuda and lab.shape == (rows, cols) and lab.dtype == dtype and conf is None
        od.check(ref.probs, unflip(lab.cpu(), flip).numpy(), order, score, f"gpu {shape} {dtype} flip={flip}")


@pytest.mark.parametrize("order", ORDERS, ids=str)
def test_kernel_under_other_orders(hip, order):
    T, N, M, rows, cols = WIDE
    L, ref, _, score = od.reference(WIDE, order)
    for flip in (False, True):
        lab, _ = hip.labelmap_ordered(L.cuda(), T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)
        od.check(ref.probs, unflip(lab.cpu(), flip).numpy(), order, score, f"gpu {WIDE} flip={flip}")


def test_both_backward_scans_write_the_same_maps(hip, monkeypatch):
    """CRW_ORDERED_BACK=1 (one back-pointer word in flight, the A/B arm of tools/ordered_timing.py) against the default (8), at row
    counts below, at and off a multiple of 8."""
    for shape in ((8, 8, 4, 5, 3), (4, 3, 16, 9, 130), (2, 2, 2, 4, 4), (3, 2, 2, 16, 48), WIDE):
        T, N, M, rows, cols = shape
        L = dr.reference(shape)[0].cuda() if shape != (3, 2, 2, 16, 48) else dr.dirichlet_rows(T, N, M, seed=2).cuda()
        monkeypatch.delenv("CRW_ORDERED_BACK", raising=False)
        with hip.routes() as hit:
            want, _ = hip.labelmap_ordered(L, T, N, M, rows, cols, range(M), dtype=torch.int8)
        assert dict(hit) == {"ordered.back_default": 1}, dict(hit)
        monkeypatch.setenv("CRW_ORDERED_BACK", "1")
        with hip.routes() as hit:
            got, _ = hip.labelmap_ordered(L, T, N, M, rows, cols, range(M), dtype=torch.int8)
        assert dict(hit) == {"ordered.back_one_word": 1}, dict(hit)      # the switch is live
        assert torch.equal(got, want), shape


# ---- 2. exact cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.EXACT, ids=str)
def test_exact_dyadic_case_equals_the_plain_loops_on_the_device(hip, shape):
    T, N, M, rows, cols = shape
    L = dr.exact_rows(T, N, M)
    probs = dr.probabilities(L.numpy(), T, N, M, rows, cols)
    for order in (tuple(range(M)), tuple(range(M - 1, -1, -1))):
        want, _ = od.decode(probs, order)
        for dtype in DTYPES:
            for flip in (False, True):
                lab, _ = hip.labelmap_ordered(L.cuda(), T, N, M, rows, cols, order, flip=flip, dtype=dtype)
                assert np.array_equal(unflip(lab.cpu(), flip).numpy().astype(np.int64), want)  # outright, the exact ties included


# ---- 3. the confidence is the dense kernel's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dr.KINDS)
def test_conf_is_the_dense_kernel_s_bit_for_bit(hip, kind):
    for shape, order in ((WIDE, (3, 0, 5)), ((4, 3, 16, 9, 130), tuple(range(16))), ((8, 8, 4, 5, 3), (1, 0)), (dr.SLAB, tuple(range(6)))):
        T, N, M, rows, cols = shape
        L = dr.reference(shape)[0].cuda()
        for flip in (False, True):
            lab, conf = hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence=kind, flip=flip)
            only, _ = hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip)
            _, want = hip.labelmap_dense(L, T, N, M, rows, cols, confidence=kind, flip=flip)
            assert torch.equal(conf.view(torch.int32), want.view(torch.int32)) and torch.equal(lab, only)


# ---- 4. windows over a poisoned workspace -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cols", [29, 61, 130])
def test_column_windows_of_a_wider_map_over_a_poisoned_workspace(hip, cols, dtype):
    T, N, M, rows = 9, 12, 6, 50
    L = dr.dirichlet_rows(T, N, M, seed=3).cuda()
    order = (0, 2, 1, 5)
    need = hip.labelmap_ordered_workspace(1, rows, cols)
    for flip in (False, True):
        lab, conf = hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence="margin", dtype=dtype, flip=flip)
        if flip:
            plain = hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence="margin", dtype=dtype)
            assert torch.equal(lab, torch.flip(plain[0], (1,))) and torch.equal(conf, torch.flip(plain[1], (1,)))
        for a, poison in ((0, 0xFF), (1, 0x00), (3, 0xFF), (5, 0x00)):
            ws = torch.full((need + 64,), poison, dtype=torch.uint8, device="cuda")
            wide = torch.full((rows, cols + 7), -7, dtype=dtype, device="cuda")
            widec = torch.full((rows, cols + 7), -7.0, device="cuda")
            out, outc = hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence="margin", dtype=dtype, flip=flip,
                                             out=wide[:, a:a + cols], out_conf=widec[:, a:a + cols], workspace=ws)
            assert out.data_ptr() == wide[:, a:].data_ptr() and outc.data_ptr() == widec[:, a:].data_ptr()
            for m, want in ((wide, lab), (widec, conf)):
                assert torch.equal(m[:, a:a + cols], want)
                assert (m[:, :a] == -7).all() and (m[:, a + cols:] == -7).all()
            assert (ws[need:] == poison).all()  # nothing behind the workspace's size is written
            # labels alone, at a pitch that is no multiple of 4, over the other poison
            odd = torch.full((rows, cols + 6), -7, dtype=dtype, device="cuda")
            hip.labelmap_ordered(L, T, N, M, rows, cols, order, dtype=dtype, flip=flip, out=odd[:, a:a + cols],
                                 workspace=torch.full((need,), 0xFF - poison, dtype=torch.uint8, device="cuda"))
            assert torch.equal(odd[:, a:a + cols], lab) and (odd[:, :a] == -7).all() and (odd[:, a + cols:] == -7).all()
    with pytest.raises(ValueError):
        hip.labelmap_ordered(L, T, N, M, rows, cols, order, out=torch.zeros(rows, 2 * cols, device="cuda")[:, ::2])


# ---- 5. batch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [3, 5])
@pytest.mark.parametrize("shape", [(5, 7, 3, 37, 61), (9, 12, 6, 50, 300), (4, 3, 16, 19, 29)], ids=str)
def test_batch_kernel_equals_the_one_map_kernel_per_configuration(hip, shape, G):
    T, N, M, rows, cols = shape
    L = torch.stack([dr.dirichlet_rows(T, N, M, seed=10 + g) for g in range(G)]).cuda()
    order = tuple(range(M - 1, -1, -2))
    for dtype in DTYPES:
        for flip in (False, True):
            lab, conf = hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, confidence="entropy", flip=flip, dtype=dtype)
            assert lab.shape == (G, rows, cols) and lab.dtype == dtype
            for g in range(G):
                one, onec = hip.labelmap_ordered(L[g], T, N, M, rows, cols, order, confidence="entropy", flip=flip, dtype=dtype)
                assert torch.equal(lab[g], one) and torch.equal(conf[g].view(torch.int32), onec.view(torch.int32))
    wide = torch.full((G, rows, cols + 5), -7, dtype=torch.int8, device="cuda")
    hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, out=wide[:, :, 3:3 + cols])
    want, _ = hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order)
    assert torch.equal(wide[:, :, 3:3 + cols], want) and (wide[:, :, :3] == -7).all() and (wide[:, :, 3 + cols:] == -7).all()


# ---- 6. status codes ------------------------------------------------------------------------------------------------------------------
def test_kernel_argument_errors_launch_nothing(hip):
    lib = hip.lib()
    L = torch.full((16, 4), 0.25, device="cuda")
    out = torch.zeros(8, 8, device="cuda")
    need = lib.crw_labelmap_ordered_workspace(1, 8, 8)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(order, S=None, M=4, ws_ptr=ws.data_ptr(), ws_bytes=need):
        arr = (ctypes.c_int * len(order))(*order)
        return lib.crw_labelmap_ordered(L.data_ptr(), 4, 4, M, 8, 8, 0, arr, len(order) if S is None else S, -1, out.data_ptr(), 0, None, 8,
                                        ws_ptr, ws_bytes, None)

    for order, kw in (((0, 1, 1), {}), ((0, 4), {}), ((-1, 0), {}), ((0, 1), dict(S=1)), ((0, 1, 2), dict(M=2)), ((0, 1), dict(ws_ptr=None))):
        assert call(order, **kw) == hip.CRW_EINVAL, (order, kw)
    assert call((0, 1), ws_bytes=need - 1) == hip.CRW_EWORKSPACE
    with pytest.raises(hip.CrwError) as e:
        hip.labelmap_ordered(L, 4, 4, 4, 8, 8, (0, 1), out=out, workspace=ws[:need - 2])
    assert e.value.status == hip.CRW_EWORKSPACE
    torch.cuda.synchronize()
    assert not out.any() and not ws.any()
    assert call((0, 1)) == hip.CRW_OK


# ---- 7. the quality claim, first case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", od.SEEDS)
def test_ordered_map_on_layered_items_with_wrong_nodes_on_the_device(hip, seed):
    case = od.QUALITY[0]
    T, N, rows, cols, temp, M, share = case
    gt, L = od.layered_case(*case, seed)
    L = torch.tensor(L).cuda()
    dense, _ = hip.labelmap_dense(L, T, N, M, rows, cols)
    lab, _ = hip.labelmap_ordered(L, T, N, M, rows, cols, range(M))
    od.check_quality(gt, dense.cpu().numpy(), lab.cpu().numpy(), M, f"gpu {case} seed {seed}")
    od.check(dr.probabilities(L.cpu().numpy(), T, N, M, rows, cols), lab.cpu().numpy(), range(M), what=f"gpu {case} seed {seed}")


# ---- 8. segment / segment_sweep / the command line ------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", ["rule", "confidence"])
def test_segment_ordered_is_the_hand_assembled_map(hip, monkeypatch, merge):
    import inference as crw_inference
    import utils as crw_utils
    enc, fresh, seg, lp, N = e2e_case(0, n_rg=2, H=100)
    forced = [6, None]
    order = (0, 1, 2, 3, 4)
    T, W = T_E2E, PATCH[1]
    rg_len, rows, rg_h = T * W, seg.shape[0], N * 8 + 8
    args = (seg, enc, lp, M_E2E, T, PATCH, OVERLAP)
    kw = dict(correction=True, use_last=True, dataset_id=3, confidence="maxprob", merge=merge, upsample="bilinear")

    def segment(**more):
        monkeypatch.setattr(crw_inference, "propagate", forced_propagate(forced))
        return crw_inference.segment(fresh(), *args, **kw, **more)

    plain, out = segment(), segment(decode="ordered", order=order)
    assert set(out) == set(plain) | {"decode", "order"} and out["order"] == list(order) and out["change_idx"] == forced
    assert torch.equal(out["forward_conf"], plain["forward_conf"])  # the confidence does not depend on the decode

    ds, segd = fresh(), seg.cuda()
    soft = lambda seq, ref, last: crw_utils.propagate(seq.cuda(), ref, enc, lp, M_E2E, False, last, soft=True)[-1]
    ordered = lambda L, frames, cols: hip.labelmap_ordered(L, frames, N, M_E2E, rows, cols, order, confidence="maxprob")
    fl, fc = [], []
    for t in range(2):
        lab, conf = ordered(soft(ds[t * T], segd[:rg_h, rg_len * t:rg_len * t + W], False), T, rg_len)
        fl.append(lab)
        fc.append(conf)
    small = T - forced[0]
    px = small * W
    tail = ordered(soft(ds.get_smaller_item(0, small), segd[:, rg_len - px:rg_len - px + W], False), small, px)
    fl[0][:, rg_len - px:], fc[0][:, rg_len - px:] = tail
    fwd, fconf = torch.cat(fl, 1), torch.cat(fc, 1)
    assert torch.equal(out["forward"], fwd) and torch.equal(out["forward_conf"], fconf)
    assert (fwd[1:] >= fwd[:-1]).all()  # the guarantee: forward is monotone in order down every column
    rl, rc = [], []
    for t in range(2):
        seq = ds[t * T]
        lab, conf = ordered(soft(seq, torch.flip(segd[:, rg_len * t:rg_len * (t + 1)], (-1,))[:, :W], True), seq.shape[0], rg_len)
        rl.append(torch.flip(lab, (-1,)))
        rc.append(torch.flip(conf, (-1,)))
    rev, rconf = torch.cat(rl, 1), torch.cat(rc, 1)
    take = rconf > fconf if merge == "confidence" else crw_inference._reverse_rule_mask(fwd, rev, 3).view_as(fwd)
    assert torch.equal(out["pred"], torch.where(take, rev, fwd)) and torch.equal(out["conf"], torch.where(take, rconf, fconf))


def test_segment_sweep_ordered_equals_segment_per_configuration(hip, monkeypatch):
    from imported.labelprop import LabelPropSweep
    from test_sweep_dense_gpu import sweep_against_segment
    enc, fresh, seg, _, _ = e2e_case(0, n_rg=2, H=100)
    sweep = LabelPropSweep(6, [6, 4], [0.1], [8, 5])
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cuda", confidence="margin", merge="confidence", upsample="bilinear",
              decode="ordered", order=(0, 1, 2, 4))
    out = sweep_against_segment(monkeypatch, fresh, (seg, enc, M_E2E, T_E2E, PATCH, OVERLAP), sweep, kw, [6, None])
    assert out["decode"] == "ordered" and out["order"] == [0, 1, 2, 4] and out["change_idx"] == [6, None]
    assert not (out["forward"] == 3).any() and len({m.cpu().numpy().tobytes() for m in out["forward"]}) > 1


def test_cli_with_decode_in_a_child_process(hip, tmp_path):
    H, W, T = 100, 2 * 16 * 10, 10
    js = tmp_path / "report.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_all.py"), "--synthetic", str(H), str(W), "--dataset", "0",
                        "--model", "0", "--seq_length", str(T), "-c", "6", "-r", "6", "-k", "8", "--output_folder",
                        str(tmp_path / "out") + "/", "--report_json", str(js), "--upsample", "bilinear", "--decode", "ordered", "--order",
                        "0", "1", "2", "3", "--horizons", "--min_run", "1"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(js.read_text())
    assert d["upsample"] == "bilinear" and d["decode"] == "ordered" and d["order"] == [0, 1, 2, 3] and "horizons" in d
    assert "decode='ordered'" in r.stdout
    saved = torch.load(tmp_path / "out" / "predicted_map.pt", map_location="cpu").long()
    assert list(saved.shape) == d["map_shape"] and (saved[1:] >= saved[:-1]).all()
