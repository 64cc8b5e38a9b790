"""GPU side of the layer horizons: the HIP kernel `crw_horizons` (csrc/horizons.hip) through `crw_hip.horizons` against the literal
reference tests/horizons_ref.py on the case table of tests/test_horizons.py -- every integer exact -- then column windows, stale
memory, repeatability, the status codes, `inference.horizons` / `horizons_sweep` and the two command lines.  Invalid labels are data
the kernel counts; windows lie inside their allocations -- nothing here provokes a fault."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from horizons_ref import check_invariants, compare, horizons_ref
from test_horizons import CASES, build, case_id, layered

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_horizons()
    return crw_hip


def host(res):
    return [None if t is None else t.cpu().numpy() for t in res]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_equals_the_reference(hip, case):
    gt, pred, aux, kw, ref = build(case[:7])
    K, slabs = case[3], case[7]
    dev = lambda t: None if t is None else t.cuda()
    g, p, a = dev(gt), dev(pred), dev(aux)
    got = hip.horizons(g, p, K, aux=a, want_picks=True, row_slabs=slabs, **kw)
    assert got[0].is_cuda and got[0].dtype == torch.int64 and got[2].dtype == torch.int32 and tuple(got[2].shape) == (2, 3, K, gt.shape[1])
    assert compare(host(got), ref) == []
    check_invariants(*host(got), gt.shape[0], gt.shape[1], K, kw["min_run"])
    mask = {k: v for k, v in kw.items() if k.startswith("ignore")}
    assert torch.equal(got[1], hip.confusion(g, p, K, aux=a, **mask)[1])
    # without picks: the same statistics; again: the same bits
    two = hip.horizons(g, p, K, aux=a, row_slabs=slabs, **kw)
    again = hip.horizons(g, p, K, aux=a, want_picks=True, row_slabs=slabs, **kw)
    assert len(two) == 2 and torch.equal(two[0], got[0]) and torch.equal(two[1], got[1])
    assert all(torch.equal(x, y) for x, y in zip(got, again))


@pytest.mark.parametrize("dt", [(torch.float32, torch.float32, None), (torch.float32, torch.int8, torch.int8), (torch.int8, torch.int8, torch.float32)],
                         ids=["f32-f32", "f32-i8-i8", "i8-i8-f32"])
@pytest.mark.parametrize("slabs", [0, 3])
def test_column_windows_of_wider_maps(hip, dt, slabs):
    """Operands are [rows, a:b] slices with odd a of wider tensors (read in place: one pitch, no copy); the picks go into a slice
    of a larger tensor whose other elements stay as they were."""
    rows, width, K, a0, b0 = 70, 333, 6, 7, 7 + 193
    gt, pr = layered(rows, width, K, 4)
    gt[rows // 2, 11] = np.nan if dt[0] == torch.float32 else K  # one invalid label inside the window, one outside
    gt[3, 2] = -1
    aux = np.where(np.random.default_rng(1).random(gt.shape) < 0.03, 9.0, 0.0)
    G, P = torch.from_numpy(gt).to(dt[0]).cuda(), torch.from_numpy(pr).to(dt[1]).cuda()
    A = None if dt[2] is None else torch.from_numpy(aux).to(dt[2]).cuda()
    kw = dict(min_run=3, tol=2, **({} if A is None else dict(ignore_aux=9)))
    ref = horizons_ref(G[:, a0:b0].cpu().numpy(), P[:, a0:b0].cpu().numpy(), K, None if A is None else A[:, a0:b0].cpu().numpy(), **kw)
    big = torch.full((5 + 2 * 3 * K * (b0 - a0) + 9,), -77, dtype=torch.int32, device="cuda")
    out = big[5:5 + 2 * 3 * K * (b0 - a0)].view(2, 3, K, b0 - a0)
    before = P.clone()
    got = hip.horizons(G[:, a0:b0], P[:, a0:b0], K, aux=None if A is None else A[:, a0:b0], row_slabs=slabs, picks_out=out, **kw)
    assert got[2].data_ptr() == out.data_ptr() and compare(host(got), ref) == []
    assert (big[:5] == -77).all() and (big[5 + out.numel():] == -77).all()
    assert torch.equal(P, before) and int(ref[1][1]) == 1
    # operands of differing pitch take the copying route: same integers
    mixed = hip.horizons(G[:, a0:b0], P[:, a0:b0].contiguous(), K, aux=None if A is None else A[:, a0:b0], row_slabs=slabs, want_picks=True, **kw)
    assert compare(host(mixed), ref) == []


def _raw_call(hip, g, p, K, rows, cols, ld, fill, picks=True, ws_short=0, over=()):
    """crw_horizons through ctypes with outputs and workspace pre-filled with `fill` -> (status, stats, dropped, picks)."""
    L = hip.lib()
    nbytes = L.crw_horizons_ws_bytes(rows, cols, K)
    out = torch.full((K * 18 + 2,), fill, dtype=torch.uint8, device="cuda").repeat_interleave(8).view(torch.int64).clone()
    pk = torch.full((2 * 3 * K * max(cols, 1) * 4,), fill, dtype=torch.uint8, device="cuda").view(torch.int32)
    ws = torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device="cuda")
    a = dict(gt=hip._ptr(g), gt_dtype=0 if g.dtype == torch.float32 else 1, pred=hip._ptr(p), pred_dtype=0 if p.dtype == torch.float32 else 1,
             aux=None, aux_dtype=1, rows=rows, cols=cols, ld=ld, K=K, ig=-1, ip=-1, ia=-1, min_run=3, tol=2, row_slabs=0,
             picks=hip._ptr(pk) if picks else None, stats=hip._ptr(out), dropped=ctypes.c_void_p(out.data_ptr() + 8 * K * 18), ws=hip._ptr(ws),
             ws_bytes=nbytes - ws_short, stream=hip._stream())
    a.update(dict(over))
    st = L.crw_horizons(*a.values())
    torch.cuda.synchronize()
    return st, out[:K * 18].view(K, 18).cpu().numpy(), out[K * 18:].cpu().numpy(), pk[:2 * 3 * K * cols].view(2, 3, K, cols).cpu().numpy()


def test_stale_memory_and_status_codes(hip):
    rows, cols, K = 70, 257, 6
    gt, pr = layered(rows, cols, K, 9)
    g, p = torch.from_numpy(gt).float().cuda(), torch.from_numpy(pr).to(torch.int8).cuda()
    ref = horizons_ref(g.cpu().numpy(), p.cpu().numpy(), K, min_run=3)
    ones = _raw_call(hip, g, p, K, rows, cols, cols, 0xFF)
    zeros = _raw_call(hip, g, p, K, rows, cols, cols, 0x00)
    assert ones[0] == zeros[0] == hip.CRW_OK
    assert compare(ones[1:], ref) == [] and compare(zeros[1:], ref) == []
    nopicks = _raw_call(hip, g, p, K, rows, cols, cols, 0xFF, picks=False)
    assert nopicks[0] == hip.CRW_OK and compare(nopicks[1:3] + (None,), ref) == [] and (nopicks[3] == -1).all()  # untouched 0xFF
    einval = [dict(K=1), dict(K=17), dict(min_run=0), dict(tol=-1), dict(row_slabs=9), dict(row_slabs=-1), dict(ld=cols - 1), dict(rows=32769),
              dict(stats=None), dict(dropped=None), dict(ig=-2), dict(ia=3), dict(gt=None), dict(gt_dtype=2), dict(ws=None)]
    for over in einval:
        assert _raw_call(hip, g, p, K, rows, cols, cols, 0, over=over)[0] == hip.CRW_EINVAL, over
    assert _raw_call(hip, g, p, K, rows, cols, cols, 0, ws_short=1)[0] == hip.CRW_EWORKSPACE
    assert hip.lib().crw_horizons_ws_bytes(rows, cols, 17) == 0 and hip.lib().crw_horizons_ws_bytes(32769, cols, K) == 0
    assert hip.lib().crw_horizons_ws_bytes(rows, cols, K) == -(-(5 * (K * 18 + 2) * 8) // 16) * 16
    # and through the binding
    with pytest.raises(ValueError):
        hip.horizons(g, p, K, row_slabs=9)
    with pytest.raises(ValueError):
        hip.horizons(g.cpu(), p, K)


def test_inference_horizons_and_sweep(hip):
    import inference as crw_inference
    rows, cols, K = 70, 257, 6
    maps = [torch.from_numpy(layered(rows, cols, K, s)[1]).to(torch.int8).cuda() for s in (1, 2, 3)]
    seg = torch.from_numpy(layered(rows, cols + 40, K, 1, speckle=0.0)[0]).float()  # wider: cut to the map's columns, as the drivers do
    one = [crw_inference.horizons(m, seg[:, :cols], 1, nclasses=K, min_run=3, want_picks=True) for m in maps]
    for (hz, picks), m in zip(one, maps):
        ref = horizons_ref(seg[:, :cols].numpy(), m.cpu().numpy(), K, ignore_gt=5, ignore_pred=5, min_run=3)
        assert compare((hz.stats, np.array(hz.dropped), picks.cpu().numpy()), ref) == [] and picks.is_cuda
        rep = crw_inference.evaluate(m, seg[:, :cols], 1, nclasses=K)
        assert tuple(rep.dropped) == hz.dropped and hz.dropped[0] > 0
    sweep = crw_inference.horizons_sweep(torch.stack(maps), seg[:, :cols], 1, nclasses=K, min_run=3)
    assert len(sweep) == 3
    for s, (hz, _) in zip(sweep, one):
        assert np.array_equal(s.stats, hz.stats) and s.dropped == hz.dropped and s.mean_mae("top") == hz.mean_mae("top")
    # dataset 0: the uncertain map is the aux operand
    unc = torch.where(torch.rand(rows, cols) < 0.05, 4.0, 0.0)
    hz0 = crw_inference.horizons(maps[0].clamp(max=3), seg[:, :cols].clamp(max=3), 0, unc_seg=unc, min_run=2)
    ref = horizons_ref(seg[:, :cols].clamp(max=3).numpy(), maps[0].clamp(max=3).cpu().numpy(), 4, unc.numpy(), ignore_aux=4, min_run=2)
    assert compare((hz0.stats, np.array(hz0.dropped), None), ref) == []
    # (e) a surviving invalid label raises
    for bad_value, dtype in ((float("nan"), torch.float32), (2.5, torch.float32), (float(K), torch.float32), (-1.0, torch.float32), (K, torch.int8),
                             (-1, torch.int8)):
        bad = maps[0].to(dtype).clone()
        bad[rows // 2, 100] = bad_value
        with pytest.raises(hip.LabelError):
            crw_inference.horizons(bad, seg[:, :cols], 3, nclasses=K)
        with pytest.raises(hip.LabelError):
            crw_inference.horizons_sweep(torch.stack([maps[1].to(dtype), bad]), seg[:, :cols], 3, nclasses=K)


def test_segment_all_with_horizons_in_a_child_process(hip, tmp_path):
    js = tmp_path / "report.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_all.py"), "--synthetic", "200", "4800", "--dataset", "0",
                        "--horizons", "--save_horizons", "--output_folder", str(tmp_path / "out") + "/", "--report_json", str(js)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(js.read_text())
    h = d["horizons"]
    rows, cols = d["map_shape"]
    n = np.array(h["n_both"]) + np.array(h["n_missing"]) + np.array(h["n_spurious"])
    assert (h["rows"], h["cols"], h["K"], h["min_run"], h["tol"]) == (rows, cols, 4, 3, 2) and (n <= cols).all() and n.max() > 0
    assert h["dropped"] == d["dropped"]
    assert "Horizons (min_run 3, tol 2 rows, distances in rows):" in r.stdout and "thickness" in r.stdout
    assert r.stdout.index("Horizons (") > r.stdout.index("Computing reports")
    picks = torch.load(tmp_path / "out" / "horizons.pt", map_location="cpu")
    assert picks.dtype == torch.int32 and tuple(picks.shape) == (2, 3, 4, cols)
    assert [int(v) for v in ((picks[0, 2] > 0) & (picks[1, 2] > 0)).sum(1)] == h["n_both"]


def test_segment_sweep_selects_by_horizon_mae_in_a_child_process(hip, tmp_path):
    js = tmp_path / "sweep.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_sweep.py"), "--synthetic", "200", "4800", "--dataset", "0",
                        "-r", "5", "10", "-t", "0.1", "-k", "5", "10", "--horizons", "--select", "horizon_mae", "--output_folder",
                        str(tmp_path / "out") + "/", "--report_json", str(js)], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(js.read_text())
    assert "Best by horizon_mae: radius" in r.stdout and "horizon mae" in r.stdout and d["select"] == "horizon_mae"
    scores = [c["horizons"]["top"]["mean_mae"] for c in d["configs"]]
    assert len(scores) == 4 and [c["score"] for c in d["configs"]] == scores
    real = [s for s in scores if s == s]
    assert d["best"]["score"] == min(real) and d["best"]["index"] == scores.index(min(real))
