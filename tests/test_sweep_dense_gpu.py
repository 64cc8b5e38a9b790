"""GPU side of the sweep's bilinear maps, confidence and calibration: the kernel of `crw_labelmap_dense_batch` against
`crw_labelmap_dense` per configuration, bit for bit (both instantiate one device function for a pixel's arithmetic, so a
difference is a bug, not rounding), column windows whose store phase changes per row and per configuration, the status codes, the
soft outputs of `utils.propagate_sweep` against `utils.propagate`, `inference.segment_sweep` with every option on against
`inference.segment` per configuration, `calibration_sweep`, and the command line.  The one-map kernel is itself held to the fp64
helper in test_dense_gpu.py; nothing here has a counterpart in the reference.  Nothing here provokes a fault."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dense_ref as dr
from conftest import PKG, ROOT, load_golden
from test_sweep_dense import OUTPUTS, distinct_soft_labels

pytestmark = pytest.mark.gpu

KINDS = (None,) + dr.KINDS
DTYPES = (torch.float32, torch.int8)
# (T, N, M, rows, cols): odd sizes in one tile; across a 256-column tile, several row tiles; M = 16; the smallest
SHAPES = [(5, 7, 3, 37, 61), (9, 12, 6, 50, 300), (4, 3, 16, 19, 29), (1, 1, 2, 5, 9)]


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_dense() and crw_hip.has_dense_batch() and crw_hip.has_sweep()
    return crw_hip


# ---- 1. the batch against the one-map kernel, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_batch_kernel_equals_the_one_map_kernel_per_configuration(hip, shape, G):
    T, N, M, rows, cols = shape
    L = distinct_soft_labels(G, T, N, M, seed=G).cuda()
    for kind in KINDS:
        for dtype in DTYPES:
            for flip in (False, True):
                lab, conf = hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, confidence=kind, flip=flip, dtype=dtype)
                assert lab.is_cuda and lab.shape == (G, rows, cols) and lab.dtype == dtype and (conf is None) == (kind is None)
                for g in range(G):
                    one, onec = hip.labelmap_dense(L[g], T, N, M, rows, cols, confidence=kind, flip=flip, dtype=dtype)
                    assert torch.equal(lab[g], one), (kind, dtype, flip, g)
                    if kind:
                        assert torch.equal(conf[g].view(torch.int32), onec.view(torch.int32)), (kind, dtype, flip, g)  # bitwise
    if G > 1 and rows * cols > 50:
        assert len({c.cpu().numpy().tobytes() for c in conf}) == G  # the slices are not all equal


@pytest.mark.parametrize("chunk", ["1", "2", "100"])
def test_every_kernel_shape_writes_the_same_maps(hip, monkeypatch, chunk):
    """CRW_DENSE_BATCH_CHUNK (read per call): one configuration per blockIdx.z, an uneven last chunk, one chunk for all."""
    G, (T, N, M, rows, cols) = 7, SHAPES[1]
    L = distinct_soft_labels(G, T, N, M, seed=2).cuda()
    monkeypatch.delenv("CRW_DENSE_BATCH_CHUNK", raising=False)
    with hip.routes() as hit:
        want = hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, confidence="entropy", flip=True)
    assert dict(hit) == {"dense.batch_chunked": 1}, dict(hit)       # the default: four configurations per workgroup
    monkeypatch.setenv("CRW_DENSE_BATCH_CHUNK", chunk)
    with hip.routes() as hit:
        got = hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, confidence="entropy", flip=True)
    assert dict(hit) == {("dense.batch_chunk1" if chunk == "1" else "dense.batch_chunked"): 1}, dict(hit)   # the switch is live
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


# ---- 2. windows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cols", [29, 61])
def test_column_windows_whose_store_phase_changes_per_row_and_configuration(hip, cols, dtype):
    G, T, N, M, rows, width = 3, 9, 12, 6, 19, 71
    assert width % 2 == 1 and (rows * width) % 4 != 0
    L = distinct_soft_labels(G, T, N, M, seed=9).cuda()
    for flip in (False, True):
        for a in (0, 1, 2, 3):
            maps = torch.full((G, rows, width), -7, dtype=dtype, device="cuda")
            cmaps = torch.full((G, rows, width), -7.0, device="cuda")
            want, wantc = maps.clone(), cmaps.clone()
            out, outc = hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, confidence="margin", flip=flip, dtype=dtype,
                                                 out=maps[:, :, a:a + cols], out_conf=cmaps[:, :, a:a + cols])
            assert out.data_ptr() == maps[:, :, a:].data_ptr() and outc.data_ptr() == cmaps[:, :, a:].data_ptr()
            for g in range(G):  # the per-configuration call into the same window of a map filled with the same sentinel
                hip.labelmap_dense(L[g], T, N, M, rows, cols, confidence="margin", flip=flip, dtype=dtype,
                                   out=want[g, :, a:a + cols], out_conf=wantc[g, :, a:a + cols])
            assert torch.equal(maps, want) and torch.equal(cmaps.view(torch.int32), wantc.view(torch.int32))
            for m in (maps, cmaps):
                assert (m[:, :, :a] == -7).all() and (m[:, :, a + cols:] == -7).all() and not (m[:, :, a:a + cols] == -7).any()
            # labels alone; and a confidence map whose 16-byte phase is not the labels' (single stores, the same values)
            only = torch.full((G, rows, width), -7, dtype=dtype, device="cuda")
            hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, flip=flip, dtype=dtype, out=only[:, :, a:a + cols])
            assert torch.equal(only, want)
            shifted = torch.full((G, rows, width), -7.0, device="cuda")
            b = (a + 1) % 4
            hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, confidence="margin", flip=flip, dtype=dtype,
                                     out=only[:, :, a:a + cols], out_conf=shifted[:, :, b:b + cols])
            assert torch.equal(shifted[:, :, b:b + cols], wantc[:, :, a:a + cols]) and torch.equal(only, want)
            assert (shifted[:, :, :b] == -7).all() and (shifted[:, :, b + cols:] == -7).all()
    with pytest.raises(ValueError):
        hip.labelmap_dense_batch(L, G, T, N, M, rows, cols, dtype=dtype, out=torch.zeros(G, rows, 2 * cols, dtype=dtype, device="cuda")[:, :, ::2])


def test_batch_kernel_status_codes(hip):
    lib = hip.lib()
    G, T, N, M, rows, cols = 3, 4, 3, 3, 8, 8
    L = torch.full((G, T * N, M), 1 / 3, device="cuda")
    out = torch.zeros(G, rows, cols, device="cuda")
    conf = torch.zeros(G, rows, cols, device="cuda")
    call = lambda G=G, M=M, kind=-1, conf=None, ld=cols, ms=rows * cols: lib.crw_labelmap_dense_batch(
        L.data_ptr(), G, T, N, M, rows, cols, 0, kind, out.data_ptr(), 0, conf, ld, ms, None)
    for bad in (dict(G=0), dict(ms=rows * cols - 1), dict(ld=cols + 1, ms=(rows - 1) * (cols + 1) + cols - 1), dict(kind=0),
                dict(conf=conf.data_ptr()), dict(M=17), dict(G=65536), dict(kind=3, conf=conf.data_ptr())):
        assert call(**bad) == hip.CRW_EINVAL, bad
    torch.cuda.synchronize()
    assert not out.any() and not conf.any()
    assert call() == hip.CRW_OK and call(kind=1, conf=conf.data_ptr()) == hip.CRW_OK
    torch.cuda.synchronize()
    assert (out == 0).all() and (conf == 0).all()  # uniform rows: class 0 on the tie, margin 0 -- and a clean launch


# ---- 3. the soft outputs of the sweep -----------------------------------------------------------------------------------------------
class _Flatten(torch.nn.Module):
    def forward(self, x):
        return x.flatten(1)


def _layered_item(T, N, C, seed):
    """An item [T, N, h, w] with h * w = C whose flattened patches are layered features (neighbouring nodes alike, frames drift)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, N, C, generator=g).cumsum(1) / 3
    return (base + 0.5 * torch.randn(T, N, C, generator=g).cumsum(0) / 4).float().reshape(T, N, C // 4, 4)


@pytest.mark.parametrize("T,N,C,M,cxt,radii,temps,knns", [
    (30, 20, 32, 3, 6, (4,), (0.05,), (3, 7)),                 # the vector kernel, one (radius, temp)
    (40, 48, 128, 4, 20, (8, 12), (0.1, 0.01), (10, 20))])    # the matrix-core path, a 2 x 2 x 2 grid
def test_propagate_sweep_soft_outputs_equal_propagate_per_configuration(hip, T, N, C, M, cxt, radii, temps, knns):
    import utils as crw_utils
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    seq = _layered_item(T, N, C, 3 + N).cuda()
    seg_ref = (torch.arange(4 * N) * M // (4 * N)).float()[:, None].repeat(1, 4).cuda()
    sweep = LabelPropSweep(cxt, radii, temps, knns)
    G = len(sweep.configs)
    plain = crw_utils.propagate_sweep(seq, seg_ref, _Flatten(), sweep, M, False, False)
    assert len(plain) == 3
    for kind in dr.KINDS:
        pred, xent, change, conf, L = crw_utils.propagate_sweep(seq, seg_ref, _Flatten(), sweep, M, False, False, confidence=kind, soft=True)
        assert pred.shape == conf.shape == (G, N, T) and L.shape == (G, T * N, M) and L.is_cuda and conf.dtype == L.dtype == torch.float32
        assert torch.equal(pred, plain[0]) and torch.equal(xent, plain[1]) and change == plain[2]
        for g, cfg in enumerate(sweep.configs):
            p1, x1, c1, conf1, L1 = crw_utils.propagate(seq, seg_ref, _Flatten(), LabelPropVOS_CRW(cfg), M, False, False, confidence=kind, soft=True)
            assert torch.equal(L[g].view(torch.int32), L1.view(torch.int32)), (kind, cfg)
            assert torch.equal(conf[g].view(torch.int32), conf1.view(torch.int32)) and torch.equal(pred[g], p1), (kind, cfg)
            assert c1 == change and torch.equal(x1, xent)
        assert (conf[:, :, 0] == 1).all()
    assert G == 1 or len({l.cpu().numpy().tobytes() for l in L}) > 1
    one = crw_utils.propagate_sweep(seq[:1], seg_ref, _Flatten(), sweep, M, False, False, confidence="margin", soft=True)
    assert one[0].shape == (G, N, 1) and (one[3] == 1).all() and one[3].is_cuda and one[4].shape == (G, N, M)
    assert torch.equal(one[4].argmax(-1).float(), one[0][:, :, 0])


def test_soft_outputs_with_the_per_config_switch_in_a_child_process():
    """CRW_SWEEP_PER_CONFIG=1: `propagate_all(soft=True)` stacks the per-configuration soft labels behind the same interface."""
    env = dict(os.environ, CRW_SWEEP_PER_CONFIG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_sweep_dense_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-k", "propagate_sweep_soft_outputs_equal", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


# ---- 4. segment_sweep with every option on ------------------------------------------------------------------------------------------
def force(fn, changes):
    """`fn` (`propagate` or `propagate_sweep`, any tuple length) with the change points forced, call by call."""
    n = {"i": 0}

    def wrapped(*a, **k):
        out = fn(*a, **k)
        i = n["i"]
        n["i"] += 1
        return out[:2] + (changes[i],) + out[3:] if i < len(changes) else out
    return wrapped


def sweep_against_segment(monkeypatch, fresh, args, sweep, kw, changes):
    """One `segment_sweep` and G `segment`s on fresh datasets, same options -> the sweep's dict after comparing all four outputs."""
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    seg, enc, M, T, patch, overlap = args
    monkeypatch.setattr(crw_inference, "propagate_sweep", force(crw_utils.propagate_sweep, changes))
    out = crw_inference.segment_sweep(fresh(), seg, enc, sweep, M, T, patch, overlap, **kw)
    G = len(sweep.configs)
    for k in OUTPUTS:
        assert out[k].is_cuda and out[k].shape[0] == G and out[k].dtype == (torch.float32 if "conf" in k else torch.int8)
    for g, cfg in enumerate(sweep.configs):
        monkeypatch.setattr(crw_inference, "propagate", force(crw_utils.propagate, changes))
        one = crw_inference.segment(fresh(), seg, enc, LabelPropVOS_CRW(cfg), M, T, patch, overlap, **kw)
        assert one["change_idx"] == out["change_idx"], cfg
        for k in ("pred", "forward"):
            assert torch.equal(out[k][g], one[k].to(torch.int8)), (cfg, k)
        for k in ("conf", "forward_conf"):
            assert torch.equal(out[k][g].view(torch.int32), one[k].view(torch.int32)), (cfg, k)
    return out


@pytest.mark.parametrize("merge", ["rule", "confidence"])
@pytest.mark.parametrize("name", ["segment_ds0_correction", "segment_ds3_correction_reverse"])
def test_segment_sweep_with_all_options_equals_segment_per_configuration(hip, monkeypatch, name, merge):
    from test_sweep import build_case, grid_around
    g = load_golden(name)
    sweep = grid_around(g)
    _, seg, ncls, T, patch, overlap, changes, kw = build_case(g, "cuda")
    kw.update(upsample="bilinear", confidence="maxprob", merge=merge)
    out = sweep_against_segment(monkeypatch, lambda: build_case(g, "cuda")[0], (seg, _Flatten(), ncls, T, patch, overlap), sweep, kw, changes)
    assert len({m.cpu().numpy().tobytes() for m in out["forward_conf"]}) > 1
    assert float(out["forward_conf"].min()) >= 1 / ncls - 1e-6 and float(out["conf"].max()) <= 1


def _cli(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_segment_sweep_and_calibration_sweep_at_a_realistic_geometry(hip, monkeypatch):
    """200 x 1600, 16 x 16 patches, overlap (8, 0), T = 50 (two radargrams of 800 columns), a random-init Resnet in train mode, a
    correction forced on the first radargram, reverse pass merged by confidence, margin, bilinear, a 2 x 2 x 2 grid."""
    import dataset as crw_dataset
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropSweep
    rows, cols, T, patch, overlap, K = 200, 1600, 50, (16, 16), (8, 0), 5
    rg = crw_dataset.synthetic_radargram(rows, cols)
    seg = _cli("segment_all").synthetic_reference(rows, cols, K)
    torch.manual_seed(11)
    enc = crw_utils.create_model(1, False).cuda()
    enc.train(True)
    sweep = LabelPropSweep(20, (5, 10), (0.1, 0.01), (5, 10))
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cuda", confidence="margin", merge="confidence", upsample="bilinear")
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap)
    out = sweep_against_segment(monkeypatch, fresh, (seg, enc, K, T, patch, overlap), sweep, kw, [30, None])
    assert tuple(out["pred"].shape) == (8, rows, cols) and out["change_idx"] == [30, None]
    assert len({p.cpu().numpy().tobytes() for p in out["pred"]}) > 1 and not torch.equal(out["pred"], out["forward"])
    cals = crw_inference.calibration_sweep(out["pred"], out["conf"], seg, 3, nclasses=K, bins=10)
    assert len(cals) == 8
    for g, cal in enumerate(cals):
        one = crw_inference.calibration(out["pred"][g], out["conf"][g], seg, 3, nclasses=K, bins=10)
        assert np.array_equal(cal.count, one.count) and np.array_equal(cal.correct, one.correct) and np.array_equal(cal.conf_sum, one.conf_sum)
        assert cal.dropped == one.dropped == (0, 0, 0) and cal.total == rows * cols and str(cal) == str(one)


# ---- 5. driver --------------------------------------------------------------------------------------------------------------------
def test_cli_with_all_options_in_a_child_process(tmp_path):
    js = tmp_path / "sweep.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_sweep.py"), "--synthetic", "200", "1600", "--dataset", "0",
                        "--seq_length", "50", "-c", "20", "-r", "5", "10", "-t", "0.1", "0.01", "-k", "5", "10", "--use_last", "true",
                        "--correction", "true", "--upsample", "bilinear", "--confidence", "maxprob", "--merge", "confidence",
                        "--select", "aurc", "--report_json", str(js), "--output_folder", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = json.load(open(js))
    assert len(d["configs"]) == 8 and (d["upsample"], d["confidence"], d["merge"], d["select"]) == ("bilinear", "maxprob", "confidence", "aurc")
    unc = _cli("segment_all").synthetic_reference(200, 1600, 4, True)[:, :d["map_shape"][1]]
    unmasked = int((unc != 4).sum())
    assert d["map_shape"][0] == 200 and d["pixels"] == 200 * d["map_shape"][1]
    for c in d["configs"]:
        assert int(np.sum(c["report"]["matrix"])) == unmasked and c["report"]["dropped"] == dict(masked=d["pixels"] - unmasked, invalid=0)
        assert c["calibration"]["total"] == unmasked and c["calibration"]["bins"] == 10 and c["score"] == c["calibration"]["aurc"]
    aurc = [c["calibration"]["aurc"] for c in d["configs"]]
    assert d["best"]["index"] == int(np.argmin(aurc)) and d["best"]["score"] == min(aurc)
    b = d["configs"][d["best"]["index"]]
    assert f"Best by aurc: radius {b['radius']} temp {b['temp']:g} knn {b['knn']}" in r.stdout
    assert "Calibration (maxprob, merge: confidence):" in r.stdout and "upsample='bilinear'" in r.stdout
    assert "ece" in r.stdout and "aurc" in r.stdout
