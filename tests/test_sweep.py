"""Label-propagation sweeps over the (radius, temp, knn) grid of the reference's scripts/launch/launch_test_batch.sh, host side:
`LabelPropSweep.configs`, `inference.segment_sweep` against maps the reference's own scripts/test/test_all.py main(args) produced
once per configuration (fixture sweep_ds3_correction_reverse.npz, tests/golden/make_golden_sweep.py) and against
`inference.segment` run per configuration, `inference.evaluate_sweep` against `evaluate`, the ABI tables and the command line.
The label propagation is the CPU oracle here; the kernels' twins are in test_sweep_gpu.py."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_golden
from oracle import crw_oracle as orc

SEGMENT_CASES = ["segment_ds0_reverse", "segment_ds1_reverse", "segment_ds3_reverse", "segment_ds0_correction",
                 "segment_ds3_correction_reverse"]
SWEEP_FIXTURE = "sweep_ds3_correction_reverse"


class CountingFlatten(torch.nn.Module):
    """The fixtures' encoder (patch pixels are the features) that records the batch shape of every forward call."""

    def __init__(self):
        super().__init__()
        self.shapes = []

    def forward(self, x):
        self.shapes.append(tuple(x.shape))
        return x.flatten(1)


def oracle_propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last):
    T, N = seq.shape[:2]
    emb = model(seq.reshape(T * N, 1, *seq.shape[2:])).reshape(T, N, -1).numpy()
    if use_last:
        emb = emb[::-1].copy()
    pred = orc.labelprop(emb, orc.seed_labels(seg_ref.numpy(), N), ncls, lp.cxt_size, lp.radius, lp.temperature, lp.topk)
    return torch.tensor(pred), torch.tensor(orc.xent_metric(emb)), None


def oracle_propagate_sweep(seq, seg_ref, model, sweep, ncls, do_pos_embed, use_last):
    """Stand-in for `utils.propagate_sweep`: ONE encoder call, then a loop of the oracle over the configurations."""
    T, N = seq.shape[:2]
    emb = model(seq.reshape(T * N, 1, *seq.shape[2:])).reshape(T, N, -1).numpy()
    if use_last:
        emb = emb[::-1].copy()
    seed = orc.seed_labels(seg_ref.numpy(), N)
    pred = np.stack([orc.labelprop(emb, seed, ncls, c["CXT_SIZE"], c["RADIUS"], c["TEMP"], c["KNN"]) for c in sweep.configs])
    return torch.tensor(pred), torch.tensor(orc.xent_metric(emb)), None


def build_case(g, device="cpu"):
    """Dataset (freshly built: `get_smaller_item` shortens it for good), reference map and geometry of a segment_* / sweep_* fixture"""
    import dataset as crw_dataset
    T, patch, overlap = int(g["T"]), tuple(int(v) for v in g["patch"]), tuple(int(v) for v in g["overlap"])
    ds = crw_dataset.RGDataset.from_tensor(torch.tensor(g["rg"]), T, patch, overlap)
    N = ds[0].shape[1]
    seg = torch.tensor(g["seg"])[:N * patch[0]]
    forced = [None if f < 0 else int(f) for f in g["forced_change"]]
    kw = dict(correction=bool(g["correction"]), use_last=bool(g["use_last"]), dataset_id=int(g["dataset_id"]), device=device)
    return ds, seg, int(g["nclasses"]), T, patch, overlap, forced, kw


def force_changes(fn, forced, calls):
    """`fn` (a propagate or a propagate_sweep) with the fixture's change indices forced, call by call, and counted -- as
    tests/test_host.py::run_segment_golden wraps `propagate` and the generator wrapped the reference's."""
    def wrapped(*a, **k):
        pred, xent, change = fn(*a, **k)
        i = calls["n"]
        calls["n"] += 1
        if forced is not None and i < len(forced):
            change = forced[i]
        return pred, xent, change
    return wrapped


def run_sweep(g, sweep, propagate_sweep_fn, device="cpu", encoder=None, force=True):
    """`inference.segment_sweep` on a fixture's inputs -> (out, number of propagate_sweep calls)"""
    import inference as crw_inference
    ds, seg, ncls, T, patch, overlap, forced, kw = build_case(g, device)
    calls = {"n": 0}
    orig = crw_inference.propagate_sweep
    crw_inference.propagate_sweep = force_changes(propagate_sweep_fn, forced if force else None, calls)
    try:
        out = crw_inference.segment_sweep(ds, seg, encoder if encoder is not None else CountingFlatten(), sweep, ncls, T, patch,
                                          overlap, **kw)
    finally:
        crw_inference.propagate_sweep = orig
    return out, calls["n"]


def run_per_config(g, cfg, propagate_fn, device="cpu", encoder=None, force=True):
    """`inference.segment` for ONE configuration on a freshly built dataset -> (out, number of propagate calls)"""
    import inference as crw_inference
    from imported.labelprop import LabelPropVOS_CRW
    ds, seg, ncls, T, patch, overlap, forced, kw = build_case(g, device)
    calls = {"n": 0}
    orig = crw_inference.propagate
    crw_inference.propagate = force_changes(propagate_fn, forced if force else None, calls)
    try:
        out = crw_inference.segment(ds, seg, encoder if encoder is not None else CountingFlatten(), LabelPropVOS_CRW(cfg), ncls, T,
                                    patch, overlap, **kw)
    finally:
        crw_inference.propagate = orig
    return out, calls["n"]


def fixture_sweep(g):
    from imported.labelprop import LabelPropSweep
    return LabelPropSweep(int(g["cxt_size"]), [int(r) for r in g["radii"]], [float(t) for t in g["temps"]], [int(k) for k in g["knns"]])


def check_sweep_golden(g, out):
    """Every configuration's saved map and final map, exactly"""
    G = len(g["saved_maps"])
    assert out["pred"].dtype == torch.int8 and out["forward"].dtype == torch.int8
    assert tuple(out["pred"].shape) == g["final_maps"].shape and tuple(out["forward"].shape) == g["saved_maps"].shape
    assert len(out["configs"]) == G
    for i in range(G):
        assert np.array_equal(out["forward"][i].cpu().numpy(), g["saved_maps"][i]), f"configuration {out['configs'][i]}: saved map"
        assert np.array_equal(out["pred"][i].cpu().numpy(), g["final_maps"][i]), f"configuration {out['configs'][i]}: final map"


def grid_around(g):
    """A 2 x 2 x 2 grid around a segment_* fixture's own parameters"""
    from imported.labelprop import LabelPropSweep
    r, t, k = int(g["radius"]), float(g["temp"]), int(g["knn"])
    return LabelPropSweep(int(g["cxt_size"]), [r, r + 2], [t, t / 10], [k - 2, k])


# ---------------------------------------------------------------------------------------------------------------- 1. the grid
def test_configs_are_the_shell_scripts_three_loops():
    from imported.labelprop import LabelPropSweep
    R, T, K = (45, 50, 55, 60, 65), (0.1, 0.01, 0.001), (15, 20, 25, 30)  # scripts/launch/launch_test_batch.sh
    s = LabelPropSweep(100, R, T, K)
    want = []
    for r in R:
        for t in T:
            for k in K:
                want.append(dict(CXT_SIZE=100, RADIUS=r, TEMP=t, KNN=k))
    assert s.configs == want and len(s) == 60
    assert s.configs[0] == dict(CXT_SIZE=100, RADIUS=45, TEMP=0.1, KNN=15) and s.configs[1]["KNN"] == 20
    assert s.configs[4] == dict(CXT_SIZE=100, RADIUS=45, TEMP=0.01, KNN=15) and s.configs[12]["RADIUS"] == 50
    for bad in (((), T, K), (R, (), K), (R, T, ())):
        with pytest.raises(ValueError):
            LabelPropSweep(100, *bad)
    with pytest.raises(RuntimeError, match="KNN=30 exceeds"):
        s.propagate_all(torch.zeros(4, 12, 8), torch.zeros(12), 3)  # KNN > nodes: refused before anything is launched


def test_segment_sweep_refuses_a_dataset_without_merge_rule():
    g = load_golden(SWEEP_FIXTURE)
    import inference as crw_inference
    ds, seg, ncls, T, patch, overlap, _, kw = build_case(g)
    kw.update(dataset_id=2)
    with pytest.raises(ValueError, match="no merge rule"):
        crw_inference.segment_sweep(ds, seg, CountingFlatten(), fixture_sweep(g), ncls, T, patch, overlap, **kw)
    with pytest.raises(ValueError, match="no merge rule"):
        crw_inference.merge_reverse_batch(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), 2)


def test_merge_reverse_batch_is_merge_reverse_per_map():
    import inference as crw_inference
    gen = torch.Generator().manual_seed(3)
    fwd = torch.randint(0, 6, (5, 9, 14), generator=gen).to(torch.int8)
    rev = torch.randint(0, 6, (5, 9, 14), generator=gen).to(torch.int8)
    rev[:, :, 3:6][rev[:, :, 3:6] == 4] = 0  # some columns without class 4
    for ds_id in (0, 1, 3):
        got = crw_inference.merge_reverse_batch(fwd, rev, ds_id)
        for i in range(5):
            assert torch.equal(got[i], crw_inference.merge_reverse(fwd[i], rev[i], ds_id)), (ds_id, i)
        assert not torch.equal(got, fwd)


# ---------------------------------------------------------------------------------------------------------------- 2. the maps
def test_segment_sweep_matches_reference_main_per_configuration():
    """The reference's test_all.py main(args), run once per configuration, against ONE segment_sweep."""
    g = load_golden(SWEEP_FIXTURE)
    assert g["saved_maps"].shape[0] == 12 and len({m.tobytes() for m in g["final_maps"]}) > 4  # the grid moves the maps
    out, _ = run_sweep(g, fixture_sweep(g), oracle_propagate_sweep)
    check_sweep_golden(g, out)
    assert out["change_idx"] == [None, 5, None]
    assert out["configs"][1] == dict(CXT_SIZE=4, RADIUS=2, TEMP=0.1, KNN=5)


@pytest.mark.parametrize("name", SEGMENT_CASES)
def test_segment_sweep_equals_segment_per_configuration(name):
    g = load_golden(name)
    sweep = grid_around(g)
    out, _ = run_sweep(g, sweep, oracle_propagate_sweep)
    assert len(sweep.configs) == 8
    for i, cfg in enumerate(sweep.configs):
        one, _ = run_per_config(g, cfg, oracle_propagate)  # a fresh dataset each time
        assert torch.equal(out["forward"][i], one["forward"].to(torch.int8)), (name, cfg)
        assert torch.equal(out["pred"][i], one["pred"].to(torch.int8)), (name, cfg)
        assert out["change_idx"] == one["change_idx"]
    own = sweep.configs.index(dict(CXT_SIZE=int(g["cxt_size"]), RADIUS=int(g["radius"]), TEMP=float(g["temp"]), KNN=int(g["knn"])))
    assert np.array_equal(out["forward"][own].numpy(), g["saved_map"]) and np.array_equal(out["pred"][own].numpy(), g["final_map"])


# ------------------------------------------------------------------------------------------------------- 3. once, not G times
@pytest.mark.parametrize("name", ["segment_ds0_correction", "segment_ds3_correction_reverse", "segment_ds1_reverse"])
def test_the_encoder_runs_once_per_pass_not_once_per_configuration(name):
    g = load_golden(name)
    sweep = grid_around(g)
    enc_s, enc_1 = CountingFlatten(), CountingFlatten()
    _, n_sweep = run_sweep(g, sweep, oracle_propagate_sweep, encoder=enc_s)
    _, n_one = run_per_config(g, sweep.configs[0], oracle_propagate, encoder=enc_1)
    assert n_sweep == n_one > 0
    assert enc_s.shapes == enc_1.shapes and len(enc_s.shapes) == n_one


# ---------------------------------------------------------------------------------------------------------------- 4. reports
@pytest.mark.parametrize("dataset_id", [0, 1, 3])
def test_evaluate_sweep_equals_evaluate_per_map(dataset_id):
    import inference as crw_inference
    K = crw_inference.NCLASSES[dataset_id]
    gen = torch.Generator().manual_seed(dataset_id + 9)
    seg = torch.randint(0, K, (20, 64), generator=gen).float()
    pred = torch.randint(0, K, (6, 20, 64), generator=gen).to(torch.int8)
    unc = seg.clone()
    unc[8:11] = 4
    kw = dict(unc_seg=unc) if dataset_id == 0 else {}
    for remove_unc in (True, False):
        got = crw_inference.evaluate_sweep(pred, seg, dataset_id, remove_unc=remove_unc, **kw)
        want = [crw_inference.evaluate(p, seg, dataset_id, remove_unc=remove_unc, **kw) for p in pred]
        assert len(got) == 6
        for a, b in zip(got, want):
            assert np.array_equal(a.counts, b.counts) and np.array_equal(a.matrix, b.matrix) and a.dropped == b.dropped
            assert str(a) == str(b) and a.matrix_str() == b.matrix_str()
        if remove_unc and dataset_id in (0, 1):
            assert got[0].dropped[0] > 0
    if dataset_id == 0:
        with pytest.raises(ValueError, match="unc_seg"):
            crw_inference.evaluate_sweep(pred, seg, 0)
    with pytest.raises(ValueError):
        crw_inference.evaluate_sweep(pred, seg[:, :60], dataset_id, remove_unc=False)
    with pytest.raises(ValueError):
        crw_inference.evaluate_sweep(pred, seg, 2)
    import crw_hip
    bad = pred.clone()
    bad[3, 0, 0] = 9 if dataset_id != 1 else 7
    with pytest.raises(crw_hip.LabelError):
        crw_inference.evaluate_sweep(bad, seg, dataset_id, remove_unc=False)


def test_header_and_binding_declare_the_sweep_entry_points_at_abi_8():
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^int\s+crw_labelprop_topk_scores\(const float \*ehat, int T, int N, int C, int cxt_size, int radius, float temp, "
                     r"int kcap, int first_frame,\s+int grid_w, float \*V, int32_t \*I, crw_stream_t stream\);", header, re.M)
    assert re.search(r"^int\s+crw_labelprop_sweep_weights\(const float \*V, int F, int kcap, int N, const int \*knns, int nk, float \*W, "
                     r"crw_stream_t stream\);", header, re.M)
    assert re.search(r"^int\s+crw_labelprop_propagate_batch\(const float \*seed, const float \*W, const int32_t \*I, size_t i_stride, int G,",
                     header, re.M)
    assert int(re.search(r"^#define\s+CRW_ABI_VERSION\s+(\d+)", header, re.M).group(1)) == crw_hip.ABI_VERSION == 8
    assert "without a bump" in header
    assert set(crw_hip.SWEEP_ENTRY_POINTS) == {"crw_labelprop_topk_scores", "crw_labelprop_sweep_weights", "crw_labelprop_propagate_batch"}
    assert set(crw_hip.SWEEP_ENTRY_POINTS) <= set(crw_hip.SIGNATURES)
    assert len(crw_hip.SIGNATURES["crw_labelprop_topk_scores"][1]) == len(crw_hip.SIGNATURES["crw_labelprop_topk_grid"][1]) == 13
    assert len(crw_hip.SIGNATURES["crw_labelprop_sweep_weights"][1]) == 8 and len(crw_hip.SIGNATURES["crw_labelprop_propagate_batch"][1]) == 14
    assert crw_hip.has_sweep() and crw_hip.lib().crw_abi_version() == 8
    # argument errors are refused on the host side of the library, before any launch (no GPU needed)
    lib = crw_hip.lib()
    assert lib.crw_labelprop_sweep_weights(None, 1, 1, 1, None, 1, None, None) == crw_hip.CRW_EINVAL
    assert lib.crw_labelprop_propagate_batch(None, None, None, 0, 1, 4, 4, 2, 3, 1, 2, None, None, None) == crw_hip.CRW_EINVAL
    assert lib.crw_labelprop_topk_scores(None, 4, 4, 8, 2, 2, 0.1, 3, 1, 1, None, None, None) == crw_hip.CRW_EINVAL


# ---------------------------------------------------------------------------------------------------------------- 5. command line
def _cli():
    spec = importlib.util.spec_from_file_location("segment_sweep", os.path.join(PKG, "scripts", "segment_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_defaults_are_the_launch_scripts_lists():
    cli = _cli()
    p = cli.get_args_parser()
    a = cli.with_defaults(p.parse_args(["--model_path", "x.pt"]))
    assert (a.radius, a.temp, a.knn) == ([45, 50, 55, 60, 65], [0.1, 0.01, 0.001], [15, 20, 25, 30])
    assert (a.model, a.dataset, a.patch_size, a.seq_length, a.overlap, a.cxt_size) == (1, 1, (16, 16), 100, (8, 0), 100)  # test_all.py
    assert (a.pos_embed, a.remove_unc, a.flip, a.use_last, a.dataset_full, a.correction, a.select, a.reports, a.save_maps) == \
        (False, True, False, False, True, False, "macro_f1", False, False)
    a = cli.with_defaults(p.parse_args(["--synthetic", "64", "640", "--dataset", "3", "-r", "3", "5", "-t", "0.5", "-k", "2", "4", "6",
                                        "--select", "mean_iou", "-c", "7"]))
    assert (a.radius, a.temp, a.knn, a.select, a.cxt_size, a.synthetic) == ([3, 5], [0.5], [2, 4, 6], "mean_iou", 7, [64, 640])
    with pytest.raises(SystemExit):
        cli.with_defaults(p.parse_args([]))
    with pytest.raises(SystemExit):
        cli.with_defaults(p.parse_args(["--synthetic", "64", "640", "--dataset", "2"]))
    with pytest.raises(SystemExit):
        p.parse_args(["--model_path", "x.pt", "--select", "luck"])


@pytest.mark.parametrize("select", ["macro_f1", "accuracy"])
def test_cli_on_a_tiny_synthetic_case(tmp_path, capsys, select):
    import inference as crw_inference
    cli = _cli()
    js = tmp_path / "s.json"
    a = cli.get_args_parser().parse_args(["--synthetic", "40", "384", "--dataset", "3", "--patch_size", "8", "8", "--overlap", "4", "0",
                                          "--seq_length", "8", "-c", "4", "-r", "2", "6", "-t", "0.1", "0.01", "-k", "3", "5",
                                          "--use_last", "true", "--model", "0", "--report_json", str(js), "--select", select,
                                          "--save_maps", "--output_folder", str(tmp_path / "out")])
    orig, orig_model = crw_inference.propagate_sweep, cli.create_model
    crw_inference.propagate_sweep = oracle_propagate_sweep
    cli.create_model = lambda id, pos_embed: CountingFlatten()
    try:
        reports, best = cli.main(a)
    finally:
        crw_inference.propagate_sweep, cli.create_model = orig, orig_model
    text = capsys.readouterr().out
    d = json.load(open(js))
    assert len(reports) == 8 == len(d["configs"]) and d["grid"] == dict(cxt_size=4, radius=[2, 6], temp=[0.1, 0.01], knn=[3, 5])
    assert [(c["radius"], c["temp"], c["knn"]) for c in d["configs"]] == [(r, t, k) for r in (2, 6) for t in (0.1, 0.01) for k in (3, 5)]
    key = {"macro_f1": lambda r: r["macro avg"]["f1-score"], "accuracy": lambda r: r["accuracy"]}[select]
    scores = [key(c["report"]) for c in d["configs"]]
    assert d["select"] == select and d["best"]["index"] == best == int(np.argmax(scores)) and d["best"]["score"] == max(scores)
    assert [c["score"] for c in d["configs"]] == scores
    for c in d["configs"]:
        assert int(np.sum(c["report"]["matrix"])) == d["pixels"] == 40 * 384 and c["report"]["dropped"] == dict(masked=0, invalid=0)
    assert f"Best by {select}: radius {d['best']['radius']} temp {d['best']['temp']:g} knn {d['best']['knn']}" in text
    assert text.count("\n") > 12 and "weighted avg" in text
    saved = sorted(os.listdir(tmp_path / "out"))
    assert len(saved) == 8 and "predicted_map_r2_t0.1_k3.pt" in saved
    m = torch.load(tmp_path / "out" / "predicted_map_r6_t0.01_k5.pt")
    assert m.dtype == torch.int8 and tuple(m.shape) == (40, 384)


def test_a_library_without_the_sweep_entry_points_is_named_stale(monkeypatch):
    """The three entry points came at ABI 8 without a bump, so an older build still loads: the wrappers must say what is wrong."""
    import crw_hip
    crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "sweep", False)
    assert not crw_hip.has_sweep()
    for call in (lambda: crw_hip.labelprop_topk_scores(torch.zeros(4, 4, 8), 2, 2, 0.1, 2),
                 lambda: crw_hip.labelprop_sweep_weights(torch.zeros(3, 2, 4), (1, 2)),
                 lambda: crw_hip.labelprop_propagate_batch(torch.zeros(4), torch.zeros(2, 3, 2, 4), torch.zeros(3, 2, 4, dtype=torch.int32),
                                                           4, 4, 3, cxt_size=2)):
        with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*crw_labelprop_topk_scores.*rebuild"):
            call()
