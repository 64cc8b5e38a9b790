"""GPU side of the (radius, temp, knn) sweeps: the three entry points against the per-configuration entry points that define them
(`crw_labelprop_topk_scores` + `crw_labelprop_sweep_weights` against `crw_labelprop_topk_grid`, `crw_labelprop_propagate_batch`
against `crw_labelprop_propagate`) -- bitwise, no tolerance --, `LabelPropSweep`, `segment_sweep` / `evaluate_sweep` against the
reference's fixture and against per-configuration `segment` / `evaluate`, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_golden
pytestmark = pytest.mark.gpu

TEMPS = (0.1, 0.01, 0.001)
KNNS = (15, 20, 25, 30)


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    assert crw_hip.has_sweep()
    return crw_hip


def _feats(hip, T, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    return hip.normalize((torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).float().cuda())


def check_scores_against_topk(hip, feats, cxt, radius, temps, knns, first=1, grid_w=1):
    """The equalities that define the two entry points, for every temperature and every knn."""
    kcap = max(knns)
    for temp in temps:
        V, I = hip.labelprop_topk_scores(feats, cxt, radius, temp, kcap, first_frame=first, grid_w=grid_w)
        Wc, Ic = hip.labelprop_topk(feats, cxt, radius, temp, kcap, first_frame=first, grid_w=grid_w)
        assert torch.equal(I, Ic), f"temp {temp}: I of the scores mode differs from crw_labelprop_topk_grid's"
        empty = V == -float("inf")
        assert bool((Wc[empty] == 0).all())  # an empty slot is an empty slot of the weights
        assert bool((I[empty] == 0).all())
        W = hip.labelprop_sweep_weights(V, knns)
        assert tuple(W.shape) == (len(knns), V.shape[0], kcap, V.shape[2])
        for i, k in enumerate(knns):
            Wk, Ik = hip.labelprop_topk(feats, cxt, radius, temp, k, first_frame=first, grid_w=grid_w)
            assert torch.equal(W[i][:, :k], Wk), f"temp {temp} knn {k}: weights are not bitwise those of the knn = {k} call"
            assert torch.equal(I[:, :k], Ik), f"temp {temp} knn {k}: lists are no prefix"
            assert bool((W[i][:, k:] == 0).all()), f"temp {temp} knn {k}: padding slots are not 0"


@pytest.mark.parametrize("T,N,C,cxt,radius,knns,first,grid_w", [
    (8, 36, 16, 4, 3, (5, 10, 15, 20), 1, 9),         # a 4 x 9 grid: the vector kernel
    (40, 48, 128, 20, 10, KNNS, 1, 1),                # matrix cores, one piece
    (60, 48, 128, 40, 20, KNNS, 1, 1),                # two halves (41 x 39 candidates: 100 KiB of scores per tile)
    (100, 48, 128, 80, 30, KNNS, 1, 1),               # runtime chunks (mc1)
    (100, 190, 128, 100, 60, KNNS, 1, 1),             # runtime chunks (mc3)
    (100, 48, 64, 80, 30, KNNS, 7, 1),                # later first frame
    (40, 48, 128, 20, 10, KNNS, 5, 1)])
def test_topk_scores_and_sweep_weights_equal_topk_grid(hip, T, N, C, cxt, radius, knns, first, grid_w):
    check_scores_against_topk(hip, _feats(hip, T, N, C, T + N + radius), cxt, radius, TEMPS, knns, first, grid_w)


def test_selection_is_per_temperature_on_a_quotient_collision_input(hip):
    """Scores that are consecutive fp32 values: division by the temperature maps neighbours onto equal quotients, and the tie rule
    (lowest candidate index) then orders them differently from their order as raw scores.  Selecting once and rescaling fails
    this; selecting per temperature passes.  Every score is exactly x_m (one non-zero product), whatever the summation order."""
    T, N, C = 6, 32, 64
    x = np.empty(T * N, dtype=np.float32)
    x[0] = np.float32(0.9)
    for i in range(1, T * N):
        x[i] = np.nextafter(x[i - 1], np.float32(2), dtype=np.float32)
    ehat = torch.zeros(T, N, C)
    ehat[:, :, 0] = torch.from_numpy(x).view(T, N)  # ascending in node index (and frame)
    # frame T-1 holds the queries: e_0 exactly; its own rows are never keys of an earlier frame
    q = torch.zeros(N, C)
    q[:, 0] = 1.0
    ehat[T - 1] = q
    ehat = ehat.cuda().contiguous()
    knns = (4, 8, 12, 16)
    _, I1 = hip.labelprop_topk(ehat, T, N, 1.0, 16, first_frame=T - 1)
    _, I01 = hip.labelprop_topk(ehat, T, N, 0.1, 16, first_frame=T - 1)
    assert bool((I1 != I01).any()), "the input is not adversarial: temp 0.1 orders the keys as temp 1.0 does"
    check_scores_against_topk(hip, ehat, T, N, (1.0,) + TEMPS, knns, first=T - 1)
    check_scores_against_topk(hip, ehat, T, N, (1.0,) + TEMPS, knns, first=T - 1, grid_w=N)  # the vector kernel


@pytest.mark.parametrize("T,N,C,cxt,radius", [(40, 48, 128, 20, 10), (100, 48, 128, 80, 30)])
def test_exact_ties_of_identical_rows(hip, T, N, C, cxt, radius):
    """Blocks of identical feature rows (zero-padded regions of a radargram encode alike): runs of exactly equal scores."""
    feats = _feats(hip, T, N, C, 5)
    feats[:, 8:20] = feats[:, 8:9].clone()
    feats[1::2] = feats[0:T - 1:2][: feats[1::2].shape[0]].clone()
    check_scores_against_topk(hip, feats.contiguous(), cxt, radius, TEMPS, KNNS)


def _configs_lists(hip, feats, cxt, radii, temps, knns, first, strided):
    """W [G, F, kmax, N] and I (shared [F, kmax, N] when one (radius, temp), else [G, F, kmax, N]) + the per-configuration lists"""
    kmax = max(knns)
    Ws, Is, per = [], [], []
    for r in radii:
        for t in temps:
            V, I = hip.labelprop_topk_scores(feats, cxt, r, t, kmax, first_frame=first)
            W = hip.labelprop_sweep_weights(V, knns)
            for i, k in enumerate(knns):
                Ws.append(W[i])
                Is.append(I)
                per.append(hip.labelprop_topk(feats, cxt, r, t, k, first_frame=first))
    W = torch.stack(Ws).contiguous()
    I = torch.stack(Is).contiguous() if strided else Is[0].contiguous()
    return W, I, per


def _layered(T, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(N + 16, C, generator=g)
    t = torch.arange(T).float()
    depth = torch.arange(N).float()[None] + 3 * torch.sin(2 * np.pi * t / 40)[:, None] + 6
    lo = depth.floor().long()
    fr = (depth - lo.float()).unsqueeze(-1)
    return (proto[lo] * (1 - fr) + proto[lo + 1] * fr + 0.3 * torch.randn(T, N, C, generator=g)).float()


@pytest.mark.parametrize("T,N,M,cxt,radii,temps,knns,first", [
    (256, 48, 4, 80, (30,), (0.1,), KNNS + KNNS + KNNS, 1),                     # G = 12, one I shared by all
    (256, 48, 4, 80, (45, 50, 55, 60, 65), TEMPS, KNNS, 1),                    # G = 60, strided I
    (256, 48, 4, 300, (10, 30), (0.1, 0.01), KNNS, 1),                         # cxt >= T: every frame chained
    (100, 190, 5, 100, (60,), (0.01,), KNNS, 1),                               # chained labels beyond the LDS: the ring
    (100, 190, 5, 100, (45, 60), (0.1, 0.01), (20, 30), 1),
    (60, 48, 4, 30, (10,), (0.1,), KNNS, 9),                                   # first_frame > 1, seed = NULL
    (60, 48, 4, 30, (10,), (0.1,), (20,), 1),                                  # G = 1
    (60, 48, 4, 30, (10,), (0.1,), (20,), 59)])                                # one frame
def test_propagate_batch_equals_propagate_per_configuration(hip, T, N, M, cxt, radii, temps, knns, first):
    feats = hip.normalize(_layered(T, N, 128, 77 + N).cuda())
    strided = len(radii) * len(temps) > 1
    W, I, per = _configs_lists(hip, feats, cxt, radii, temps, knns, first, strided)
    G = W.shape[0]
    seed = (torch.arange(N) * M // N).float().cuda()
    if first == 1:
        L, pred = hip.labelprop_propagate_batch(seed, W, I, T, N, M, first_frame=1, cxt_size=cxt)
        L0 = None
    else:  # the frames before first_frame from a propagation of their own
        Wf, If = hip.labelprop_topk(feats[:first].contiguous(), cxt, radii[0], temps[0], knns[0])
        Lf, pf = hip.labelprop_gather(seed, Wf, If, first, N, M, cxt_size=cxt)
        L0 = torch.zeros(T * N, M, device="cuda")
        L0[:first * N] = Lf
        L = L0[None].repeat(G, 1, 1).contiguous()
        pred = torch.zeros(G, N, T, device="cuda")
        hip.labelprop_propagate_batch(None, W, I, T, N, M, first_frame=first, cxt_size=cxt, L=L, pred=pred)
    for g, (Wg, Ig) in enumerate(per):
        if first == 1:
            Lg, pg = hip.labelprop_gather(seed, Wg, Ig, T, N, M, cxt_size=cxt)
        else:
            Lg, pg = L0.clone(), torch.zeros(N, T, device="cuda")
            hip.labelprop_gather(None, Wg, Ig, T, N, M, first_frame=first, L=Lg, pred=pg, cxt_size=cxt)
        assert torch.equal(L[g][first * N:], Lg[first * N:]), f"configuration {g}: soft labels differ"
        assert torch.equal(pred[g][:, first:], pg[:, first:]), f"configuration {g}: label map differs"
        if first == 1:
            assert torch.equal(L[g], Lg) and torch.equal(pred[g], pg)
        assert pred[g][:, first:].unique().numel() > 1, f"configuration {g}: a trivial label map proves nothing"


def test_propagate_batch_argument_errors(hip):
    T, N, M = 10, 16, 3
    W = torch.zeros(2, T - 1, 4, N, device="cuda")
    I = torch.zeros(T - 1, 4, N, device="cuda", dtype=torch.int32)
    seed = torch.zeros(N, device="cuda")
    with pytest.raises(ValueError):
        hip.labelprop_propagate_batch(seed, W, I, T, N, M)
    with pytest.raises(RuntimeError):
        hip.labelprop_propagate_batch(seed, W, I[:, :3].contiguous(), T, N, M, cxt_size=4)
    with pytest.raises(hip.CrwError) as e:
        hip.labelprop_propagate_batch(seed, W, I, T, N, M, cxt_size=0)
    assert e.value.status == hip.CRW_EINVAL
    V = torch.zeros(T - 1, 4, N, device="cuda")
    for bad in ((5,), (0,), tuple(range(1, 5)) * 5):
        with pytest.raises(hip.CrwError) as e:
            hip.labelprop_sweep_weights(V, bad)
        assert e.value.status == hip.CRW_EINVAL
    with pytest.raises(hip.CrwError):
        hip.labelprop_topk_scores(torch.zeros(T, N, 16, device="cuda"), 4, 3, 0.1, 65)


# ------------------------------------------------------------------------------------------------- LabelPropSweep and the drivers
@pytest.mark.parametrize("T,N,C,M,cxt,radii,temps,knns", [
    (100, 48, 128, 4, 80, (45, 50, 55, 60, 65), TEMPS, KNNS),     # the reference's grid at the mc1 geometry
    (100, 190, 128, 5, 100, (45, 65), (0.1, 0.001), KNNS),         # mc3 geometry
    (40, 24, 64, 3, 10, (3, 8), (0.1, 0.01), (5, 10, 20)),
    (30, 20, 32, 3, 6, (4,), (0.05,), (3, 7))])                    # vector kernel, one (radius, temp): I shared
def test_sweep_propagate_all_equals_labelprop_per_configuration(hip, T, N, C, M, cxt, radii, temps, knns):
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    feats = hip.normalize(_layered(T, N, C, 5 + N).cuda())
    seed = (torch.arange(N) * M // N).float().cuda()
    sweep = LabelPropSweep(cxt, radii, temps, knns)
    pred = sweep.propagate_all(feats, seed, M)
    assert tuple(pred.shape) == (len(sweep.configs), N, T)
    for g, cfg in enumerate(sweep.configs):
        want, _ = LabelPropVOS_CRW(cfg).propagate_all(feats, seed, M)
        assert torch.equal(pred[g], want), cfg
    assert len({p.cpu().numpy().tobytes() for p in pred}) > 1 or len(sweep.configs) == 1


def test_sweep_per_config_switch_in_a_child_process():
    """CRW_SWEEP_PER_CONFIG=1: the loop over `LabelPropVOS_CRW.propagate_all` behind the same interface (the A/B arm)."""
    env = dict(os.environ, CRW_SWEEP_PER_CONFIG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_sweep_gpu.py"), "-x", "-q", "-m", "gpu", "-k",
                        "sweep_propagate_all_equals or segment_sweep_on_the_hip_path", "-p", "no:cacheprovider"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_segment_sweep_on_the_hip_path_matches_reference_main(hip):
    import utils as crw_utils
    from test_sweep import SWEEP_FIXTURE, check_sweep_golden, fixture_sweep, run_sweep
    g = load_golden(SWEEP_FIXTURE)
    out, n = run_sweep(g, fixture_sweep(g), crw_utils.propagate_sweep, "cuda")
    check_sweep_golden(g, out)
    assert out["pred"].is_cuda and n == 7  # three forward passes, one correction, three reverse passes


@pytest.mark.parametrize("name", ["segment_ds0_correction", "segment_ds3_correction_reverse"])
def test_segment_sweep_on_the_hip_path_equals_segment_per_configuration(hip, name):
    import utils as crw_utils
    from test_sweep import grid_around, run_per_config, run_sweep
    g = load_golden(name)
    sweep = grid_around(g)
    out, n = run_sweep(g, sweep, crw_utils.propagate_sweep, "cuda")
    for i, cfg in enumerate(sweep.configs):
        one, n1 = run_per_config(g, cfg, crw_utils.propagate, "cuda")
        assert n1 == n
        assert torch.equal(out["forward"][i], one["forward"].to(torch.int8)), cfg
        assert torch.equal(out["pred"][i], one["pred"].to(torch.int8)), cfg


def _cli(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_segment_sweep_at_a_real_geometry_with_the_reference_encoder(hip):
    """410-row radargram, 16 x 16 patches, overlap (8, 0), T = 100 (N = 50), three radargrams, the reference's 5 x 3 x 4 grid, a
    random-init Resnet in train mode (test_all.py never calls .eval()), correction at the change points `propagate` finds, reverse
    pass: every one of the 60 maps against `segment` for that configuration on a fresh dataset.  Both arms run the same arithmetic,
    so the maps are equal, not close."""
    import dataset as crw_dataset
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    cli = _cli("segment_all")
    rows, cols, T, patch, overlap, K = 410, 4800, 100, (16, 16), (8, 0), 5
    rg = crw_dataset.synthetic_radargram(rows, cols)
    seg = cli.synthetic_reference(rows, cols, K)
    torch.manual_seed(11)
    enc = crw_utils.create_model(1, False).cuda()
    enc.train(True)
    sweep = LabelPropSweep(100, (45, 50, 55, 60, 65), TEMPS, KNNS)
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap)
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cuda")
    out = crw_inference.segment_sweep(fresh(), seg, enc, sweep, K, T, patch, overlap, **kw)
    assert tuple(out["pred"].shape) == (60, rows, cols) and out["pred"].dtype == torch.int8
    assert len(out["change_idx"]) == 3
    differ = []
    for g, cfg in enumerate(sweep.configs):
        one = crw_inference.segment(fresh(), seg, enc, LabelPropVOS_CRW(cfg), K, T, patch, overlap, **kw)
        assert one["change_idx"] == out["change_idx"], cfg
        if not (torch.equal(out["forward"][g], one["forward"].to(torch.int8)) and torch.equal(out["pred"][g], one["pred"].to(torch.int8))):
            differ.append((cfg, int((out["pred"][g] != one["pred"].to(torch.int8)).sum())))
    assert not differ, differ
    assert len({bytes(p.cpu().numpy().tobytes()) for p in out["pred"][::7]}) > 1  # the grid moves the maps
    assert all(p.unique().numel() > 1 for p in out["pred"][::7])


@pytest.mark.parametrize("dataset_id", [0, 1, 3])
def test_evaluate_sweep_on_device_maps_equals_evaluate(hip, dataset_id):
    import inference as crw_inference
    K = crw_inference.NCLASSES[dataset_id]
    gen = torch.Generator().manual_seed(dataset_id + 9)
    seg = torch.randint(0, K, (410, 1600), generator=gen).float().cuda()
    seg[3, 3] = 0  # the pixel that gets an invalid prediction below is not one the dataset-1 rule masks
    pred = torch.randint(0, K, (7, 410, 1600), generator=gen).to(torch.int8).cuda()
    unc = seg.clone()
    unc[100:130] = 4
    kw = dict(unc_seg=unc) if dataset_id == 0 else {}
    got = crw_inference.evaluate_sweep(pred, seg, dataset_id, **kw)
    want = [crw_inference.evaluate(p, seg, dataset_id, **kw) for p in pred]
    assert len(got) == 7
    for a, b in zip(got, want):
        assert np.array_equal(a.counts, b.counts) and a.dropped == b.dropped and str(a) == str(b)
    bad = pred.clone()
    bad[5, 3, 3] = 11
    with pytest.raises(hip.LabelError):
        crw_inference.evaluate_sweep(bad, seg, dataset_id, **kw)


@pytest.mark.parametrize("select", ["macro_f1", "mean_iou"])
def test_cli_synthetic_run_in_a_child_process(tmp_path, select):
    js = tmp_path / "sweep.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "scripts", "segment_sweep.py"), "--synthetic", "200", "1600", "--dataset", "0",
                        "--seq_length", "50", "-c", "20", "-r", "5", "10", "-t", "0.1", "0.01", "-k", "5", "10", "--use_last", "true",
                        "--correction", "true", "--select", select, "--report_json", str(js), "--output_folder", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = json.load(open(js))
    assert len(d["configs"]) == 8 and d["grid"]["radius"] == [5, 10] and d["grid"]["knn"] == [5, 10]
    unc = _cli("segment_all").synthetic_reference(200, 1600, 4, True)[:, :d["map_shape"][1]]
    unmasked = int((unc != 4).sum())
    assert d["map_shape"][0] == 200 and d["pixels"] == 200 * d["map_shape"][1]
    for c in d["configs"]:
        assert int(np.sum(c["report"]["matrix"])) == unmasked and c["report"]["dropped"] == dict(masked=d["pixels"] - unmasked, invalid=0)
    key = {"macro_f1": lambda r_: r_["macro avg"]["f1-score"], "mean_iou": lambda r_: r_["mean_iou"]}[select]
    scores = [key(c["report"]) for c in d["configs"]]
    assert d["best"]["index"] == int(np.argmax(scores)) and d["select"] == select
    b = d["configs"][d["best"]["index"]]
    assert f"Best by {select}: radius {b['radius']} temp {b['temp']:g} knn {b['knn']}" in r.stdout
