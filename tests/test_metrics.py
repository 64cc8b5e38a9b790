"""Segmentation reports on the host: `inference.evaluate` / `metrics.Report` against what the reference's own
scripts/test/test_all.py passed to and got back from scikit-learn (fixtures report_*.npz, tests/golden/make_golden_reports.py;
no test imports scikit-learn), the mask rules one by one, invalid labels, the ABI tables and the command line.  CPU tensors take
`crw_hip.confusion`'s torch.bincount route; the kernel's twins are in test_metrics_gpu.py."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_golden

REPORT_CASES = ["report_ds0_unc_band", "report_ds1_reverse", "report_ds3_correction_reverse", "report_ds0_flip_plain",
                "report_ds1_unpredicted_class", "report_ds0_class_removed"]


def fixture_maps(g, device="cpu", dtype=torch.float32):
    """-> (final_pred, seg, unc_seg | None) of a report fixture as tensors, plus evaluate's keyword arguments."""
    t = lambda a: torch.tensor(a.astype(np.float32)).to(dtype).to(device)
    unc = t(g["unc_seg"]) if "unc_seg" in g else None
    return t(g["final_pred"]), t(g["seg"]), dict(dataset_id=int(g["dataset_id"]), remove_unc=bool(g["remove_unc"]), unc_seg=unc)


def expected_counts(g, K):
    """The fixture's recorded matrix (sklearn drops absent classes) spread back over all K classes."""
    full = np.zeros((K, K), dtype=np.int64)
    idx = g["d_labels"].astype(int)
    full[np.ix_(idx, idx)] = g["matrix"]
    return full


def check_report(rep, g):
    """Matrix exact; every recorded number of sklearn's dict to 1e-12 relative (the same float64 formulas on the same integers:
    four decimal orders over float64 rounding); both printed texts character for character."""
    assert rep.labels == list(g["d_labels"])
    assert rep.matrix.dtype == np.int64 and np.array_equal(rep.matrix, g["matrix"])
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
    close(rep.precision, g["d_precision"])
    close(rep.recall, g["d_recall"])
    close(rep.f1, g["d_f1"])
    assert np.array_equal(rep.support, g["d_support"].astype(np.int64))
    close(rep.accuracy, g["d_accuracy"])
    for avg, want in ((rep.macro, g["d_macro"]), (rep.weighted, g["d_weighted"])):
        close([avg["precision"], avg["recall"], avg["f1"]], want[:3])
        assert avg["support"] == int(want[3])
    assert str(rep) == str(g["report"])
    assert rep.matrix_str() == str(g["matrix_str"])
    assert rep.total == len(g["gt"]) and rep.dropped == (g["final_pred"].size - len(g["gt"]), 0)


@pytest.mark.parametrize("case", REPORT_CASES)
def test_evaluate_matches_the_reference_report(case):
    import inference as crw_inference
    g = load_golden(case)
    pred, seg, kw = fixture_maps(g)
    rep = crw_inference.evaluate(pred, seg, **kw)
    check_report(rep, g)
    assert np.array_equal(rep.counts, expected_counts(g, int(g["nclasses"])))
    # int8 maps (what the drivers save) give the same report
    pred8, seg8, kw8 = fixture_maps(g, dtype=torch.int8)
    check_report(crw_inference.evaluate(pred8, seg8, **kw8), g)


def test_fixtures_cover_what_they_claim():
    g = load_golden("report_ds0_unc_band")
    assert (g["unc_seg"] == 4).any() and 0 < len(g["gt"]) < g["seg"].size
    g = load_golden("report_ds1_reverse")
    assert (g["seg"] == 5).any() and (g["final_pred"] == 5).any() and list(g["d_labels"]) == [0, 1, 2, 3, 4]
    g = load_golden("report_ds3_correction_reverse")
    assert bool(g["remove_unc"]) and len(g["gt"]) == g["seg"].size
    g = load_golden("report_ds0_flip_plain")
    assert bool(g["flip"]) and not bool(g["remove_unc"])
    g = load_golden("report_ds1_unpredicted_class")
    i = list(g["d_labels"]).index(4.0)
    assert g["d_precision"][i] == 0.0 and g["d_support"][i] > 0 and "0.00      0.00      0.00" in str(g["report"])
    g = load_golden("report_ds0_class_removed")
    assert (g["seg"] == 3).any() and list(g["d_labels"]) == [0, 1, 2] and g["matrix"].shape == (3, 3)


def test_import_swap_functions_have_sklearns_call_shapes():
    """`from metrics import classification_report, confusion_matrix` in place of sklearn.metrics: same calls, same returns, on the
    arrays the script passed (already masked), tensors or numpy."""
    import metrics as crw_metrics
    g = load_golden("report_ds1_unpredicted_class")
    gt, pred = torch.tensor(g["gt"]).float(), torch.tensor(g["pred"]).float()
    assert crw_metrics.classification_report(gt, pred) == str(g["report"])
    m = crw_metrics.confusion_matrix(gt, pred)
    assert isinstance(m, np.ndarray) and np.array_equal(m, g["matrix"]) and str(m) == str(g["matrix_str"])
    assert crw_metrics.classification_report(g["gt"].astype(np.float32), g["pred"].astype(np.float32)) == str(g["report"])
    d = crw_metrics.classification_report(gt, pred, output_dict=True)
    assert set(d) == {str(v) for v in g["d_labels"]} | {"accuracy", "macro avg", "weighted avg"}
    assert set(d["0.0"]) == {"precision", "recall", "f1-score", "support"}
    np.testing.assert_allclose(d["macro avg"]["f1-score"], g["d_macro"][2], rtol=1e-12)


GT = torch.tensor([[0., 0., 1., 1.], [2., 2., 3., 3.], [0., 1., 2., 3.]])
PR = torch.tensor([[0., 1., 1., 1.], [2., 3., 3., 0.], [0., 1., 2., 2.]])


def _plain_counts(gt, pred, K, keep):
    out = np.zeros((K, K), dtype=np.int64)
    for g, p, k in zip(gt.flatten().tolist(), pred.flatten().tolist(), keep.flatten().tolist()):
        if k:
            out[int(g), int(p)] += 1
    return out


def test_mask_rules_one_by_one():
    import crw_hip
    import inference as crw_inference
    every = torch.ones(3, 4, dtype=torch.bool)
    c, d = crw_hip.confusion(GT, PR, 4)
    assert c.dtype == torch.int64 and c.shape == (4, 4) and d.tolist() == [0, 0]
    assert np.array_equal(c.numpy(), _plain_counts(GT, PR, 4, every))
    c, d = crw_hip.confusion(GT, PR, 4, ignore_gt=3)
    assert d.tolist() == [3, 0] and np.array_equal(c.numpy(), _plain_counts(GT, PR, 4, GT != 3))
    c, d = crw_hip.confusion(GT, PR, 4, ignore_pred=1)
    assert d.tolist() == [4, 0] and np.array_equal(c.numpy(), _plain_counts(GT, PR, 4, PR != 1))
    aux = torch.tensor([[4., 0., 0., 0.], [0., 4., 4., 0.], [1., 2., 3., 4.]])
    c, d = crw_hip.confusion(GT, PR, 4, aux=aux, ignore_aux=4)
    assert d.tolist() == [4, 0] and np.array_equal(c.numpy(), _plain_counts(GT, PR, 4, aux != 4))
    c, d = crw_hip.confusion(GT, PR, 4, aux=aux, ignore_aux=4, ignore_gt=0, ignore_pred=2)  # a pixel masked thrice counts once
    keep = (aux != 4) & (GT != 0) & (PR != 2)
    assert d.tolist() == [12 - int(keep.sum()), 0] and np.array_equal(c.numpy(), _plain_counts(GT, PR, 4, keep))
    # evaluate: dataset 0 masks by the uncertain map, 1 by class 5 in either map, 3 and remove_unc=False by nothing
    rep = crw_inference.evaluate(PR, GT, 0, unc_seg=aux)
    assert rep.dropped == (4, 0) and np.array_equal(rep.counts, _plain_counts(GT, PR, 4, aux != 4))
    gt5, pr5 = GT.clone(), PR.clone()
    gt5[0, 0], pr5[2, 3], pr5[0, 0] = 5, 5, 4
    rep = crw_inference.evaluate(pr5, gt5, 1)
    assert rep.dropped == (2, 0) and np.array_equal(rep.counts, _plain_counts(gt5, pr5, 6, (gt5 != 5) & (pr5 != 5)))
    assert crw_inference.evaluate(PR, GT, 3).dropped == (0, 0) and crw_inference.evaluate(PR, GT, 3).counts.shape == (5, 5)
    assert crw_inference.evaluate(PR, GT, 0, remove_unc=False).dropped == (0, 0)
    assert np.array_equal(crw_inference.evaluate(PR, GT, 0, remove_unc=False).counts, _plain_counts(GT, PR, 4, every))
    with pytest.raises(ValueError):
        crw_inference.evaluate(PR, GT, 0)  # remove_unc on dataset 0 needs the uncertain map
    for bad in (2, 4, -1):
        with pytest.raises(ValueError):
            crw_inference.evaluate(PR, GT, bad, remove_unc=False)
    with pytest.raises(ValueError):
        crw_inference.evaluate(PR[:, :3], GT, 3)
    # the 4s of the uncertain map are aux values: never binned, although K = 4
    rep = crw_inference.evaluate(PR, GT, 0, unc_seg=torch.full((3, 4), 4.0))
    assert rep.dropped == (12, 0) and rep.total == 0 and rep.labels == [] and rep.accuracy == 0.0


@pytest.mark.parametrize("bad", [-1.0, 2.5, float("nan"), 4.0, 1e30])
def test_invalid_labels_are_counted_and_raise(bad):
    import crw_hip
    import inference as crw_inference
    import metrics as crw_metrics
    gt = GT.clone()
    gt[1, 2] = bad
    c, d = crw_hip.confusion(gt, PR, 4)
    assert d.tolist() == [0, 1] and int(c.sum()) == 11
    c, d = crw_hip.confusion(PR, gt, 4)  # as a prediction too
    assert d.tolist() == [0, 1] and int(c.sum()) == 11
    # masked by another operand: not invalid
    c, d = crw_hip.confusion(gt, PR, 4, ignore_pred=int(PR[1, 2]))
    assert d[1].item() == 0
    with pytest.raises(ValueError) as e:
        crw_inference.evaluate(PR, gt, 0, remove_unc=False)
    assert isinstance(e.value, crw_hip.CrwError) and e.value.invalid == 1 and not e.value.device_failure
    with pytest.raises(crw_hip.LabelError):
        crw_metrics.confusion_matrix(gt, PR, K=4)


def test_confusion_argument_checks_and_empty_input():
    import crw_hip
    for K in (1, 0, 17, -3):
        with pytest.raises(ValueError):
            crw_hip.confusion(GT, PR, K)
    for K in (2, 16):
        c, d = crw_hip.confusion(torch.zeros(5), torch.ones(5), K)
        assert c.shape == (K, K) and c[0, 1].item() == 5 and int(c.sum()) == 5
    with pytest.raises(ValueError):
        crw_hip.confusion(GT, PR[:, :3], 4)
    with pytest.raises(ValueError):
        crw_hip.confusion(GT, PR, 4, aux=GT[:2], ignore_aux=1)
    with pytest.raises(ValueError):
        crw_hip.confusion(GT, PR, 4, ignore_aux=1)  # no aux
    with pytest.raises(ValueError):
        crw_hip.confusion(GT, PR, 4, ignore_gt=-2)
    c, d = crw_hip.confusion(torch.zeros(0), torch.zeros(0), 5)
    assert c.shape == (5, 5) and c.dtype == torch.int64 and not c.any() and d.tolist() == [0, 0]
    # other dtypes are converted: int64 / float64 / uint8 / bool maps
    c64, _ = crw_hip.confusion(GT.long(), PR.double(), 4)
    cu8, _ = crw_hip.confusion(GT.to(torch.uint8), PR.to(torch.int16), 4)
    want, _ = crw_hip.confusion(GT, PR, 4)
    assert torch.equal(c64, want) and torch.equal(cu8, want)


def test_report_degenerate_ratios_and_iou():
    import metrics as crw_metrics
    rep = crw_metrics.Report(np.array([[3, 1, 0], [0, 0, 0], [2, 0, 4]]))  # class 1 is predicted once and never true
    assert rep.labels == [0.0, 1.0, 2.0] and rep.recall[1] == 0.0 and rep.precision[1] == 0.0 and rep.f1[1] == 0.0
    np.testing.assert_allclose(rep.iou, [3 / 6, 0.0, 4 / 6])
    np.testing.assert_allclose(rep.mean_iou, (0.5 + 4 / 6) / 3)
    np.testing.assert_allclose(rep.accuracy, 0.7)
    assert "mean" in rep.iou_str() and "iou" not in str(rep)
    d = rep.as_dict()
    assert d["1.0"]["support"] == 0 and d["weighted avg"]["support"] == 10 and d["mean_iou"] == rep.mean_iou
    with pytest.raises(ValueError):
        crw_metrics.Report(np.zeros((2, 3)))


def test_header_and_binding_declare_crw_confusion():
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^int\s+crw_confusion\(const void \*gt, int gt_dtype, const void \*pred, int pred_dtype", header, re.M)
    assert re.search(r"^size_t\s+crw_confusion_ws_bytes\(size_t P, int K\);", header, re.M)
    assert "test_all.py:161-187" in header and "/* evaluation" in header
    assert int(re.search(r"^#define\s+CRW_ABI_VERSION\s+(\d+)", header, re.M).group(1)) == crw_hip.ABI_VERSION == 8
    res, args = crw_hip.SIGNATURES["crw_confusion"]
    assert len(args) == 16 and "crw_confusion_ws_bytes" in crw_hip.SIGNATURES
    assert (crw_hip.DT_F32, crw_hip.DT_I8) == tuple(int(re.search(rf"^#define\s+{n}\s+(\d+)", header, re.M).group(1))
                                                    for n in ("CRW_DT_F32", "CRW_DT_I8"))
    lib = crw_hip.lib()
    assert lib.crw_abi_version() == 8
    # host-side queries: workspace grows with the grid up to 2 048 workgroups of K*K+2 32-bit partials; bad K -> 0
    assert lib.crw_confusion_ws_bytes(1, 5) == 112 and lib.crw_confusion_ws_bytes(0, 5) == 112
    assert lib.crw_confusion_ws_bytes(410 * 8192 * 3, 5) == 2048 * 27 * 4
    assert lib.crw_confusion_ws_bytes(1 << 40, 16) == 2048 * 258 * 4
    assert lib.crw_confusion_ws_bytes(1 << 44, 16) == (1 << 13) * 258 * 4  # no workgroup sees more than 2^31 pixels
    assert lib.crw_confusion_ws_bytes(100, 1) == 0 and lib.crw_confusion_ws_bytes(100, 17) == 0
    # argument errors are refused before anything is launched (no device needed)
    assert lib.crw_confusion(None, 0, None, 0, None, 0, 10, 5, -1, -1, -1, None, None, None, 0, None) == crw_hip.CRW_EINVAL


def _cli():
    spec = importlib.util.spec_from_file_location("segment_all", os.path.join(PKG, "scripts", "segment_all.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags_and_the_references_defaults():
    cli = _cli()
    p = cli.get_args_parser()
    a = cli.with_defaults(p.parse_args(["--model_path", "x.pt"]))  # test_all.py:17-41
    assert (a.model, a.dataset, a.patch_size, a.seq_length, a.overlap, a.cxt_size, a.radius, a.temp, a.knn) == \
        (1, 1, (16, 16), 100, (8, 0), 100, 10, 0.1, 20)
    assert (a.pos_embed, a.remove_unc, a.flip, a.use_last, a.dataset_full, a.correction, a.single) == \
        (False, True, False, False, True, False, False)
    a = cli.with_defaults(p.parse_args(["--single", "--model_path", "x.pt"]))  # test.py:12-31
    assert (a.model, a.dataset, a.patch_size, a.seq_length, a.overlap, a.cxt_size, a.radius, a.temp, a.knn, a.pos_embed) == \
        (1, 3, (16, 16), 80, (8, 0), 80, 16, 0.01, 10, False)
    a = cli.with_defaults(p.parse_args(["--synthetic", "200", "4800", "--dataset", "0", "--remove_unc", "false", "--use_last", "true",
                                        "--flip", "True", "--correction", "1", "-r", "7", "-t", "0.5", "--patch_size", "8", "8",
                                        "--overlap", "4", "0", "--report_json", "r.json"]))
    assert (a.synthetic, a.dataset, a.remove_unc, a.use_last, a.flip, a.correction, a.radius, a.temp, a.patch_size, a.overlap,
            a.report_json, a.model_path) == ([200, 4800], 0, False, True, True, True, 7, 0.5, (8, 8), (4, 0), "r.json", None)
    with pytest.raises(SystemExit):
        cli.with_defaults(p.parse_args([]))  # neither a checkpoint nor --synthetic
    with pytest.raises(SystemExit):
        cli.with_defaults(p.parse_args(["--synthetic", "64", "640", "--dataset", "2"]))
    with pytest.raises(SystemExit):
        p.parse_args(["--model_path", "x.pt", "--use_last", "maybe"])


def test_cli_synthetic_data_matches_the_datasets_geometry():
    cli = _cli()
    a = cli.with_defaults(cli.get_args_parser().parse_args(["--synthetic", "72", "400", "--dataset", "0", "--seq_length", "8",
                                                           "--flip", "true"]))
    ds, nclasses, seg, unc = cli.load_data(a)
    assert nclasses == 4 and seg.shape == (72, 400) and unc.shape == seg.shape
    assert sorted(seg.unique().tolist()) == [0, 1, 2, 3] and sorted(unc.unique().tolist()) == [0, 1, 2, 3, 4]
    plain = cli.synthetic_reference(72, 400, 4)
    assert torch.equal(seg, torch.flip(plain, (1,))) and torch.equal(unc[unc != 4], seg[unc != 4])
    assert ds[0].shape == (8, 8, 16, 16)
    a = cli.with_defaults(cli.get_args_parser().parse_args(["--synthetic", "72", "400", "--dataset", "1", "--seq_length", "8"]))
    _, nclasses, seg, unc = cli.load_data(a)
    assert nclasses == 6 and unc is None and seg.max().item() == 5
