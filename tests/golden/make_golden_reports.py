#!/usr/bin/env python3
"""Fixtures of the evaluation reports: the reference's own ``scripts/test/test_all.py`` ``main(args)`` run to its last line on
synthetic data, with ``sklearn.metrics.classification_report`` and ``confusion_matrix`` REAL (scikit-learn, build container
only -- no test imports it) behind thin recorders -> ``report_*.npz``.

Plumbing as in make_golden.py (its helpers are imported, nothing of the reference is edited): private-data factories pointed at
synthetic tensors, plots off, 'cuda' redirected to the CPU, ``propagate`` wrapped for forced change points.  ``get_reference``
also answers id 2, the "uncertain" map of dataset 0 (test_all.py:163), and honours ``flip`` like the reference's.

Every case runs ``main`` twice on the same inputs: once with ``remove_unc`` off to record the UNMASKED final map (what
``inference.evaluate`` is given), once as the case says to record what the script passed to sklearn and what came back:
  gt, pred ............ as passed to classification_report (after the script's own masking)
  report .............. the returned text;  matrix: confusion_matrix's array and its str()
  d_* ................. classification_report(..., output_dict=True) flattened: labels, precision, recall, f1, support [n],
                        accuracy, macro / weighted [precision, recall, f1, support]
  final_pred, seg, unc_seg (dataset 0 with remove_unc) ... the unmasked maps [rows, cols]
Fixtures hold arrays and the recorded strings only.

Seeds: a printed two-digit value must not sit on a rounding boundary (x.xx5 within 1e-6), or float noise could change the text;
``_check_rounding`` asserts that for every recorded number.  Seed 61 of the first case gave a score of exactly 0.375 and was replaced by 71; 62 ... 66 pass.

Usage:  python tests/golden/make_golden_reports.py        (rewrites report_*.npz, bit for bit)
"""
import argparse
import importlib
import os
import sys
import tempfile
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg

GEOM = dict(T=8, hw=(8, 8), oh=4, H_rg=52, n_rg=3, seg_rows_extra=2)  # make_golden.py's segment_* geometry
LPC = dict(CXT_SIZE=4, RADIUS=4, TEMP=0.1, KNN=5)


def _radargram(H_rg, W_rg, gen):
    """make_golden.run_segment_case's layered medium (patch pixels ARE the features)."""
    r = torch.arange(H_rg).float()[:, None]
    c = torch.arange(W_rg).float()[None, :]
    return (torch.sin(2 * np.pi * (r + 2.5 * torch.sin(2 * np.pi * c / 61.0)) / 9.0) + 0.5 * torch.cos(0.37 * r + 0.011 * c)
            + 0.25 * torch.randn(H_rg, W_rg, generator=gen)).float()


def _check_rounding(values, name):
    for v in values:
        frac = abs(v * 100 - np.floor(v * 100) - 0.5)
        assert frac > 1e-4, f"{name}: {v!r} sits on a two-digit rounding boundary -- pick another seed"


def _run_main(ref_dataset, rg_path, seg_full, unc_fn, dataset_id, nclasses, remove_unc, flip, use_last, correction, forced_change):
    from sklearn.metrics import classification_report as sk_report, confusion_matrix as sk_matrix
    sys.path.insert(0, os.path.join(mg.REF, "scripts", "test"))
    import test_all as ref_main
    importlib.reload(ref_main)
    rec, saved, calls = {}, {}, {"n": 0}

    def create_dataset(id, length, dim, overlap, full=False, flip=False):
        return ref_dataset.RGDataset(filepath=rg_path, length=length, dim=dim, overlap=overlap, flip=flip)

    def get_reference(id, h, w, flip=False, length=None, dim=None, overlap=None):
        if id == 2:
            data, n = unc_fn(saved["map"]), 4  # asked for after the maps are final (test_all.py:163)
        else:
            data, n = seg_full, nclasses
        data = data[:h, :].clone()
        data = torch.flip(data, (1,)) if flip else data
        if id == 2:
            rec["unc_seg"] = data.clone()
        return n, data

    orig_propagate = ref_main.propagate

    def propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last):
        pred, xent, change = orig_propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last=use_last)
        i = calls["n"]
        calls["n"] += 1
        if forced_change is not None and i < len(forced_change):
            change = forced_change[i]
        return pred, xent, change

    def classification_report(gt, pred):
        g, p = np.asarray(gt), np.asarray(pred)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # UndefinedMetricWarning: the 0 / 0 -> 0.0 cases are wanted
            text = sk_report(gt, pred)
            d = sk_report(gt, pred, output_dict=True)
        rec.update(gt=g.copy(), pred=p.copy(), report=text, dict=d)
        return text

    def confusion_matrix(gt, pred):
        m = sk_matrix(gt, pred)
        rec.update(matrix=m, matrix_str=str(m))
        return m

    ref_main.create_dataset = create_dataset
    ref_main.get_reference = get_reference
    ref_main.create_model = lambda id, pos_embed: mg.PatchFlatten()
    ref_main.load = lambda path: {}
    ref_main.plot = lambda **k: None
    ref_main.propagate = propagate
    ref_main.device_count = lambda: 1
    ref_main.classification_report = classification_report
    ref_main.confusion_matrix = confusion_matrix
    _save = torch.save
    ref_main.torch.save = lambda obj, path: saved.update(map=obj.clone())
    g = GEOM
    args = argparse.Namespace(model=0, dataset=dataset_id, patch_size=g["hw"], seq_length=g["T"], overlap=(g["oh"], 0),
                              cxt_size=LPC["CXT_SIZE"], radius=LPC["RADIUS"], temp=LPC["TEMP"], knn=LPC["KNN"], model_path="",
                              output_folder=tempfile.gettempdir() + "/", pos_embed=False, remove_unc=remove_unc, flip=flip,
                              use_last=use_last, dataset_full=True, correction=correction)
    try:
        with mg.cuda_is_cpu():
            ref_main.main(args)
    finally:
        torch.save = _save
    rec["rows"] = saved["map"].shape[0]
    return rec


def run_report_case(ref_dataset, name, dataset_id, nclasses, seed, remove_unc=True, flip=False, use_last=False, correction=False,
                    forced_change=None, seg_edit=None, unc_fn=None):
    g = GEOM
    gen = torch.Generator().manual_seed(seed)
    W_rg = g["n_rg"] * g["T"] * g["hw"][1]
    rg = _radargram(g["H_rg"], W_rg, gen)
    seg_full = mg.layered_segmentation(g["H_rg"] + g["seg_rows_extra"], W_rg, nclasses, gen)
    if seg_edit is not None:
        seg_full = seg_edit(seg_full)
    with tempfile.TemporaryDirectory() as tmp:
        rg_path = os.path.join(tmp, "rg.pt")
        torch.save(rg, rg_path)
        run = lambda unc: _run_main(ref_dataset, rg_path, seg_full, unc_fn, dataset_id, nclasses, unc, flip, use_last, correction,
                                    forced_change)
        plain = run(False)
        rec = run(remove_unc) if remove_unc else plain
    rows = plain["rows"]
    final_pred, seg = plain["pred"].reshape(rows, -1), plain["gt"].reshape(rows, -1)
    out = dict(dataset_id=np.int32(dataset_id), nclasses=np.int32(nclasses), remove_unc=np.bool_(remove_unc), flip=np.bool_(flip),
               final_pred=final_pred.astype(np.int8), seg=seg.astype(np.int8), gt=rec["gt"].astype(np.int8),
               pred=rec["pred"].astype(np.int8), report=np.array(rec["report"]), matrix=rec["matrix"].astype(np.int64),
               matrix_str=np.array(rec["matrix_str"]))
    assert np.array_equal(final_pred, out["final_pred"]) and np.array_equal(seg, out["seg"])  # small integer labels
    if "unc_seg" in rec:
        out["unc_seg"] = rec["unc_seg"][:rows, :seg.shape[1]].numpy().astype(np.int8)
        keep = out["unc_seg"].reshape(-1) != 4  # the script's own mask, redone on the stored maps: the fixture is self-consistent
        assert np.array_equal(out["gt"], out["seg"].reshape(-1)[keep]) and np.array_equal(out["pred"], out["final_pred"].reshape(-1)[keep])
    d = rec["dict"]
    labels = sorted(k for k in d if k not in ("accuracy", "macro avg", "weighted avg"))
    out["d_labels"] = np.array([float(k) for k in labels])
    for key, short in (("precision", "precision"), ("recall", "recall"), ("f1-score", "f1"), ("support", "support")):
        out["d_" + short] = np.array([d[k][key] for k in labels], dtype=np.float64)
    out["d_accuracy"] = np.float64(d["accuracy"])
    for key, short in (("macro avg", "macro"), ("weighted avg", "weighted")):
        out["d_" + short] = np.array([d[key][k] for k in ("precision", "recall", "f1-score", "support")], dtype=np.float64)
    _check_rounding(list(out["d_precision"]) + list(out["d_recall"]) + list(out["d_f1"]) + [float(out["d_accuracy"])]
                    + list(out["d_macro"][:3]) + list(out["d_weighted"][:3]), name)
    np.savez(os.path.join(HERE, name + ".npz"), **out)
    print(f"{name}: map{final_pred.shape} scored {len(out['gt'])} of {final_pred.size} pixels, classes {labels}, "
          f"accuracy {float(out['d_accuracy']):.4f}, zero precision: {[k for k in labels if d[k]['precision'] == 0.0]}")
    return out


def _band_unc(saved_map):
    """Dataset 0's uncertain map: an undulating band of 4s (the uncertain class) over four flat layers."""
    rows, cols = GEOM["H_rg"] + GEOM["seg_rows_extra"], saved_map.shape[1]
    mid = 24 + 3.0 * torch.sin(2 * np.pi * torch.arange(cols).float() / 47.0)
    r = torch.arange(rows).float()[:, None]
    unc = torch.floor(r * 4 / rows).repeat(1, cols)
    unc[(r - mid[None, :]).abs() < 3.5] = 4.0
    return unc


def main():
    torch.set_num_threads(8)
    _, _, _, ref_dataset, _ = mg.import_reference()
    # dataset 0, remove_unc: pixels inside the uncertain map's band of 4s are dropped (aux mask)
    run_report_case(ref_dataset, "report_ds0_unc_band", 0, 4, 71, unc_fn=_band_unc)
    # dataset 1, remove_unc, reverse pass: class 5 is in both maps and is dropped from both after the merge (gt / pred mask)
    r = run_report_case(ref_dataset, "report_ds1_reverse", 1, 6, 62, use_last=True)
    assert (r["seg"] == 5).any() and (r["final_pred"] == 5).any() and 5.0 not in r["d_labels"]
    # dataset 3, correction + reverse: remove_unc is on and masks nothing
    r = run_report_case(ref_dataset, "report_ds3_correction_reverse", 3, 5, 63, use_last=True, correction=True,
                        forced_change=[None, 5, None])
    assert len(r["gt"]) == r["seg"].size
    # dataset 0, remove_unc off, flipped dataset and reference
    run_report_case(ref_dataset, "report_ds0_flip_plain", 0, 4, 64, remove_unc=False, flip=True)

    # dataset 1 with a class the prediction never produces: a patch of class 4 away from every seed column -> precision 0 / 0
    def lens(seg):
        seg = seg.clone()
        seg[seg == 4] = 3
        seg[10:16, 20:50] = 4
        return seg

    r = run_report_case(ref_dataset, "report_ds1_unpredicted_class", 1, 6, 65, seg_edit=lens)
    i = list(r["d_labels"]).index(4.0)
    assert r["d_precision"][i] == 0.0 and r["d_support"][i] > 0 and not (r["final_pred"] == 4).any()

    # dataset 0 where the uncertain band covers every pixel that has class 3 in the reference or in the prediction: the class is
    # absent from both after masking -> sklearn drops its row and column, macro average over three classes
    def cover3(saved_map):
        rows = saved_map.shape[0]
        return torch.where((seg66[:rows] == 3) | (saved_map.float() == 3), 4.0, 0.0)

    gen = torch.Generator().manual_seed(66)
    W_rg = GEOM["n_rg"] * GEOM["T"] * GEOM["hw"][1]
    _radargram(GEOM["H_rg"], W_rg, gen)  # same generator order as run_report_case
    seg66 = mg.layered_segmentation(GEOM["H_rg"] + GEOM["seg_rows_extra"], W_rg, 4, gen)
    r = run_report_case(ref_dataset, "report_ds0_class_removed", 0, 4, 66, unc_fn=cover3)
    assert list(r["d_labels"]) == [0.0, 1.0, 2.0] and r["matrix"].shape == (3, 3) and (r["seg"] == 3).any()


if __name__ == "__main__":
    main()
