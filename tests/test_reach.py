"""Accuracy against the distance from the nearest labelled trace, on the CPU: `crw_hip.column_groups` and the CPU route of
`crw_hip.confusion_grouped` against the plain loops of tests/reach_ref.py, `metrics.Reach`, `inference.labelled_columns` against a hand
count, the command-line flags, and THE TABLE of the README: the nine drifting items of tests/sliding_ref.py binned by frames from the
seed under the two context rules.  No GPU."""
import json

import numpy as np
import pytest
import torch

import reach_ref as rr
from test_confidence import Flatten, _cli, run_cli


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------ column groups
GROUP_CASES = [
    # cols, labelled, step, edges, segments, direction
    (40, [3, 29], 1, None, None, "both"),
    (40, [3, 29], 1, None, None, "forward"),
    (40, [3, 29], 1, None, None, "backward"),
    (61, [0, 1, 2, 3, 57, 58, 59, 60], 4, None, None, "both"),
    (50, [7], 3, None, None, "both"),                          # a step that does not divide the distances
    (50, [7, 8, 30], 5, [1, 4, 6], None, "forward"),           # custom edges
    (64, [5, 6], 2, None, [0, 20, 64], "both"),                # two segments, a labelled column in only one
    (64, [5, 40], 2, [2, 3, 10], [0, 20, 64], "backward"),
    (30, [], 1, None, None, "both"),                           # nothing labelled: every column unreached
    (700, [0, 699], 1, None, None, "forward"),                 # the far default groups: 257-
]


@pytest.mark.parametrize("case", GROUP_CASES, ids=lambda c: f"{c[0]}-{c[2]}-{c[5]}")
def test_column_groups_are_the_loops(case):
    import crw_hip
    cols, labelled, step, edges, segments, direction = case
    want_g, want_f = rr.column_groups(cols, labelled, step, edges, segments, direction)
    group, frames = crw_hip.column_groups(cols, labelled, step, edges=edges, segments=segments, direction=direction)
    assert group.dtype == torch.uint8 and frames.dtype == torch.int64 and tuple(group.shape) == tuple(frames.shape) == (cols,)
    assert np.array_equal(group.numpy(), want_g) and np.array_equal(frames.numpy(), want_f)
    n = len(rr.DEFAULT_EDGES if edges is None else edges)
    assert int(group.max()) <= n + 1 and ((frames < 0) == (group == n + 1)).all()


def test_column_groups_by_hand():
    import crw_hip
    assert crw_hip.REACH_EDGES == rr.DEFAULT_EDGES
    group, frames = crw_hip.column_groups(12, [2], 1)
    assert frames.tolist() == [2, 1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9] and group.tolist() == [2, 1, 0, 1, 2, 3, 3, 4, 4, 4, 4, 5]
    group, frames = crw_hip.column_groups(8, [2], 3, direction="forward")
    assert frames.tolist() == [-1, -1, 0, 1, 1, 1, 2, 2] and group.tolist() == [11, 11, 0, 1, 1, 1, 2, 2]
    group, frames = crw_hip.column_groups(6, [0], 1, segments=[0, 3, 6])               # an item never reads another item's labels
    assert frames.tolist() == [0, 1, 2, -1, -1, -1]


def test_column_groups_refusals():
    import crw_hip
    cg = crw_hip.column_groups
    for kw, msg in ((dict(step=0), "step must be at least 1"), (dict(direction="left"), "direction must be one of"),
                    (dict(edges=[0, 1]), "strictly increasing integers >= 1"), (dict(edges=[1, 3, 3]), "strictly increasing"),
                    (dict(edges=[1.5, 2]), "strictly increasing integers"), (dict(edges=list(range(1, 64))), "at most 62 edges"),
                    (dict(segments=[1, 10]), "segments must be offsets"), (dict(segments=[0, 5, 5, 10]), "segments must be offsets"),
                    (dict(segments=[0, 9]), "segments must be offsets"), (dict(labelled=[10]), "lie outside"),
                    (dict(labelled=[-1]), "lie outside"), (dict(labelled=[1.5]), "must be integers"), (dict(cols=-1), "cols must be")):
        args = dict(cols=10, labelled=[0], step=1)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            cg(args.pop("cols"), args.pop("labelled"), args.pop("step"), **args)
    assert cg(10, [0], 1, edges=list(range(1, 63)))[0].max() <= 63                      # 62 edges: 64 groups


# ------------------------------------------------------------------------------------------------ the CPU route
CPU_CASES = [
    # rows, cols, K, dg, dp, da, conf, ignore, groups
    (1, 1, 2, "f32", "f32", None, False, False, "one"),
    (3, 5, 2, "f32", "i8", None, True, False, "default"),
    (7, 33, 5, "i8", "i8", "i8", True, True, "own"),
    (37, 131, 5, "f32", "f32", "f32", True, True, "holes"),
    (64, 256, 16, "f32", "i8", "i8", False, True, "default"),
    (20, 64, 16, "i8", "i8", None, True, False, "own"),
]


def _both(c, group, groups, K):
    import crw_hip
    kw = dict(aux=c["aux"], ignore_gt=c["ignore_gt"], ignore_pred=c["ignore_pred"], ignore_aux=c["ignore_aux"])
    want = rr.confusion_grouped(c["gt"], c["pred"], K, group, groups, conf=c["conf"], **kw)
    kw["aux"] = _t(c["aux"])
    got = crw_hip.confusion_grouped(_t(c["gt"]), _t(c["pred"]), K, _t(group), groups, conf=_t(c["conf"]), **kw)
    return want, got


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_cpu_route_is_the_loops(case):
    rows, cols, K, dg, dp, da, conf, ignore, kind = case
    c = rr.case(rows, cols, K, rows * cols + K, dg, dp, da, conf, ignore)
    group, groups = rr.group_maps(cols, kind)
    (wc, ws, wd), (counts, conf_sum, dropped) = _both(c, group, groups, K)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (groups, K, K) and tuple(dropped.shape) == (4,)
    assert np.array_equal(counts.numpy(), wc) and np.array_equal(dropped.numpy(), wd)
    assert int(counts.sum() + dropped.sum()) == rows * cols
    if conf:
        assert conf_sum.dtype == torch.float64 and np.allclose(conf_sum.numpy(), ws, rtol=rows * cols * 2.0 ** -52, atol=0)
    else:
        assert conf_sum is None and wd[2] == 0
    if rows * cols >= 200:                                                              # what is planted shows
        assert wd[1] > 0 and (not ignore or wd[0] > 0) and (not conf or wd[2] > 0) and (kind != "holes" or wd[3] > 0)


def test_cpu_route_on_windows_empty_maps_and_its_refusals():
    import crw_hip
    K = 5
    c = rr.case(9, 50, K, 3, "f32", "i8", None, True, False)
    group, groups = rr.group_maps(20, "default")
    win = lambda a: _t(a)[:, 11:31]                                                     # a column window of a wider map
    got = crw_hip.confusion_grouped(win(c["gt"]), win(c["pred"]), K, _t(group), groups, conf=win(c["conf"]))
    want = rr.confusion_grouped(c["gt"][:, 11:31], c["pred"][:, 11:31], K, group, groups, conf=c["conf"][:, 11:31])
    assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[2].numpy(), want[2])
    one = crw_hip.confusion_grouped(win(c["gt"]), win(c["pred"]), K, torch.zeros(20, dtype=torch.uint8), 1)
    plain = crw_hip.confusion(win(c["gt"]), win(c["pred"]), K)
    assert torch.equal(one[0][0], plain[0]) and torch.equal(one[2][:2], plain[1]) and one[1] is None
    for shape in ((0, 7), (7, 0)):
        e = torch.zeros(shape)
        counts, conf_sum, dropped = crw_hip.confusion_grouped(e, e, K, torch.zeros(shape[1], dtype=torch.uint8), 3, conf=e)
        assert not counts.any() and not conf_sum.any() and not dropped.any()
    g, p, grp = _t(c["gt"]), _t(c["pred"]), torch.zeros(50, dtype=torch.uint8)
    for call, msg in ((lambda: crw_hip.confusion_grouped(g, p, K, grp, 0), "groups must be in 1 ... 64"),
                      (lambda: crw_hip.confusion_grouped(g, p, K, grp, 65), "groups must be in 1 ... 64"),
                      (lambda: crw_hip.confusion_grouped(g, p, 17, grp, 1), "K must be in 2 ... 16"),
                      (lambda: crw_hip.confusion_grouped(g.reshape(-1), p.reshape(-1), K, grp, 1), r"\[rows, cols\] map"),
                      (lambda: crw_hip.confusion_grouped(g, p[:, :49], K, grp, 1), "same number of pixels"),
                      (lambda: crw_hip.confusion_grouped(g, p, K, grp[:49], 1), "col_group must be uint8"),
                      (lambda: crw_hip.confusion_grouped(g, p, K, grp.to(torch.int64), 1), "col_group must be uint8"),
                      (lambda: crw_hip.confusion_grouped(g, p, K, grp, 1, conf=p), "floating-point map"),
                      (lambda: crw_hip.confusion_grouped(g, p, K, grp, 1, ignore_aux=4), "ignore_aux needs aux")):
        with pytest.raises(ValueError, match=msg):
            call()


# ------------------------------------------------------------------------------------------------ metrics.Reach
def _hand_counts(acc_by_group, K=3, n=100):
    """[groups, K, K] counts with n pixels per group (0 where the accuracy is None), `acc` of them on the diagonal"""
    counts = np.zeros((len(acc_by_group), K, K), np.int64)
    for g, a in enumerate(acc_by_group):
        if a is not None:
            right = int(round(a * n))
            counts[g, 0, 0], counts[g, 1, 1], counts[g, 0, 2] = right // 2, right - right // 2, n - right
    return counts


def test_reach_arithmetic_on_hand_made_counts():
    from metrics import Reach, Report
    # groups {0} {1} {2} {3-4} {5-8} {9-16} {17-32} {33-64} {65-128} {129-256} {257-} unreached
    acc = [1.0, 0.97, 0.95, None, 0.92, 0.91, 0.5, 0.99, None, None, None, 0.3]
    r = Reach(_hand_counts(acc), conf_sum=np.arange(12) * 10.0, dropped=(4, 0, 2, 7))
    assert r.groups == 12 and r.K == 3 and r.unreached == 11 and r.total == 800
    assert r.frames[:4] == [(0, 0), (1, 1), (2, 2), (3, 4)] and r.frames[10] == (257, None) and r.frames[11] is None
    assert r.pixels.tolist() == [100, 100, 100, 0, 100, 100, 100, 100, 0, 0, 0, 100] and r.correct[1] == 97
    assert r.accuracy[1] == 0.97 and np.isnan(r.accuracy[3]) and np.isnan(r.mean_iou[3]) and np.isnan(r.mean_confidence[8])
    assert r.mean_confidence[4] == 0.4 and r.mean_iou[6] == Report(r.counts[6]).mean_iou == r.report(6).mean_iou
    assert r.report(1).accuracy == 0.97 and r.report(1).dropped == (4, 0)
    # the run 1, 2, (3-4 empty: skipped), 5-8, 9-16 holds 0.9; 17-32 breaks it, whatever lies behind
    assert r.reach_at(0.9) == 16 and r.reach_at(0.915) == 8 and r.reach_at(0.96) == 1 and r.reach_at(0.98) == 0 and r.reach_at(0.0) == 64
    # a group the map only partly fills counts up to the distance it holds; the unreached group never counts
    part = Reach(_hand_counts(acc), last_frame=[0, 1, 2, -1, 8, 12, 29, 40, -1, -1, -1, -1])
    assert part.frames[5] == (9, 12) and part.frames[3] == (3, 4) and part.reach_at(0.9) == 12 and part.reach_at(0.0) == 40
    assert np.isnan(part.mean_confidence).all()
    every = Reach(_hand_counts([1.0] + [0.95] * 10 + [0.0]))
    assert every.reach_at(0.9) == 257                                                   # the open group counts from its first distance
    assert Reach(_hand_counts([None] * 12)).reach_at(0.5) == 0 and Reach(_hand_counts([1.0, 0.2] + [1.0] * 10)).reach_at(0.9) == 0
    d = r.to_dict()
    assert json.loads(json.dumps(d).replace("NaN", "null"))["pixels"] == r.pixels.tolist()
    assert d["groups"] == 12 and d["frames"][3] == [3, 4] and d["frames"][11] is None and d["edges"] == list(rr.DEFAULT_EDGES)
    assert d["dropped"] == dict(masked=4, invalid=0, invalid_confidence=2, excluded=7) and d["accuracy"][1] == 0.97 and d["total"] == 800
    for bad, msg in ((dict(counts=np.zeros((11, 3, 3))), "len\\(edges\\) \\+ 2"), (dict(counts=np.zeros((12, 3, 2))), "K, K"),
                     (dict(counts=-np.ones((12, 3, 3))), "non-negative"), (dict(conf_sum=np.zeros(5)), "one sum per group"),
                     (dict(last_frame=[0] * 5), "one distance per group"), (dict(last_frame=[0, 1, 2, 9] + [-1] * 8), "group 3 holds")):
        kw = dict(counts=_hand_counts(acc))
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            Reach(**kw)


def test_reach_table_text():
    from metrics import Reach
    acc = [1.0, 0.97, None, 0.5]
    r = Reach(_hand_counts(acc), conf_sum=[90.0, 80.0, 0.0, 25.0], edges=(1, 3), last_frame=[0, 2, -1, -1])
    lines = str(r).split("\n")
    assert lines[0] == "{:>13} {:>12} {:>12} {:>10} {:>10} {:>10}".format("frames", "pixels", "correct", "accuracy", "mean IoU", "mean conf")
    assert lines[1] == "" and len(lines) == 7 and lines[6] == "" and len({len(l) for l in lines[2:6]}) == 1
    assert lines[2].split() == ["0", "100", "100", "1.0000", "1.0000", "0.9000"]
    assert lines[3].split() == ["1-2", "100", "97", "0.9700", f"{r.mean_iou[1]:.4f}", "0.8000"]
    assert lines[4].split() == ["3-", "0", "0", "-", "-", "-"] and lines[5].split()[0] == "unreached" and lines[5].split()[3] == "0.5000"


def test_label_reach_follows_evaluates_rules_and_raises_on_invalid_labels():
    import crw_hip
    import inference
    rng = np.random.default_rng(5)
    rows, cols = 12, 40
    seg = torch.from_numpy(rng.integers(0, 6, (rows, cols))).to(torch.int8)
    pred = torch.from_numpy(rng.integers(0, 6, (rows, cols))).to(torch.int8)
    conf = torch.from_numpy(rng.random((rows, cols)).astype(np.float32))
    r = inference.label_reach(pred, seg, 1, [0, 1], 2, conf=conf)                      # dataset 1: gt or pred 5 is masked
    ev = inference.evaluate(pred, seg, 1)
    assert r.total == ev.total and int(r.correct.sum()) == int(np.trace(ev.counts)) and r.dropped[:2] == ev.dropped
    assert np.array_equal(r.counts.sum(0), ev.counts) and r.dropped[2:] == (0, 0)
    group, frames = crw_hip.column_groups(cols, [0, 1], 2)
    want = rr.confusion_grouped(seg.numpy(), pred.numpy(), 6, group.numpy(), 12, conf=conf.numpy(), ignore_gt=5, ignore_pred=5)
    assert np.array_equal(r.counts, want[0]) and np.allclose(r.conf_sum, want[1], rtol=1e-12)
    assert r.frames[5] == (9, 16) and r.frames[6] == (17, 19) and r.frames[7] == (33, 64) and r.pixels[7] == 0      # 38 columns: 19 frames
    unc = (torch.arange(cols)[None, :] % 7 == 0).to(torch.int8).expand(rows, cols) * 4
    r0 = inference.label_reach(pred.clamp(max=3), seg.clamp(max=3), 0, [0], 1, unc_seg=unc, direction="forward")
    assert r0.dropped[0] == rows * 6 and r0.total == rows * cols - rows * 6
    sweep = inference.label_reach_sweep(torch.stack([pred, seg]), seg, 1, [0, 1], 2, conf=torch.stack([conf, conf]))
    assert np.array_equal(sweep[0].counts, r.counts) and np.array_equal(sweep[0].conf_sum, r.conf_sum) and sweep[0].frames == r.frames
    assert sweep[1].accuracy[0] == 1.0 and int(sweep[1].correct.sum()) == sweep[1].total
    bad = pred.float()
    bad[3, 7] = 2.5
    with pytest.raises(crw_hip.LabelError, match="1 unmasked label"):
        inference.label_reach(bad, seg, 1, [0], 1)
    with pytest.raises(crw_hip.LabelError):
        inference.label_reach_sweep(torch.stack([pred.float(), bad]), seg, 1, [0], 1)
    with pytest.raises(ValueError, match=r"\[rows, cols\] map"):
        inference.label_reach(pred.reshape(-1), seg, 1, [0], 1)
    with pytest.raises(ValueError, match="conf .* must cover the same pixels"):
        inference.label_reach(pred, seg, 1, [0], 1, conf=conf[:, :5])


# ------------------------------------------------------------------------------------------------ labelled_columns
def test_labelled_columns_against_a_hand_count():
    """96 x 320 with 16 x 16 patches, seq_length 10: two items of 160 columns, frames of 16 columns"""
    import crw_hip
    import inference
    args = (320, 10, (16, 16), (0, 0))
    lab, segments, direction, step = inference.labelled_columns(*args, False)
    assert lab == list(range(0, 16)) + list(range(160, 176)) and segments == [0, 160, 320] and direction == "forward" and step == 16
    group, frames = crw_hip.column_groups(320, lab, step, segments=segments, direction=direction)
    assert frames.tolist() == [c % 160 // 16 for c in range(320)]                        # the distance IS the frame index
    assert torch.bincount(group.long(), minlength=12).tolist() == [32, 32, 32, 64, 128, 32, 0, 0, 0, 0, 0, 0]
    lab, segments, direction, step = inference.labelled_columns(*args, True)
    assert lab == sorted(list(range(0, 16)) + list(range(144, 176)) + list(range(304, 320))) and direction == "both"
    group, frames = crw_hip.column_groups(320, lab, step, segments=segments, direction=direction)
    assert frames.tolist() == [min(c % 160 // 16, 9 - c % 160 // 16) for c in range(320)]
    assert torch.bincount(group.long(), minlength=12).tolist() == [64, 64, 64, 128, 0, 0, 0, 0, 0, 0, 0, 0]
    lab, _, _, _ = inference.labelled_columns(*args, False, anchor_cols=[70])           # column 70: frame 4 of item 0, columns 64 ... 79
    assert lab == list(range(0, 16)) + list(range(64, 80)) + list(range(160, 176))
    _, frames = crw_hip.column_groups(320, lab, step, segments=segments, direction="forward")
    assert frames[:160].tolist() == [f if f < 4 else f - 4 for f in (c // 16 for c in range(160))]
    lab, _, direction, _ = inference.labelled_columns(*args, True, anchor_cols=[170], seeds=False)      # a seedless run: the anchors alone
    assert lab == list(range(160, 176)) and direction == "both"
    group, _ = crw_hip.column_groups(320, lab, step, segments=segments)
    assert (group[:160] == 11).all() and (group[160:] < 11).all()                       # the item without anchors is unreached
    # overlapping frames: 8 fresh columns per frame, the seed frame still 16 wide; a map wider than its whole items
    lab, segments, _, step = inference.labelled_columns(200, 10, (16, 16), (0, 8), True, anchor_cols=[87])
    assert step == 8 and segments == [0, 88, 176] and lab == sorted(set(range(0, 16)) | set(range(72, 104)) | set(range(160, 176)))
    with pytest.raises(ValueError, match="outside"):
        inference.labelled_columns(*args, False, anchor_cols=[320])
    with pytest.raises(ValueError, match="hold no item"):
        inference.labelled_columns(100, 10, (16, 16), (0, 0), False)


# ------------------------------------------------------------------------------------------------ the command line
def test_segment_all_flags(monkeypatch, capsys, tmp_path):
    import inference
    cli = _cli()
    p = cli.get_args_parser()
    for bad, msg in ((["--reach", "--single"], "not available with --single"), (["--reach", "--correction", "true"], "do not combine"),
                     (["--reach_edges", "1", "2"], "need --reach"), (["--reach_accuracy", "0.5"], "need --reach"),
                     (["--reach", "--reach_edges", "2", "2"], "strictly increasing"), (["--reach", "--reach_accuracy", "1.5"], "0 ... 1")):
        with pytest.raises(SystemExit, match=msg):
            cli.check_reach_flags(cli.with_defaults(p.parse_args(["--model_path", "x.pt"] + bad)))
    plain, _, d0 = run_cli(monkeypatch, capsys, tmp_path / "a", [])
    assert "reach" not in d0 and "nearest labelled trace" not in plain and "reach" not in plain.split("\n")[0]
    given = []
    real = inference.label_reach
    monkeypatch.setattr(inference, "label_reach", lambda *a, **kw: given.append((a, kw)) or real(*a, **kw))
    text, files, d = run_cli(monkeypatch, capsys, tmp_path / "b", ["--reach", "--reach_edges", "1", "2", "4", "--reach_accuracy", "0.5",
                                                                  "--confidence", "maxprob"])
    (a, kw), = given
    # CLI_ARGS: 384 columns, patches 8 x 8, seq_length 8, --use_last: six items of 64 columns, both directions
    assert kw["segments"] == list(range(0, 385, 64)) and kw["direction"] == "both" and kw["edges"] == [1, 2, 4] and a[4] == 8
    assert a[3] == sorted(c for t in range(6) for c in list(range(64 * t, 64 * t + 8)) + list(range(64 * t + 56, 64 * t + 64)))
    assert kw["conf"] is not None and tuple(a[0].shape) == (40, 384)
    r = d["reach"]
    assert r["groups"] == 5 and r["step"] == 8 and r["direction"] == "both" and r["at_accuracy"] == 0.5 and r["frames"][:3] == [[0, 0], [1, 1], [2, 3]]
    assert r["pixels"][3:] == [0, 0] and all(r["pixels"][:3]) and r["total"] == int(np.sum(d["matrix"])) == sum(r["pixels"])   # frames 0 ... 3
    assert r["dropped"] == dict(masked=d["dropped"]["masked"], invalid=0, invalid_confidence=0, excluded=0)
    assert sum(r["correct"]) == int(np.trace(np.array(d["matrix"]))) and r["reach"] == real(*a, **kw).reach_at(0.5)
    i_iou, i_reach = text.index("iou\n"), text.index("Accuracy against the distance from the nearest labelled trace (frames of 8 columns, both):")
    assert i_iou < i_reach and f"Reach at accuracy 0.5: {r['reach']} frames" in text and "reach=True" in text.split("\n")[0]
    rest = lambda s: s[s.index("\n"):]
    text2, _, d2 = run_cli(monkeypatch, capsys, tmp_path / "c", ["--reach"])            # nothing else changes but the block
    end = text2.index("frames\n", text2.index("Reach at accuracy 0.9")) + len("frames\n")
    assert d2["reach"]["at_accuracy"] == 0.9 and d2["matrix"] == d0["matrix"]
    assert rest(text2[:text2.index("Accuracy against the distance") - 1] + text2[end:]) == rest(plain)


def _sweep_cli():
    import importlib.util
    import os
    import sys
    from test_confidence import PKG
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("segment_sweep", os.path.join(PKG, "scripts", "segment_sweep.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(PKG, "scripts"))
    return mod


def test_segment_sweep_flags(monkeypatch, capsys, tmp_path):
    """the reach column, --select reach (the LARGEST wins, ties go to the first in grid order) and the json, on stub reaches"""
    import inference
    from metrics import Reach
    cli = _sweep_cli()
    with pytest.raises(SystemExit):
        cli.get_args_parser().parse_args(["--select", "reach"])                        # offered only with --reach
    p = cli.get_args_parser(reach=True)
    base = ["--synthetic", "40", "128", "--dataset", "3", "--patch_size", "8", "8", "--overlap", "0", "0", "--seq_length", "8", "-c", "2",
            "-r", "2", "3", "-t", "0.1", "-k", "2", "3", "--model", "0", "--output_folder", str(tmp_path)]
    with pytest.raises(SystemExit, match="--select reach needs --reach"):
        cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + ["--select", "reach"])))

    def stub_sweep(dataset, seg, encoder, sweep, nclasses, T, patch, overlap, **kw):
        G = len(sweep.configs)
        return dict(pred=seg[None, :, :128].expand(G, -1, -1).contiguous().to(torch.int8), forward=seg[None, :, :128].expand(G, -1, -1).to(torch.int8),
                    xent=[], change_idx=[None, None])

    # reach at 0.9 of the four configurations: 1, 4, 4, 2 -> configuration 1 wins (the first of the two largest)
    accs = ([1, .95, .5, .5, .5], [1, .95, .95, .95, .5], [1, .95, .95, .95, .5], [1, .95, .95, .5, .5])
    given = []

    def stub_reach(pred, seg, dataset_id, labelled, step, **kw):
        given.append((labelled, step, kw))
        return [Reach(_hand_counts(list(a) + [None] * 7), last_frame=[0, 1, 2, 4, 7] + [-1] * 7) for a in accs]

    monkeypatch.setattr(inference, "segment_sweep", stub_sweep)
    monkeypatch.setattr(inference, "label_reach_sweep", stub_reach)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    js = tmp_path / "s.json"
    capsys.readouterr()
    reports, best = cli.main(p.parse_args(base + ["--reach", "--select", "reach", "--report_json", str(js)]))
    text = capsys.readouterr().out
    assert best == 1 and "Best by reach: radius 2 temp 0.1 knn 3 (4.0000)" in text
    (labelled, step, kw), = given
    assert step == 8 and labelled == list(range(0, 8)) + list(range(64, 72)) and kw["segments"] == [0, 64, 128] and kw["direction"] == "forward"
    head = next(l for l in text.split("\n") if l.lstrip().startswith("radius"))
    rows = text.split("\n")[text.split("\n").index(head) + 1:][:4]
    assert head.endswith("  reach") and [l.split()[-1] for l in rows] == ["1", "4", "4", "2"]
    d = json.load(open(js))
    assert [c["reach"]["reach"] for c in d["configs"]] == [1, 4, 4, 2] and d["reach"] == dict(step=8, direction="forward", at_accuracy=0.9)
    assert d["select"] == "reach" and d["best"]["index"] == 1 and "Accuracy against the distance" in text
    del given[:]
    cli.main(cli.get_args_parser().parse_args(base + ["--report_json", str(js)]))      # without the flag: no column, no key, no call
    text = capsys.readouterr().out
    d = json.load(open(js))
    assert not given and "reach" not in text and "reach" not in d and all("reach" not in c for c in d["configs"])


# ------------------------------------------------------------------------------------------------ THE TABLE
def _drift_reach(cls, pred, M):
    import inference
    return inference.label_reach(torch.from_numpy(pred), torch.from_numpy(cls), 3, [0], 1, direction="forward", nclasses=M)


def test_the_table_labels_travel_under_the_sliding_rule_only():
    """The nine drifting items, node maps [N, T] as label maps with one column per frame, labelled column 0, direction forward:
    wrong node labels by frames from the seed.  Sliding rule: every populated group >= 0.9 (measured worst 12 / 13) and
    reach_at(0.9) == T - 1; reference rule: the last populated group <= 0.6 (measured highest 0.55) and reach_at(0.9) <= 16
    (measured 16, 8, 8, then 16 for the six others)."""
    names = {3: "3-4", 4: "5-8", 5: "9-16", 6: "17-32", 7: "33-64"}
    for T, N, M, cxt, seed, cls, ref, sliding in rr.drift_maps():
        rs, rf = _drift_reach(cls, sliding, M), _drift_reach(cls, ref, M)
        filled = [g for g in range(rs.groups) if rs.pixels[g]]
        assert rs.total == rf.total == N * T and rs.pixels.tolist() == rf.pixels.tolist() and rs.frames[filled[-1]][1] == T - 1
        wrong = lambda r: ", ".join(f"{names.get(g, g)}: {int(r.pixels[g] - r.correct[g])} of {int(r.pixels[g])}" for g in filled)
        print(f"[{T}, {N}] cxt {cxt} seed {seed}: reference {wrong(rf)}; reach {rf.reach_at(0.9)} | sliding {wrong(rs)}; reach {rs.reach_at(0.9)}")
        assert all(rs.accuracy[g] >= 0.9 for g in filled), (T, N, seed, rs.accuracy)
        assert rs.reach_at(0.9) == T - 1
        assert rf.accuracy[filled[-1]] <= 0.6, (T, N, seed, rf.accuracy)
        assert rf.reach_at(0.9) <= 16
        assert rs.accuracy[0] == rf.accuracy[0] == 1.0                                  # the seed frame is the reference's labels
