"""Anchors in the parameter sweep, without a device: `segment_sweep.py --anchors / --anchor_every` (segment_all.py's flags and
refusals), the run with them through a stubbed `propagate_sweep` -- the same anchors in both passes, the count printed, the json's
``anchors`` --, the run without them against the recorded stdout, and `utils.propagate_sweep`'s hand-over to the sweep.  The maps
themselves are tests/test_sweep_anchored_gpu.py's."""
import os

import pytest
import torch

from conftest import ROOT
from test_sweep_posterior import BASE, GOLDEN_ARGS, _cli, run_sweep_cli, stub_propagate_sweep

SLIDING = ["--context", "sliding"]


def test_the_script_has_segment_alls_two_flags_and_refusals():
    cli = _cli()
    check = lambda *extra: cli.segment_all.check_anchor_flags(cli.check_confidence_flags(cli.with_defaults(cli.get_args_parser().parse_args(BASE + list(extra)))))
    plain = check()
    assert plain.anchors is None and plain.anchor_every is None
    a = check("--anchor_every", "3", *SLIDING)
    assert a.anchor_every == 3 and a.anchors is None
    assert check("--anchors", "a.pt", *SLIDING).anchors == "a.pt"
    for flags, msg in ((["--anchor_every", "4"], "need --context sliding"),
                       (["--anchor_every", "4", "--correction", "true", *SLIDING], "--correction"),
                       (["--anchor_every", "0", *SLIDING], "at least 1"),
                       (["--anchor_every", "4", "--anchors", "a.pt", *SLIDING], "one of the two")):
        with pytest.raises(SystemExit, match=msg):
            check(*flags)


def test_without_the_flags_the_script_prints_the_recorded_stdout(monkeypatch, capsys, tmp_path):
    text, d = run_sweep_cli(monkeypatch, capsys, tmp_path, GOLDEN_ARGS, propagate_sweep=stub_propagate_sweep)
    assert text == open(os.path.join(ROOT, "tests", "golden", "segment_sweep_stdout.txt")).read()
    assert "anchors" not in d and "anchor" not in text.lower()


def test_with_anchor_every_both_passes_get_the_anchors_and_the_count_is_reported(monkeypatch, capsys, tmp_path):
    seen = []

    def stub(seq, seg_ref, model, sweep, ncls, do_pos_embed, use_last, confidence=None, soft=False, anchors=None):
        seen.append((use_last, None if anchors is None else anchors.clone()))
        return stub_propagate_sweep(seq, seg_ref, model, sweep, ncls, do_pos_embed, use_last, confidence=confidence, soft=soft)

    text, d = run_sweep_cli(monkeypatch, capsys, tmp_path, GOLDEN_ARGS + SLIDING + ["--anchor_every", "3"], propagate_sweep=stub)
    T, step, rg_len = 8, 8, 64                                  # BASE: two radargrams of 8 frames of 8 columns
    cols = [t * rg_len + f * step for t in range(2) for f in (3, 6)]
    assert "Anchored traces: 4\n" in text and "anchor_every=3" in text and "context='sliding'" in text
    assert d["anchors"] == dict(traces=4, columns=cols, source="every 3 frames of the reference map") and d["context"] == "sliding"
    assert [u for u, _ in seen] == [False, False, True, True]
    for (_, a), t in zip(seen, (0, 1, 0, 1)):                   # the item's frame order in BOTH passes: the flip is `propagate_sweep`'s
        assert a.dtype == torch.int8 and a.shape[0] == T and a.ne(-1).any(1).nonzero().reshape(-1).tolist() == [3, 6]
        assert torch.equal(a, seen[t][1])


def test_propagate_sweep_flips_the_anchors_with_the_item(monkeypatch):
    import crw_hip
    import utils as crw_utils
    T, N, M = 5, 4, 3
    anchors = torch.full((T, N), -1, dtype=torch.int8)
    anchors[1], anchors[3, 2] = 2, 1
    got = {}

    class Sweep:
        configs = [dict(), dict()]

        def propagate_all(self, feats, seed, nclasses, soft=False, anchors=None):
            got["anchors"] = anchors
            return torch.zeros(2, N, T)

    monkeypatch.setattr(crw_utils, "_features_and_seed", lambda *a: (torch.zeros(T, N, 8), torch.zeros(N)))
    monkeypatch.setattr(crw_hip, "xent_metric", lambda feats: torch.zeros(N, T - 1))
    monkeypatch.setattr(crw_utils, "column_diffs_async", lambda xent: None)
    monkeypatch.setattr(crw_utils, "change_point", lambda xent, diffs: None)
    seq = torch.zeros(T, N, 4, 4)
    for use_last in (False, True):
        crw_utils.propagate_sweep(seq, torch.zeros(8, 4), None, Sweep(), M, False, use_last, anchors=anchors)
        assert torch.equal(got["anchors"], torch.flip(anchors, (0,)) if use_last else anchors) and got["anchors"].is_contiguous()
    crw_utils.propagate_sweep(seq, torch.zeros(8, 4), None, Sweep(), M, False, False)
    assert got["anchors"] is None
