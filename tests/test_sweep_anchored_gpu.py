"""Anchors in the parameter sweep, on the device: `inference.segment_sweep(..., anchors=)` against `inference.segment(..., anchors=)`
per configuration.  The case is tests/test_anchored_gpu.py::test_segment_with_anchors_at_three_columns': 96 x 320, two radargrams
of T = 10, reverse pass, 'maxprob', merge='confidence', anchors at three columns -- on a 2 x 1 x 2 grid (two (radius, temp) pairs:
the batch call takes a per-configuration I; knn 4 is padded to 8).  Labels compared after .to(int8), confidences bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = dict(radii=[4, 6], temps=[0.1], knns=[4, 8])


@pytest.fixture(scope="module")
def case():
    import crw_hip
    import inference as crw_inference
    from imported.labelprop import LabelPropSweep
    from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_sliding() and crw_hip.has_sweep() and crw_hip.has_anchor_lists()
    enc, fresh, seg, _, N = e2e_case(0, n_rg=2, H=100)
    T, Wp = T_E2E, PATCH[1]
    step = Wp - OVERLAP[1]
    rg_len = T * step + OVERLAP[1]
    assert (seg.shape[0], 2 * rg_len) == (96, 320)
    cols = [2 * step + 5, 6 * step, rg_len + 4 * step + 9]                    # frames 2 and 6 of radargram 0, frame 4 of radargram 1
    sweep = LabelPropSweep(6, context="sliding", **GRID)
    kw = dict(use_last=True, dataset_id=2, confidence="maxprob", merge="confidence")
    run = lambda **extra: crw_inference.segment_sweep(fresh(), seg, enc, sweep, M_E2E, T, PATCH, OVERLAP, **kw, **extra)
    return dict(enc=enc, fresh=fresh, seg=seg, N=N, T=T, step=step, rg_len=rg_len, cols=cols, sweep=sweep, kw=kw, run=run, M=M_E2E,
                patch=PATCH, overlap=OVERLAP, out=run(anchors=(seg, cols)))


def test_slice_g_is_segment_with_the_same_anchors(case):
    import inference as crw_inference
    from imported.labelprop import LabelPropVOS_CRW
    out, c = case["out"], case
    assert out["anchor_cols"] == sorted(c["cols"]) and len(c["sweep"].configs) == 4 == out["pred"].shape[0]
    for g, cfg in enumerate(c["sweep"].configs):
        one = crw_inference.segment(c["fresh"](), c["seg"], c["enc"], LabelPropVOS_CRW(cfg), c["M"], c["T"], c["patch"], c["overlap"],
                                    anchors=(c["seg"], c["cols"]), **c["kw"])
        for k in ("pred", "forward"):
            assert torch.equal(out[k][g], one[k].to(torch.int8)), (k, cfg)
        for k in ("conf", "forward_conf"):
            assert torch.equal(out[k][g].view(torch.int32), one[k].view(torch.int32)), (k, cfg)
        assert one["anchor_cols"] == out["anchor_cols"]
    assert len({tuple(out["pred"][g].flatten().tolist()) for g in range(4)}) > 1          # the configurations differ


def test_anchored_frames_carry_the_node_labels_with_confidence_1_in_every_configuration(case):
    import inference as crw_inference
    import utils as crw_utils
    c, out = case, case["out"]
    rows = c["seg"].shape[0]
    rg_h = c["N"] * (c["patch"][0] - c["overlap"][0]) + c["overlap"][0]
    nodes = crw_utils.anchor_nodes(c["seg"], c["cols"], c["rg_len"], c["T"], c["N"], rg_h, c["step"])
    for t, f in ((0, 2), (0, 6), (1, 4)):
        a = t * c["rg_len"] + f * c["step"]
        want = crw_inference._upsample(nodes[t][f].float()[:, None], rows, c["step"]).cuda().to(torch.int8)
        for g in range(4):
            for k in ("forward", "pred"):
                assert torch.equal(out[k][g][:, a:a + c["step"]], want), (k, g, t, f)
            for k in ("forward_conf", "conf"):
                assert (out[k][g][:, a:a + c["step"]] == 1).all(), (k, g, t, f)


def test_anchors_none_is_the_call_without_the_argument_and_the_anchors_are_live(case):
    plain, none = case["run"](), case["run"](anchors=None)
    assert "anchor_cols" not in none and set(none) == set(plain)
    for k in ("pred", "forward", "conf", "forward_conf"):
        assert torch.equal(none[k].view(torch.uint8), plain[k].view(torch.uint8)), k
    assert not torch.equal(case["out"]["pred"], plain["pred"])


def test_the_per_configuration_arm_gives_the_same_maps(case, monkeypatch):
    """CRW_SWEEP_PER_CONFIG=1: the loop of `LabelPropVOS_CRW.propagate_all(anchors=)` -- the sweep's other arm takes the anchors too"""
    monkeypatch.setenv("CRW_SWEEP_PER_CONFIG", "1")
    loop = case["run"](anchors=(case["seg"], case["cols"]))
    for k in ("pred", "forward", "conf", "forward_conf"):
        assert torch.equal(loop[k].view(torch.uint8), case["out"][k].view(torch.uint8)), k
