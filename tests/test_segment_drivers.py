"""The reference's per-dataset drivers (scripts/test/test_mc1.py, test_mc3.py, test_sharad.py) as `inference.segment_radargrams`
and `scripts/segment_drivers.py`: host logic against the maps the reference's own `main(args)` saved (fixtures drivers_*.npz,
tests/golden/make_golden_drivers.py), the label propagation being the CPU oracle here; the GPU twins are in
test_segment_drivers_gpu.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import PKG, load_golden
from oracle import crw_oracle as orc

DRIVER_CASES = {"mc1": "drivers_mc1", "mc3": "drivers_mc3", "sharad": "drivers_sharad"}


class PatchFlatten(torch.nn.Module):
    def forward(self, x):
        return x.flatten(1)


def fixture_inputs(driver, g, device):
    """A fixture holds the three input files as the script loads them; sharad flips its first radargram and reference
    (test_sharad.py:54,58 -- scripts/segment_drivers.py load_inputs does the same)."""
    rg = [torch.tensor(g[f"rg{i}"].astype(np.float32), device=device) for i in range(3)]
    sg = [torch.tensor(g[f"sg{i}"].astype(np.float32), device=device) for i in range(3)]
    sgr = [torch.tensor(g[f"sgr{i}"].astype(np.float32), device=device) for i in range(3)] if "sgr0" in g else None
    if driver == "sharad":
        rg[0], sg[0] = torch.flip(rg[0], (1,)), torch.flip(sg[0], (1,))
    return rg, sg, sgr


def run_driver_golden(driver, g, propagate_fn, device):
    """`segment_radargrams(driver)` on a fixture's inputs with `propagate_fn` standing in for `utils.propagate` (the CPU oracle
    here, the HIP path in the GPU tests) -> (outputs, number of propagate calls)."""
    import inference as crw_inference
    rg, sg, sgr = fixture_inputs(driver, g, device)
    calls = {"n": 0}

    def propagate(*a, **k):
        calls["n"] += 1
        return propagate_fn(*a, **k)

    orig = crw_inference.propagate
    crw_inference.propagate = propagate
    try:
        out = crw_inference.segment_radargrams(driver, rg, sg, PatchFlatten(), refs_reversed=sgr,
                                               patch_size=tuple(int(v) for v in g["patch"]), seq_length=int(g["seq_length"]),
                                               overlap=tuple(int(v) for v in g["overlap"]))
    finally:
        crw_inference.propagate = orig
    return out, calls["n"]


def oracle_propagate(seq, seg_ref, model, lp, ncls, do_pos_embed, use_last):
    T, N = seq.shape[:2]
    emb = model(seq.reshape(T * N, 1, *seq.shape[2:])).reshape(T, N, -1).numpy()
    if use_last:
        emb = emb[::-1].copy()
    pred = orc.labelprop(emb, orc.seed_labels(seg_ref.numpy(), N), ncls, lp.cxt_size, lp.radius, lp.temperature, lp.topk)
    return torch.tensor(pred), torch.tensor(orc.xent_metric(emb)), None


def check_outputs(driver, g, out):
    """Every saved map exactly, every xent list to 1e-4, and nothing else saved."""
    import inference as crw_inference
    assert tuple(out) == crw_inference.DRIVERS[driver]["outputs"]
    for name, objs in out.items():
        key = name[:-3]
        assert len(objs) == 3
        for i, x in enumerate(objs):
            want = g[f"{key}.{i}"]
            got = x.detach().cpu().numpy()
            assert got.shape == want.shape, (name, i, got.shape, want.shape)
            if "xent" in name:
                np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
            else:
                got = got.astype(np.int8)
                assert np.array_equal(got, want), f"{name}[{i}]: {(got != want).sum()} of {want.size} pixels differ"


def test_driver_defaults_are_the_scripts():
    import inference as crw_inference
    d = crw_inference.DRIVERS
    assert set(d) == {"mc1", "mc3", "sharad"}
    assert (d["mc1"]["patch_size"], d["mc1"]["overlap"], d["mc1"]["cxt_size"], d["mc1"]["radius"], d["mc1"]["temp"],
            d["mc1"]["knn"], d["mc1"]["nclasses"]) == ((32, 32), (24, 0), 80, 30, 0.1, 20, 4)
    assert (d["mc3"]["overlap"], d["mc3"]["cxt_size"], d["mc3"]["radius"], d["mc3"]["temp"], d["mc3"]["nclasses"],
            d["mc3"]["change_idx"]) == ((30, 0), 100, 60, 0.01, 5, (38, 36, 52))
    assert (d["sharad"]["patch_size"], d["sharad"]["overlap"], d["sharad"]["radius"], d["sharad"]["change_idx"]) == \
        ((16, 16), (8, 0), 10, (80, 67, 98))
    assert all(v["seq_length"] == 100 and v["model"] == 1 for v in d.values())


@pytest.mark.parametrize("driver", sorted(DRIVER_CASES))
def test_segment_radargrams_matches_reference_main(driver):
    """Forward pass, hand-set correction on the item's TAIL, reverse pass and merge of each driver against what the reference's
    script saved, the pre-merge maps of mc3 included (label propagation: the CPU oracle)."""
    g = load_golden(DRIVER_CASES[driver])
    out, n = run_driver_golden(driver, g, oracle_propagate, "cpu")
    assert n == int(g["n_calls"])
    check_outputs(driver, g, out)
    if driver == "mc3":  # the merge changed something after the save, so the clone is what pins the save-time state
        assert any(not np.array_equal(g[f"mc3_res.{i}"], g[f"mc3_resy.{i}"]) for i in range(3))


def test_merge_mc1_reads_the_updated_map():
    """test_mc1.py:129-133: the second rule (class 1) tests `fwd != 2` on the map the first rule has just written."""
    import inference as crw_inference
    fwd = torch.tensor([[0., 1., 3., 2.], [3., 0., 1., 0.]])
    rev = torch.tensor([[2., 1., 1., 1.], [1., 2., 0., 1.]])
    out = crw_inference.merge_mc1(fwd, rev)
    assert out is fwd  # in place, as the script's aliased list
    assert torch.equal(fwd, torch.tensor([[2., 1., 1., 2.], [1., 2., 1., 1.]]))
    # a pixel that the first rule turned into 2 is not overwritten by the second rule
    fwd = torch.tensor([[0.]])
    crw_inference.merge_mc1(fwd, torch.tensor([[2.]]))
    assert fwd.item() == 2.0


def test_merge_mc3_respects_columns_with_class_4():
    import inference as crw_inference
    fwd = torch.tensor([[0., 4., 1.], [1., 0., 1.], [0., 1., 0.]])
    rev = torch.tensor([[2., 2., 3.], [3., 3., 2.], [0., 2., 0.]])
    crw_inference.merge_mc3(fwd, rev)
    # column 1 holds a 4: untouched; columns 0 and 2: 2 then 3 written where the reverse map holds them
    assert torch.equal(fwd, torch.tensor([[2., 4., 3.], [3., 0., 2.], [0., 1., 0.]]))


def test_segment_radargrams_argument_checks():
    import inference as crw_inference
    rg = [torch.zeros(8, 16)] * 3
    with pytest.raises(ValueError):
        crw_inference.segment_radargrams("mc2", rg, rg, PatchFlatten())
    with pytest.raises(ValueError):
        crw_inference.segment_radargrams("mc1", rg, rg, PatchFlatten())  # no reversed references
    with pytest.raises(ValueError):
        crw_inference.segment_radargrams("mc3", rg, rg, PatchFlatten(), use_last=False)


def _cli():
    spec = importlib.util.spec_from_file_location("segment_drivers", os.path.join(PKG, "scripts", "segment_drivers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_loader_applies_the_scripts_data_fixes(tmp_path):
    """mc3: radargrams cast to float, sg2[870:900, 1132:1200] = 2 (test_mc3.py:61); sharad: radargram and reference 1 flipped
    along the columns (test_sharad.py:54,58); mc1: files as they are, the reversed references beside."""
    cli = _cli()
    g = torch.Generator().manual_seed(5)
    for n in ("mc3_1", "mc3_2", "mc3_3y"):
        torch.save(torch.randn(4, 6, generator=g).half(), tmp_path / f"{n}.pt")
    big = torch.zeros(880, 1140, dtype=torch.int8)
    torch.save(big, tmp_path / "mc3_2ref.pt")
    for n in ("mc3_1ref", "mc3_3refy"):
        torch.save(torch.zeros(4, 6, dtype=torch.int8), tmp_path / f"{n}.pt")
    rg, sg, sgr = cli.load_inputs("mc3", str(tmp_path), "cpu")
    assert sgr is None and all(r.dtype == torch.float32 for r in rg)
    assert (sg[1][870:880, 1132:1140] == 2).all() and sg[1].sum().item() == 2 * 10 * 8
    assert not sg[0].any() and not sg[2].any()

    s = {n: torch.randn(3, 5, generator=g) for n in ("s_1", "s_4", "s_3")}
    r = {n: torch.randint(0, 5, (3, 5), generator=g) for n in ("s_1ref", "s_4ref", "s_3ref")}
    for n, v in {**s, **r}.items():
        torch.save(v, tmp_path / f"{n}.pt")
    rg, sg, _ = cli.load_inputs("sharad", str(tmp_path), "cpu")
    assert torch.equal(rg[0], torch.flip(s["s_1"], (1,))) and torch.equal(sg[0], torch.flip(r["s_1ref"], (1,)))
    assert torch.equal(rg[1], s["s_4"]) and torch.equal(rg[2], s["s_3"]) and torch.equal(sg[2], r["s_3ref"])

    for i in (1, 2, 3):
        torch.save(torch.full((2, 3), float(i)), tmp_path / f"mc1_{i}.pt")
        torch.save(torch.full((2, 3), i), tmp_path / f"mc1_{i}ref.pt")
        torch.save(torch.full((2, 3), 10 + i), tmp_path / f"mc1_{i}ref_r.pt")
    rg, sg, sgr = cli.load_inputs("mc1", str(tmp_path), "cpu")
    assert [int(x[0, 0]) for x in rg] == [1, 2, 3] and [int(x[0, 0]) for x in sgr] == [11, 12, 13]


def test_cli_flags_and_defaults(tmp_path):
    cli = _cli()
    p = cli.get_args_parser()
    a = cli.with_defaults(p.parse_args(["--driver", "mc3", "--model_path", "x.pt"]))
    assert (a.patch_size, a.seq_length, a.overlap, a.cxt_size, a.radius, a.temp, a.knn, a.use_last, a.correction, a.change_idx,
            a.model) == ((32, 32), 100, (30, 0), 100, 60, 0.01, 20, True, True, (38, 36, 52), 1)
    a = cli.with_defaults(p.parse_args(["--driver", "sharad", "--model_path", "x.pt", "-r", "5", "--change_idx", "1", "none", "3",
                                        "--use_last", "false", "--patch_size", "8", "8", "--overlap", "4", "0"]))
    assert (a.radius, a.change_idx, a.use_last, a.patch_size, a.overlap) == (5, (1, None, 3), False, (8, 8), (4, 0))
    # a checkpoint saved from DataParallel (keys prefixed with "module.") loads into the bare encoder
    import encoder as crw_encoder
    torch.manual_seed(3)
    net = crw_encoder.CNN(False)
    torch.save({"module." + k: v for k, v in net.state_dict().items()}, tmp_path / "dp.pt")
    enc = cli.load_encoder(0, str(tmp_path / "dp.pt"), "cpu")
    for (k, v), (_, w) in zip(net.state_dict().items(), enc.state_dict().items()):
        assert torch.equal(v, w), k
