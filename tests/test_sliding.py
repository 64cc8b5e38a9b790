"""The 'sliding' context rule on the CPU: the definition (tests/sliding_ref.py) against fixtures made with the reference's own
`predict` on the windowed lists (tests/golden/make_golden_sliding.py), the translation helper, what the rule is worth on drifting
layers (the README's table), planted defects against the one check the GPU tests use, and the host surface (cfg key, flags, json).
The device code is held to the same definition in tests/test_sliding_gpu.py."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import sliding_ref as sr
from conftest import PKG, ROOT, load_golden
from oracle import crw_oracle as orc

FIXTURES = ["T14N10", "T30N13", "T20N24", "T12N10", "T8N10"]
PERIODIC = dict(seed=0, T=33, N=16, C=16, M=6, cxt=8, radius=3, temp=0.01, knn=5)  # M = 6: N * M = 96 outputs, two compute waves


def fixture_case(name):
    g = load_golden("sliding_" + name)
    emb = g["emb"][::-1].copy() if bool(g["use_last"]) else g["emb"]
    cfg = dict(CXT_SIZE=int(g["cxt_size"]), RADIUS=int(g["radius"]), TEMP=float(g["temp"]), KNN=int(g["knn"]))
    return g, emb, orc.seed_labels(g["seg_ref"], emb.shape[1]), int(g["nclasses"]), cfg


def periodic_case():
    p = PERIODIC
    emb = sr.periodic_item(p["seed"], p["T"], p["N"], p["C"], p["cxt"])
    seed = (np.arange(p["N"]) * p["M"] // p["N"]).astype(np.float32)
    return emb, seed


def violations(seed, W, R, M, L, pred, first_frame=1, L_init=None, pred_init=None):
    fn = lambda s, w, r, li, pi: sr.gather(s, w, r, M, first_frame, li, pi)
    return sr.definition_violations(fn, seed, W, R, M, first_frame, L, pred, L_init, pred_init)


# ------------------------------------------------------------------------------------------------ 1. the definition and the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_definition_is_the_references_predict_on_windowed_lists(name):
    g, emb, seed, M, cfg = fixture_case(name)
    T, N, _ = emb.shape
    pred, L, W, I = sr.labelprop_sliding(emb, seed, M, cfg["CXT_SIZE"], cfg["RADIUS"], cfg["TEMP"], cfg["KNN"])
    assert np.array_equal(pred, g["pred"])  # label for label
    per_frame = np.abs(L.reshape(T, N * M) - g["L"].reshape(T, N * M)).max(1)
    print(f"{name}: worst frame {per_frame.max():.3e}, bound {orc.gather_bound(cfg['KNN']):.3e}")
    assert (per_frame <= orc.gather_bound(cfg["KNN"])).all()
    assert not any(violations(seed, W, sr.rows(I, N, cfg["CXT_SIZE"]), M, L, pred).values())


def test_nothing_slides_within_the_context():
    """T <= CXT_SIZE + 1: the fixture of the sliding rule is the reference rule's map, and frames <= cxt + 1 agree on every item."""
    g, emb, seed, M, cfg = fixture_case("T8N10")
    pred, L = orc.labelprop(emb, seed, M, cfg["CXT_SIZE"], cfg["RADIUS"], cfg["TEMP"], cfg["KNN"], return_soft=True)
    assert np.array_equal(pred, g["pred"]) and np.abs(L.reshape(g["L"].shape) - g["L"]).max() <= orc.gather_bound(cfg["KNN"])
    for name in FIXTURES:
        g, emb, seed, M, cfg = fixture_case(name)
        N, c = emb.shape[1], cfg["CXT_SIZE"]
        pred, L = orc.labelprop(emb, seed, M, c, cfg["RADIUS"], cfg["TEMP"], cfg["KNN"], return_soft=True)
        ps, Ls, _, _ = sr.labelprop_sliding(emb, seed, M, c, cfg["RADIUS"], cfg["TEMP"], cfg["KNN"])
        assert np.array_equal(pred[:, :c + 2], ps[:, :c + 2]) and np.array_equal(pred[:, :c + 2], g["pred"][:, :c + 2])
        assert np.allclose(L[:(c + 2) * N], Ls[:(c + 2) * N], rtol=0, atol=orc.gather_bound(cfg["KNN"]))


@pytest.mark.parametrize("first_frame", [1, 9])
def test_sliding_rows_is_the_loops_translation(first_frame):
    import crw_hip
    N, cxt, knn, T = 7, 4, 3, 16
    rng = np.random.default_rng(5)
    I = np.stack([rng.integers(0, min(n, cxt + 1) * N, (knn, N)) for n in range(first_frame, T)]).astype(np.int32)
    want = np.empty_like(I)
    for f in range(I.shape[0]):
        n = first_frame + f
        for j in range(knn):
            for q in range(N):
                i = I[f, j, q]
                want[f, j, q] = i if (i < N or n <= cxt + 1) else i + (n - cxt - 1) * N
    got = crw_hip.sliding_rows(torch.tensor(I), N, cxt, first_frame)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want) and np.array_equal(sr.rows(I, N, cxt, first_frame), want)
    assert (want < (np.arange(first_frame, T) * N)[:, None, None]).all() and (want != I).any()
    batched = crw_hip.sliding_rows(torch.tensor(I)[None].expand(2, *I.shape), N, cxt, first_frame)  # leading dimensions pass through
    assert np.array_equal(batched[1].numpy(), want)


# ------------------------------------------------------------------------------------------------ 2. what the rule is worth
def test_the_table_drifting_layers_are_followed_only_from_the_scored_frames():
    """Synthetic layered items whose boundaries drift (sliding_ref.drifting_item): wrong labels among the frames n >= cxt + 2.
    Bars: sliding <= 1 % (the reference's predict on windowed lists gives 0), the reference rule >= 20 % (measured minimum 25 %)."""
    for (T, N, C, M, cxt, radius, temp, knn, amp) in sr.DRIFT_SHAPES:
        row = []
        for seed in sr.DRIFT_SEEDS:
            emb, cls = sr.drifting_item(seed, T, N, C, M, amp)
            ps = sr.labelprop_sliding(emb, cls[0].astype(np.float32), M, cxt, radius, temp, knn)[0]
            pr = orc.labelprop(emb, cls[0].astype(np.float32), M, cxt, radius, temp, knn)
            (es, tot), (er, _) = sr.late_errors(ps, cls, cxt), sr.late_errors(pr, cls, cxt)
            row.append((er, es, tot))
            assert es <= 0.01 * tot and er >= 0.20 * tot, (T, N, seed, er, es, tot)
        print(f"[{T}, {N}] cxt {cxt}: reference rule {' / '.join(str(r[0]) for r in row)}, sliding {' / '.join(str(r[1]) for r in row)} of {row[0][2]}")


# ------------------------------------------------------------------------------------------------ 3. planted defects
def _lists(emb, seed, M, cxt, radius, temp, knn):
    _, _, W, I = sr.labelprop_sliding(emb, seed, M, cxt, radius, temp, knn)
    return W, I


def _defect_rows(I, N, cxt, kind):
    n = np.arange(1, 1 + I.shape[0])[:, None, None]
    shift = np.maximum(n - cxt - 1, 0) * N
    if kind == "translation dropped":
        return I
    if kind == "frame-0 indices translated":
        return (I + shift).astype(I.dtype)
    if kind == "off by one frame":
        return np.where((I >= N) & (n > cxt + 1), I + (n - cxt - 2) * N, I).astype(I.dtype)
    if kind == "applied already at n = cxt + 1":  # the list of frame cxt + 1 still holds every frame: nothing to translate yet
        return np.where(I >= N, I + np.maximum(n - cxt, 0) * N * (n == cxt + 1) + shift, I).astype(I.dtype)
    raise KeyError(kind)


def _ring_of_cxt_slots(seed, W, R, M, N, cxt):
    """The propagation with a ring of cxt slots, where frame n takes the slot of frame n - cxt: outputs are stored as they are made,
    so an output made later in the same frame reads frame n's rows where it meant frame n - cxt's (the worst interleaving)."""
    F, knn, _ = W.shape
    T = F + 1
    L = np.zeros((T * N, M), np.float32)
    L[:N] = seed[:, None] == np.arange(M)[None]
    pred = np.zeros((N, T), np.float32)
    pred[:, 0] = seed
    for n in range(1, T):
        view = L.copy()  # what the LDS holds: the slot of frame n - cxt is overwritten row by row
        for q in range(N):
            p = np.zeros(M, np.float32)
            for j in range(knn):
                p = p + view[R[n - 1, j, q]] * W[n - 1, j, q]
            L[n * N + q] = p
            if n - cxt >= 1:
                view[(n - cxt) * N + q] = p
        pred[:, n] = L[n * N:(n + 1) * N].argmax(-1)
    return L, pred


@pytest.mark.parametrize("kind", ["translation dropped", "frame-0 indices translated", "off by one frame", "applied already at n = cxt + 1"])
def test_a_wrong_translation_is_reported(kind):
    g, emb, seed, M, cfg = fixture_case("T30N13")
    N, cxt = emb.shape[1], cfg["CXT_SIZE"]
    W, I = _lists(emb, seed, M, cxt, cfg["RADIUS"], cfg["TEMP"], cfg["KNN"])
    R = sr.rows(I, N, cxt)
    good = violations(seed, W, R, M, *sr.gather(seed, W, R, M))
    assert not any(good.values())
    bad = violations(seed, W, R, M, *sr.gather(seed, W, _defect_rows(I, N, cxt, kind), M))
    assert bad["bits_L"] > 0 and bad["audit_soft"] > 0, (kind, bad)


def test_the_periodic_item_selects_the_oldest_frame_and_a_ring_of_cxt_slots_is_reported():
    p = PERIODIC
    emb, seed = periodic_case()
    W, I = _lists(emb, seed, p["M"], p["cxt"], p["radius"], p["temp"], p["knn"])
    frac = sr.oldest_top_fraction(I, p["N"], p["cxt"])
    print(f"top neighbour in frame n - cxt: {frac:.2f} of the late queries")
    assert frac >= 0.25
    R = sr.rows(I, p["N"], p["cxt"])
    assert not any(violations(seed, W, R, p["M"], *sr.gather(seed, W, R, p["M"])).values())
    bad = violations(seed, W, R, p["M"], *_ring_of_cxt_slots(seed, W, R, p["M"], p["N"], p["cxt"]))
    assert bad["bits_L"] > 0, bad
    # ... and cxt + 1 slots are enough: the slot frame n takes is that of frame n - cxt - 1, which no index of frame n reaches
    late = np.arange(1, p["T"])[:, None, None] > p["cxt"] + 1
    assert (np.where(late & (R >= p["N"]), R // p["N"], 10 ** 6) >= (np.arange(1, p["T"]) - p["cxt"])[:, None, None]).all()


def test_the_last_maximum_of_a_tied_row_is_reported():
    N, M, T, knn = 4, 3, 3, 2
    seed = np.array([0, 1, 2, 1], np.float32)
    W = np.full((T - 1, knn, N), 0.5, np.float32)
    I = np.zeros((T - 1, knn, N), np.int32)
    I[:, 0], I[:, 1] = [0, 1, 2, 3], [1, 2, 3, 0]  # every row averages two one-hot rows: exact ties
    L, pred = sr.gather(seed, W, I, M)
    assert (np.sort(L[N:2 * N], -1)[:, -1] == np.sort(L[N:2 * N], -1)[:, -2]).any()
    assert not any(violations(seed, W, I, M, L, pred).values())
    bad = violations(seed, W, I, M, *sr.gather(seed, W, I, M, last_max=True))
    assert bad["bits_pred"] > 0 and bad["audit_pred"] > 0 and bad["bits_L"] == 0


# ------------------------------------------------------------------------------------------------ 4. host surface
def test_header_and_binding_declare_the_sliding_entry_points_at_abi_8():
    import re
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^int\s+crw_labelprop_propagate_sliding\(const float \*seed, const float \*W, const int32_t \*I, int T, int N, int M, "
                     r"int knn, int first_frame,\s+int cxt_size, float \*L, float \*pred, crw_stream_t stream\);", header, re.M)
    assert re.search(r"^int\s+crw_labelprop_propagate_sliding_batch\(const float \*seed, const float \*W, const int32_t \*I, size_t i_stride, "
                     r"int G,", header, re.M)
    assert crw_hip.ABI_VERSION == 8 and "crw_hip.has_sliding()" in header
    assert crw_hip.SLIDING_ENTRY_POINTS == ("crw_labelprop_propagate_sliding", "crw_labelprop_propagate_sliding_batch")
    assert set(crw_hip.SLIDING_ENTRY_POINTS) <= set(crw_hip.SIGNATURES)
    assert crw_hip.SIGNATURES["crw_labelprop_propagate_sliding"] == crw_hip.SIGNATURES["crw_labelprop_propagate"]
    assert crw_hip.SIGNATURES["crw_labelprop_propagate_sliding_batch"] == crw_hip.SIGNATURES["crw_labelprop_propagate_batch"]
    assert crw_hip.has_sliding()
    lib = crw_hip.lib()  # argument errors are refused on the host side of the library, before any launch (no GPU needed)
    assert lib.crw_labelprop_propagate_sliding(None, None, None, 4, 4, 2, 3, 1, 2, None, None, None) == crw_hip.CRW_EINVAL
    assert lib.crw_labelprop_propagate_sliding_batch(None, None, None, 0, 1, 4, 4, 2, 3, 1, 2, None, None, None) == crw_hip.CRW_EINVAL


def test_a_library_without_the_sliding_entry_points_is_named_stale(monkeypatch):
    import crw_hip
    crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "sliding", False)
    W, I = torch.zeros(3, 2, 4), torch.zeros(3, 2, 4, dtype=torch.int32)
    for call in (lambda: crw_hip.labelprop_gather(torch.zeros(4), W, I, 4, 4, 3, cxt_size=2, context="sliding"),
                 lambda: crw_hip.labelprop_propagate_batch(torch.zeros(4), W[None], I, 4, 4, 3, cxt_size=2, context="sliding")):
        with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*crw_labelprop_propagate_sliding.*rebuild"):
            call()


def test_context_is_validated_everywhere():
    import crw_hip
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    cfg = dict(CXT_SIZE=4, RADIUS=2, TEMP=0.1, KNN=3)
    assert LabelPropVOS_CRW(cfg).context == "reference" and LabelPropVOS_CRW(dict(cfg, CONTEXT="sliding")).context == "sliding"
    assert LabelPropVOS_CRW(dict(cfg, CONTEXT="reference")).context == "reference"
    for bad in ("Sliding", "window", None, 1):
        with pytest.raises(ValueError, match="CONTEXT"):
            LabelPropVOS_CRW(dict(cfg, CONTEXT=bad))
        with pytest.raises(ValueError, match="context"):
            LabelPropSweep(4, [2], [0.1], [3], context=bad)
    plain, slid = LabelPropSweep(4, [2, 3], [0.1], [3, 5]), LabelPropSweep(4, [2, 3], [0.1], [3, 5], context="sliding")
    assert all("CONTEXT" not in c for c in plain.configs) and plain.context == "reference"  # the dicts are what they were
    assert [dict(c, CONTEXT="sliding") for c in plain.configs] == slid.configs and slid.context == "sliding"
    assert all(LabelPropVOS_CRW(c).context == "sliding" for c in slid.configs)  # the CRW_SWEEP_PER_CONFIG=1 arm routes on the key
    W, I = torch.zeros(3, 2, 4), torch.zeros(3, 2, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="context"):
        crw_hip.labelprop_gather(torch.zeros(4), W, I, 4, 4, 3, cxt_size=2, context="both")
    with pytest.raises(ValueError, match="cxt_size"):
        crw_hip.labelprop_gather(torch.zeros(4), W, I, 4, 4, 3, context="sliding")
    with pytest.raises(ValueError, match="context"):
        crw_hip.labelprop_propagate_batch(torch.zeros(4), W[None], I, 4, 4, 3, cxt_size=2, context="both")


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_scripts_take_the_flag():
    for name, base in (("segment_all", ["--model_path", "x.pt"]), ("segment_sweep", ["--model_path", "x.pt"]),
                       ("segment_drivers", ["--driver", "mc3", "--model_path", "x.pt"])):
        p = _script(name).get_args_parser()
        assert p.parse_args(base).context == "reference" and p.parse_args(base + ["--context", "sliding"]).context == "sliding"
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--context", "window"])


def test_segment_all_routes_the_flag_and_reports_it_only_when_set(monkeypatch, capsys, tmp_path):
    """Through test_confidence's stubbing (its `stub_propagate` stands in for `propagate`): the lp object carries the rule, the json
    gains the key only with the flag, and without the flag stdout is the recorded one."""
    import inference as crw_inference
    import test_confidence as tc
    seen = []

    def spy(seq, seg_ref, model, lp, *a, **k):
        seen.append(lp.context)
        return tc.stub_propagate(seq, seg_ref, model, lp, *a, **k)

    def run(extra, sub):
        cli = tc._cli()
        monkeypatch.setattr(crw_inference, "propagate", spy)
        monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: tc.Flatten())
        out_dir, js = tmp_path / sub / "out", tmp_path / sub / "r.json"
        torch.manual_seed(11)
        cli.main(cli.get_args_parser().parse_args(tc.CLI_ARGS + ["--output_folder", str(out_dir), "--report_json", str(js)] + extra))
        text = capsys.readouterr().out.replace(str(tmp_path / sub), "TMP")
        import re
        return re.sub(r"(Time elapsed \([a-z +]+\):) [0-9.e-]+", r"\1 *", text), json.load(open(js))

    os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b")
    text, d = run([], "a")
    assert text == open(os.path.join(ROOT, "tests", "golden", "segment_all_stdout.txt")).read() and "context" not in d
    assert seen and set(seen) == {"reference"}
    del seen[:]
    text2, d2 = run(["--context", "sliding"], "b")
    assert d2["context"] == "sliding" and set(seen) == {"sliding"}
    assert {k: v for k, v in d2.items() if not k.startswith("elapsed") and k != "context"} == {k: v for k, v in d.items() if not k.startswith("elapsed")}
    assert text2.split("\n", 1)[1] == text.split("\n", 1)[1]  # (the first line prints the arguments)


def test_segment_sweep_routes_the_flag_and_reports_it_only_when_set(monkeypatch, capsys, tmp_path):
    import inference as crw_inference
    import test_sweep as ts
    cli = ts._cli()
    seen = []

    def spy(seq, seg_ref, model, sweep, *a, **k):
        seen.append((sweep.context, [c.get("CONTEXT") for c in sweep.configs]))
        return ts.oracle_propagate_sweep(seq, seg_ref, model, sweep, *a, **k)

    monkeypatch.setattr(crw_inference, "propagate_sweep", spy)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: ts.CountingFlatten())
    base = ["--synthetic", "40", "384", "--dataset", "3", "--patch_size", "8", "8", "--overlap", "4", "0", "--seq_length", "8", "-c", "4",
            "-r", "2", "-t", "0.1", "-k", "3", "5", "--model", "0"]
    ds = []
    for i, extra in enumerate(([], ["--context", "sliding"])):
        js = tmp_path / f"s{i}.json"
        cli.main(cli.get_args_parser().parse_args(base + ["--report_json", str(js), "--output_folder", str(tmp_path / f"o{i}")] + extra))
        ds.append(json.load(open(js)))
    capsys.readouterr()
    assert "context" not in ds[0] and ds[1]["context"] == "sliding"
    assert seen[0] == ("reference", [None, None]) and seen[-1] == ("sliding", ["sliding", "sliding"])
    assert sorted(ds[1]) == sorted(list(ds[0]) + ["context"])


def test_segment_radargrams_hands_the_rule_to_its_label_propagation(monkeypatch):
    import inference as crw_inference
    seen = []

    class Stop(Exception):
        pass

    def spy(seq, seg_ref, model, lp, *a, **k):
        seen.append(lp.context)
        raise Stop

    monkeypatch.setattr(crw_inference, "propagate", spy)
    rg = [torch.zeros(64, 4000)] * 3
    for context, want in ((None, "reference"), ("reference", "reference"), ("sliding", "sliding")):
        with pytest.raises(Stop):
            crw_inference.segment_radargrams("sharad", rg, rg, torch.nn.Flatten(), context=context)
        assert seen[-1] == want
    with pytest.raises(ValueError, match="CONTEXT"):
        crw_inference.segment_radargrams("sharad", rg, rg, torch.nn.Flatten(), context="window")
