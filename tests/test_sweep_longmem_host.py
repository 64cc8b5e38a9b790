"""include/crw_hip_sweepmem.h (the memory bank in the parameter sweep, a companion of include/crw_hip.h) against the binding and the
library, the way tests/test_longmem_host.py holds crw_hip_longmem.h; the grid with the bias axis; the refusals of the host path
(`crw_hip.labelprop_propagate_batch`, `LabelPropSweep`, `utils.propagate_sweep`, `inference.segment_sweep`, scripts/segment_sweep.py);
and the hand-over script -> `segment_sweep` -> `propagate_sweep` -> `LabelPropSweep.propagate_all` with stubs in place of the device.
No GPU."""
import ctypes
import os
import re

import pytest
import torch

from test_sweep_posterior import GOLDEN_ARGS, _cli, run_sweep_cli, stub_propagate_sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLIDING = ["--context", "sliding"]


def _declared():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crw_hip_sweepmem.h")).read(), flags=re.S)
    return dict(re.findall(r"\b(crw_[a-z0-9_]+)\s*\(([^()]*)\)", header))


def test_sweepmem_header_binding_and_library_agree():
    import crw_hip
    if not os.path.exists(crw_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    decls = _declared()
    assert len(decls) == 1 and set(decls) == set(crw_hip.SWEEPMEM_SIGNATURES), set(decls) ^ set(crw_hip.SWEEPMEM_SIGNATURES)
    others = (crw_hip.SIGNATURES, crw_hip.CHAIN_SIGNATURES, crw_hip.RESTART_SIGNATURES, crw_hip.LONGMEM_SIGNATURES, crw_hip.ALIGN_SIGNATURES)
    assert not any(set(decls) & set(o) for o in others)                                      # one header each
    handle = ctypes.CDLL(crw_hip.LIB_PATH)
    for name, params in decls.items():
        assert hasattr(handle, name), f"{name} declared in crw_hip_sweepmem.h but not exported"
        res, args = crw_hip.SWEEPMEM_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == params.count(",") + 1, name
        kinds = [ctypes.c_void_p if "*" in p or "crw_stream_t" in p else ctypes.c_size_t if "size_t" in p else
                 ctypes.c_float if "float" in p else ctypes.c_int for p in params.split(",")]
        assert args == kinds, name                                                          # type by type, in the header's order
        assert getattr(crw_hip.lib(), name).argtypes == args
    text = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert "#define CRW_ABI_VERSION 8" in text and crw_hip.ABI_VERSION == 8                 # added without a bump
    for other in ("crw_hip.h", "crw_hip_longmem.h", "crw_hip_align.h"):                      # no declaration in the existing headers
        assert "crw_labelprop_propagate_long_batch" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_the_entry_point_is_banded():
    text = open(os.path.join(ROOT, "tests", "test_sweep_longmem_gpu.py")).read()
    for name, params in _declared().items():
        assert "*" in params and "run_banded" in text and "run_twice" in text and re.search(rf"\blib\.{name}\b", text), name


def test_sweep_memory_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    names = crw_hip.SWEEP_MEMORY_ENTRY_POINTS
    assert names and set(names) == set(crw_hip.SWEEPMEM_SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS["sweep_memory"] is names
    assert crw_hip.has_sweep_memory() is True and crw_hip._sweep_memory_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, "sweep_memory", False)      # a library from before the entry point
    assert crw_hip.has_sweep_memory() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._sweep_memory_lib()
    assert all(name in str(err.value) for name in names)


def test_the_launch_is_told_in_the_route_table_and_the_kernel_has_its_log():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    src = open(os.path.join(ROOT, "radar-sounder-crw_amd", "csrc", "labelprop.hip")).read()
    # logged through the sliding batch's one site: no route name of its own, and the row of that route says so
    assert src.count('CRW_ROUTE("labelprop.batch_slide")') == 1 and src.count("route_propagate_batch<true, false>()") == 1
    row = next(line for line in design.splitlines() if line.startswith("| `labelprop.batch_slide` |"))
    assert "launch_propagate_long_batch" in row and "crw_labelprop_propagate_long_batch" in row
    log = open(os.path.join(ROOT, "profiles", "sweep_longmem_isa_diff.log")).read()
    assert ", 0 not identical, 1 new" in log and "NEW" in log and "labelprop_chain_batch_kernel<true, false, true>" in log


# ================================================================================================ the grid
def test_grid_order_and_the_bias_key_only_when_asked():
    from imported.labelprop import LabelPropSweep
    plain = LabelPropSweep(4, [3, 5], [0.1, 0.01], [2, 4])
    assert plain.biases == [0.0] and len(plain) == 8 and all("MEMORY_BIAS" not in c for c in plain.configs)
    same = LabelPropSweep(4, [3, 5], [0.1, 0.01], [2, 4], biases=(0.0,))
    assert same.configs == plain.configs
    assert LabelPropSweep(4, [3], [0.1], [2], context="sliding").configs == [dict(CXT_SIZE=4, RADIUS=3, TEMP=0.1, KNN=2, CONTEXT="sliding")]
    s = LabelPropSweep(4, [3, 5], [0.1, 0.01], [2, 4], context="sliding", biases=[0.0, 0.05, 0.2])
    assert len(s) == 2 * 2 * 3 * 2
    want = [(r, t, b, k) for r in (3, 5) for t in (0.1, 0.01) for b in (0.0, 0.05, 0.2) for k in (2, 4)]
    assert [(c["RADIUS"], c["TEMP"], c["MEMORY_BIAS"], c["KNN"]) for c in s.configs] == want
    assert LabelPropSweep(4, [3], [0.1], [2], biases=[0.1]).configs[0]["MEMORY_BIAS"] == 0.1
    for bad in ([], [float("nan")], [0.0, float("inf")]):
        with pytest.raises(ValueError, match="biases must hold|memory_bias must be a finite number"):
            LabelPropSweep(4, [3], [0.1], [2], biases=bad)


# ================================================================================================ refusals
def test_every_refusal_has_its_message():
    import crw_hip
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropSweep
    T, N, C, M, B = 6, 5, 4, 3, 2
    feats, seed = torch.zeros(T, N, C), torch.zeros(N)
    memory = (torch.zeros(B, N, C), torch.zeros(B, N, dtype=torch.int8))
    sliding = LabelPropSweep(2, [2], [0.1], [2], context="sliding")
    with pytest.raises(ValueError, match="memory_bias needs memory"):
        LabelPropSweep(2, [2], [0.1], [2], context="sliding", biases=[0.0, 0.1]).propagate_all(feats, seed, M)
    with pytest.raises(ValueError, match="seed=None needs memory"):
        sliding.propagate_all(feats, None, M)
    with pytest.raises(ValueError, match="memory needs CONTEXT 'sliding'"):
        LabelPropSweep(2, [2], [0.1], [2]).propagate_all(feats, seed, M, memory=memory)
    with pytest.raises(ValueError, match="memory and anchor_context='restart' are not combined"):
        sliding.propagate_all(feats, seed, M, memory=memory, anchor_context="restart", anchors=torch.zeros(T, N, dtype=torch.int8))
    with pytest.raises(ValueError, match="memory is defined on N x 1 grids only"):
        LabelPropSweep(2, [2], [0.1], [2], context="sliding").propagate_all(torch.zeros(T, 6, C), torch.zeros(6), M, grid_w=2,
                                                                            memory=(torch.zeros(B, 6, C), torch.zeros(B, 6, dtype=torch.int8)))
    with pytest.raises(ValueError, match="a bank serves items of its own N"):
        sliding.propagate_all(feats, seed, M, memory=(torch.zeros(B, N + 1, C), torch.zeros(B, N + 1, dtype=torch.int8)))
    with pytest.raises(ValueError, match="fully labelled"):
        sliding.propagate_all(feats, seed, M, memory=(memory[0], torch.full((B, N), M, dtype=torch.int8)))
    # the binding
    W, I = torch.zeros(1, T - 1, 2, N), torch.zeros(1, T - 1, 2, N, dtype=torch.int32)
    L, p = torch.zeros(1, T * N, M), torch.zeros(1, N, T)
    with pytest.raises(ValueError, match="n_long and origin are not combined"):
        crw_hip.labelprop_propagate_batch(None, W, I, T, N, M, 1, 2, L, p, context="sliding", origin=torch.zeros(T, dtype=torch.int32), n_long=2)
    with pytest.raises(ValueError, match="n_long needs context='sliding'.*consistently"):
        crw_hip.labelprop_propagate_batch(None, W, I, T, N, M, 1, 2, L, p, n_long=2)
    for bad in (0, T):
        with pytest.raises(ValueError, match="n_long must be in 1"):
            crw_hip.labelprop_propagate_batch(None, W, I, T, N, M, 1, 2, L, p, context="sliding", n_long=bad)
    assert crw_hip.sweep_memory_fits(96, 80, 3) and not crw_hip.sweep_memory_fits(96, 80, 4)
    # propagate_sweep / segment_sweep: refused before anything is encoded
    seq = torch.zeros(T, N, 8, 8)
    biased = LabelPropSweep(2, [2], [0.1], [2], context="sliding", biases=[0.1])
    with pytest.raises(ValueError, match="memory_align and memory_bias need memory"):
        crw_utils.propagate_sweep(seq, None, None, biased, M, False, False)
    with pytest.raises(ValueError, match="memory_align and memory_bias need memory"):
        crw_utils.propagate_sweep(seq, None, None, sliding, M, False, False, memory_align="center")
    with pytest.raises(ValueError, match="memory_align must be None or 'center'"):
        crw_utils.propagate_sweep(seq, None, None, sliding, M, False, False, memory_align="centre")
    bank = crw_utils.memory_bank(torch.zeros(B, N, 8, 8), torch.zeros(B, N, dtype=torch.int8))
    with pytest.raises(ValueError, match="memory needs CONTEXT 'sliding'"):
        crw_utils.propagate_sweep(seq, None, None, LabelPropSweep(2, [2], [0.1], [2]), M, False, False, memory=bank)
    with pytest.raises(ValueError, match="memory and anchor_context='restart' are not combined"):
        crw_utils.propagate_sweep(seq, None, None, sliding, M, False, False, memory=bank, anchor_context="restart",
                                  anchors=torch.zeros(T, N, dtype=torch.int8))
    with pytest.raises(ValueError, match="a bank serves items of its own N and patch size"):
        crw_utils.propagate_sweep(torch.zeros(T, N + 1, 8, 8), None, None, sliding, M, False, False, memory=bank)
    with pytest.raises(ValueError, match="seg_ref=None .no seed. needs memory"):
        crw_utils.propagate_sweep(seq, None, None, sliding, M, False, False)
    ds, seg = [seq], torch.zeros(24, 48)
    call = lambda sw=sliding, **kw: crw_inference.segment_sweep(ds, seg, None, sw, M, T, (8, 8), (4, 0), **kw)
    for kw in (dict(memory=bank), dict(memory_align="center"), dict(memory_bias=0.1)):
        with pytest.raises(ValueError, match="memory is not offered in segment_sweep.*bank=.*LabelPropSweep\\(biases=\\)"):
            call(**kw)
    with pytest.raises(ValueError, match="memory_align and memory_bias need memory"):
        call(bank_align="center")
    with pytest.raises(ValueError, match="memory_align and memory_bias need memory"):
        call(biased)
    with pytest.raises(ValueError, match="seedless=True needs memory"):
        call(seedless=True)
    with pytest.raises(ValueError, match="seedless=True and correction=True do not combine"):
        call(bank=bank, seedless=True, correction=True)
    with pytest.raises(ValueError, match="memory needs CONTEXT 'sliding'"):
        call(LabelPropSweep(2, [2], [0.1], [2]), bank=bank)
    with pytest.raises(ValueError, match="memory and anchor_context='restart' do not combine"):
        call(bank=bank, anchor_context="restart", anchors=(seg, [8]))
    with pytest.raises(ValueError, match="a bank serves items of its own N"):
        call(bank=crw_utils.memory_bank(torch.zeros(B, N + 1, 8, 8), torch.zeros(B, N + 1, dtype=torch.int8)))
    with pytest.raises(ValueError, match="memory_align must be None or 'center'"):
        call(bank=bank, bank_align="centre")
    with pytest.raises(TypeError, match="unexpected keyword argument 'banks'"):
        call(banks=bank)


def test_the_script_has_segment_alls_flags_and_refusals():
    cli = _cli()
    base = ["--synthetic", "40", "192"]

    def check(*extra):
        args = cli.check_confidence_flags(cli.with_defaults(cli.get_args_parser().parse_args(base + list(extra))))
        return cli.check_memory_flags(args), args
    assert check()[0] is False
    banked, a = check("--memory_cols", "0", "16", "--memory_bias", "0", "0.05", "0.1", *SLIDING)
    assert banked and a.memory_bias == [0.0, 0.05, 0.1] and a.memory_cols == [0, 16]
    assert check("--memory_bank", "b.npz", "--seedless", "--memory_align", "center", *SLIDING)[1].memory_bias is None
    for flags, msg in ((["--memory_bias", "0.1"], "--memory_align and --memory_bias need --memory_cols or --memory_bank"),
                       (["--memory_align", "center"], "--memory_align and --memory_bias need"),
                       (["--seedless"], "--seedless and --save_memory_bank need"),
                       (["--memory_cols", "0", "--memory_bank", "b.npz", *SLIDING], "one of the two"),
                       (["--memory_cols", "0"], "need --context sliding"),
                       (["--memory_cols", "0", "--memory_bias", "0", "nan", *SLIDING], "--memory_bias must be a finite number"),
                       (["--memory_cols", "0", "--anchor_context", "restart", "--anchor_every", "2", *SLIDING], "do not combine with --anchor_context restart"),
                       (["--memory_cols", "0", "--seedless", "--correction", "true", *SLIDING], "--seedless and --correction do not combine")):
        with pytest.raises(SystemExit, match=msg):
            check(*flags)


# ================================================================================================ the hand-over
def test_without_the_flags_the_script_prints_the_recorded_stdout(monkeypatch, capsys, tmp_path):
    text, d = run_sweep_cli(monkeypatch, capsys, tmp_path, GOLDEN_ARGS, propagate_sweep=stub_propagate_sweep)
    assert text == open(os.path.join(ROOT, "tests", "golden", "segment_sweep_stdout.txt")).read()
    assert "memory" not in text.lower() and "bias" not in text and "seedless" not in text
    assert not any("memory" in k or k == "seedless" for k in d) and "memory_bias" not in d["grid"] and all("memory_bias" not in c for c in d["configs"])


def test_the_flags_reach_propagate_sweep_and_the_report(monkeypatch, capsys, tmp_path):
    """script -> `segment_sweep(bank=, bank_align=, seedless=)` -> `propagate_sweep(memory=, memory_align=)`, both passes, no seed"""
    import utils as crw_utils
    seen = []

    def stub(seq, seg_ref, model, sweep, ncls, do_pos_embed, use_last, confidence=None, soft=False, memory=None, memory_align=None):
        seen.append((use_last, seg_ref, memory, memory_align, len(sweep.configs), list(sweep.biases)))
        return stub_propagate_sweep(seq, torch.zeros(40, 8), model, sweep, ncls, do_pos_embed, use_last, confidence=confidence, soft=soft)

    flags = SLIDING + ["--memory_cols", "0", "24", "72", "--memory_bias", "0", "0.1", "--memory_align", "center", "--seedless",
                       "--save_memory_bank", str(tmp_path / "bank.npz")]
    text, d = run_sweep_cli(monkeypatch, capsys, tmp_path, GOLDEN_ARGS + flags, propagate_sweep=stub)
    assert len(seen) == 4 and [s[0] for s in seen] == [False, False, True, True]
    for use_last, seg_ref, memory, align, G, biases in seen:
        assert seg_ref is None and isinstance(memory, crw_utils.MemoryBank) and len(memory) == 3 and memory is seen[0][2]
        assert align == "center" and G == 8 and biases == [0.0, 0.1]
    assert os.path.exists(tmp_path / "bank.npz") and len(crw_utils.MemoryBank.load(str(tmp_path / "bank.npz"))) == 3
    assert "Memory bank traces: 3 (no item is seeded)" in text and "Configurations: 8" in text
    assert "memory_bias=[0.0, 0.1]" in text and "memory_align='center'" in text and "seedless=True" in text
    head = next(line for line in text.splitlines() if line.lstrip().startswith("radius"))
    assert head.split()[:5] == ["radius", "temp", "knn", "bias", "accuracy"]
    rows = [line.split() for line in text.splitlines() if re.match(r"\s+4\s+0\.0?1\s+[35]\s", line)]
    assert [r[3] for r in rows] == ["0", "0", "0.1", "0.1"] * 2
    assert d["memory_traces"] == 3 and d["seedless"] is True and d["memory_align"] == "center" and d["grid"]["memory_bias"] == [0.0, 0.1]
    assert [c["memory_bias"] for c in d["configs"]] == [0.0, 0.0, 0.1, 0.1] * 2 and [c["knn"] for c in d["configs"]] == [5, 3] * 4
    b = d["best"]
    assert b["memory_bias"] == d["configs"][b["index"]]["memory_bias"] and f"knn {b['knn']} bias {b['memory_bias']:g} (" in text
    # a bank alone: the axis is absent, the bias column reads 0, the Namespace line hides the two flags
    seen.clear()
    text, d = run_sweep_cli(monkeypatch, capsys, tmp_path, GOLDEN_ARGS + SLIDING + ["--memory_cols", "0", "24"], propagate_sweep=stub)
    assert all(s[1] is not None and s[3] is None and s[4] == 4 and s[5] == [0.0] for s in seen) and len(seen) == 4
    assert "memory_bias" not in text and "memory_align" not in text and "Memory bank traces: 2" in text
    assert d["seedless"] is False and d["memory_align"] is None and d["grid"]["memory_bias"] == [0.0] and {c["memory_bias"] for c in d["configs"]} == {0.0}


def test_propagate_sweep_encodes_the_bank_with_the_item_and_hands_it_on(monkeypatch):
    import crw_hip
    import utils as crw_utils
    T, N, C, M, B = 5, 4, 3, 3, 2
    seq = torch.zeros(T, N, 8, 8)
    bank = crw_utils.memory_bank(torch.ones(B, N, 8, 8), torch.tensor([[0, 1, 1, 2], [0, 0, 1, 2]], dtype=torch.int8))
    feats, mem = torch.randn(T, N, C), torch.randn(B, N, C)
    front = []

    def features_and_seed(s, seg_ref, model, pe, use_last, memory=None, memory_align=None):
        front.append((seg_ref, memory, memory_align))
        return feats, None, mem
    monkeypatch.setattr(crw_utils, "_features_and_seed", features_and_seed)
    monkeypatch.setattr(crw_hip, "xent_metric", lambda f: torch.zeros(N, T - 1))
    monkeypatch.setattr(crw_utils, "column_diffs_async", lambda x: None)
    monkeypatch.setattr(crw_utils, "change_point", lambda x, d=None: None)
    monkeypatch.setattr(crw_hip, "labelprop_confidence", lambda L, T_, N_, M_, kind: torch.ones(N_, T_))

    class Sweep:
        context, biases, configs = "sliding", [0.0, 0.1], [{}] * 4

        def propagate_all(self, f, seed, ncls, **kw):
            self.got = (f, seed, kw)
            G = len(self.configs)
            return torch.zeros(G, N, T), torch.zeros(G, T * N, M)
    sw = Sweep()
    anchors = torch.full((T, N), -1, dtype=torch.int8)
    anchors[2] = 1
    out = crw_utils.propagate_sweep(seq, None, "enc", sw, M, False, True, confidence="maxprob", anchors=anchors, memory=bank, memory_align="center")
    assert front == [(None, bank, "center")]
    f, seed, kw = sw.got
    assert f is feats and seed is None and kw["soft"] is True and kw["memory"][0] is mem and torch.equal(kw["memory"][1], bank.labels)
    assert torch.equal(kw["anchors"], torch.flip(anchors, (0,))) and "anchor_context" not in kw and "memory_bias" not in kw
    assert out[0].shape == (4, N, T) and out[3].shape == (4, N, T)


class _Device:
    """stands in for the four `crw_hip` calls of `LabelPropSweep._propagate_memory`: remembers them, fills every later frame with class 1"""

    def __init__(self):
        self.topk, self.batch = [], None

    def labelprop_topk_scores(self, ehat, cxt, radius, temp, kcap, **kw):
        V, I = kw.pop("out")
        self.topk.append(dict(ehat=ehat.clone(), radius=radius, temp=temp, kcap=kcap, **kw))
        V.fill_(len(self.topk))
        I.fill_(0)
        return V, I

    def labelprop_sweep_weights(self, V, knns, out=None):
        for i, k in enumerate(knns):
            out[i] = 0
            out[i][:, :k] = V[:, :k] / k
        return out

    def labelprop_propagate_batch(self, seed, W, I, T, N, M, **kw):
        self.batch = dict(seed=seed, W=W.clone(), I=I.clone(), T=T, L_in=kw["L"].clone(), pred_in=kw["pred"].clone(),
                          **{k: v for k, v in kw.items() if k not in ("L", "pred")})
        ff = kw["first_frame"]
        kw["L"][:, ff * N:] = torch.eye(M)[1]
        kw["pred"][:, :, ff:] = 1
        return kw["L"], kw["pred"]


@pytest.mark.parametrize("seeded", (True, False))
def test_propagate_all_builds_the_virtual_item_once_for_the_grid(monkeypatch, seeded):
    import crw_hip
    from imported.labelprop import LabelPropSweep
    T, N, C, M, B = 7, 5, 4, 3, 2
    dev = _Device()
    for name in ("labelprop_topk_scores", "labelprop_sweep_weights", "labelprop_propagate_batch"):
        monkeypatch.setattr(crw_hip, name, getattr(dev, name))
    g = torch.Generator().manual_seed(0)
    feats, mem_feats = torch.randn(T, N, C, generator=g), torch.randn(B, N, C, generator=g)
    mem_labels = torch.tensor([[0, 0, 1, 2, 2], [0, 1, 1, 1, 2]], dtype=torch.int8)
    seed = torch.tensor([2.0, 2, 0, 0, 1]) if seeded else None
    anchors = torch.full((T, N), -1, dtype=torch.int8)
    anchors[0], anchors[3, 1], anchors[5] = 2, 0, torch.tensor([0, 1, 2, 0, 1], dtype=torch.int8)
    sweep = LabelPropSweep(2, [2, 3], [0.1], [2, 1], context="sliding", biases=[0.0, 0.2])
    pred, L = sweep.propagate_all(feats, seed, M, soft=True, anchors=anchors, memory=(mem_feats, mem_labels))
    K, G = (B + 1 if seeded else B), 8
    # one selection per (radius, temp, bias), at kmax, with the bias of its place -- and none at 0
    assert [(t["radius"], t.get("long_bias")) for t in dev.topk] == [(2, None), (2, 0.2), (3, None), (3, 0.2)]
    assert all(t["n_long"] == K and t["first_frame"] == K and t["kcap"] == 2 and t["route"] == "auto" for t in dev.topk)
    assert all(torch.equal(t["ehat"], torch.cat([mem_feats, feats])) for t in dev.topk)
    b = dev.batch
    assert b["seed"] is None and b["T"] == B + T and b["n_long"] == K and b["first_frame"] == K and b["context"] == "sliding" and b["cxt_size"] == 2
    assert b["W"].shape == (G, B + T - K, 2, N) and b["I"].shape == b["W"].shape
    free = ~(torch.isinf(b["W"][:, :, 0]) & (b["W"][:, :, 0] < 0))                             # [G, F, N]
    for g_, (p, k) in enumerate((p, k) for p in range(1, 5) for k in (2, 1)):                  # W[g]: selection p's weights at knn k
        assert torch.equal(b["W"][g_, :, 0][free[g_]], torch.full((int(free[g_].sum()),), p / k)), g_
        assert not b["W"][g_, :, k:].any()
    front = torch.cat([mem_labels.long(), seed.long()[None]]) if seeded else mem_labels.long()
    for g_ in range(G):
        assert torch.equal(b["L_in"][g_, :K * N], torch.eye(M)[front.reshape(-1)])           # the rows in front: one-hot, in every slice
        assert torch.equal(b["pred_in"][g_, :, :K], front.t().float())
        want = torch.zeros(B + T - K, N, dtype=torch.bool)                                   # the anchors moved B frames down
        want[B + 3 - K, 1], want[B + 5 - K] = True, True
        if not seeded:
            want[0] = True
        assert torch.equal(~free[g_], want), g_
        assert b["I"][g_, B + 5 - K, 0].tolist() == [0, 1, 2, 0, 1]
    assert pred.shape == (G, N, T) and L.shape == (G, T * N, M) and bool((pred[:, :, 1:] == 1).all())
    if seeded:
        assert torch.equal(pred[0, :, 0], seed) and torch.equal(L[3, :N], torch.eye(M)[seed.long()])


def test_the_per_configuration_arm_hands_every_configuration_its_bias(monkeypatch):
    from imported import labelprop as lp_mod
    T, N, C, M, B = 5, 4, 3, 3, 2
    calls = []

    class One:
        def __init__(self, cfg):
            self.cfg = cfg

        def propagate_all(self, feats, seed, ncls, **kw):
            calls.append((self.cfg, kw))
            return torch.zeros(N, T), torch.zeros(T * N, M)
    monkeypatch.setattr(lp_mod, "LabelPropVOS_CRW", One)
    monkeypatch.setenv("CRW_SWEEP_PER_CONFIG", "1")
    sweep = lp_mod.LabelPropSweep(2, [2], [0.1], [2, 1], context="sliding", biases=[0.0, 0.3])
    memory = (torch.zeros(B, N, C), torch.zeros(B, N, dtype=torch.int8))
    pred = sweep.propagate_all(torch.zeros(T, N, C), None, M, memory=memory)
    assert pred.shape == (4, N, T) and [c[0] for c in calls] == sweep.configs
    assert [c[1]["memory_bias"] for c in calls] == [0.0, 0.0, 0.3, 0.3] and all(c[1]["memory"] is memory for c in calls)
