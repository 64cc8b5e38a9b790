"""GPU side of the 'sliding' context rule (crw_labelprop_propagate_sliding, crw_labelprop_propagate_sliding_batch).  Every case is
held to the definition by `sliding_ref.definition_violations`, the check tests/test_sliding.py proves on planted defects:
  * bit equality of L and pred with `labelprop_gather(seed, W, sliding_rows(I, ...), cxt_size=None)`, the general gather on
    translated lists;
  * `oracle.gather_audit` on the translated lists with zero violations ((knn + 2) * 2^-24 teacher-forced; structure exact),
on the default route AND with CRW_LABELPROP_SLIDING_GENERAL=1 (the general kernels translating in the kernel).  Then the fixtures of
the reference's own `predict` on windowed lists, the drifting items end to end, and `segment` / `segment_sweep` with every option on.
Nothing here provokes a fault."""
import numpy as np
import pytest
import torch

import sliding_ref as sr
from conftest import load_golden
from oracle import crw_oracle as orc
from test_sliding import FIXTURES, PERIODIC, fixture_case, periodic_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_sliding() and crw_hip.has_sweep()
    return crw_hip


def features(T, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, N, C, generator=g)


def check(hip, monkeypatch, emb, M, cxt, radius, temp, knn, first_frame=1, fill=None, seed_labels=None, route=None):
    """emb [T, N, C] (CPU, raw) -> (W, I, L, pred) of the default route, after holding both routes to the definition.
    route: what the default run's route name must start with ("labelprop.slide_ring" / "labelprop.slide_general_").
    first_frame > 1: no seed, L and pred prefilled (frames before first_frame random soft labels); fill: byte the outputs hold before."""
    T, N, C = emb.shape
    ehat = hip.normalize(emb.cuda().contiguous())
    W, I = hip.labelprop_topk(ehat, cxt, radius, temp, knn, first_frame=first_frame)
    R = hip.sliding_rows(I, N, cxt, first_frame)
    if first_frame == 1:
        seed = (torch.arange(N) * M // N).float().cuda() if seed_labels is None else torch.as_tensor(seed_labels).float().cuda()
        L0 = torch.empty(T * N, M, device="cuda")
        p0 = torch.empty(N, T, device="cuda")
        for t in (L0, p0):
            t.view(torch.uint8).fill_(0 if fill is None else fill)
        L_init = pred_init = None
    else:
        seed = None
        g = torch.Generator().manual_seed(first_frame)
        L0 = torch.softmax(torch.randn(T * N, M, generator=g) * 3, -1).cuda()
        L0[:N] = torch.nn.functional.one_hot(torch.arange(N) * M // N, M).float()
        p0 = torch.full((N, T), 7.0, device="cuda")
        L_init, pred_init = L0.clone(), p0.clone()
    gather = lambda s, w, r, li, pi: hip.labelprop_gather(s, w, r, T, N, M, first_frame=first_frame, cxt_size=None,
                                                          L=None if li is None else li.clone(), pred=None if pi is None else pi.clone())
    out = None
    for general in (False, True):
        if general:
            monkeypatch.setenv("CRW_LABELPROP_SLIDING_GENERAL", "1")
        else:
            monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
        with hip.routes() as hit:
            L, pred = hip.labelprop_gather(seed, W, I, T, N, M, first_frame=first_frame, L=L0.clone(), pred=p0.clone(), cxt_size=cxt,
                                           context="sliding")
        torch.cuda.synchronize()
        # the library's own account of the route (include/crw_hip_routes.h): one sliding launch, the switch's arm on the general kernels
        assert len(hit) == 1 and all(k.startswith("labelprop.slide_") for k in hit), dict(hit)
        assert not general or next(iter(hit)).startswith("labelprop.slide_general_"), dict(hit)
        if route is not None and not general:
            assert next(iter(hit)).startswith(route), (route, dict(hit))
        v = sr.definition_violations(gather, seed, W, R, M, first_frame, L, pred, L_init, pred_init)
        print(("general" if general else "default"), v)
        assert not any(v.values()), (general, v)
        out = out or (W, I, L, pred)
    monkeypatch.delenv("CRW_LABELPROP_SLIDING_GENERAL", raising=False)
    return out


# name: (T, N, M, C, cxt, radius, temp, knn)
CASES = {
    "ring wraps many times, N * M = 39": (30, 13, 3, 8, 4, 3, 0.1, 4),
    "first translated frame is the last, T = cxt + 3": (9, 24, 3, 16, 6, 4, 0.05, 5),
    "T = cxt + 2: no frame is translated": (8, 24, 3, 16, 6, 4, 0.05, 5),
    "window of one frame": (12, 10, 3, 8, 1, 3, 0.1, 3),
    "knn 4 (8 registers)": (20, 16, 4, 16, 5, 4, 0.1, 4),
    "knn 10 (16 registers)": (20, 16, 4, 16, 5, 6, 0.1, 10),
    "knn 20 (24 registers)": (20, 24, 4, 16, 5, 8, 0.1, 20),
    "general: knn 30, LDS kernel": (16, 40, 3, 16, 4, 12, 0.1, 30),
    "general: N * M = 500": (14, 100, 5, 16, 4, 4, 0.1, 6),
    "general: ring exceeds the LDS": (108, 48, 8, 16, 100, 5, 0.1, 6),
    "empty slots: radius 1, knn 5": (14, 12, 3, 8, 4, 1, 0.1, 5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_every_route_is_the_gather_on_translated_lists(hip, monkeypatch, name):
    T, N, M, C, cxt, radius, temp, knn = CASES[name]
    # a case named "general: ..." claims the general kernels by its shape, every other the ring kernel
    route = "labelprop.slide_general_" if name.startswith("general:") else "labelprop.slide_ring"
    W, I, L, pred = check(hip, monkeypatch, features(T, N, C, len(name)), M, cxt, radius, temp, knn, route=route)
    if T > cxt + 2:  # the rule matters: the reference rule's labels differ somewhere
        Lr, _ = hip.labelprop_gather((torch.arange(N) * M // N).float().cuda(), W, I, T, N, M, cxt_size=cxt)
        assert not torch.equal(L, Lr)
    if "empty" in name:
        assert (W == 0).any()


@pytest.mark.parametrize("T", [3, 5])
def test_nothing_slides_within_the_context_bit_equal_to_the_reference_rule(hip, monkeypatch, T):
    N, M, cxt = 13, 3, 4  # T <= cxt + 1
    W, I, L, pred = check(hip, monkeypatch, features(T, N, 8, T), M, cxt, 3, 0.1, 4)
    Lr, pr = hip.labelprop_gather((torch.arange(N) * M // N).float().cuda(), W, I, T, N, M, cxt_size=cxt, context="reference")
    assert torch.equal(L.view(torch.int32), Lr.view(torch.int32)) and torch.equal(pred, pr)


def test_the_oldest_frame_of_the_window_is_selected(hip, monkeypatch):
    """Periodic features (period = cxt): the top neighbour of a late query lies in frame n - cxt, whose ring slot is the next to be
    overwritten -- a ring of cxt slots would be storing frame n into it while other waves still read (N * M = 96: two compute waves)."""
    p = PERIODIC
    emb, seed = periodic_case()
    W, I, L, pred = check(hip, monkeypatch, torch.tensor(emb), p["M"], p["cxt"], p["radius"], p["temp"], p["knn"], seed_labels=seed)
    frac = sr.oldest_top_fraction(I.cpu().numpy(), p["N"], p["cxt"])
    print(f"top neighbour in frame n - cxt: {frac:.2f}")
    assert frac >= 0.25


def test_a_later_first_frame_without_a_seed_leaves_earlier_frames_untouched(hip, monkeypatch):
    T, N, M, cxt = 20, 13, 3, 4
    check(hip, monkeypatch, features(T, N, 8, 3), M, cxt, 3, 0.1, 4, first_frame=cxt + 4)  # `untouched` is one of the audit's conditions


def test_stale_memory_does_not_reach_the_results(hip, monkeypatch):
    T, N, M, cxt = 20, 13, 3, 4
    a = check(hip, monkeypatch, features(T, N, 8, 4), M, cxt, 3, 0.1, 4, fill=0xFF)
    b = check(hip, monkeypatch, features(T, N, 8, 4), M, cxt, 3, 0.1, 4, fill=0x00)
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[3], b[3])


@pytest.mark.parametrize("per_config", [False, True])
def test_batch_slices_are_the_one_configuration_calls(hip, monkeypatch, per_config):
    """G = 6 (2 radii x one temp x 3 knn): P = 2 lists of indices, one per radius, so the batch reads a per-configuration I; both arms
    of LabelPropSweep against LabelPropVOS_CRW per configuration, and the batch entry point against the definition."""
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    T, N, M, C, cxt = 24, 16, 4, 16, 5
    feats = hip.normalize(features(T, N, C, 9).cuda())
    seed = (torch.arange(N) * M // N).float().cuda()
    sweep = LabelPropSweep(cxt, (3, 6), (0.1,), (3, 5, 8), context="sliding")
    if per_config:
        monkeypatch.setenv("CRW_SWEEP_PER_CONFIG", "1")
    pred, L = sweep.propagate_all(feats, seed, M, soft=True)
    assert tuple(pred.shape) == (6, N, T) and tuple(L.shape) == (6, T * N, M)
    monkeypatch.delenv("CRW_SWEEP_PER_CONFIG", raising=False)
    for g, cfg in enumerate(sweep.configs):
        assert cfg["CONTEXT"] == "sliding"
        p1, L1 = LabelPropVOS_CRW(cfg).propagate_all(feats, seed, M)
        assert torch.equal(L[g].view(torch.int32), L1.view(torch.int32)) and torch.equal(pred[g], p1), cfg
        W, I = hip.labelprop_topk(feats, cxt, cfg["RADIUS"], cfg["TEMP"], cfg["KNN"])
        gather = lambda s, w, r, li, pi: hip.labelprop_gather(s, w, r, T, N, M, cxt_size=None)
        v = sr.definition_violations(gather, seed, W, hip.sliding_rows(I, N, cxt), M, 1, L[g], pred[g])
        assert not any(v.values()), (cfg, v)
    ref = LabelPropSweep(cxt, (3, 6), (0.1,), (3, 5, 8)).propagate_all(feats, seed, M)
    assert not torch.equal(ref, pred)


# ------------------------------------------------------------------------------------------------ fixtures of the reference's predict
@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_through_propagate_all_and_predict(hip, name):
    """The reference's own `predict` on windowed lists: labels exact; L within the fixture's recorded deviation from fp64 plus the
    project's bound."""
    from imported.labelprop import LabelPropVOS_CRW
    g, emb, seed, M, cfg = fixture_case(name)
    T, N, C = emb.shape
    tol = float(g["deviation"]) + orc.gather_bound(cfg["KNN"])
    lp = LabelPropVOS_CRW(dict(cfg, CONTEXT="sliding"))
    feats = hip.normalize(torch.tensor(emb).cuda())
    pred, L = lp.propagate_all(feats, torch.tensor(seed).cuda(), M)
    err = float((L.reshape(T, N, M).cpu() - torch.tensor(g["L"])).abs().max())
    print(f"{name}: propagate_all {err:.3e} (tolerance {tol:.3e})")
    assert np.array_equal(pred.cpu().numpy(), g["pred"]) and err <= tol
    as_feat = lambda n: feats[n].t().reshape(1, C, N, 1)
    masks = [torch.nn.functional.one_hot(torch.tensor(seed).long(), M).float().t().reshape(1, M, N, 1).cuda()]
    fs = [as_feat(0)]
    for n in range(1, T):
        masks.append(lp.predict(fs, masks, as_feat(n)))  # the FULL lists: the rule windows them
        fs.append(as_feat(n))
    Lp = torch.cat(masks, 0)[..., 0].permute(0, 2, 1).cpu()
    err = float((Lp - torch.tensor(g["L"])).abs().max())
    print(f"{name}: predict {err:.3e}")
    assert np.array_equal(Lp.argmax(-1).t().float().numpy(), g["pred"]) and err <= tol
    assert torch.equal(Lp.reshape(T * N, M), L.cpu())  # frame by frame or all at once: the same bits


def test_drifting_layers_end_to_end_on_the_device(hip):
    """The README's table through `LabelPropVOS_CRW.propagate_all`: sliding leaves <= 1 % of the late labels wrong, the reference rule
    >= 20 % -- on the code before the rule existed the CONTEXT key was ignored and both maps were the reference rule's."""
    from imported.labelprop import LabelPropVOS_CRW
    for (T, N, C, M, cxt, radius, temp, knn, amp) in sr.DRIFT_SHAPES:
        for s in sr.DRIFT_SEEDS:
            emb, cls = sr.drifting_item(s, T, N, C, M, amp)
            feats, seed = hip.normalize(torch.tensor(emb).cuda()), torch.tensor(cls[0]).float().cuda()
            cfg = dict(CXT_SIZE=cxt, RADIUS=radius, TEMP=temp, KNN=knn)
            ps = LabelPropVOS_CRW(dict(cfg, CONTEXT="sliding")).propagate_all(feats, seed, M)[0].cpu().numpy()
            pr = LabelPropVOS_CRW(cfg).propagate_all(feats, seed, M)[0].cpu().numpy()
            (es, tot), (er, _) = sr.late_errors(ps, cls, cxt), sr.late_errors(pr, cls, cxt)
            print(f"[{T}, {N}] seed {s}: reference rule {er}, sliding {es} of {tot}")
            assert es <= 0.01 * tot and er >= 0.20 * tot, (T, N, s, er, es, tot)


# ------------------------------------------------------------------------------------------------ segment / segment_sweep
def _synthetic(rows, cols, K):
    import dataset as crw_dataset
    import utils as crw_utils
    from test_sweep_dense_gpu import _cli
    rg = crw_dataset.synthetic_radargram(rows, cols)
    seg = _cli("segment_all").synthetic_reference(rows, cols, K)
    torch.manual_seed(11)
    enc = crw_utils.create_model(1, False).cuda()
    enc.train(True)
    return rg, seg, enc


def test_segment_with_every_option_equals_the_translated_lists_definition(hip, monkeypatch):
    """200 x 4800 (three items of T = 100 at CXT_SIZE 20), bilinear maps, maxprob confidence, reverse pass merged by confidence, a forced
    correction: `segment` under CONTEXT 'sliding' against the same call with `propagate_all` replaced by the definition -- the
    general gather on `sliding_rows(I)`."""
    import dataset as crw_dataset
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    from test_sweep_dense_gpu import force
    rows, cols, T, patch, overlap, K = 200, 4800, 100, (16, 16), (8, 0), 5
    rg, seg, enc = _synthetic(rows, cols, K)
    cfg = dict(CXT_SIZE=20, RADIUS=10, TEMP=0.1, KNN=10)
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cuda", confidence="maxprob", merge="confidence", upsample="bilinear")
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap)

    def run(lp):
        monkeypatch.setattr(crw_inference, "propagate", force(crw_utils.propagate, [60, None, None]))
        return crw_inference.segment(fresh(), seg, enc, lp, K, T, patch, overlap, **kw)

    out = run(LabelPropVOS_CRW(dict(cfg, CONTEXT="sliding")))

    class Definition(LabelPropVOS_CRW):
        def propagate_all(self, feats, seed, nclasses, grid_w=1):
            Tn, N, _ = feats.shape
            W, I = hip.labelprop_topk(feats, self.cxt_size, self.radius, self.temperature, self.topk, first_frame=1, grid_w=grid_w)
            L, pred = hip.labelprop_gather(seed.float().contiguous(), W, hip.sliding_rows(I, N, self.cxt_size), Tn, N, nclasses, cxt_size=None)
            return pred, L

    want = run(Definition(dict(cfg, CONTEXT="sliding")))
    ref = run(LabelPropVOS_CRW(cfg))
    assert out["change_idx"] == want["change_idx"]
    for k in ("pred", "forward"):
        assert torch.equal(out[k], want[k]), k
    for k in ("conf", "forward_conf"):
        assert torch.equal(out[k].view(torch.int32), want[k].view(torch.int32)), k
    assert tuple(out["pred"].shape) == (rows, cols) and not torch.equal(out["forward"], ref["forward"])


def test_segment_sweep_equals_segment_per_configuration_under_the_sliding_rule(hip, monkeypatch):
    import dataset as crw_dataset
    from imported.labelprop import LabelPropSweep
    from test_sweep_dense_gpu import sweep_against_segment
    rows, cols, T, patch, overlap, K = 200, 1600, 50, (16, 16), (8, 0), 5
    rg, seg, enc = _synthetic(rows, cols, K)
    sweep = LabelPropSweep(10, (5, 10), (0.1,), (5, 10), context="sliding")
    kw = dict(correction=True, use_last=True, dataset_id=3, device="cuda", confidence="margin", merge="confidence", upsample="bilinear")
    fresh = lambda: crw_dataset.RGDataset.from_tensor(rg, T, patch, overlap)
    out = sweep_against_segment(monkeypatch, fresh, (seg, enc, K, T, patch, overlap), sweep, kw, [30, None])
    plain = LabelPropSweep(10, (5, 10), (0.1,), (5, 10))
    ref = sweep_against_segment(monkeypatch, fresh, (seg, enc, K, T, patch, overlap), plain, kw, [30, None])
    assert not torch.equal(out["forward"], ref["forward"])
