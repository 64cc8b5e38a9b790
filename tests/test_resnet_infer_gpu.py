"""The two forward-only passes of the `Resnet` on the MI355X against fp64 PyTorch modules, on a trained-like state
(resnet_infer_ref.py: gamma of both signs and zero, beta off zero, running statistics of ANOTHER batch distribution than the one
run): crw_rn_eval_fwd (`encoder.train(False)`, BatchNorm on the running statistics) and crw_rn_train_fwd_nograd (train-mode
BatchNorm under `torch.no_grad()`), at every stem route (patch per wave, band, gathered -- the latter in eval mode launches
rn_stem_apply_kernel, which nothing else does), both input channel counts, batches around the 128-patch tile (1, 127, 128, 129,
257) and final maps of 1x1, 2x2 and 2x3.

Bars, none new: features max |y - y64| <= 1e-4 max |y64| (test_resnet_step_at_bench_batch_matches_fp64's bar for the training
forward); running statistics after a no-grad pass rtol 1e-3 / atol 1e-5 (test_resnet_hip_matches_pytorch_modules).
test_resnet_infer.py shows on the host that the cases are well posed at a tenth of these bars and that one-line mistakes move
the result by more than a hundred of them.  Every PyTorch convolution / batch-norm / pool entry point is disabled and warnings
are errors while the device runs: a silent fallback fails.  `pytest -s` prints worst error / bar, the route and the bitwise notes
per case (profiles/resnet_infer_tests.log)."""
import copy
import warnings

import pytest
import torch

import resnet_infer_ref as R
from test_resnet_hip import _no_library_convs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available()
    return crw_hip


def _expected_route(hip, h, w, route):
    """the table's route, checked against the band kernel's own geometry rule (None in the table: whatever that rule says)"""
    if (h, w) == (16, 16):
        assert route == R.PPW
        return route
    ok = hip.rn_stem_band_ok(h, w)
    if route is None:
        return R.BAND if ok else R.GATHERED
    assert ok == (route == R.BAND), f"crw_rn_stem_band_ok({h}, {w}) = {ok}: the table expects {route}; replace the size, keep the route"
    return route


def _device(case, train):
    h, w, cin, P, _ = case
    enc = copy.deepcopy(R.case_net(h, w, cin)).cuda().train(train)
    assert enc.hip_convs == "bf16x3"
    return enc, R.case_input(h, w, cin, P).cuda()


def _run(hip, monkeypatch, enc, x, grad=False):
    """enc(x) on the hand-written kernels alone -> (y, {route: count})"""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _no_library_convs(monkeypatch)
        with torch.set_grad_enabled(grad), hip.routes() as hit:
            y = enc(x)
    monkeypatch.undo()
    torch.cuda.synchronize()
    return y, dict(hit)


def _stem_routes(hit):
    return {k for k in hit if k.startswith("rn_stem.")}


@pytest.mark.parametrize("case", R.cases("eval"), ids=R.case_id)
def test_eval_forward_matches_fp64(hip, monkeypatch, case):
    h, w, cin, P, route = case
    route = _expected_route(hip, h, w, route)
    y64 = R.case_reference(h, w, cin, P, "eval")
    enc, x = _device(case, False)
    before = {k: v.clone() for k, v in enc.named_buffers()}
    y, hit = _run(hip, monkeypatch, enc, x)
    assert y.shape == (P, 128) and not y.requires_grad and bool(torch.isfinite(y).all())
    err, scale = R.feature_error(y, y64)
    print(f"\n  eval {R.case_id(case)}: {sorted(_stem_routes(hit))}, worst error / bar = {err / R.FEATURE_BAR:.3f} (feature scale {scale:.3f})")
    assert _stem_routes(hit) == {route}, hit
    assert err <= R.FEATURE_BAR, (err, scale)
    for k, v in enc.named_buffers():  # eval mode updates nothing, num_batches_tracked included
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("case", R.cases("nograd"), ids=R.case_id)
def test_nograd_forward_matches_fp64(hip, monkeypatch, case):
    h, w, cin, P, route = case
    route = _expected_route(hip, h, w, route)
    y64, buf64 = R.case_reference(h, w, cin, P, "nograd")
    enc, x = _device(case, True)
    y, hit = _run(hip, monkeypatch, enc, x)
    assert y.shape == (P, 128) and not y.requires_grad and bool(torch.isfinite(y).all())
    err, scale = R.feature_error(y, y64)
    got = dict(enc.named_buffers())
    worst, where = R.buffer_error(got, buf64)
    # the same module with grad enabled (crw_rn_train_fwd, keep = true): the no-grad pass drops nothing the forward needs
    twin, _ = _device(case, True)
    y2, hit2 = _run(hip, monkeypatch, twin, x, grad=True)
    same = torch.equal(y2.detach(), y)
    print(f"\n  no-grad {R.case_id(case)}: {sorted(_stem_routes(hit))}, worst error / bar = {err / R.FEATURE_BAR:.3f} (feature scale {scale:.3f}), "
          f"running statistics {worst:.3f} of their bar ({where}), bit for bit the grad-enabled forward: {same}")
    assert _stem_routes(hit) == {route} and _stem_routes(hit2) == {route}, (hit, hit2)
    assert err <= R.FEATURE_BAR, (err, scale)
    assert worst <= 1.0, (worst, where)
    for k, v in got.items():
        if not v.is_floating_point():
            assert int(v) == int(buf64[k]) == 101, k  # num_batches_tracked + 1
    assert y2.requires_grad and same
    for (k, u), (_, v) in zip(enc.named_buffers(), twin.named_buffers()):
        assert torch.equal(u, v), k


@pytest.mark.parametrize("case", [c for c in R.cases("eval") if c[3] == 129], ids=R.case_id)
def test_eval_does_not_depend_on_batch_composition(hip, monkeypatch, case):
    """129 patches at once against their first 128 and their last 1 run separately: in eval mode a patch's features are its own"""
    h, w, cin, P, _ = case
    scale = R.case_reference(h, w, cin, P, "eval").abs().max().item()
    enc, x = _device(case, False)
    y, _ = _run(hip, monkeypatch, enc, x)
    ya, _ = _run(hip, monkeypatch, enc, x[:128])
    yb, _ = _run(hip, monkeypatch, enc, x[128:])
    parts = torch.cat([ya, yb])
    diff = (y - parts).abs().max().item() / scale
    print(f"\n  eval {R.case_id(case)} against 128 + 1: {diff / R.FEATURE_BAR:.3g} x bar apart, bit for bit: {torch.equal(y, parts)}")
    assert diff <= 2 * R.FEATURE_BAR


def test_eval_through_propagate_at_a_gathered_size(hip, monkeypatch):
    """`utils.propagate` with the eval-mode, trained-like encoder at 16x85 patches (gathered stem): the label map against the
    oracle's label propagation on the device's features -- the audit test_resnet_inference_through_propagate holds in train mode"""
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    from oracle import crw_oracle as orc
    T, N, M, h, w, ov = 6, 20, 4, 16, 85, 8
    assert not hip.rn_stem_band_ok(h, w)
    enc = copy.deepcopy(R.case_net(h, w, 1)).cuda().train(False)
    g = torch.Generator().manual_seed(h * w)
    rows = N * (h - ov) + ov
    rg = torch.sin(torch.arange(rows)[:, None] / 9.0 + 0.01 * torch.arange(T * w)[None, :]) + 0.5 * torch.randn(rows, T * w, generator=g)
    seq = torch.stack([torch.stack([rg[n * (h - ov):n * (h - ov) + h, t * w:(t + 1) * w] for n in range(N)]) for t in range(T)]).cuda()
    seg = (torch.arange(rows)[:, None] * M // rows).float().repeat(1, w).cuda()
    cfg = dict(CXT_SIZE=4, RADIUS=5, TEMP=0.1, KNN=5)
    stats = {k: v.clone() for k, v in enc.named_buffers()}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _no_library_convs(monkeypatch)
        with hip.routes() as hit:
            pred, xent, _ = crw_utils.propagate(seq, seg, enc, LabelPropVOS_CRW(cfg), M, False, False)
        with torch.no_grad():
            y = enc(seq.reshape(T * N, 1, h, w))
    monkeypatch.undo()
    assert _stem_routes(hit) == {R.GATHERED}, hit
    for k, v in enc.named_buffers():
        assert torch.equal(v, stats[k]), k
    assert pred.shape == (N, T) and xent.shape == (N, T - 1)
    assert torch.equal(pred[:, 0], crw_utils.seed_labels(seg, N))
    feats = hip.normalize(y.reshape(T, N, -1).float().contiguous())
    pred2, L = LabelPropVOS_CRW(cfg).propagate_all(feats, crw_utils.seed_labels(seg, N), M)
    assert torch.equal(pred, pred2)  # the same features both times: eval mode has no state
    audit = orc.labelprop_tie_audit(feats.cpu().numpy(), L.cpu().numpy(), pred.cpu().numpy(), cfg["CXT_SIZE"], cfg["RADIUS"],
                                    cfg["TEMP"], cfg["KNN"], eps=1e-5)
    print(f"\n  eval through propagate at {h}x{w}: {sorted(_stem_routes(hit))}, labels per class {torch.bincount(pred.flatten().long().cpu(), minlength=M).tolist()}, "
          f"audit {audit}")
    assert audit["not_ties"] == 0 and audit["max_soft_err"] <= 1e-4, audit
