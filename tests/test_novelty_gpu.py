"""GPU side of the context novelty: `crw_labelprop_novelty` (include/crw_hip_novelty.h) through the C ABI and the binding, held to
the fp64 definition of tests/novelty_ref.py by its checker (which tests/test_novelty.py proves on planted defects).
  * every nov entry within (C + 2) 2^-24 of the definition (`oracle.topk_score_bound(C, 1.0)`), every score within
    (C + 2 + 2 (top + 1)) 2^-24 (`novelty_ref.score_bound`), on both routes; 'auto' bitwise the route the shape selects; the two
    routes within twice the bound of each other; nov against 1 - temp V[:, 0, :] of `labelprop_topk_scores`, origins included.
  * shapes: the smallest at which each branch can go wrong -- N < 16 and C = 8 (vector only, truncated context), N no multiple of
    16 on the matrix route, three query tiles, radius 1 and radius >= N, first_frame 3, top 1 and top N, origins from
    `restart_ref.patterns`.
  * the picks from the device's scores equal the fp64 picks on the emerging and the two-onset [30, 13] items.
  * the entry point under `run_banded` and `run_twice` of tests/stale_ref.py, both routes; the CRW_EINVAL cases.
  * `segment(..., suggest=2)` on a synthetic 96 x 320 radargram pair, and segment_all.py --suggest_anchors in a child process.
Nothing here provokes a fault."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import anchored_ref as ar
import novelty_ref as nr
import restart_ref as rr
import sliding_ref as slr
import stale_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I32 = torch.float32, torch.int32
U = 2.0 ** -24
# (T, N, C, cxt, radius)
SHAPES = ((30, 13, 8, 4, 3), (40, 24, 16, 6, 4), (64, 48, 32, 10, 5))


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_novelty() and crw_hip.has_sweep() and crw_hip.has_anchor_restart()
    return crw_hip


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def eq_bits(a, b):
    return torch.equal(a.view(I32), b.view(I32))


def features(hip, T, N, C, seed=0):
    g = torch.Generator().manual_seed(T + N + C + seed)
    return hip.normalize((torch.randn(1, N, C, generator=g) + 0.5 * torch.randn(T, N, C, generator=g)).cuda())


def call(lib, ehat, cxt, radius, first, top, origin, route, out=None):
    T, N, C = ehat.shape
    nov, score = out or (torch.empty(T - first, N, device="cuda"), torch.empty(T - first, device="cuda"))
    return lib.crw_labelprop_novelty(_p(ehat), T, N, C, cxt, radius, first, top, _p(origin), _p(nov), _p(score), route, _stream()), nov, score


def routes_of(C):
    return (1, 2) if C % 16 == 0 else (1,)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_both_routes_are_the_definition(hip, shape):
    T, N, C, cxt, radius = shape
    lib, ehat = hip.lib(), features(hip, *shape[:3])
    M = 3
    origins = {"none": None}
    for name in ("a full frame at 1", "two consecutive full frames", "a restart at 2, after which the window slides again",
                 "every frame full", "partial rows between full frames"):
        pat = rr.patterns(T, N, M, cxt)
        if name in pat:
            origins[name] = torch.from_numpy(rr.origins(pat[name][0], M, pat[name][1]))
    assert len(origins) >= 5 and any(o is not None and o.any() for o in origins.values())
    cases = [(cxt, radius, 1, nr.default_top(N), k) for k in origins]
    cases += [(cxt, 1, 1, nr.default_top(N), "none"), (cxt, N, 1, 1, "none"), (cxt, N + 7, 1, N, "every frame full"),
              (cxt, radius, 3, nr.default_top(N), "none"), (cxt, radius, 3, N, "two consecutive full frames"), (T + 5, radius, 1, 1, "none")]
    worst = dict(nov=0.0, score=0.0)
    for cx, rad, first, top, oname in cases:
        origin = origins[oname]
        od = None if origin is None else origin.cuda()
        ref = nr.reference(ehat, cx, rad, top, origin, first)
        got = {}
        for route in routes_of(C):
            st, nov, score = call(lib, ehat, cx, rad, first, top, od, route)
            assert st == 0, (st, route)
            v = nr.violations(ehat, cx, rad, top, origin, first, nov, score, ref=ref)
            en, es = np.abs(nov.cpu().numpy() - ref[0]).max() / nr.nov_bound(C), np.abs(score.cpu().numpy() - ref[1]).max() / nr.score_bound(C, top)
            worst = dict(nov=max(worst["nov"], en), score=max(worst["score"], es))
            assert not any(v.values()), (cx, rad, first, top, oname, route, v, en, es)
            got[route] = (nov, score)
        st, nov, score = call(lib, ehat, cx, rad, first, top, od, 0)
        auto = 2 if C % 16 == 0 else 1
        assert st == 0 and eq_bits(nov, got[auto][0]) and eq_bits(score, got[auto][1]), (cx, rad, first, top, oname)
        if len(got) == 2:                                                  # the two routes: each within the bound of the definition
            assert (got[1][0] - got[2][0]).abs().max().item() <= 2 * nr.nov_bound(C)
            assert (got[1][1] - got[2][1]).abs().max().item() <= 2 * nr.score_bound(C, top)
        if origin is not None and not origin.any():                       # all-zero origins: the call without them, bit for bit
            st, n0, s0 = call(lib, ehat, cx, rad, first, top, None, 0)
            assert st == 0 and eq_bits(n0, nov) and eq_bits(s0, score)
        # against the top-k's own best logit: 1 - temp V[:, 0, :]
        temp = 0.1
        V, _ = hip.labelprop_topk_scores(ehat, cx, rad, temp, 1, first_frame=first, origin=origin)
        assert ((1 - temp * V[:, 0, :].double()) - nov.double()).abs().max().item() <= nr.nov_bound(C) + 2 * U
        # the binding: the same bits
        bn, bs = hip.labelprop_novelty(ehat, cx, rad, top=top, first_frame=first, origin=origin, route=("vector", "matrix")[auto - 1])
        assert eq_bits(bn, nov) and eq_bits(bs, score)
    print(f"{shape}: worst error / bound: nov {worst['nov']:.3g}, score {worst['score']:.3g}")
    if C % 16:
        assert call(lib, ehat, cxt, radius, 1, 1, None, 2)[0] == hip.CRW_EINVAL       # the matrix route cannot take C = 8
        with pytest.raises(hip.CrwError, match="CRW_EINVAL"):
            hip.labelprop_novelty(ehat, cxt, radius, route="matrix")


def test_what_the_entry_point_refuses(hip):
    lib, ehat = hip.lib(), features(hip, 6, 20, 16)
    E = hip.CRW_EINVAL
    ok = lambda **k: call(lib, ehat, **{**dict(cxt=3, radius=2, first=1, top=5, origin=None, route=0), **k})[0]
    assert ok() == 0
    assert ok(top=0) == E and ok(top=21) == E and ok(first=0) == E and ok(first=6) == E and ok(route=3) == E and ok(route=-1) == E
    assert ok(cxt=0) == E and ok(radius=0) == E
    nov, score = torch.empty(5, 20, device="cuda"), torch.empty(5, device="cuda")
    args = lambda e, T, N, C, n, s: lib.crw_labelprop_novelty(_p(e), T, N, C, 3, 2, 1, 5, None, _p(n), _p(s), 0, _stream())
    assert args(None, 6, 20, 16, nov, score) == E and args(ehat, 6, 20, 16, None, score) == E and args(ehat, 6, 20, 16, nov, None) == E
    assert args(ehat, 1, 20, 16, nov, score) == E and args(ehat, 6, 4097, 16, nov, score) == E and args(ehat, 6, 0, 16, nov, score) == E
    assert args(ehat, 6, 20, 0, nov, score) == E
    assert lib.crw_labelprop_novelty(_p(ehat), 6, 20, 16, 3, 2, 1, 5, None, _p(nov), _p(score), 2, _stream()) == 0
    off = ehat.reshape(-1)[1:1 + 5 * 20 * 16].view(5, 20, 16)            # 4-byte aligned only: no float4 loads, so no matrix route
    assert call(lib, off, 3, 2, 1, 5, None, 2)[0] == E and call(lib, off, 3, 2, 1, 5, None, 0)[0] == 0
    with pytest.raises(ValueError, match="top must lie"):
        hip.labelprop_novelty(ehat, 3, 2, top=21)


def test_the_picks_from_the_device_are_the_fp64_picks(hip):
    from imported.labelprop import LabelPropVOS_CRW
    T, N, C, M, cxt, radius, temp, knn, amp = slr.DRIFT_SHAPES[0]
    lp = LabelPropVOS_CRW(dict(CXT_SIZE=cxt, RADIUS=radius, TEMP=temp, KNN=knn, CONTEXT="sliding"))
    for s in slr.DRIFT_SEEDS:
        for emb, cls in (ar.emerging_item(s, T, N, C, M, amp)[:2], nr.two_onsets_item(s, T, N, C, M + 1, amp)[:2]):
            want = nr.suggest(emb, cxt, radius, 3)
            nov, score = lp.novelty(hip.normalize(torch.from_numpy(emb).cuda()))
            got = hip.suggest_frames(score, cxt, 3)
            assert [f for f, _, _ in got] == [f for f, _, _ in want], (s, got, want)
            assert max(abs(a[1] - b[1]) for a, b in zip(got, want)) <= 2 * nr.score_bound(C, N // 4)
            # with the first pick labelled: under 'restart' the keys start there, and it is not proposed again
            anchor = torch.full((T, N), -1, dtype=torch.int8)
            anchor[want[0][0]] = torch.from_numpy(cls[want[0][0]]).to(torch.int8)
            origin = rr.origins(anchor.numpy(), int(cls.max()) + 1)
            n2, s2 = lp.novelty(hip.normalize(torch.from_numpy(emb).cuda()), anchors=anchor, anchor_context="restart", nclasses=int(cls.max()) + 1)
            assert not any(nr.violations(nr.normalized(emb), cxt, radius, None, origin, 1, n2, s2).values())
            want2 = nr.suggest(emb, cxt, radius, 2, origin=origin, anchored=[want[0][0]])
            assert [f for f, _, _ in hip.suggest_frames(s2, cxt, 2, anchored=[want[0][0]])] == [f for f, _, _ in want2]
            n3, s3 = lp.novelty(hip.normalize(torch.from_numpy(emb).cuda()), anchors=anchor)              # clamp: the keys are unchanged
            assert eq_bits(n3, nov) and eq_bits(s3, score)


# ================================================================================================ stale memory and guard bands
def banded_case(hip, home, shape, route):
    T, N, C, cxt, radius = shape
    lib, first, top = hip.lib(), 1, nr.default_top(N)
    origin = torch.zeros(T, dtype=I32)
    for n in range(1, T):
        origin[n] = n - 1 if n - 1 in (2, 3, T - 4) else origin[n - 1]
    ehat, od = home.many(ehat=features(hip, T, N, C), origin=origin.cuda())
    F = T - first
    bufs = dict(nov=sr.Buf(F * N * 4, F32, step=N * 4), score=sr.Buf(F * 4, F32), nov0=sr.Buf(F * N * 4, F32, step=N * 4), score0=sr.Buf(F * 4, F32))
    view = lambda t, k, *s: t[k][:int(np.prod(s)) * 4].view(F32).view(*s)

    def run(_, t):
        for o, (a, b) in ((od, ("nov", "score")), (None, ("nov0", "score0"))):
            st = lib.crw_labelprop_novelty(_p(ehat), T, N, C, cxt, radius, first, top, _p(o), _p(view(t, a, F, N)), _p(view(t, b, F)), route, _stream())
            assert st == 0, st
        torch.cuda.synchronize()

    def check(t):
        ref = nr.reference(ehat, cxt, radius, top, origin, first)
        assert not any(nr.violations(ehat, cxt, radius, top, origin, first, view(t, "nov", F, N), view(t, "score", F), ref=ref).values())
        assert not any(nr.violations(ehat, cxt, radius, top, None, first, view(t, "nov0", F, N), view(t, "score0", F)).values())
    return sr.Case(f"crw_labelprop_novelty (route {route})", None, bufs, run, device="cuda", home=home), check


@pytest.mark.parametrize("shape,route", [(SHAPES[0], 1), (SHAPES[1], 1), (SHAPES[1], 2), (SHAPES[2], 2)], ids=str)
def test_entry_point_over_stale_memory_and_between_guard_bands(hip, shape, route):
    case, check = banded_case(hip, sr.Home("cuda"), shape, route)
    assert case.home.operands
    check(sr.run_banded(case))
    check(sr.run_twice(case))


# ================================================================================================ end to end
def test_segment_suggests_and_changes_nothing_else(hip, tmp_path):
    """two synthetic radargrams of T = 10 on a 96 x 320 map: `segment(..., suggest=2)` -- pred bitwise that of suggest=0, the new keys,
    the novelty against the definition on the features the pass ran on, anchors honoured; segment_all.py --suggest_anchors 2."""
    import inference as crw_inference
    import utils
    from imported.labelprop import LabelPropVOS_CRW
    from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case
    enc, fresh, seg, _, N = e2e_case(0, n_rg=2, H=100)
    T, step = T_E2E, PATCH[1] - OVERLAP[1]
    rg_len = T * step + OVERLAP[1]
    assert (seg.shape[0], 2 * rg_len) == (96, 320)
    cfg = dict(CXT_SIZE=6, RADIUS=6, TEMP=0.1, KNN=8, CONTEXT="sliding")
    run = lambda **k: crw_inference.segment(fresh(), seg, enc, LabelPropVOS_CRW(dict(cfg)), M_E2E, T, PATCH, OVERLAP, use_last=True, dataset_id=2,
                                            confidence="maxprob", merge="confidence", **k)
    base, out = run(), run(suggest=2)
    assert set(out) - set(base) == {"novelty", "suggested"}
    for k in ("pred", "forward", "conf", "forward_conf"):
        assert torch.equal(out[k].view(I32) if out[k].dtype == F32 else out[k], base[k].view(I32) if base[k].dtype == F32 else base[k]), k
    s = out["novelty"]
    assert tuple(s.shape) == (2, T) and s.dtype == F32 and s.device.type == "cpu" and (s[:, 0] == 0).all() and (s[:, 1:] > 0).all()
    assert len(out["suggested"]) == 2
    for t, picks in enumerate(out["suggested"]):
        assert [(p["frame"], p["z"], p["score"]) for p in picks] == hip.suggest_frames(s[t, 1:], 6, 2) and len(picks) == 2
        for p in picks:
            assert p["radargram"] == t and p["item"] == t * T and p["column"] == t * rg_len + p["frame"] * step == p["columns"][0]
    # `propagate(novelty=True)`: the entry behind conf, before L; labels untouched; the definition on the pass's own features
    ds = fresh()
    seq = ds[0].cuda()
    lp = LabelPropVOS_CRW(dict(cfg))
    plain = utils.propagate(seq, seg[:, :PATCH[1]].cuda(), enc, lp, M_E2E, False, False, confidence="maxprob", soft=True)
    res = utils.propagate(seq, seg[:, :PATCH[1]].cuda(), enc, lp, M_E2E, False, False, confidence="maxprob", soft=True, novelty=True)
    assert len(res) == len(plain) + 1 and torch.equal(res[0], plain[0]) and eq_bits(res[3], plain[3]) and eq_bits(res[5], plain[4])
    nov, score = res[4]
    assert tuple(nov.shape) == (N, T) and tuple(score.shape) == (T,) and not nov[:, 0].any() and score[0] == 0
    assert torch.equal(score[1:].cpu(), s[0, 1:])
    feats, _ = utils._features_and_seed(seq, seg[:, :PATCH[1]].cuda(), enc, False, False)
    assert not any(nr.violations(feats, 6, 6, None, None, 1, nov[:, 1:].t().contiguous(), score[1:]).values())
    # anchors: a fully labelled trace at the first pick of radargram 0 -- not proposed again; under 'restart' other scores behind it
    col = out["suggested"][0][0]["column"]
    for ctx in ("clamp", "restart"):
        o2 = run(suggest=2, anchors=(seg, [col]), anchor_context=ctx)
        f0 = out["suggested"][0][0]["frame"]
        assert all(abs(p["frame"] - f0) > 2 for p in o2["suggested"][0]) and o2["suggested"][1] == out["suggested"][1]
        assert torch.equal(o2["novelty"][1], s[1]) and torch.equal(o2["novelty"][0, :f0 + 1], s[0, :f0 + 1])
        assert torch.equal(o2["novelty"][0], s[0]) == (ctx == "clamp" or f0 == T - 1)
    # the script, in a child process
    report = tmp_path / "r.json"
    cmd = [sys.executable, os.path.join(ROOT, "radar-sounder-crw_amd", "scripts", "segment_all.py"), "--synthetic", "96", "320", "--seq_length", "10",
           "--patch_size", str(PATCH[0]), str(PATCH[1]), "--overlap", str(OVERLAP[0]), str(OVERLAP[1]), "--dataset", "0", "-c", "6", "-r", "6",
           "-k", "8", "--suggest_anchors", "2", "--report_json", str(report), "--output_folder", str(tmp_path)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "Suggested anchor traces" in done.stdout
    d = json.loads(report.read_text())["suggested_anchors"]
    assert d["per_radargram"] == 2 and d["min_gap"] == 2 and len(d["picks"]) == 2 * (d["picks"][-1]["radargram"] + 1)
    assert set(d["picks"][0]) == {"radargram", "item", "frame", "column", "columns", "z", "score"}
