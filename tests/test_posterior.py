"""The posterior of the ordered label maps on the host: the reference (posterior_ref.py) proved by enumeration of every monotone
path, the CPU route of `crw_hip.labelmap_ordered_posterior` / `labelmap_ordered_joint_posterior` against it within the derived bound
rho, planted defects that the check must report, the quality figures on the synthetic layered items, and the host surface: argument
errors, the `posterior` entry-point group, the header, the status codes, `segment(..., posterior=True)`, `horizon_bars` and the
command line.  The kernel's twins are in test_posterior_gpu.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dense_ref as dr
import joint_ref as jr
import ordered_ref as od
import posterior_ref as pr
from conftest import ROOT
from test_confidence import Flatten, synthetic_case
from test_dense import oracle_propagate_soft
from test_sweep_dense import forced

CASE_IDS = [jr.case_id(c) for c in jr.CASES]
SHAPE_IDS = ["x".join(map(str, s)) for s in dr.SHAPES]


def orders(M):
    """The two orders a shape is run under: the identity over every class, and the classes backwards without the last one (no
    identity, S < M where M > 2)."""
    return tuple(range(M)), tuple(reversed(range(M)))[:max(2, M - 1)]


# ---- 1. the reference is the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,S", [(1, 2), (1, 3), (2, 2), (2, 3), (3, 3), (4, 2), (5, 2), (5, 3)])
def test_reference_against_the_enumeration_of_every_monotone_path(rows, S):
    g = np.random.default_rng(100 * rows + S)
    M, cols = S + 1, 4
    probs = g.dirichlet(np.ones(M), size=(rows, cols)).transpose(2, 0, 1)
    probs[0, 0, 0] = 0.0  # under the floor
    order = tuple(int(k) for k in g.permutation(M)[:S])
    labels = g.integers(0, M, size=(rows, cols))  # any labels: a class outside the order, columns that step back
    floor = 0.05
    post, hz = pr.posterior(probs, order, labels, floor)
    f, pick = pr.evidence(probs, order, floor), pr.picks(labels, order)
    pos = pr.positions(labels, order)
    worst = 0.0
    for c in range(cols):
        gamma, m1, m2 = pr.enumerate_paths(f[:, :, c], pick[:, c])
        want = np.array([gamma[r, pos[r, c]] if pos[r, c] >= 0 else 0.0 for r in range(rows)])
        worst = max(worst, np.abs(want - post[:, c]).max(), np.abs(m1 - hz[1, :, c]).max(), np.abs(m2 - hz[2, :, c] ** 2).max())
        assert np.array_equal(hz[0, :, c], pick[:, c])
    print(f"rows {rows}, S {S}: worst difference from the enumeration {worst:.3e}")
    assert worst <= 1e-12


# ---- 2. the CPU route against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.SHAPES, ids=SHAPE_IDS)
def test_cpu_route_against_the_reference(shape):
    """Both orders, both flips, both label dtypes, and a window inside a wider map (ld > cols, an odd offset)."""
    import crw_hip
    T, N, M, rows, cols = shape
    L, ref = dr.reference(shape)
    for order in orders(M):
        for flip in (False, True):
            probs = ref.probs[:, :, ::-1] if flip else ref.probs
            lab8, _ = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)
            post, hz = crw_hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, lab8, flip=flip)
            assert post.shape == (rows, cols) and hz.shape == (3, len(order) - 1, cols) and post.dtype == hz.dtype == torch.float32
            pr.check(probs, order, lab8.numpy(), post.numpy(), hz.numpy(), what=f"cpu {shape} {order} flip={flip}")
            wide_lab = torch.full((rows, cols + 7), -7.0)
            wide_lab[:, 3:3 + cols] = lab8.float()
            wide, wide_hz = torch.full((rows, cols + 7), -7.0), torch.full((3, len(order) - 1, cols + 9), -7.0)
            out, out_hz = crw_hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, wide_lab[:, 3:3 + cols], flip=flip,
                                                             out=wide[:, 3:3 + cols], out_hz=wide_hz[:, :, 5:5 + cols])
            assert out.data_ptr() == wide[:, 3:].data_ptr() and torch.equal(out, post) and torch.equal(out_hz, hz)  # fp32 labels, a window
            assert (wide[:, :3] == -7).all() and (wide[:, 3 + cols:] == -7).all()
            assert (wide_hz[:, :, :5] == -7).all() and (wide_hz[:, :, 5 + cols:] == -7).all()


@pytest.mark.parametrize("index", range(len(jr.CASES)), ids=CASE_IDS)
def test_cpu_joint_route_against_the_reference(index):
    """Teacher-forced on the route's own `took`; the same source twice is the single call."""
    import crw_hip
    c = jr.case(index)
    N, M, rows, ncols, order = c.shared
    kind = dr.KINDS[index % 3]
    lab, _ = crw_hip.labelmap_ordered_joint(c.source(0), c.source(1), *c.shared, confidence=kind, dtype=torch.int8)
    post, hz = crw_hip.labelmap_ordered_joint_posterior(c.source(0), c.source(1), *c.shared, lab, confidence=kind)
    ca, cb = (jr.dense_confidence(crw_hip, c.source(k), N, M, rows, ncols, kind) for k in (0, 1))
    probs = jr.selected((cb > ca).numpy(), *c.probs)
    pr.check(probs, order, lab.numpy(), post.numpy(), hz.numpy(), what=f"cpu joint {CASE_IDS[index]} {kind}")
    for k in (0, 1):
        L, T, cols, col0, flip = src = c.source(k)
        lab1 = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)[0]
        one, one_hz = crw_hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, lab1, flip=flip)
        win = lab1[:, col0:col0 + ncols]
        two, two_hz = crw_hip.labelmap_ordered_joint_posterior(src, src, *c.shared, win, confidence=kind)
        # (torch's CPU kernels vectorise a 1-column and a 5-column tensor differently: the two agree as two routes do, within 2 rho;
        # the kernel's two entry points agree bit for bit, test_posterior_gpu.py)
        pr.check(c.probs[k], order, win.numpy(), two.numpy(), two_hz.numpy(), slack=2.0, what=f"cpu joint {CASE_IDS[index]} source {k} twice",
                 against=(one[:, col0:col0 + ncols].numpy(), one_hz[:, :, col0:col0 + ncols].numpy()))


def test_labels_outside_the_order_and_the_range_of_post():
    import crw_hip
    shape = dr.SHAPES[3]
    T, N, M, rows, cols = shape
    L, ref = dr.reference(shape)
    order = (4, 0, 2)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(-2, M + 1, (rows, cols), generator=g).to(torch.int8)  # any labels, -2 ... M
    post, hz = crw_hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, labels)
    outside = ~torch.isin(labels, torch.tensor(order, dtype=torch.int8))
    assert outside.any() and (post[outside] == 0).all() and (post[~outside] > 0).all() and post.max() <= 1
    pr.check(ref.probs, order, labels.numpy(), post.numpy(), hz.numpy(), what="cpu, any labels")


# ---- 3. planted defects ----------------------------------------------------------------------------------------------------------------
DEFECTS = ("prefix_without_s", "beta_one_row_off", "no_floor", "no_final_normalisation", "labels_flipped_alone", "bar_about_the_mean")


def forward_backward(probs, order, labels, floor, defect=None):
    """The kernel's route in fp64 numpy (normalised messages, the boundary's distribution from the transitions), with one of DEFECTS
    planted.  Without a defect it passes `posterior_ref.check`."""
    e = np.stack([probs[int(k)] for k in order], 1)
    f = e if defect == "no_floor" else np.maximum(e, floor)
    rows, S, cols = f.shape
    A = np.empty_like(f)
    prev = np.zeros((S, cols))
    prev[0] = 1
    for r in range(rows):
        before = np.cumsum(prev, 0)
        if defect == "prefix_without_s" and r > 0:
            before = before - prev
        a = f[r] * before
        prev = A[r] = a / np.maximum(a.sum(0), 1e-300)
    if defect == "labels_flipped_alone":
        labels = labels[:, ::-1]
    pos, pick = pr.positions(labels, order), pr.picks(labels, order).astype(np.float64)
    b = np.ones((S, cols))
    bs = [None] * rows
    for r in range(rows - 1, -1, -1):
        bs[r] = b
        b = np.cumsum((f[r] * b / b[0])[::-1], 0)[::-1]
    if defect == "beta_one_row_off":
        bs = bs[1:] + [np.ones((S, cols))]
    post, m1, m2 = np.empty((rows, cols)), np.zeros((S - 1, cols)), np.zeros((S - 1, cols))
    for r in range(rows - 1, -1, -1):
        g = A[r] * bs[r]
        Z = g.sum(0)
        inv = 1.0 if defect == "no_final_normalisation" else 1 / Z
        g = g * inv
        post[r] = np.where(pos[r] >= 0, np.take_along_axis(g, np.maximum(pos[r], 0)[None], 0)[0], 0.0)
        p = np.cumsum(A[r], 0)[:-1] * bs[r][1:] / Z
        m1 += (r + 1) * p
        m2 += (r + 1 - pick) ** 2 * p
    m2 += pick ** 2 * np.cumsum(g[::-1], 0)[::-1][1:]
    if defect == "bar_about_the_mean":
        m2 = m2 - (pick - m1) ** 2  # E[(B - E B)^2]
    return np.clip(post, 0, 1), np.stack([pick, m1, np.sqrt(np.maximum(m2, 0))])


def test_the_check_reports_every_planted_defect():
    """One-hot nodes (every interpolated value is 0 or a product of two weights, at least 1 / 74 * 1 / 58: rho stays small while
    exact zeros meet the floor), the reverse pass's geometry (flip), labels from the CPU route's decode."""
    import crw_hip
    T, N, M, rows, cols = 6, 7, 3, 37, 29
    g = np.random.default_rng(5)
    classes = np.sort(g.integers(0, M, size=(T, N)), axis=1)
    wrong = g.random((T, N)) < 0.15  # nodes that contradict the order: there the path has to cross an exact zero, and the floor counts
    classes[wrong] = g.integers(0, M, size=int(wrong.sum()))
    L = torch.nn.functional.one_hot(torch.tensor(classes.reshape(-1)), M).float()
    order = (0, 1, 2)
    probs = np.ascontiguousarray(dr.probabilities(L.numpy(), T, N, M, rows, cols)[:, :, ::-1])
    assert (probs < pr.FLOOR).any()
    labels = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, flip=True, dtype=torch.int8)[0].numpy()
    assert not np.array_equal(labels, labels[:, ::-1])
    pr.check(probs, order, labels, *forward_backward(probs, order, labels, pr.FLOOR), what="no defect")
    pr.check(probs, order, labels, *(t.numpy() for t in crw_hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, torch.tensor(labels),
                                                                                          flip=True)), what="the CPU route")
    for defect in DEFECTS:
        with np.errstate(all="ignore"):  # (without the floor a column's weights can all be zero)
            got = forward_backward(probs, order, labels, pr.FLOOR, defect)
        with pytest.raises(AssertionError):
            pr.check(probs, order, labels, *got, what=defect)


# ---- 4. quality ----------------------------------------------------------------------------------------------------------------------
def single_quality(hip, index, device="cpu"):
    q, seed = jr.PAIRS[index]
    T, N, rows, cols, temp, M, share = q
    gt, L = od.layered_case(*q, seed)
    L, order = torch.tensor(L).to(device), tuple(range(M))
    lab, conf = hip.labelmap_ordered(L, T, N, M, rows, cols, order, confidence="maxprob", dtype=torch.int8)
    post, hz = hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, lab)
    return pr.quality(gt, lab.cpu().numpy(), conf.cpu().numpy(), post.cpu().numpy(), hz.cpu().numpy(), order, what=f"single {q} seed {seed} on {device}")


def joint_quality(hip, index, device="cpu"):
    gt, Lf, Lr, (T, N, rows, cols, M) = jr.paired_case(index)
    a, b, order = (Lf.to(device), T, cols, 0, False), (Lr.to(device), T, cols, 0, True), tuple(range(M))
    lab, conf = hip.labelmap_ordered_joint(a, b, N, M, rows, cols, order, confidence="maxprob", dtype=torch.int8)
    post, hz = hip.labelmap_ordered_joint_posterior(a, b, N, M, rows, cols, order, lab, confidence="maxprob")
    return pr.quality(gt, lab.cpu().numpy(), conf.cpu().numpy(), post.cpu().numpy(), hz.cpu().numpy(), order, what=f"joint {jr.PAIRS[index]} on {device}")


@pytest.mark.parametrize("index", range(len(jr.PAIRS)), ids=[f"q{i // 3}seed{i % 3}" for i in range(len(jr.PAIRS))])
def test_quality_on_the_layered_items(index):
    """ECE of post <= 0.5 x ECE of maxprob, mean bar coverage >= 0.85 (README "Evaluation" quotes the printout); the AURC is
    printed and not asserted: the posterior is the better calibrated, not the better ranker."""
    import crw_hip
    single_quality(crw_hip, index)
    joint_quality(crw_hip, index)


# ---- 5. the host surface -------------------------------------------------------------------------------------------------------------
def test_argument_errors_in_python():
    import crw_hip
    shape = dr.SHAPES[2]
    T, N, M, rows, cols = shape
    L, _ = dr.reference(shape)
    order = (0, 1, 2)
    lab = crw_hip.labelmap_ordered(L, T, N, M, rows, cols, order, dtype=torch.int8)[0]
    run = lambda labels=lab, order=order, **kw: crw_hip.labelmap_ordered_posterior(L, T, N, M, rows, cols, order, labels, **kw)
    for floor in (0.0, 2.0 ** -21, 0.26, float("nan"), -1e-4):
        with pytest.raises(ValueError, match="floor must lie in"):
            run(floor=floor)
    run(floor=2.0 ** -20), run(floor=0.25)
    with pytest.raises(ValueError, match="order"):
        run(order=(0, 0))
    with pytest.raises(ValueError, match="labels must be torch.float32 or torch.int8"):
        run(labels=lab.long())
    with pytest.raises(ValueError, match="labels must be"):
        run(labels=lab[:, :-1])
    with pytest.raises(ValueError, match="share one pitch"):
        run(out=torch.zeros(rows, cols + 1)[:, :cols])
    with pytest.raises(ValueError, match="out_hz must be"):
        run(out_hz=torch.zeros(3, 2, cols + 1))
    with pytest.raises(ValueError, match="out_hz must be"):
        run(out_hz=torch.zeros(3, 2, 2 * cols)[:, :, ::2])
    c = jr.case(2)
    labj = crw_hip.labelmap_ordered_joint(c.source(0), c.source(1), *c.shared, confidence="maxprob")[0]
    with pytest.raises(TypeError):
        crw_hip.labelmap_ordered_joint_posterior(c.source(0), c.source(1), *c.shared, labj)  # the kind is mandatory
    with pytest.raises(ValueError, match="needs the confidence kind"):
        crw_hip.labelmap_ordered_joint_posterior(c.source(0), c.source(1), *c.shared, labj, confidence=None)
    sig = inspect.signature(crw_hip.labelmap_ordered_posterior).parameters
    assert list(sig)[:8] == ["L", "T", "N", "M", "rows", "cols", "order", "labels"]
    assert [k for k, v in sig.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["flip", "floor", "out", "out_hz", "workspace"]
    assert sig["floor"].default == 1e-4
    sig = inspect.signature(crw_hip.labelmap_ordered_joint_posterior).parameters
    assert list(sig)[:8] == ["a", "b", "N", "M", "rows", "ncols", "order", "labels"] and sig["floor"].default == 1e-4


def test_the_posterior_group_is_told_and_named_when_the_library_lacks_it(monkeypatch):
    import crw_hip
    group = "posterior"
    names = crw_hip.POSTERIOR_ENTRY_POINTS
    assert names == ("crw_labelmap_posterior_workspace", "crw_labelmap_ordered_posterior", "crw_labelmap_ordered_joint_posterior")
    assert set(names) <= set(crw_hip.SIGNATURES) and crw_hip.OPTIONAL_ENTRY_POINTS[group] is names
    assert crw_hip.has_posterior() is True and crw_hip._posterior_lib() is crw_hip.lib()
    monkeypatch.setitem(crw_hip._present, group, False)
    assert crw_hip.has_posterior() is False
    with pytest.raises(RuntimeError, match="stale libcrw_hip.so.*rebuild") as err:
        crw_hip._posterior_lib()
    assert all(name in str(err.value) for name in names)
    shape = dr.SHAPES[1]  # the CPU route needs no library
    L, _ = dr.reference(shape)
    crw_hip.labelmap_ordered_posterior(L, *shape, (0, 1), torch.zeros(4, 4))


def test_header_binding_and_status_codes_at_abi_8():
    """Every refusal comes before a launch (no device needed); 16 is a pointer that is never followed."""
    import crw_hip
    header = open(os.path.join(ROOT, "include", "crw_hip.h")).read()
    assert re.search(r"^#define\s+CRW_ABI_VERSION\s+8\s*$", header, re.M)
    assert re.search(r"^size_t\s+crw_labelmap_posterior_workspace\(int rows, int cols, int S\);", header, re.M)
    assert re.search(r"^int\s+crw_labelmap_ordered_posterior\(const float \*L, int T, int N, int M, int rows, int cols, int flip, const int "
                     r"\*order_host, int S,\s+float floor, const void \*labels, int label_dtype, size_t ld, float \*post, float \*hz, size_t "
                     r"hz_ld,\s+void \*ws, size_t ws_bytes, crw_stream_t stream\);", header, re.M)
    assert re.search(r"^int\s+crw_labelmap_ordered_joint_posterior\(const float \*La, .*?int S, int conf_kind, float floor, const void \*labels",
                     header, re.M | re.S)
    assert "crw_labelmap_ordered_posterior, crw_labelmap_ordered_joint_posterior (crw_hip.has_posterior())" in header
    assert len(crw_hip.SIGNATURES["crw_labelmap_ordered_posterior"][1]) == 19
    assert len(crw_hip.SIGNATURES["crw_labelmap_ordered_joint_posterior"][1]) == 27
    lib = crw_hip.lib()
    assert lib.crw_abi_version() == crw_hip.ABI_VERSION == 8 and crw_hip.has_posterior()
    assert lib.crw_labelmap_posterior_workspace(8, 8, 4) == 4 * 8 * 4 * 64 and lib.crw_labelmap_posterior_workspace(410, 8192, 4) == 4 * 410 * 8192 * 4
    assert lib.crw_labelmap_posterior_workspace(0, 8, 4) == lib.crw_labelmap_posterior_workspace(8, 0, 4) == 0
    assert lib.crw_labelmap_posterior_workspace(8, 8, 1) == lib.crw_labelmap_posterior_workspace(8, 8, 17) == 0
    need = lib.crw_labelmap_posterior_workspace(8, 8, 4)
    ok = dict(La=16, Ta=4, ca=8, oa=0, fa=0, Lb=16, Tb=3, cb=20, ob=12, fb=1, N=4, M=4, rows=8, ncols=8, order=(0, 1, 2, 3), kind=0,
              floor=1e-4, labels=16, dt=0, ld=8, post=16, hz=16, hz_ld=8, ws=16, wsb=need)

    def call(single=True, joint=True, **bad):
        a = dict(ok, **bad)
        order = None if a["order"] is None else (ctypes.c_int * len(a["order"]))(*a["order"])
        S = a.get("S", 0 if a["order"] is None else len(a["order"]))
        tail = (a["floor"], a["labels"], a["dt"], a["ld"], a["post"], a["hz"], a["hz_ld"], a["ws"], a["wsb"], None)
        codes = set()
        if joint:
            codes.add(lib.crw_labelmap_ordered_joint_posterior(a["La"], a["Ta"], a["ca"], a["oa"], a["fa"], a["Lb"], a["Tb"], a["cb"], a["ob"],
                                                               a["fb"], a["N"], a["M"], a["rows"], a["ncols"], order, S, a["kind"], *tail))
        if single:
            codes.add(lib.crw_labelmap_ordered_posterior(a["La"], a["Ta"], a["N"], a["M"], a["rows"], a["ncols"], a["fa"], order, S, *tail))
        assert len(codes) == 1, (bad, codes)
        return codes.pop()

    # the posterior's own
    for bad in (dict(floor=0.0), dict(floor=2.0 ** -21), dict(floor=0.2500001), dict(floor=float("nan")), dict(floor=-1.0),
                dict(post=None, hz=None), dict(post=18), dict(hz=18), dict(hz_ld=7), dict(ws=None), dict(ws=18),
                # the order's
                dict(order=(0, 1, 1)), dict(order=(0, 4)), dict(order=(-1, 0)), dict(order=(2,)), dict(order=(0, 1, 2, 3, 0)),
                dict(order=(0, 1, 2), M=2), dict(order=None), dict(order=(0, 1), S=1),
                # the window's
                dict(La=None), dict(La=18), dict(Ta=0), dict(labels=None), dict(N=0), dict(M=1), dict(M=17), dict(rows=0), dict(ncols=0),
                dict(rows=(1 << 22) + 1), dict(dt=2), dict(ld=7), dict(labels=18)):
        assert call(**bad) == crw_hip.CRW_EINVAL, bad
    for bad in (dict(Lb=None), dict(Lb=18), dict(Tb=0), dict(cb=0), dict(cb=(1 << 22) + 1), dict(oa=-1), dict(ob=-1), dict(oa=1), dict(ob=13),
                dict(ca=0), dict(kind=-1), dict(kind=3), dict(kind=-2)):  # the joint call's sources and kind
        assert call(single=False, **bad) == crw_hip.CRW_EINVAL, bad
    assert call(joint=False, ncols=(1 << 22) + 1, ld=(1 << 22) + 1, hz_ld=(1 << 22) + 1) == crw_hip.CRW_EINVAL
    assert call(wsb=need - 1) == crw_hip.CRW_EWORKSPACE and call(wsb=0) == crw_hip.CRW_EWORKSPACE
    assert call(wsb=need - 1, post=None) == call(wsb=need - 1, hz=None) == crw_hip.CRW_EWORKSPACE  # either output may be null
    assert call(dt=1, labels=17, wsb=0) == crw_hip.CRW_EWORKSPACE  # int8 labels need no alignment


# ---- 6. segment / horizon_bars / the command line ----------------------------------------------------------------------------------------
def test_segment_option_errors():
    import inference as crw_inference
    ds, seg, lp, M, T = synthetic_case(n_rg=1)
    order = (0, 1, 2, 3, 4)
    run = lambda **kw: crw_inference.segment(ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0), device="cpu", posterior=True, **kw)
    with pytest.raises(ValueError, match="posterior=True needs decode='ordered'"):
        run()
    with pytest.raises(ValueError, match="posterior=True needs decode='ordered'"):
        run(upsample="bilinear", confidence="maxprob")
    for merge in ("rule", "confidence"):
        with pytest.raises(ValueError, match="posterior=True with use_last needs merge='ordered'"):
            run(upsample="bilinear", decode="ordered", order=order, confidence="maxprob", merge=merge, use_last=True)
    with pytest.raises(ValueError, match="floor must lie in"):
        run(upsample="bilinear", decode="ordered", order=order, floor=0.5)
    assert "posterior" not in inspect.signature(crw_inference.segment_sweep).parameters  # the sweep does not take the option


@pytest.mark.parametrize("use_last", [False, True], ids=["forward", "use_last"])
def test_segment_posterior_on_the_oracle(monkeypatch, use_last):
    """With a correction that succeeds on radargram 0: every earlier key bit for bit, every window of post / horizon the direct
    call on that window's sources."""
    import crw_hip
    import inference as crw_inference
    M, T = 5, 8
    rg_len = T * 8
    changes = [5, None]
    order = (0, 1, 2, 3, 4)
    kind = "maxprob"

    def segment(**kw):
        ds, seg, lp, _, _ = synthetic_case(n_rg=2)
        monkeypatch.setattr(crw_inference, "propagate", forced(oracle_propagate_soft, changes, T))
        return crw_inference.segment(ds, seg, Flatten(), lp, M, T, (8, 8), (4, 0), correction=True, use_last=use_last, dataset_id=2,
                                     device="cpu", confidence=kind, upsample="bilinear", decode="ordered", order=order,
                                     merge="ordered" if use_last else "rule", **kw)

    plain, out = segment(), segment(posterior=True, floor=1e-3)
    assert set(out) == set(plain) | {"post", "horizon", "floor"} and out["floor"] == 1e-3
    for k in plain:
        assert torch.equal(out[k], plain[k]) if torch.is_tensor(plain[k]) else True, k
    assert out["change_idx"] == plain["change_idx"] == changes
    rows, width = out["pred"].shape
    assert out["post"].shape == (rows, width) and out["horizon"].shape == (3, M - 1, width)
    assert out["post"].min() >= 0 and out["post"].max() <= 1 and torch.isfinite(out["horizon"]).all()
    # by hand
    ds, seg, lp, _, _ = synthetic_case(n_rg=2)
    N = ds[0].shape[1]
    run = lambda seq, ref, last: oracle_propagate_soft(seq, ref, Flatten(), lp, M, False, last, soft=True)[-1]
    fwd = [run(ds[t * T], seg[:N * 4 + 4, rg_len * t:rg_len * t + 8], False) for t in range(2)]
    px = (T - 5) * 8
    tail = run(ds.get_smaller_item(0, T - 5), seg[:, rg_len - px:rg_len - px + 8], False)
    for t in range(2):
        a, b = rg_len * t, rg_len * (t + 1)
        cut = px if t == 0 else 0
        windows = []  # (first column, last, the direct call)
        if use_last:
            seq = ds[t * T]
            rev = (run(seq, torch.flip(seg[:, a:b], (-1,))[:, :8], True), seq.shape[0], rg_len)
            joint = lambda x, y, lo, hi: crw_hip.labelmap_ordered_joint_posterior(x, y, N, M, rows, hi - lo, order, out["pred"][:, lo:hi],
                                                                                   confidence=kind, floor=1e-3)
            windows.append((a, b - cut, joint((fwd[t], T, rg_len, 0, False), (*rev, 0, True), a, b - cut)))
            if cut:
                windows.append((b - cut, b, joint((tail, T - 5, px, 0, False), (*rev, rg_len - px, True), b - cut, b)))
        else:
            whole = crw_hip.labelmap_ordered_posterior(fwd[t], T, N, M, rows, rg_len, order, crw_hip.labelmap_ordered(
                fwd[t], T, N, M, rows, rg_len, order)[0], floor=1e-3)
            windows.append((a, b - cut, tuple(m[..., :rg_len - cut] for m in whole)))
            if cut:
                windows.append((b - cut, b, crw_hip.labelmap_ordered_posterior(tail, T - 5, N, M, rows, px, order, out["pred"][:, b - cut:b],
                                                                              floor=1e-3)))
        for lo, hi, (post, hz) in windows:
            assert torch.equal(out["post"][:, lo:hi], post), (t, lo, hi)
            assert torch.equal(out["horizon"][:, :, lo:hi], hz), (t, lo, hi)
    bars = crw_inference.horizon_bars(out["horizon"], seg, order)
    print(bars)
    assert bars.n.shape == (M - 1,) and (bars.n == width).all()


def test_horizon_bars_against_a_count_by_hand():
    import inference as crw_inference
    from metrics import HorizonBars
    order = (2, 0, 1)
    seg = torch.tensor([[2, 2, 2, 3], [0, 2, 2, 0], [0, 1, 2, 1], [1, 1, 2, 1]]).float()  # boundaries: (1, 2, 4, 1), (3, 2, 4, 2)
    horizon = torch.tensor([[[1.0, 0, 4, 3], [3, 4, 1, 2]], [[1.2, 0.5, 3.9, 2.0], [3, 3, 3, 3]], [[0.0, 0.4, 1, 0.5], [0, 0.5, 0, 0.1]]])
    bars = crw_inference.horizon_bars(horizon, seg, order, z=2.0, slack=1.0)
    assert isinstance(bars, HorizonBars)
    # boundary 1 is present in columns 0, 1, 3: |ref - pick| = 0, 2, 2 against 1, 1.8, 2; boundary 2 in the same: 0, 2, 0 against 1, 2, 1.2
    assert bars.n.tolist() == [3, 3] and bars.n_inside.tolist() == [2, 3]
    np.testing.assert_allclose(bars.mae, [4 / 3, 2 / 3])
    np.testing.assert_allclose(bars.mean_bar, [0.3, 0.2], rtol=1e-6)
    np.testing.assert_allclose(bars.coverage, [2 / 3, 1.0])
    d = bars.to_dict()
    assert d["n"] == [3, 3] and d["z"] == 2.0 and abs(d["mean_coverage"] - 5 / 6) < 1e-12 and d["rows"] == 4
    lines = str(bars).splitlines()
    assert len({len(line) for line in lines[1:] if line}) == 1 and "inside" in lines[1]  # a fixed-width table
    none = crw_inference.horizon_bars(horizon, torch.full((4, 4), 2.0), order)
    assert none.n.tolist() == [0, 0] and np.isnan(none.coverage).all() and np.isnan(none.mean_coverage) and "-" in str(none)
    with pytest.raises(ValueError, match="horizon must be"):
        crw_inference.horizon_bars(horizon[:, :1], seg, order)


def test_cli_posterior_flags_and_run(monkeypatch, capsys, tmp_path):
    """Without the flags: the recorded stdout, files and keys.  With them: the two tables after the others, the two files, the
    `posterior` key."""
    import json
    import inference as crw_inference
    import test_confidence as tc
    from test_sweep_dense_gpu import _cli
    text, files, d = tc.run_cli(monkeypatch, capsys, tmp_path / "plain", [])
    assert text == open(os.path.join(ROOT, "tests", "golden", "segment_all_stdout.txt")).read()
    assert files == ["predicted_map.pt"] and "posterior" not in d
    cli = _cli("segment_all")
    p = cli.get_args_parser()
    base = ["--synthetic", "40", "128"]
    ordered = ["--upsample", "bilinear", "--decode", "ordered", "--order", "0", "1", "2", "3", "4"]
    check = lambda extra: cli.check_posterior_flags(cli.check_confidence_flags(cli.with_defaults(p.parse_args(base + extra))))
    a = check(ordered + ["--posterior"])
    assert a.posterior and a.floor == 1e-4 and not a.save_posterior
    assert check([]).floor is None
    for bad, msg in ((["--posterior"], "--posterior needs --decode ordered"), (["--floor", "1e-3"], "need --posterior"),
                     (["--save_posterior"], "need --posterior"), (ordered + ["--posterior", "--floor", "0.5"], "--floor 0.5"),
                     (ordered + ["--posterior", "--use_last", "true"], "needs --merge ordered"),
                     (ordered + ["--posterior", "--use_last", "true", "--confidence", "margin", "--merge", "confidence"], "needs --merge ordered")):
        with pytest.raises(SystemExit, match=msg):
            check(bad)
    monkeypatch.setattr(crw_inference, "propagate", oracle_propagate_soft)
    monkeypatch.setattr(cli, "create_model", lambda id, pos_embed: Flatten())
    js = tmp_path / "r.json"
    args = base + ["--dataset", "3", "--patch_size", "8", "8", "--overlap", "4", "0", "--seq_length", "8", "-c", "4", "-r", "4", "-k", "5",
                   "--model", "0", "--output_folder", str(tmp_path / "out"), "--report_json", str(js), "--use_last", "true", "--confidence",
                   "maxprob", "--merge", "ordered", "--posterior", "--floor", "1e-3", "--save_posterior"] + ordered
    cli.main(p.parse_args(args))
    text = capsys.readouterr().out
    assert text.index("Calibration (maxprob, merge: ordered)") < text.index("Calibration (posterior of the ordered decode, floor 0.001)") \
        < text.index("Horizon error bars") < text.index("Time elapsed (inference + metrics)")
    assert sorted(os.listdir(tmp_path / "out")) == ["horizon_bars.pt", "posterior_map.pt", "predicted_map.pt"]
    post, bars = torch.load(tmp_path / "out" / "posterior_map.pt"), torch.load(tmp_path / "out" / "horizon_bars.pt")
    d = json.load(open(js))
    assert post.dtype == torch.float32 and list(post.shape) == d["map_shape"] and bars.shape == (3, 4, post.shape[1])
    assert d["posterior"]["floor"] == 1e-3 and d["posterior"]["calibration"]["total"] == d["calibration"]["total"]
    assert len(d["posterior"]["horizon_bars"]["coverage"]) == 4
