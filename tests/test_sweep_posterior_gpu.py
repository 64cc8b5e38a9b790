"""GPU side of the sweep's posterior: crw_labelmap_ordered_posterior_batch / crw_labelmap_ordered_joint_posterior_batch (the kernel of
csrc/labelmap_dense.hip with the configuration as a grid dimension) against the one-map entry points on the same slice, bit for
bit -- one kernel text serves both, so a difference is a bug, not rounding; test_posterior_gpu.py holds the one-map calls to the
fp64 definition.  Shapes of dense_ref.py and geometry cases of joint_ref.py, the 1-column window at M = 16 with int8 labels and a
confidence kind, column windows inside wider maps, what the workspace held before, G = 1, the binding's split of G configurations
over several launches, every refusal before a launch, and `segment_sweep(..., posterior=True)` against `segment` per configuration.
Every call here is an ordinary valid call or a refusal before a launch: nothing provokes a fault."""
import ctypes

import pytest
import torch

import dense_ref as dr
import joint_ref as jr
from conftest import load_golden
from test_posterior import CASE_IDS, orders

pytestmark = pytest.mark.gpu

G3 = 3
BATCH_SHAPES = [dr.SHAPES[0], dr.SHAPES[2], dr.SHAPES[5]]  # (1,1,2,3,5), (5,7,3,37,29), (4,3,16,9,130): MCAP 16, three waves, the last partial
assert BATCH_SHAPES == [(1, 1, 2, 3, 5), (5, 7, 3, 37, 29), (4, 3, 16, 9, 130)]

bits = lambda t: t.contiguous().view(torch.int32)
same = lambda a, b: torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_posterior() and crw_hip.has_posterior_batch()
    return crw_hip


def stacked(G, T, N, M, seed):
    """L [G, T*N, M] on the device: every configuration its own Dirichlet rows."""
    return torch.stack([dr.dirichlet_rows(T, N, M, seed=seed + 7 * g) for g in range(G)]).cuda()


# ---- 1. the single batch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BATCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_equals_the_single_call_per_configuration(hip, shape):
    T, N, M, rows, cols = shape
    G = G3
    L = stacked(G, T, N, M, seed=60)
    for order in orders(M):
        S = len(order)
        for flip in (False, True):
            lab8 = hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)[0]
            for labels in (lab8, lab8.float()):
                post, hz = hip.labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, labels, flip=flip)
                assert post.is_cuda and post.shape == (G, rows, cols) and hz.shape == (G, 3, S - 1, cols) and post.dtype == hz.dtype == torch.float32
                for g in range(G):
                    one, one_hz = hip.labelmap_ordered_posterior(L[g], T, N, M, rows, cols, order, labels[g], flip=flip)
                    assert same(post[g], one) and same(hz[g], one_hz), (shape, order, flip, labels.dtype, g)
                # post only, hz only (the C entry point: either output may be null)
                only_post, only_hz = raw_single_batch(hip, L, G, shape, order, flip, labels, want_post=True, want_hz=False), \
                    raw_single_batch(hip, L, G, shape, order, flip, labels, want_post=False, want_hz=True)
                assert same(only_post[0], post) and (only_post[1] == -7).all()
                assert same(only_hz[1], hz) and (only_hz[0] == -7).all()
    if rows * cols > 50:
        assert len({p.cpu().numpy().tobytes() for p in post}) == G  # the slices are not all equal


def raw_single_batch(hip, L, G, shape, order, flip, labels, want_post, want_hz):
    """crw_labelmap_ordered_posterior_batch itself over sentinel-filled outputs -> (post, hz); an output not asked for is passed as null."""
    T, N, M, rows, cols = shape
    S = len(order)
    lib = hip.lib()
    post, hz = torch.full((G, rows, cols), -7.0, device="cuda"), torch.full((G, 3, S - 1, cols), -7.0, device="cuda")
    need = lib.crw_labelmap_posterior_workspace_batch(G, rows, cols, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    labels = labels.contiguous()
    st = lib.crw_labelmap_ordered_posterior_batch(L.data_ptr(), G, T, N, M, rows, cols, int(flip), (ctypes.c_int * S)(*order), S, 1e-4,
                                                  labels.data_ptr(), 1 if labels.dtype == torch.int8 else 0, cols, rows * cols,
                                                  post.data_ptr() if want_post else None, hz.data_ptr() if want_hz else None, cols,
                                                  3 * (S - 1) * cols, ws.data_ptr(), need, None)
    assert st == hip.CRW_OK
    torch.cuda.synchronize()
    return post, hz


# ---- 2. the joint batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(jr.CASES)), ids=CASE_IDS)
def test_joint_batch_equals_the_joint_call_per_configuration(hip, index):
    c = jr.case(index)
    N, M, rows, ncols, order = c.shared
    G = G3
    kind = dr.KINDS[index % 3]
    Ls = [stacked(G, T, N, M, seed=80 + 3 * index + k) for k, (T, _, _, _) in enumerate(c.geo)]
    a, b = c.source(0, Ls[0]), c.source(1, Ls[1])
    lab = hip.labelmap_ordered_joint_batch(a, b, G, *c.shared, confidence=kind, dtype=torch.int8)[0]
    for labels in (lab, lab.float()):
        post, hz = hip.labelmap_ordered_joint_posterior_batch(a, b, G, *c.shared, labels, confidence=kind)
        assert post.shape == (G, rows, ncols) and hz.shape == (G, 3, len(order) - 1, ncols)
        for g in range(G):
            one, one_hz = hip.labelmap_ordered_joint_posterior(c.source(0, Ls[0][g]), c.source(1, Ls[1][g]), *c.shared, labels[g], confidence=kind)
            assert same(post[g], one) and same(hz[g], one_hz), (CASE_IDS[index], kind, labels.dtype, g)
    for k, src in enumerate((a, b)):  # the same tensor twice: a tie keeps a, and the output is the single batch's on that window
        Lk, T, cols, col0, flip = src
        lab1 = hip.labelmap_ordered_batch(Lk, G, T, N, M, rows, cols, order, flip=flip, dtype=torch.int8)[0]
        one, one_hz = hip.labelmap_ordered_posterior_batch(Lk, G, T, N, M, rows, cols, order, lab1, flip=flip)
        two, two_hz = hip.labelmap_ordered_joint_posterior_batch(src, src, G, *c.shared, lab1[:, :, col0:col0 + ncols], confidence=kind)
        assert same(two, one[:, :, col0:col0 + ncols]) and same(two_hz, one_hz[:, :, :, col0:col0 + ncols]), (CASE_IDS[index], k)


def test_one_column_window_at_mcap_16_with_int8_labels_and_a_kind(hip):
    """The instantiation and the shape the first version of the kernel took an illegal access in: 63 of a wave's 64
    lanes lie behind the window and repeat its only column.  An ordinary valid call; G = 2."""
    G, N, M, rows, order, kind = 2, 12, 16, 70, (3, 15, 0, 7, 9), "margin"
    geo = ((1, 1, 0, False), (2, 5, 2, True))
    Ls = [stacked(G, T, N, M, seed=90 + k) for k, (T, _, _, _) in enumerate(geo)]
    a, b = ((L, *g) for L, g in zip(Ls, geo))
    lab = hip.labelmap_ordered_joint_batch(a, b, G, N, M, rows, 1, order, confidence=kind, dtype=torch.int8)[0]
    assert lab.dtype == torch.int8 and lab.shape == (G, rows, 1)
    post, hz = hip.labelmap_ordered_joint_posterior_batch(a, b, G, N, M, rows, 1, order, lab, confidence=kind)
    torch.cuda.synchronize()
    for g in range(G):
        one, one_hz = hip.labelmap_ordered_joint_posterior((Ls[0][g], *geo[0]), (Ls[1][g], *geo[1]), N, M, rows, 1, order, lab[g], confidence=kind)
        assert same(post[g], one) and same(hz[g], one_hz), g
    assert post.min() >= 0 and post.max() <= 1 and torch.isfinite(hz).all() and not same(post[0], post[1])


# ---- 3. windows, the workspace, G = 1, chunks ----------------------------------------------------------------------------------------
def test_windows_inside_wider_maps_keep_their_surroundings(hip):
    """ld > cols, a column offset inside [G, rows, width] maps and a [G, 3, S-1, width] tensor: every byte outside the windows keeps
    its fill, and the labels are only read."""
    T, N, M, rows, cols = dr.SHAPES[5]
    G, order = G3, (15, 3, 0, 8, 9, 1)
    S = len(order)
    L = stacked(G, T, N, M, seed=61)
    c = jr.case(3)
    Lj = [stacked(G, Tk, c.N, c.M, seed=62 + k) for k, (Tk, _, _, _) in enumerate(c.geo)]
    single = lambda **kw: hip.labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, flip=True, **kw)
    joint = lambda **kw: hip.labelmap_ordered_joint_posterior_batch(c.source(0, Lj[0]), c.source(1, Lj[1]), G, *c.shared, confidence="entropy", **kw)
    lab_single = hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, flip=True, dtype=torch.int8)[0]
    lab_joint = hip.labelmap_ordered_joint_batch(c.source(0, Lj[0]), c.source(1, Lj[1]), G, *c.shared, confidence="entropy", dtype=torch.int8)[0]
    for call, lab, (nr, nc), nS in ((single, lab_single, (rows, cols), S), (joint, lab_joint, (c.rows, c.ncols), len(c.order))):
        want, want_hz = call(labels=lab)
        for labels, off in ((lab, 1), (lab.float(), 3), (lab, 6)):
            wide_lab = torch.full((G, nr, nc + 7), -7, dtype=labels.dtype, device="cuda")
            wide_lab[:, :, off:off + nc] = labels
            before = wide_lab.clone()
            wide, wide_hz = torch.full((G, nr, nc + 7), -7.0, device="cuda"), torch.full((G, 3, nS - 1, nc + 9), -7.0, device="cuda")
            out, out_hz = call(labels=wide_lab[:, :, off:off + nc], out=wide[:, :, off:off + nc], out_hz=wide_hz[:, :, :, off + 2:off + 2 + nc])
            assert out.data_ptr() == wide[:, :, off:].data_ptr() and out_hz.data_ptr() == wide_hz[:, :, :, off + 2:].data_ptr()
            assert same(out, want) and same(out_hz, want_hz), (labels.dtype, off)
            assert (wide[:, :, :off] == -7).all() and (wide[:, :, off + nc:] == -7).all()
            assert (wide_hz[..., :off + 2] == -7).all() and (wide_hz[..., off + 2 + nc:] == -7).all()
            assert torch.equal(wide_lab, before)


def test_what_the_workspace_held_before_is_never_read(hip):
    T, N, M, rows, cols = dr.SHAPES[2]
    G, order = G3, (2, 0, 1)
    S = len(order)
    L = stacked(G, T, N, M, seed=63)
    lab = hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, dtype=torch.int8)[0]
    need = hip.labelmap_posterior_workspace_batch(G, rows, cols, S)
    assert need == G * hip.labelmap_posterior_workspace(rows, cols, S) == G * 4 * rows * S * 64
    outs = []
    for poison in (0xFF, 0x00):
        ws = torch.full((need + 64,), poison, dtype=torch.uint8, device="cuda")
        outs.append(hip.labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, lab, workspace=ws))
        outs.append(hip.labelmap_ordered_joint_posterior_batch((L, T, cols, 0, False), (L, T, cols, 0, False), G, N, M, rows, cols, order, lab,
                                                                confidence="maxprob", workspace=ws))
        assert (ws[need:] == poison).all()  # nothing behind the workspace's size is written
    for post, hz in outs[1:]:
        assert same(post, outs[0][0]) and same(hz, outs[0][1])


def test_one_configuration_is_the_single_call(hip):
    for shape in BATCH_SHAPES:
        T, N, M, rows, cols = shape
        order = orders(M)[1]
        L = stacked(1, T, N, M, seed=64)
        lab = hip.labelmap_ordered(L[0], T, N, M, rows, cols, order, dtype=torch.int8)[0]
        post, hz = hip.labelmap_ordered_posterior_batch(L, 1, T, N, M, rows, cols, order, lab[None])
        one, one_hz = hip.labelmap_ordered_posterior(L[0], T, N, M, rows, cols, order, lab)
        assert post.shape == (1, rows, cols) and same(post[0], one) and same(hz[0], one_hz)
        src = (L, T, cols, 0, False)
        post, hz = hip.labelmap_ordered_joint_posterior_batch(src, src, 1, N, M, rows, cols, order, lab[None], confidence="margin")
        assert same(post[0], one) and same(hz[0], one_hz)


def test_the_split_over_several_launches_changes_nothing(hip, monkeypatch):
    """CRW_POSTERIOR_BATCH_WS (read per call) at two and a half configurations' workspace: G = 5 runs as 2 + 2 + 1 launches."""
    T, N, M, rows, cols = dr.SHAPES[2]
    G, order = 5, (0, 1, 2)
    L = stacked(G, T, N, M, seed=65)
    lab = hip.labelmap_ordered_batch(L, G, T, N, M, rows, cols, order, dtype=torch.int8)[0]
    src = (L, T, cols, 0, False), (torch.flip(L.view(G, T, N, M), (1,)).contiguous().view(G, T * N, M), T, cols, 0, True)
    calls = (lambda: hip.labelmap_ordered_posterior_batch(L, G, T, N, M, rows, cols, order, lab),
             lambda: hip.labelmap_ordered_joint_posterior_batch(*src, G, N, M, rows, cols, order, lab, confidence="maxprob"))
    monkeypatch.delenv("CRW_POSTERIOR_BATCH_WS", raising=False)
    assert hip.posterior_batch_chunks(G, rows, cols, len(order)) == [5]
    want = [call() for call in calls]
    one = hip.labelmap_posterior_workspace(rows, cols, len(order))
    monkeypatch.setenv("CRW_POSTERIOR_BATCH_WS", str(2 * one + one // 2))
    assert hip.posterior_batch_chunks(G, rows, cols, len(order)) == [2, 2, 1]
    for call, (post, hz) in zip(calls, want):
        got, got_hz = call()
        assert same(got, post) and same(got_hz, hz)
    monkeypatch.setenv("CRW_POSTERIOR_BATCH_WS", "1")  # less than one configuration's: one configuration per launch
    assert hip.posterior_batch_chunks(G, rows, cols, len(order)) == [1] * 5
    got, got_hz = calls[0]()
    assert same(got, want[0][0]) and same(got_hz, want[0][1])
    for g in range(G):
        one_post, one_hz = hip.labelmap_ordered_posterior(L[g], T, N, M, rows, cols, order, lab[g])
        assert same(got[g], one_post) and same(got_hz[g], one_hz)


# ---- 4. status codes -------------------------------------------------------------------------------------------------------------------
def test_batch_argument_errors_launch_nothing(hip):
    lib = hip.lib()
    G = 3
    La, Lb = torch.full((G, 16, 4), 0.25, device="cuda"), torch.full((G, 16, 4), 0.25, device="cuda")
    labels = torch.zeros(G, 8, 8, device="cuda")
    post, hz = torch.full((G, 8, 8), -7.0, device="cuda"), torch.full((G, 3, 1, 8), -7.0, device="cuda")
    need = lib.crw_labelmap_posterior_workspace_batch(G, 8, 8, 2)
    assert need == G * lib.crw_labelmap_posterior_workspace(8, 8, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    order = (ctypes.c_int * 2)(0, 1)

    def call(joint, G=G, floor=1e-4, labels_ptr=labels.data_ptr(), post_ptr=post.data_ptr(), hz_ptr=hz.data_ptr(), ld=8, ms=64, hz_ld=8,
             hz_stride=24, ws_ptr=ws.data_ptr(), ws_bytes=need, kind=0, S=2, col0_b=8, M=4, rows=8, La_ptr=La.data_ptr()):
        tail = (floor, labels_ptr, 0, ld, ms, post_ptr, hz_ptr, hz_ld, hz_stride, ws_ptr, ws_bytes, None)
        if joint:
            return lib.crw_labelmap_ordered_joint_posterior_batch(La_ptr, 4, 8, 0, 0, Lb.data_ptr(), 4, 16, col0_b, 1, G, 4, M, rows, 8, order,
                                                                  S, kind, *tail)
        return lib.crw_labelmap_ordered_posterior_batch(La_ptr, G, 4, 4, M, rows, 8, 0, order, S, *tail)

    for joint in (False, True):
        # the batch's own: G, the two strides, slices that overflow a size_t
        for kw in (dict(G=0), dict(G=-1), dict(G=65536), dict(ms=63), dict(ld=9, ms=7 * 9 + 7), dict(hz_stride=23), dict(hz_ld=9, hz_stride=26),
                   dict(ms=1 << 62), dict(hz_stride=1 << 62), dict(hz_ld=1 << 62, hz_stride=1 << 63),
                   # each of the single calls' refusals
                   dict(floor=0.0), dict(floor=2.0 ** -21), dict(floor=0.3), dict(floor=float("nan")), dict(post_ptr=None, hz_ptr=None),
                   dict(post_ptr=post.data_ptr() + 2), dict(hz_ptr=hz.data_ptr() + 2), dict(hz_ld=7), dict(ws_ptr=None),
                   dict(ws_ptr=ws.data_ptr() + 2), dict(S=1), dict(S=5), dict(La_ptr=None), dict(labels_ptr=None), dict(M=1), dict(M=17),
                   dict(rows=0), dict(ld=7)):
            assert call(joint, **kw) == hip.CRW_EINVAL, (joint, kw)
        assert call(joint, ws_bytes=need - 1) == hip.CRW_EWORKSPACE
        assert call(joint, ws_bytes=need - 1, post_ptr=None) == hip.CRW_EWORKSPACE
    for kw in (dict(kind=-1), dict(kind=3), dict(col0_b=9), dict(col0_b=-1)):
        assert call(True, **kw) == hip.CRW_EINVAL, kw
    assert lib.crw_labelmap_posterior_workspace_batch(0, 8, 8, 2) == lib.crw_labelmap_posterior_workspace_batch(3, 0, 8, 2) == 0
    assert lib.crw_labelmap_posterior_workspace_batch(3, 8, 8, 1) == lib.crw_labelmap_posterior_workspace_batch(3, 8, 8, 17) == 0
    with pytest.raises(hip.CrwError) as e:
        hip.labelmap_ordered_posterior_batch(La, G, 4, 4, 4, 8, 8, (0, 1), labels, out=post, out_hz=hz, workspace=ws[:need - 4])
    assert e.value.status == hip.CRW_EWORKSPACE
    torch.cuda.synchronize()
    assert (post == -7).all() and (hz == -7).all() and not ws.any()
    assert call(False) == hip.CRW_OK
    torch.cuda.synchronize()
    first, first_hz = post.clone(), hz.clone()
    post.fill_(-7.0), hz.fill_(-7.0)
    assert call(True) == hip.CRW_OK
    torch.cuda.synchronize()
    # uniform rows: every monotone path weighs the same; label 0 at row r is state 0 there: (rows - r) of the rows + 1 paths
    want = (8 - torch.arange(8.0, device="cuda")) / 9
    assert torch.allclose(post, want[None, :, None].expand(G, 8, 8), rtol=1e-5) and same(post, first) and same(hz, first_hz)
    assert (hz[:, 0] == 8).all()


# ---- 5. segment_sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,use_last", [("segment_ds0_correction", False), ("segment_ds3_correction_reverse", True)],
                         ids=["forward", "use_last"])
def test_segment_sweep_posterior_equals_segment_per_configuration(hip, monkeypatch, name, use_last):
    import inference as crw_inference
    import utils as crw_utils
    from imported.labelprop import LabelPropVOS_CRW
    from test_sweep import build_case, grid_around
    from test_sweep_dense_gpu import _Flatten, force
    g = load_golden(name)
    sweep = grid_around(g)
    G = len(sweep.configs)
    _, seg, ncls, T, patch, overlap, changes, kw = build_case(g, "cuda")
    order = tuple(range(ncls))
    kw.update(use_last=use_last, upsample="bilinear", confidence="maxprob", decode="ordered", order=order, merge="ordered" if use_last else "rule")
    fresh = lambda: build_case(g, "cuda")[0]

    def run_sweep(**extra):
        monkeypatch.setattr(crw_inference, "propagate_sweep", force(crw_utils.propagate_sweep, changes))
        return crw_inference.segment_sweep(fresh(), seg, _Flatten(), sweep, ncls, T, patch, overlap, **kw, **extra)

    plain, out = run_sweep(), run_sweep(posterior=True)
    assert set(out) == set(plain) | {"post", "horizon", "floor"} and out["floor"] == 1e-4 and out["change_idx"] == plain["change_idx"]
    for k in ("pred", "forward", "conf", "forward_conf"):
        assert same(out[k].float(), plain[k].float()), k
    rows, width = out["pred"].shape[1:]
    assert out["post"].shape == (G, rows, width) and out["horizon"].shape == (G, 3, ncls - 1, width)
    assert out["post"].dtype == out["horizon"].dtype == torch.float32 and out["post"].is_cuda
    for i, cfg in enumerate(sweep.configs):
        monkeypatch.setattr(crw_inference, "propagate", force(crw_utils.propagate, changes))
        one = crw_inference.segment(fresh(), seg, _Flatten(), LabelPropVOS_CRW(cfg), ncls, T, patch, overlap, posterior=True, **kw)
        assert one["change_idx"] == out["change_idx"]
        assert torch.equal(out["pred"][i], one["pred"].to(torch.int8)), cfg
        assert same(out["post"][i], one["post"]) and same(out["horizon"][i], one["horizon"]), cfg
    assert len({p.cpu().numpy().tobytes() for p in out["post"]}) > 1
    bars = crw_inference.horizon_bars_sweep(out["horizon"], seg[:, :width], order)
    assert len(bars) == G
    for i, b in enumerate(bars):
        assert str(b) == str(crw_inference.horizon_bars(out["horizon"][i], seg[:, :width], order))
