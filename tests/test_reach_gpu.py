"""GPU side of the accuracy-against-distance report: crw_confusion_grouped (include/crw_hip_reach.h) through the C ABI, held integer
for integer to the plain loops of tests/reach_ref.py.
  * every case runs between guard bands and over stale memory (`stale_ref.run_banded`, `run_twice`): the maps, the confidences and
    the group map are windows of wider, poisoned buffers -- NaN / 127 labels, confidences of 2, group 0 around the group map: a pixel
    read outside a window changes a count --, the workspace is stale, and the outputs of the 0xFF and the 0x00 runs are equal;
  * shapes rows x cols (ld): 1 x 1, 3 x 5, 7 x 33 (40, base pointer off by one element), 37 x 131, 64 x 256 and 410 x 1600 -- one lane
    and one wave, a strip that is not full, more than one strip with a ragged last one, whole strips, more than one slab of rows --
    crossed with the operand dtypes, aux, conf, K = 2 / 5 / 16 and the groupings of `reach_ref.group_maps`; K = 16 with 64 groups is
    the LDS worst case.  The kernel has ONE route (no selector, no switch), so the route log has no name to assert: asserted
    instead is that a call registers no route;
  * conf_sum within pixels x 2^-52 relative of the fp64 sum of the same fp32 values, and bit-identical between calls;
  * against the yardsticks `crw_hip.confusion` and `crw_hip.calibration(bins=1)` on the same windows;
  * `inference.label_reach` on the first [30, 13] item, after `inference.segment` on the 96 x 320 synthetic case, and
    `label_reach_sweep` after `segment_sweep` on a 2 x 1 x 2 grid."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import reach_ref as rr
import stale_ref as sr

pytestmark = pytest.mark.gpu

F32, F64, I64 = torch.float32, torch.float64, torch.int64
DT = {"f32": 0, "i8": 1}


@pytest.fixture(scope="module")
def hip():
    import crw_hip
    crw_hip.lib()
    assert torch.cuda.is_available() and crw_hip.has_reach() and crw_hip.has_confidence() and crw_hip.has_routes()
    return crw_hip


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# rows, cols, ld, offset (elements), K, gt dtype, pred dtype, aux dtype, conf, ignore labels, grouping
CASES = [
    (1, 1, 1, 0, 2, "f32", "f32", None, False, False, "one"),
    (1, 1, 1, 0, 5, "i8", "i8", "i8", True, False, "own"),
    (3, 5, 5, 0, 5, "f32", "i8", None, True, False, "default"),
    (3, 5, 9, 0, 2, "i8", "i8", "f32", False, True, "own"),
    (7, 33, 40, 1, 5, "i8", "i8", "i8", True, True, "own"),
    (7, 33, 40, 1, 16, "f32", "f32", "f32", True, True, "own"),          # K = 16 with 64 groups: the LDS worst case
    (7, 33, 40, 1, 2, "f32", "i8", None, False, False, "holes"),
    (37, 131, 131, 0, 2, "f32", "i8", "f32", False, True, "holes"),
    (37, 131, 131, 0, 16, "i8", "i8", None, True, False, "default"),
    (37, 131, 131, 0, 5, "f32", "f32", "i8", True, True, "one"),
    (64, 256, 256, 0, 5, "f32", "f32", "i8", True, True, "default"),
    (64, 256, 256, 0, 16, "f32", "i8", None, False, False, "holes"),
    (64, 256, 256, 0, 2, "i8", "i8", "f32", True, False, "one"),
    (410, 1600, 1600, 0, 5, "f32", "i8", "i8", True, True, "default"),
    (410, 1600, 1600, 0, 16, "i8", "i8", None, False, False, "holes"),
]


@functools.lru_cache(maxsize=None)
def reference(spec):
    """(the case's maps, its group map, the loops' result), computed once per case"""
    rows, cols, ld, off, K, dg, dp, da, conf, ignore, kind = spec
    c = rr.case(rows, cols, K, rows * cols + K + len(kind), dg, dp, da, conf, ignore)
    group, groups = rr.group_maps(cols, kind)
    want = rr.confusion_grouped(c["gt"], c["pred"], K, group, groups, conf=c["conf"], aux=c["aux"], ignore_gt=c["ignore_gt"],
                                ignore_pred=c["ignore_pred"], ignore_aux=c["ignore_aux"])
    return c, group, groups, want


def _wide(a, ld, off, poison):
    """the window `a` inside a wider 1-D buffer of off + rows * ld elements, `poison` everywhere else"""
    rows, cols = a.shape
    wide = np.full(off + rows * ld, poison, a.dtype)
    wide[off:].reshape(rows, ld)[:, :cols] = a
    return torch.from_numpy(wide).cuda()


def banded_case(hip, home, spec):
    lib = hip.lib()
    rows, cols, ld, off, K, dg, dp, da, conf, ignore, kind = spec
    c, group, groups, want = reference(spec)
    poison = lambda a: 127 if a.dtype == np.int8 else np.nan                 # a label no map holds: counted as invalid if it is read
    ops = dict(gt=_wide(c["gt"], ld, off, poison(c["gt"])), pred=_wide(c["pred"], ld, off, poison(c["pred"])))
    if da is not None:
        ops["aux"] = _wide(c["aux"], ld, off, 4)                             # the ignore label: masked if it is read
    if conf:
        ops["conf"] = _wide(c["conf"], ld, off, 2.0)
    ops["grp"] = _wide(group[None], cols + 3, 2, 0)                          # two bytes in front, one behind: group 0
    dev = dict(zip(ops, home.many(**ops)))
    at = lambda name, o: None if name not in dev else ctypes.c_void_p(dev[name].data_ptr() + o * dev[name].element_size())
    nbytes = lib.crw_confusion_grouped_ws_bytes(rows, cols, K, groups)
    bufs = dict(ws=sr.Buf(nbytes, None, ws=True), counts=sr.Buf(groups * K * K * 8, None), dropped=sr.Buf(32, None))
    if conf:
        bufs["conf_sum"] = sr.Buf(groups * 8, F64)

    def run(_, t):
        p = lambda name: ctypes.c_void_p(t[name].data_ptr()) if name in t else None
        st = lib.crw_confusion_grouped(at("gt", off), DT[dg], at("pred", off), DT[dp], at("aux", off), DT[da or "i8"], at("conf", off), rows, cols,
                                       ld, at("grp", 2), groups, K, c["ignore_gt"], c["ignore_pred"], c["ignore_aux"], p("counts"),
                                       p("conf_sum"), p("dropped"), p("ws"), nbytes, _stream())
        assert st == 0, st
        torch.cuda.synchronize()

    case = sr.Case(f"crw_confusion_grouped {spec}", None, bufs, run, device="cuda", home=home)

    def check(t):
        counts = t["counts"][:groups * K * K * 8].view(I64).view(groups, K, K).cpu().numpy()
        dropped = t["dropped"][:32].view(I64).cpu().numpy()
        assert np.array_equal(dropped, want[2]), (dropped, want[2])
        assert np.array_equal(counts, want[0]), np.argwhere(counts != want[0])[:5]
        assert counts.sum() + dropped.sum() == rows * cols
        if not conf:
            return counts, dropped, None
        sums = t["conf_sum"][:groups * 8].view(F64).cpu().numpy()
        pixels = counts.sum((1, 2))
        err = np.abs(sums - want[1])
        print(f"{spec}: worst |conf_sum - fp64| / (pixels 2^-52 sum) {np.max(err / np.maximum(pixels * 2.0 ** -52 * np.abs(want[1]), 1e-300)):.3g}")
        assert (err <= pixels * 2.0 ** -52 * np.abs(want[1])).all() and not sums[pixels == 0].any()
        return counts, dropped, sums

    return case, check


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(map(str, s)))
def test_grouped_counts_are_the_loops_between_guard_bands_and_over_stale_memory(hip, spec):
    with hip.routes() as hit:
        case, check = banded_case(hip, sr.Home("cuda"), spec)
        assert case.home.operands
        a = check(sr.run_banded(case))
        b = check(sr.run_twice(case))
    assert not hit, hit                                                       # one route: nothing selects, nothing is named
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if a[2] is not None:
        assert np.array_equal(a[2].view(np.int64), b[2].view(np.int64))      # bit-identical from call to call
    want = reference(spec)[3]
    if spec[0] * spec[1] >= 200:                                              # what is planted shows
        assert want[2][1] > 0 and (not spec[9] or want[2][0] > 0) and (not spec[8] or want[2][2] > 0) and (spec[10] != "holes" or want[2][3] > 0)
    if spec[10] == "default":
        assert (want[0].sum((1, 2)) == 0).any()                               # empty groups


def test_empty_windows_give_zeros(hip):
    lib = hip.lib()
    for rows, cols in ((0, 70), (9, 0), (0, 0)):
        out = torch.full((3 * 25 + 3 + 4,), -1, dtype=I64, device="cuda")
        p = lambda o: ctypes.c_void_p(out.data_ptr() + 8 * o)
        conf = torch.zeros(1, device="cuda")
        st = lib.crw_confusion_grouped(None, 0, None, 0, None, 1, ctypes.c_void_p(conf.data_ptr()), rows, cols, cols, None, 3, 5, -1, -1, -1, p(0), p(75),
                                       p(78), None, 0, _stream())
        assert st == 0 and not out.cpu().any()


@pytest.mark.parametrize("rows,cols,K,dg,dp,da", [(37, 131, 5, "f32", "i8", "i8"), (64, 256, 16, "i8", "i8", None), (130, 200, 2, "f32", "f32", "f32")])
def test_against_confusion_and_calibration_through_the_binding(hip, rows, cols, K, dg, dp, da):
    """windows [:, 3:3 + cols] of wider device maps, read where they lie"""
    c = rr.case(rows, cols + 9, K, rows + cols, dg, dp, da, True, True)
    dev = {k: (torch.from_numpy(v).cuda()[:, 3:3 + cols] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    mask = dict(aux=dev["aux"], ignore_gt=c["ignore_gt"], ignore_pred=c["ignore_pred"], ignore_aux=c["ignore_aux"])
    counts0, dropped0 = hip.confusion(dev["gt"], dev["pred"], K, **mask)
    one, none, d1 = hip.confusion_grouped(dev["gt"], dev["pred"], K, torch.zeros(cols, dtype=torch.uint8), 1, **mask)
    assert none is None and torch.equal(one[0], counts0) and torch.equal(d1[:2], dropped0) and not d1[2:].any()
    for kind in ("default", "own") if cols <= 64 else ("default",):
        group, groups = rr.group_maps(cols, kind)
        counts, _, d = hip.confusion_grouped(dev["gt"], dev["pred"], K, torch.from_numpy(group), groups, **mask)
        assert torch.equal(counts.sum(0), counts0) and torch.equal(d[:2], dropped0) and not d[2:].any()
    group, groups = rr.group_maps(cols, "default")
    counts, sums, d = hip.confusion_grouped(dev["gt"], dev["pred"], K, torch.from_numpy(group).cuda(), groups, conf=dev["conf"], **mask)
    cal, cal_sum, cal_d = hip.calibration(dev["gt"].contiguous(), dev["pred"].contiguous(), dev["conf"].contiguous(), K, bins=1,
                                          aux=None if dev["aux"] is None else dev["aux"].contiguous(), ignore_gt=c["ignore_gt"],
                                          ignore_pred=c["ignore_pred"], ignore_aux=c["ignore_aux"])
    correct = counts.diagonal(dim1=1, dim2=2).sum()
    assert int(counts.sum()) == int(cal[0, 0]) and int(correct) == int(cal[0, 1]) and torch.equal(d[:3], cal_d) and int(d[2]) > 0
    total = float(cal_sum[0])
    assert abs(float(sums.sum()) - total) <= rows * cols * 2.0 ** -52 * total
    want = rr.confusion_grouped(c["gt"][:, 3:3 + cols], c["pred"][:, 3:3 + cols], K, group, groups, conf=c["conf"][:, 3:3 + cols],
                                aux=None if c["aux"] is None else c["aux"][:, 3:3 + cols], ignore_gt=c["ignore_gt"], ignore_pred=c["ignore_pred"],
                                ignore_aux=c["ignore_aux"])
    assert np.array_equal(counts.cpu().numpy(), want[0]) and np.array_equal(d.cpu().numpy(), want[2])


def test_label_reach_on_the_first_drifting_item(hip):
    """the [30, 13] seed-0 cells of tests/test_reach.py, through the device"""
    import inference
    T, N, M, cxt, seed, cls, ref, sliding = rr.drift_maps()[0]
    assert (T, N, seed) == (30, 13, 0)
    for pred in (ref, sliding):
        cpu = inference.label_reach(torch.from_numpy(pred), torch.from_numpy(cls), 3, [0], 1, direction="forward", nclasses=M)
        dev = inference.label_reach(torch.from_numpy(pred).cuda(), torch.from_numpy(cls).cuda(), 3, [0], 1, direction="forward", nclasses=M)
        assert np.array_equal(dev.counts, cpu.counts) and dev.dropped == cpu.dropped == (0, 0, 0, 0) and dev.frames == cpu.frames
        assert dev.reach_at(0.9) == cpu.reach_at(0.9)
    assert cpu.reach_at(0.9) == T - 1


@pytest.fixture(scope="module")
def e2e():
    from test_confidence_gpu import M_E2E, OVERLAP, PATCH, T_E2E, e2e_case
    enc, fresh, seg, lp, N = e2e_case(0, n_rg=2, H=100)
    assert tuple(seg.shape) == (96, 320)
    return dict(enc=enc, fresh=fresh, seg=seg, lp=lp, M=M_E2E, T=T_E2E, patch=PATCH, overlap=OVERLAP)


def _same(reach, pred, conf, seg, K, marks):
    labelled, segments, direction, step = marks
    group, frames = rr.column_groups(pred.shape[1], labelled, step, None, segments, direction)
    want = rr.confusion_grouped(seg.cpu().numpy(), pred.cpu().numpy(), K, group, 12, conf=conf.cpu().numpy())
    assert np.array_equal(reach.counts, want[0]) and reach.dropped == tuple(want[2])
    pixels = want[0].sum((1, 2))
    assert (np.abs(reach.conf_sum - want[1]) <= pixels * 2.0 ** -52 * np.abs(want[1])).all()
    assert [f[1] for f in reach.frames[:-1] if f[1] is not None][:4] == [0, 1, 2, 4] and reach.pixels[4:].sum() == 0      # 10 frames, both directions


def test_label_reach_after_segment_and_its_sweep(hip, e2e):
    import inference
    from imported.labelprop import LabelPropSweep, LabelPropVOS_CRW
    c = e2e
    marks = inference.labelled_columns(320, c["T"], c["patch"], c["overlap"], True)
    assert marks[1:] == ([0, 160, 320], "both", 16)
    kw = dict(use_last=True, dataset_id=3, confidence="maxprob")
    out = inference.segment(c["fresh"](), c["seg"], c["enc"], c["lp"], c["M"], c["T"], c["patch"], c["overlap"], **kw)
    reach = inference.label_reach(out["pred"], c["seg"], 3, marks[0], marks[3], segments=marks[1], direction=marks[2], conf=out["conf"],
                                  nclasses=c["M"])
    _same(reach, out["pred"], out["conf"], c["seg"], c["M"], marks)
    ev = inference.evaluate(out["pred"], c["seg"], 3, nclasses=c["M"])
    assert reach.total == ev.total and np.array_equal(reach.counts.sum(0), ev.counts)
    sweep = LabelPropSweep(6, radii=[4, 6], temps=[0.1], knns=[4, 8])
    outs = inference.segment_sweep(c["fresh"](), c["seg"], c["enc"], sweep, c["M"], c["T"], c["patch"], c["overlap"], **kw)
    reaches = inference.label_reach_sweep(outs["pred"], c["seg"], 3, marks[0], marks[3], segments=marks[1], direction=marks[2],
                                          conf=outs["conf"], nclasses=c["M"])
    assert len(reaches) == 4
    for g, r in enumerate(reaches):
        single = inference.label_reach(outs["pred"][g], c["seg"], 3, marks[0], marks[3], segments=marks[1], direction=marks[2],
                                       conf=outs["conf"][g], nclasses=c["M"])
        assert np.array_equal(r.counts, single.counts) and np.array_equal(r.conf_sum.view(np.int64), single.conf_sum.view(np.int64))
        assert r.dropped == single.dropped and r.frames == single.frames
        _same(r, outs["pred"][g], outs["conf"][g], c["seg"], c["M"], marks)
