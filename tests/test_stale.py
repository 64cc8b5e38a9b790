"""tests/stale_ref.py on fake "entry points" written in torch (CPU): a clean one passes; one that adds its workspace into the
result, one that leaves part of an output unwritten and one that writes outside its declared region are each reported, by buffer
and by property; so are broken padding promises, oversized workspaces and state carried from one call to the next.  The guard-band
properties of `run_banded` likewise: a read in front of an input, a read past its end multiplied by zero, a write past an output
and a write into an input's band are each reported by operand and property, and each goes unseen with its check switched off; a
read past the end that a select discards passes."""
import pytest
import torch

import stale_ref as sr

P, PPAD, C = 5, 8, 6
F = 4


def _f32(t, n=None):
    v = t.view(torch.float32)
    return v if n is None else v[:n]


def _bufs(**over):
    """y [PPAD][C] fp32: rows < P written, rows P .. PPAD-1 promised zero (so: written too); part [3][C] fp32; n [2] int32
    (byte-compared only); tick: a ticket word inside the workspace, left zeroed"""
    row = C * F
    b = dict(y=sr.Buf(PPAD * row, zero=[sr.rows(P, PPAD, row)]), part=sr.Buf(3 * row, written=[sr.rows(0, 2, row)]),
             n=sr.Buf(8, dtype=None), ws=sr.Buf(3 * row + 4, ws=True, zero=[(3 * row, 3 * row + 4)]))
    b.update(over)
    return b


def _clean(x, t, add_ws=False, skip_row=None, spill=False, keep_pad=False, keep_ticket=False, n_rows=2):
    ws = _f32(t["ws"][:3 * C * F]).view(3, C)         # two slices hold rows; the third holds none and is never written
    tick = t["ws"][3 * C * F:].view(torch.int32)
    if not keep_ticket:
        tick.zero_()                                   # the entry point zeroes its own ticket ...
    ws[0] = x[:3].sum(0)                               # ... and writes every partial before it reads it
    ws[1] = x[3:].sum(0)
    tick += 2
    y = _f32(t["y"]).view(PPAD, C)
    for r in range(P):
        if r != skip_row:
            y[r] = x[r] * 2 + (ws[0] + ws[1] if not add_ws else ws.sum(0))
    if not keep_pad:
        y[P:] = 0
    part = _f32(t["part"]).view(3, C)
    part[0], part[1] = ws[0], ws[1]
    if spill:
        part[2, 1] = 1.0
    t["n"].view(torch.int32)[:n_rows] = torch.tensor([P, C], dtype=torch.int32)[:n_rows]
    tick -= 2                                          # left zeroed


def _case(run=_clean, bufs=None, **kw):
    x = torch.arange(P * C, dtype=torch.float32).reshape(P, C) / 7 - 1
    return sr.Case("fake_entry", x, bufs or _bufs(), lambda inp, t: run(inp, t, **kw))


def test_clean_entry_point_passes():
    out = sr.run_twice(_case())
    assert _f32(out["y"]).view(PPAD, C)[:P].abs().sum() > 0
    sr.run_reused(_case(), _case().inputs * -3 + 1)


def _reported(case, buffer, prop, fn=sr.run_twice, *a):
    with pytest.raises(sr.StaleError) as e:
        fn(case, *a)
    assert (e.value.entry, e.value.buffer, e.value.prop) == ("fake_entry", buffer, prop), str(e.value)
    assert "fake_entry" in str(e.value) and f"'{buffer}'" in str(e.value) and prop in str(e.value)


def test_workspace_added_into_the_result_is_reported():
    """adds all three slabs of the workspace, the third of which nobody wrote: NaN under 0xFF, the right answer under 0x00"""
    _reported(_case(add_ws=True), "y", sr.STALE)


def test_unwritten_part_of_an_output_is_reported():
    _reported(_case(skip_row=3), "y", sr.STALE)
    _reported(_case(n_rows=1), "n", sr.STALE)          # an integer output: no NaN to see, the two fills differ


def test_write_outside_the_declared_region_is_reported():
    _reported(_case(spill=True), "part", sr.REGION)


def test_padding_rows_not_zeroed_is_reported():
    """with rows P .. PPAD-1 declared unwritten instead, the 0x00 run would hide it: the promise is held in both runs"""
    _reported(_case(keep_pad=True), "y", sr.STALE)
    row = C * F
    lax = _bufs(y=sr.Buf(PPAD * row, written=[sr.rows(0, P, row)], zero=[sr.rows(P, PPAD, row)]))
    _reported(_case(keep_pad=True, bufs=lax), "y", sr.PADDING)


def test_workspace_longer_than_asked_is_reported():
    case = _case()
    tensors = {k: sr.filled(b.nbytes + (16 if k == "ws" else 0), 0, "cpu") for k, b in case.bufs.items()}
    with pytest.raises(sr.StaleError) as e:
        sr._execute(case, case.inputs, 0, tensors)
    assert (e.value.buffer, e.value.prop) == ("ws", sr.REGION)


def test_ticket_not_zeroed_is_reported():
    """an entry point that relies on its ticket being zero on entry: wrong under the 0xFF fill"""
    _reported(_case(keep_ticket=True), "ws", sr.PADDING)


def test_state_carried_between_calls_is_reported():
    """a slab of the previous call added into this one: the reuse run names it on buffers that only ever held finite numbers"""
    def carry(x, t):
        ws = _f32(t["ws"][:3 * C * F]).view(3, C)
        y = _f32(t["y"]).view(PPAD, C)
        y[:P] = x + ws[1]                              # ws[1]: whatever the previous call left
        y[P:] = 0
        ws[0], ws[1] = x[0], x[1]
        _f32(t["part"]).view(3, C)[:2] = ws[:2]
        t["n"].zero_()
        t["ws"][3 * C * F:] = 0
    case = sr.Case("fake_entry", _case().inputs, _bufs(), carry)
    _reported(case, "y", sr.REUSE, sr.run_reused, case.inputs + 1)


# ================================================================================================ guard bands (run_banded)
def _neighbour(t, offset, n=1):
    """n elements of t's storage starting `offset` elements from t's first: what an index that ran over addresses"""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + offset)


def _banded(defect=None, device="cpu"):
    """y [P][C] = 2 x + s, s [C] an in/out operand (a running sum: s += column sums of x), on inputs that live between bands.
    (device: tests/test_guard_bands_gpu.py plants the same defects on the GPU; every access stays inside the allocations.)"""
    home = sr.Home(device)
    x = home((torch.arange(P * C, dtype=torch.float32).reshape(P, C) / 7 - 1).to(device), "x")
    s0 = torch.linspace(-1, 1, C).to(device)

    def run(_, t):
        y, s = _f32(t["y"]).view(P, C), _f32(t["s"])
        s += x.sum(0)
        y.copy_(x * 2 + s)
        if defect == "reads in front":
            y[0, 0] += _neighbour(x, -1)[0]
        if defect == "reads a row past the end, times zero":
            y[P - 1] += _neighbour(x, P * C, C) * 0.0
        if defect == "reads past the end, discarded by select":
            y[P - 1] += torch.where(torch.zeros(C, dtype=torch.bool, device=device), _neighbour(x, P * C, C), torch.zeros(C, device=device))
        if defect == "writes past the output":
            _neighbour(y, P * C)[0] = 1.0
        if defect == "writes in front of an input":
            _neighbour(x, -1)[0] = 1.0
    bufs = dict(y=sr.Buf(P * C * F, step=C * F), s=sr.Buf(C * F, init=s0))
    return sr.Case("fake_entry", None, bufs, run, device=device, home=home)


def test_clean_entry_point_passes_between_guard_bands():
    out = sr.run_banded(_banded())
    y, s = _f32(out["y"]).view(P, C), _f32(out["s"])
    assert torch.equal(s, torch.linspace(-1, 1, C) + (torch.arange(P * C, dtype=torch.float32).reshape(P, C) / 7 - 1).sum(0))
    assert y.abs().sum() > 0                          # (the in/out operand started from its own copy in both runs)


def test_read_in_front_of_an_input_is_reported():
    _reported(_banded("reads in front"), "y", sr.SURROUND_READ, sr.run_banded)
    sr.run_banded(_banded("reads in front"), hold=(sr.SURROUND_WRITTEN,))          # without its check the defect goes unseen


def test_read_past_the_end_times_zero_is_reported():
    """the case that zero-filled memory hides and the reason one fill is NaN: 0 * NaN is NaN, 0 * 0 the right answer.  With both
    bands zero -- memory fresh from the allocator -- the two runs agree and nothing is seen."""
    case = _banded("reads a row past the end, times zero")
    _reported(case, "y", sr.SURROUND_READ, sr.run_banded)
    assert "first at element" in str(pytest.raises(sr.StaleError, sr.run_banded, case).value)
    sr.run_banded(case, hold=(sr.SURROUND_WRITTEN,))
    fills, sr.FILLS = sr.FILLS, (0x00, 0x00)
    try:
        sr.run_banded(case)
    finally:
        sr.FILLS = fills


def test_read_past_the_end_discarded_by_select_passes():
    """loads are issued unconditionally and the value is dropped by a select.  Such a load is no defect as
    long as it stays inside mapped memory (the band stands for the next tensor): no byte of the result depends on it, and
    SURROUNDINGS-READ holds results, not addresses."""
    sr.run_banded(_banded("reads past the end, discarded by select"))


def test_write_past_an_output_is_reported():
    case = _banded("writes past the output")
    _reported(case, "y", sr.SURROUND_WRITTEN, sr.run_banded)
    assert "0 bytes past the operand's end" in str(pytest.raises(sr.StaleError, sr.run_banded, case).value)
    sr.run_banded(case, hold=(sr.SURROUND_READ,))


def test_write_into_the_band_of_an_input_is_reported():
    case = _banded("writes in front of an input")
    _reported(case, "x", sr.SURROUND_WRITTEN, sr.run_banded)
    assert "1 bytes before the operand's first byte" in str(pytest.raises(sr.StaleError, sr.run_banded, case).value)
    sr.run_banded(case, hold=(sr.SURROUND_READ,))


def test_guard_band_geometry():
    """at least 256 KiB, a multiple of 256 bytes and no shorter than the operand's largest index step; the operand keeps its shape,
    dtype and content; an unbanded case is refused"""
    home = sr.Home("cpu")
    t = torch.arange(2 * 3 * 300 * 300, dtype=torch.float32).reshape(2, 3, 300, 300)
    v = home(t, "A")
    op = home.operands[0]
    assert sr.largest_step(t) == 3 * 300 * 300 * 4 and sr.largest_step(t[:1]) == 300 * 300 * 4
    assert op.band >= sr.largest_step(t) > sr.BAND and op.band % 256 == 0 and op.front.numel() == op.back.numel() == op.band
    assert torch.equal(v, t) and v.dtype == t.dtype and v.shape == t.shape and v.data_ptr() == op.raw.data_ptr() + op.band
    small = sr.Banded("b", 10, None, "cpu")
    assert small.band == sr.BAND and small.raw.numel() == 2 * sr.BAND + 10
    assert sr.PLAIN(t, "A") is t and home(None) is None
    assert home.many(a=t[0, 0], b=None)[1] is None and home.operands[-1].name == "a"
    with pytest.raises(ValueError):
        sr.run_banded(_case())


def test_filled_and_rows():
    t = sr.filled(0, 0xFF)
    assert t.numel() == 1 and int(t[0]) == 0xFF
    assert torch.isnan(sr.filled(8, 0xFF).view(torch.float32)).all() and torch.isnan(sr.filled(8, 0xFF).view(torch.bfloat16)).all()
    assert torch.isnan(sr.filled(8, 0xFF).view(torch.float64)).all()
    assert sr.rows(2, 5, 12) == (24, 60)
