"""tests/stale_ref.py on fake "entry points" written in torch (CPU): a clean one passes; one that adds its workspace into the
result, one that leaves part of an output unwritten and one that writes outside its declared region are each reported, by buffer
and by property; so are broken padding promises, oversized workspaces and state carried from one call to the next."""
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


def test_filled_and_rows():
    t = sr.filled(0, 0xFF)
    assert t.numel() == 1 and int(t[0]) == 0xFF
    assert torch.isnan(sr.filled(8, 0xFF).view(torch.float32)).all() and torch.isnan(sr.filled(8, 0xFF).view(torch.bfloat16)).all()
    assert torch.isnan(sr.filled(8, 0xFF).view(torch.float64)).all()
    assert sr.rows(2, 5, 12) == (24, 60)
