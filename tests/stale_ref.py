"""Does an entry point read memory it did not write?  A harness for "stale workspace" tests (tests/test_encoder_stale_gpu.py; its
proof on planted defects: tests/test_stale.py).  No GPU import at module level: everything here runs on any torch device.

A `Case` names an entry point (or a short sequence of them), its inputs (built once), and its buffers: workspaces with the byte
counts the library asks for, and outputs.  For every output the case declares the region the header documents as written (default:
all of it) and the regions the header promises to be zero.  `run_twice` executes the sequence once with every buffer filled with
byte 0xFF (NaN as fp32, bf16 and fp64; 0xFFFFFFFF as a ticket) and once with 0x00 and holds three properties:

  1. STALE    every declared-written region is finite (float dtypes) and bit-identical between the two runs
  2. REGION   every byte outside the declared region still holds the fill byte; a workspace is exactly as long as asked
  3. PADDING  every region promised zero is zero in both runs

`run_reused` runs the sequence on one set of inputs and again, on the SAME un-refilled buffers, on a second set; that second
result must equal, bit for bit, the second set's result on freshly 0x00-filled buffers (state carried from call to call).

A failure is a `StaleError` whose message names the entry point, the buffer and the property."""
import torch

FILLS = (0xFF, 0x00)
STALE, REGION, PADDING, REUSE = ("depends on memory it did not write (property 1: finite and bit-identical under 0xFF / 0x00 fills)",
                                 "bytes outside the declared-written region changed (property 2)",
                                 "rows promised zero are not zero (property 3)",
                                 "depends on what the previous call left in the buffers (reuse)")


class StaleError(AssertionError):
    def __init__(self, entry, buffer, prop, detail=""):
        self.entry, self.buffer, self.prop = entry, buffer, prop
        super().__init__(f"{entry}: buffer '{buffer}': {prop}" + (f" -- {detail}" if detail else ""))


def filled(nbytes, byte, device="cpu"):
    """a byte tensor of max(nbytes, 1) bytes, every one `byte`; on the GPU at the allocator's 256-byte aligned address"""
    t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
    if torch.device(device).type != "cpu":
        assert t.data_ptr() % 256 == 0
    return t.fill_(byte)


class Buf:
    """One buffer of a case.  nbytes: exactly what the library asks for (a workspace) or the tensor's size (an output).
    dtype: how the written region is read for the finiteness check (None: bytes only, e.g. codes, tickets, int counts).
    written: None = all of it, else a list of (first byte, end byte) ranges the header documents as written.
    zero: byte ranges the header promises to be zero after the call (they must lie inside `written`).
    init: a byte tensor copied in after the fill -- an in/out operand (running statistics): each run starts from its own copy.
    ws: a workspace -- its content is not an output; only its length is held (and `zero`, e.g. tickets left zeroed)."""

    def __init__(self, nbytes, dtype=torch.float32, written=None, zero=(), init=None, ws=False):
        self.nbytes, self.dtype, self.zero, self.init, self.ws = int(nbytes), dtype, list(zero), init, ws
        self.written = None if written is None else list(written)


def rows(first, last, row_bytes):
    """the byte range of rows first .. last-1 of a [*, row_bytes] buffer"""
    return (first * row_bytes, last * row_bytes)


class Case:
    """entry: the name reported.  inputs: anything, handed to `run`.  bufs: {name: Buf}.  run(inputs, tensors) executes the call
    sequence with tensors = {name: byte tensor} and synchronises."""

    def __init__(self, entry, inputs, bufs, run, device="cpu"):
        self.entry, self.inputs, self.bufs, self.run, self.device = entry, inputs, bufs, run, device


def _mask(buf, n):
    m = torch.zeros(n, dtype=torch.bool)
    if buf.written is None:
        m[:buf.nbytes] = True
    for a, b in buf.written or ():
        assert 0 <= a <= b <= buf.nbytes, (a, b, buf.nbytes)
        m[a:b] = True
    return m


def _execute(case, inputs, byte, tensors=None):
    if tensors is None:
        tensors = {k: filled(b.nbytes, byte, case.device) for k, b in case.bufs.items()}
    for k, b in case.bufs.items():
        if tensors[k].numel() != max(b.nbytes, 1):
            raise StaleError(case.entry, k, REGION, f"{tensors[k].numel()} bytes allocated, {b.nbytes} asked for")
        if b.init is not None:
            tensors[k][:b.nbytes].copy_(b.init.reshape(-1).view(torch.uint8))
    case.run(inputs, tensors)
    return tensors


def _finite(case, name, buf, t, mask, byte):
    if buf.dtype is None or not buf.dtype.is_floating_point:
        return
    size = torch.empty((), dtype=buf.dtype).element_size()
    assert buf.nbytes % size == 0
    v = t[:buf.nbytes].view(buf.dtype)
    bad = ~torch.isfinite(v) & mask[:buf.nbytes].view(-1, size)[:, 0].to(t.device)
    if bad.any():
        raise StaleError(case.entry, name, STALE, f"{int(bad.sum())} of {v.numel()} declared-written values not finite with "
                         f"every buffer filled with 0x{byte:02X} (first at element {int(bad.nonzero()[0])})")


def _check_run(case, tensors, byte):
    """properties 2 and 3 and finiteness of one run"""
    for name, buf in case.bufs.items():
        t = tensors[name]
        if buf.ws and not buf.zero:
            continue
        if not buf.ws:
            mask = _mask(buf, t.numel())
            _finite(case, name, buf, t, mask, byte)
            outside = ~mask.to(t.device)
            outside[buf.nbytes:] = False                                  # (the one byte of a zero-length buffer)
            touched = outside & (t != byte)
            if touched.any():
                raise StaleError(case.entry, name, REGION, f"{int(touched.sum())} bytes changed with the fill 0x{byte:02X} "
                                 f"(first at byte {int(touched.nonzero()[0])})")
        for a, b in buf.zero:
            nz = t[a:b] != 0
            if nz.any():
                raise StaleError(case.entry, name, PADDING, f"{int(nz.sum())} non-zero bytes in [{a}, {b}) with the fill "
                                 f"0x{byte:02X} (first at byte {a + int(nz.nonzero()[0])})")


def _compare(case, a, b, prop, what):
    for name, buf in case.bufs.items():
        if buf.ws:
            continue
        m = _mask(buf, a[name].numel()).to(a[name].device)
        diff = m & (a[name] != b[name])
        if diff.any():
            raise StaleError(case.entry, name, prop, f"{int(diff.sum())} bytes of the declared-written region differ {what} "
                             f"(first at byte {int(diff.nonzero()[0])})")


def run_twice(case):
    """-> the tensors of the 0x00 run (for checks of the caller's own, e.g. that the result is not all zeros)"""
    runs = []
    for byte in FILLS:
        runs.append(_execute(case, case.inputs, byte))
        _check_run(case, runs[-1], byte)
    _compare(case, runs[0], runs[1], STALE, "between the 0xFF-filled and the 0x00-filled run")
    return runs[1]


def run_reused(case, inputs2):
    """the sequence on case.inputs, then on inputs2 in the same tensors un-refilled, against inputs2 on fresh 0x00-filled ones"""
    tensors = _execute(case, case.inputs, 0x00)
    tensors = _execute(case, inputs2, 0x00, tensors)
    fresh = _execute(case, inputs2, 0x00)
    _check_run(case, fresh, 0x00)
    _compare(case, tensors, fresh, REUSE, "between reused and fresh buffers")
    return fresh
