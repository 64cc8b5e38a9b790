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

`run_banded` asks WHERE a kernel reads and writes (GPU cases: tests/test_encoder_stale_gpu.py, tests/test_guard_bands_gpu.py).  Every
operand of the case -- the inputs, which the builder passes through a `Home`, as well as the outputs and workspaces -- is a view,
of the operand's own shape and dtype, into the middle of a larger byte allocation: a guard band of at least 256 KiB (a multiple of
256 bytes, and no shorter than the operand's largest index step, which is asserted) lies in front of it and another behind it,
and the operand itself stays at the allocator's 256-byte alignment, so every kernel takes the route it takes in production.  The
sequence runs once with every band filled with 0xFF (NaN as fp32, bf16 and fp64, a huge index as int32) and once with 0x00 --
memory outside a fresh allocation is very often zero, which is exactly what a halo, a partial tile or a ragged last chunk wants
to see; the inputs and the fill of the operands themselves (0x00) are the same in both runs.  Held:

  4. SURROUNDINGS-READ     every declared-written region is finite and bit-identical between the two runs: a value fetched from
                           outside an operand and multiplied by zero is NaN under the 0xFF bands; one discarded by a select is
                           harmless and passes
  5. SURROUNDINGS-WRITTEN  after each run every byte of every band, around inputs, outputs and workspaces, still holds its fill

The bands see an index that is off by up to one plane, frame or matrix, not a wild pointer: a read further away than the band is
out of scope.  So are operands at addresses that are not 256-byte aligned.

A failure is a `StaleError` whose message names the entry point, the buffer and the property; for the two band properties also
the first differing byte, or the first changed band byte with its distance from the operand (which index ran over).

`BANDED`, `WINDOWED_ELSEWHERE` and `HOST_ONLY` at the end of this file say, for every entry point of include/crw_hip.h, where its
operands are banded; tests/test_host.py holds the list against the header."""
import torch

FILLS = (0xFF, 0x00)
BAND = 256 * 1024                  # the least length of a guard band, bytes
OPERAND_FILL = 0x00                # what outputs and workspaces hold before a banded run, in both runs
SURROUND_READ, SURROUND_WRITTEN = ("depends on memory outside its operands (property 4, SURROUNDINGS-READ: finite and bit-identical "
                                   "under 0xFF / 0x00 guard bands)",
                                   "bytes of a guard band changed (property 5, SURROUNDINGS-WRITTEN)")
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
    ws: a workspace -- its content is not an output; only its length is held (and `zero`, e.g. tickets left zeroed).
    step: the largest index step inside the buffer, bytes (a frame, a plane, a matrix): its guard bands are at least that long
    (None: flat or opaque, the 256 KiB of every band)."""

    def __init__(self, nbytes, dtype=torch.float32, written=None, zero=(), init=None, ws=False, step=None):
        self.nbytes, self.dtype, self.zero, self.init, self.ws = int(nbytes), dtype, list(zero), init, ws
        self.step = step
        self.written = None if written is None else list(written)


def rows(first, last, row_bytes):
    """the byte range of rows first .. last-1 of a [*, row_bytes] buffer"""
    return (first * row_bytes, last * row_bytes)


class Case:
    """entry: the name reported.  inputs: anything, handed to `run`.  bufs: {name: Buf}.  run(inputs, tensors) executes the call
    sequence with tensors = {name: byte tensor} and synchronises.  home: the `Home` the builder passed its inputs through
    (`run_banded` needs a banded one)."""

    def __init__(self, entry, inputs, bufs, run, device="cpu", home=None):
        self.entry, self.inputs, self.bufs, self.run, self.device, self.home = entry, inputs, bufs, run, device, home


def largest_step(t):
    """the largest index step of a dense tensor, bytes: its largest stride over the dimensions that have more than one entry"""
    steps = [st for n, st in zip(t.shape, t.stride()) if n > 1]
    return max(steps + [1]) * t.element_size()


class Banded:
    """nbytes bytes (`mid`) between two guard bands inside one allocation `raw`; each band is max(BAND, step) rounded up to 256."""

    def __init__(self, name, nbytes, step, device):
        self.name, self.nbytes, step = name, max(int(nbytes), 1), int(step or 1)
        self.band = max(BAND, -(-step // 256) * 256)
        assert self.band >= BAND and self.band % 256 == 0 and step <= self.band, (name, step, self.band)
        self.raw = torch.empty(2 * self.band + self.nbytes, dtype=torch.uint8, device=device)
        if torch.device(device).type != "cpu":
            assert self.raw.data_ptr() % 256 == 0
        self.front, self.mid, self.back = self.raw[:self.band], self.raw[self.band:self.band + self.nbytes], self.raw[self.band + self.nbytes:]
        assert self.back.numel() == self.band

    def fill_bands(self, byte):
        self.front.fill_(byte)
        self.back.fill_(byte)

    def check_bands(self, entry, byte):
        """property 5 for this operand"""
        for side, band in (("in front of", self.front), ("behind", self.back)):
            hit = band != byte
            if hit.any():
                idx = hit.nonzero().reshape(-1)
                first = int(idx[-1] if side == "in front of" else idx[0])      # the changed byte nearest to the operand
                where = (f"{self.band - first} bytes before the operand's first byte" if side == "in front of" else
                         f"{first} bytes past the operand's end (byte {self.nbytes + first} from its start)")
                raise StaleError(entry, self.name, SURROUND_WRITTEN, f"{int(hit.sum())} bytes of the {self.band}-byte band {side} the operand "
                                 f"changed with the bands filled with 0x{byte:02X}; the nearest one lies {where}")


class Home:
    """Where a case's device inputs live.  A builder passes EVERY input through its `home` -- those another entry point produced
    (packed planes, packed weights) included: home(t, name) -> a tensor of t's shape, dtype and content.  Home(banded=False)
    (`PLAIN`) hands t back as it is; a banded Home copies it between two guard bands and keeps the allocation, so that
    `run_banded` can fill the bands and hold them afterwards."""

    def __init__(self, device="cpu", banded=True):
        self.device, self.banded, self.operands = device, banded, []

    def __call__(self, t, name=None):
        if t is None or not self.banded:
            return t
        assert t.is_contiguous(), name
        name = name or f"input {len(self.operands)}"
        op = Banded(name, t.numel() * t.element_size(), largest_step(t), self.device)
        if t.numel():
            op.mid.copy_(t.reshape(-1).view(torch.uint8))
        self.operands.append(op)
        return op.mid[:t.numel() * t.element_size()].view(t.dtype).view(t.shape)

    def many(self, **named):
        """home(t, name) for each keyword, in order"""
        return tuple(self(t, k) for k, t in named.items())


PLAIN = Home(banded=False)


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


def _finite(case, name, buf, t, mask, byte, prop=STALE, what="every buffer"):
    if buf.dtype is None or not buf.dtype.is_floating_point:
        return
    size = torch.empty((), dtype=buf.dtype).element_size()
    assert buf.nbytes % size == 0
    v = t[:buf.nbytes].view(buf.dtype)
    bad = ~torch.isfinite(v) & mask[:buf.nbytes].view(-1, size)[:, 0].to(t.device)
    if bad.any():
        raise StaleError(case.entry, name, prop, f"{int(bad.sum())} of {v.numel()} declared-written values not finite with "
                         f"{what} filled with 0x{byte:02X} (first at element {int(bad.nonzero()[0])})")


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


def run_banded(case, hold=(SURROUND_READ, SURROUND_WRITTEN)):
    """properties 4 and 5 (`hold`: which of them; tests/test_stale.py shows each planted defect going unseen without its check)
    -> the tensors of the run with 0x00 bands"""
    home = case.home
    if not isinstance(home, Home) or not home.banded:
        raise ValueError(f"{case.entry}: run_banded needs a case whose builder passed its inputs through a banded Home")
    runs = []
    for byte in FILLS:
        for k, b in case.bufs.items():          # a band must outreach one index step: checked, not assumed (a workspace is opaque)
            assert b.step is not None or b.ws or b.nbytes <= BAND, f"{case.entry}: buffer '{k}' is longer than a band: declare its `step`"
        outer = {k: Banded(k, b.nbytes, b.step, case.device) for k, b in case.bufs.items()}
        for op in outer.values():
            op.mid.fill_(OPERAND_FILL)
        for op in home.operands + list(outer.values()):
            op.fill_bands(byte)
        tensors = _execute(case, case.inputs, OPERAND_FILL, {k: op.mid for k, op in outer.items()})
        if SURROUND_WRITTEN in hold:
            for op in home.operands + list(outer.values()):
                op.check_bands(case.entry, byte)
        if SURROUND_READ in hold:
            for name, buf in case.bufs.items():
                if not buf.ws:
                    _finite(case, name, buf, tensors[name], _mask(buf, tensors[name].numel()), byte, SURROUND_READ, "every guard band")
        runs.append(tensors)
    if SURROUND_READ in hold:
        _compare(case, runs[0], runs[1], SURROUND_READ, "between the run with 0xFF and the run with 0x00 guard bands")
    return runs[1]


# ================================================================================================ who bands what
# Every entry point of include/crw_hip.h that takes a device pointer is in exactly one of BANDED and WINDOWED_ELSEWHERE; the rest
# is HOST_ONLY.  tests/test_host.py test_every_device_entry_point_is_banded_or_windowed holds the three against the header, and
# each named file against the entry point's name: a new entry point fails there until somebody decides where it is covered.
_ENC, _GB = "tests/test_encoder_stale_gpu.py", "tests/test_guard_bands_gpu.py"

# entry point -> the test file that runs it under `run_banded`
BANDED = {
    **{name: _GB for name in (
        "crw_normalize", "crw_affinity_fwd", "crw_affinity_bwd", "crw_walk_fwd", "crw_walk_bwd", "crw_gemm_f32", "crw_gemm_bf16",
        "crw_xent_metric", "crw_adam_step", "crw_labelprop_topk", "crw_labelprop_topk_grid", "crw_labelprop_topk_scores",
        "crw_labelprop_sweep_weights", "crw_labelprop_gather", "crw_labelprop_propagate", "crw_labelprop_propagate_batch",
        "crw_labelprop_propagate_sliding", "crw_labelprop_propagate_sliding_batch", "crw_labelprop_confidence",
        "crw_enc_pack_weights", "crw_enc_pack_input", "crw_enc_pack_input_map", "crw_enc_gap_bwd", "crw_enc_front_pack",
        "crw_enc_front_fwd_map", "crw_rn_pack_conv", "crw_rn_pack_stem", "crw_rn_pack_stem16", "crw_rn_split", "crw_rn_bn_apply",
        "crw_rn_bn_pool")},
    **{name: _ENC for name in (
        "crw_enc_conv3x3", "crw_enc_conv3x3_map", "crw_enc_conv3x3_wgrad", "crw_enc_conv3x3_wgrad_map", "crw_enc_front_fwd",
        "crw_enc_front_bwd", "crw_enc_front_bwd_map", "crw_linear128_wgrad", "crw_rn_conv", "crw_rn_wgrad", "crw_rn_bn_stats",
        "crw_rn_bn_stats_rows", "crw_rn_bn_bwd", "crw_rn_pool_bwd", "crw_rn_stem_fwd", "crw_rn_stem_bwd", "crw_rn_stem_stats",
        "crw_rn_stem16_fwd", "crw_rn_stem_band_fwd", "crw_rn_stem16_wgrad", "crw_rn_stem16_bwd", "crw_rn_colsum", "crw_rn_train_fwd",
        "crw_rn_train_fwd_nograd", "crw_rn_train_bwd", "crw_rn_eval_fwd")},
}

# the evaluation kernels: entry point -> the existing test that runs it inside a wider, poisoned map (column windows, offsets into a
# wider buffer) and holds the surroundings
WINDOWED_ELSEWHERE = {
    "crw_confusion": "tests/test_metrics_gpu.py",
    "crw_calibration": "tests/test_confidence_gpu.py",
    "crw_merge_confidence": "tests/test_confidence_gpu.py",
    "crw_horizons": "tests/test_horizons_gpu.py",
    "crw_labelmap_dense": "tests/test_dense_gpu.py",
    "crw_labelmap_dense_batch": "tests/test_sweep_dense_gpu.py",
    "crw_labelmap_ordered": "tests/test_ordered_gpu.py",
    "crw_labelmap_ordered_batch": "tests/test_ordered_gpu.py",
    "crw_labelmap_ordered_joint": "tests/test_joint_gpu.py",
    "crw_labelmap_ordered_joint_batch": "tests/test_joint_gpu.py",
    "crw_labelmap_ordered_posterior": "tests/test_posterior_gpu.py",
    "crw_labelmap_ordered_joint_posterior": "tests/test_posterior_gpu.py",
    "crw_labelmap_ordered_posterior_batch": "tests/test_sweep_posterior_gpu.py",
    "crw_labelmap_ordered_joint_posterior_batch": "tests/test_sweep_posterior_gpu.py",
}

# pure host queries: no pointer among their parameters (sizes, geometry, build info, the timing switch) ...
HOST_ONLY = (
    "crw_abi_version", "crw_build_arch", "crw_last_hip_error", "crw_padded_nodes", "crw_walk_state_bytes", "crw_walk_scratch_bytes",
    "crw_affinity_ws_bytes", "crw_confusion_ws_bytes", "crw_horizons_ws_bytes", "crw_calibration_ws_bytes",
    "crw_labelmap_ordered_workspace", "crw_labelmap_posterior_workspace", "crw_labelmap_posterior_workspace_batch",
    "crw_linear128_wgrad_ws_bytes", "crw_enc_wgrad_ws_bytes", "crw_enc_front_saved_bytes", "crw_enc_front_ws_bytes",
    "crw_rn_padded_patches", "crw_rn_stem_toeplitz_ld", "crw_rn_stem_cols", "crw_rn_conv_part_floats", "crw_rn_wgrad_ws_bytes",
    "crw_rn_bn_stats_ws_bytes", "crw_rn_bn_bwd_ws_bytes", "crw_rn_pool_bwd_ws_bytes", "crw_rn_stem_ws_bytes", "crw_rn_stem16_rows",
    "crw_rn_stem_band_ok", "crw_rn_stem16_ws_bytes", "crw_rn_colsum_ws_bytes", "crw_rn_train_ws_bytes", "crw_rn_timing_enable",
    "crw_gemm_bf16_ws_bytes")
# ... and the two whose pointers are HOST arrays, as the header says: the change-point search and the timing records
HOST_POINTERS = ("crw_pelt_rbf", "crw_rn_timing_read")
