"""Cases, the model and drivers for the softargmax operator (qnnp_*_softargmax_nc_q8; hip/q8softargmax.hip behind
softargmax.c).

The case list restates the parameters of the reference's operator tests, test/softargmax.cc (12 tests), loop for loop
(the float loop in float32, as the C++ runs it), with the tester's defaults (test/softargmax-operator-tester.h: input
scale 0.176080093, output 1/256 and 0, batch 1, strides = the channel count). The tester runs each case for a few
iterations of fresh random input; here each case runs once, on input seeded by its name. Its input zero point only moves
the tester's own float reference (the operator has no such argument), so those cases differ in their input alone.

model() is the operator's definition in numpy with 64-bit intermediates, all values uint32 (reference
src/operator-run.c:625-637, src/u8lut32norm/scalar.c):

    m    = max over the row of x[c]
    t_c  = table[x[c] + (255 - m)]
    vsum = (sum over c of t_c) mod 2^32              the reference's sum WRAPS, so does the model's
    y[c] = min(((t_c << 8) + (vsum >> 1)) // vsum, 255)

with the table of reference src/softargmax.c:86-91 from math.exp and round (the same libm and the same
round-half-to-even as the C code). It is PINNED by the compiled reference: the CPU tier runs every case on the reference
and compares byte for byte; the GPU tier compares the product with the reference's bytes.

THE FENCE. Where a row's vsum is 0 modulo 2^32 the reference divides by zero and the process dies (its assert is compiled
out): a constant row of 1024, 4096 or 65536 channels does it at any input scale. run_reference() therefore computes the
model's row sums first and RAISES, before any call into the reference, if a row's sum is 0; a case marked zero_sum=True is
meant to hold such rows and never reaches the reference at all. For those rows the product's output is defined as all 0
(the sum can only be 0 modulo 2^32 by being at least 2^32, and every t_c << 8 is below 2^31), and the model with that
rule is the truth.

Every tensor handed to a library sits between PAD bytes of FILL on either side, and the output buffer starts filled with
FILL: the bytes before the first row, between strided rows and behind the last row must come back as FILL.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

FILL = 0xA5
PAD = 32                      # bytes of FILL in front of and behind every tensor
DEFAULT_SCALE = 0.176080093   # test/softargmax-operator-tester.h

# hip/q8softargmax.hip: rows of up to GROUP_MAX channels live in the registers of a lane group, rows of up to LDS_MAX
# channels in a workgroup's LDS, longer rows are read three times. The kernel names carry both thresholds, so
# tests/test_gpu_softargmax.py fails if these drift from the kernels'.
GROUP_MAX = 1024
LDS_MAX = 32768
LANE_PIECES = {16: 2, 1: 16}  # pieces (of 16 bytes, of 1 byte) a lane of the group kernel holds
# one pass of the loops on the MI355X: 256 compute units x 8 workgroups of row groups, x 4 workgroups of rows
GROUP_PASS_BLOCKS = 256 * 8
BLOCK_PASS_ROWS = 256 * 4


def row_pieces(channels: int, vec: int) -> int:
    """pieces of `vec` bytes that can touch a row at any alignment"""
    return channels if vec == 1 else (channels + 2 * vec - 2) // vec


def group_lanes(channels: int, vec: int) -> int:
    """lanes per row in the group kernel: the smallest power of two whose lanes hold the row's pieces"""
    lanes = 1
    while lanes * LANE_PIECES[vec] < row_pieces(channels, vec):
        lanes *= 2
    assert lanes <= 64, (channels, vec)
    return lanes


def kernel_name(channels: int, vec: int) -> str:
    if channels <= GROUP_MAX:
        return f"q8_softargmax_group{GROUP_MAX}_x{vec}"
    if channels <= LDS_MAX:
        return f"q8_softargmax_lds{LDS_MAX}_x{vec}"
    return f"q8_softargmax_stream_x{vec}"


def selection_boundaries() -> List[int]:
    """the largest channel count of every lane-group size (for both piece widths) and of every kernel"""
    out = set()
    for vec in LANE_PIECES:
        for c in range(1, GROUP_MAX):
            if group_lanes(c, vec) != group_lanes(c + 1, vec):
                out.add(c)
    return sorted(out | {GROUP_MAX, LDS_MAX})


def _seed(name: str) -> int:
    return 0x50F7 ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class Case:
    name: str
    batch: int
    channels: int
    in_stride: int = 0            # 0: the channel count
    out_stride: int = 0
    input_scale: float = 0.0      # 0: the tester's default
    rows: str = "random"          # what the rows hold: see _fill_rows
    next_batch: int = 0           # a second setup on new buffers with this batch (0: none)
    misalign_in: int = 0          # GPU tier: device base pointer offsets (bytes)
    misalign_out: int = 0
    host: bool = False            # GPU tier: host pointers (the staged path)
    in_place: bool = False        # output is the input tensor (equal strides)
    next_out_of_place: bool = False   # the second setup of an in-place case has an output tensor of its own
    zero_sum: bool = False        # holds rows whose table sum is 0 modulo 2^32: never handed to the reference

    @property
    def scale(self) -> float:
        return float(np.float32(self.input_scale or DEFAULT_SCALE))

    def in_place_at(self, setup: int) -> bool:
        return self.in_place and not (setup > 0 and self.next_out_of_place)

    def strides_at(self, setup: int):
        si = self.in_stride or self.channels
        return (si, si if self.in_place_at(setup) else (self.out_stride or self.channels))

    def batches(self):
        return [self.batch] + ([self.next_batch] if self.next_batch else [])

    def create_args(self):
        """the arguments of the operator's create after `channels`"""
        return (self.scale, 0, 1.0 / 256.0)


def _float_loop(start, stop, factor):
    """for (float v = start; v < stop; v *= factor), in float32"""
    v, stop, factor = np.float32(start), np.float32(stop), np.float32(factor)
    out = []
    while v < stop:
        out.append(float(v))
        v = np.float32(v * factor)
    return out


CHANNELS_5 = list(range(1, 100, 5))


# ---- the reference's test list (test/softargmax.cc), loop for loop -----------------------------------------------

def _reference_tests(add):
    add("zero_batch", batch=0, channels=1)
    add("single_class", batch=1, channels=1)
    add("two_classes", batch=1, channels=2)
    for c in range(3, 100):
        add("many_classes", batch=1, channels=c)
    for c in (10, 100):
        add("cifar_classes", batch=1, channels=c)
    for c in (1000, 1001, 21841):
        add("imagenet_classes", batch=1, channels=c)
    for c in CHANNELS_5:
        for s in _float_loop(1.0e-2, 1.0e+2, 3.14159265):
            add("many_channels_with_input_scale", batch=1, channels=c, input_scale=s)
    for c in CHANNELS_5:
        for _zp in range(0, 256, 51):
            add("many_channels_with_input_zero_point", batch=1, channels=c)
    for c in CHANNELS_5:
        add("small_batch", batch=3, channels=c)
    for c in CHANNELS_5:
        add("small_batch_with_input_stride", batch=3, channels=c, in_stride=129)
    for c in CHANNELS_5:
        add("small_batch_with_output_stride", batch=3, channels=c, out_stride=117)
    for c in CHANNELS_5:
        add("strided_batch_with_input_and_output_stride", batch=3, channels=c, in_stride=129, out_stride=117)


def reference_cases() -> List[Case]:
    out: List[Case] = []
    counts = {}

    def add(test, **kw):
        k = counts.get(test, 0)
        counts[test] = k + 1
        out.append(Case(f"ref/{test}/{k}", **kw))
    _reference_tests(add)
    return out


# ---- beyond the reference's list ---------------------------------------------------------------------------------

def boundary_cases() -> List[Case]:
    """channels B - 1, B, B + 1 around every boundary of the lane-group and kernel selection, and 1 .. 70: contiguous
    (16-byte pieces on aligned buffers) and with strides (c + 5, c + 2) (single bytes); 29 rows, so the last wave of the
    group kernel is part full"""
    channels = set(range(1, 71))
    for b in selection_boundaries():
        channels |= {b - 1, b, b + 1}
    out = []
    for c in sorted(ch for ch in channels if ch >= 1):
        out.append(Case(f"x/boundary/c{c}", 29, c))
        out.append(Case(f"x/boundary/c{c}_strided", 29, c, in_stride=c + 5, out_stride=c + 2))
    return out


MISALIGNED_CHANNELS = (1, 7, 21, 33, 100, 1000)


def misaligned_cases(channels: int) -> List[Case]:
    """input and output base misaligned by 0 .. 15 independently, strided rows (the strides differ by 16, so equal
    misalignments take 16-byte pieces, the others single bytes); equal misalignments contiguous as well"""
    out = []
    for mi in range(16):
        for mo in range(16):
            out.append(Case(f"x/misaligned/c{channels}_m{mi}_{mo}", 5, channels, in_stride=channels + 19,
                            out_stride=channels + 3, misalign_in=mi, misalign_out=mo))
        out.append(Case(f"x/misaligned/c{channels}_m{mi}_contiguous", 5, channels, misalign_in=mi, misalign_out=mi))
    return out


CONTENT_CHANNELS = (21, 513, 1000, 1025, 21841)
CONTENTS = ("random", "top", "dominant", "tie", "constant", "max_first", "max_last")
ZERO_SUM_CHANNELS = (1024, 4096)


def content_cases() -> List[Case]:
    return [Case(f"x/content/c{c}_{rows}", 4, c, rows=rows) for c in CONTENT_CHANNELS for rows in CONTENTS]


def zero_sum_cases() -> List[Case]:
    """a constant row (table sum 0 modulo 2^32) between two random rows: product against model only"""
    return [Case(f"x/zero_sum/c{c}", 3, c, rows="zero_sum_middle", zero_sum=True) for c in ZERO_SUM_CHANNELS]


def sweep_cases() -> List[Case]:
    """more than one pass of each kernel's loop on the MI355X"""
    return [
        # group kernel: 21 channels are 2 lanes a row, 128 rows a workgroup
        Case("x/sweep/group", GROUP_PASS_BLOCKS * 128 + 77, 21),
        Case("x/sweep/lds", BLOCK_PASS_ROWS + 76, GROUP_MAX + 1),
        Case("x/sweep/stream", BLOCK_PASS_ROWS + 76, LDS_MAX + 1),      # 36 MB
    ]


def extra_cases() -> List[Case]:
    out = boundary_cases() + content_cases()
    for c in (21, 1000):
        for s in (1e-6, 0.01, 1.0, 97.0):
            out.append(Case(f"x/scale/c{c}_s{s:g}", 3, c, input_scale=s))
            out.append(Case(f"x/scale/c{c}_s{s:g}_top", 3, c, input_scale=s, rows="top"))
    for c in (21, 100, 1000, 1500, LDS_MAX + 200):
        out += [
            Case(f"x/in_place/c{c}", 9, c, in_place=True),
            Case(f"x/in_place/c{c}_strided", 9, c, in_stride=c + 7, in_place=True),
            Case(f"x/in_place/c{c}_strided16", 9, c, in_stride=c + 16, in_place=True),
            Case(f"x/in_place/c{c}_m3", 9, c, in_place=True, misalign_in=3),
            Case(f"x/in_place/c{c}_strided_m3", 9, c, in_stride=c + 7, in_place=True, misalign_in=3),
        ]
    for c in (40, 1500):
        out += [
            Case(f"x/host/c{c}", 13, c, host=True),
            Case(f"x/host/c{c}_strided", 13, c, in_stride=c + 5, out_stride=c + 1, host=True),
            Case(f"x/host/c{c}_in_place_strided", 13, c, in_stride=c + 5, host=True, in_place=True),
            Case(f"x/resetup/c{c}_larger", 7, c, next_batch=31),
            Case(f"x/resetup/c{c}_in_place_to_out_of_place", 31, c, in_stride=c + 6, out_stride=c + 2, next_batch=5,
                 in_place=True, next_out_of_place=True),
        ]
    out.append(Case("x/zero_batch/c21", 0, 21))
    return out


def all_cases() -> List[Case]:
    return (reference_cases() + extra_cases() + [c for ch in MISALIGNED_CHANNELS for c in misaligned_cases(ch)] +
            zero_sum_cases() + sweep_cases())


# ---- tensors ------------------------------------------------------------------------------------------------------
def _span(batch: int, stride: int, channels: int) -> int:
    return (batch - 1) * stride + channels if batch else 0


def _pixels(buf: np.ndarray, n: int, stride: int, channels: int) -> np.ndarray:
    """the [n][channels] view of the rows of a strided tensor (no copy)"""
    return np.lib.stride_tricks.as_strided(buf, shape=(n, channels), strides=(stride, 1))


def _fill_rows(kind: str, rows: np.ndarray, rng) -> None:
    n, c = rows.shape
    if kind == "random":
        return
    if kind == "top":                      # every byte at or near the maximum: the sum is as large as it gets
        rows[...] = rng.integers(250, 256, size=(n, c), dtype=np.uint8)
    elif kind == "dominant":               # one class far above the rest: 255 beside zeros
        rows[...] = 7
        rows[np.arange(n), rng.integers(0, c, size=n)] = 200
    elif kind == "tie":                    # two equal maxima far above the rest: 128 and 128
        rows[...] = 7
        for i in range(n):
            rows[i, rng.choice(c, size=min(2, c), replace=False)] = 200
    elif kind == "constant":               # the sum is channels * table[255]: it wraps beyond 512 channels
        rows[...] = rng.integers(0, 256, size=(n, 1), dtype=np.uint8)
    elif kind in ("max_first", "max_last"):
        rows[...] = rng.integers(0, 200, size=(n, c), dtype=np.uint8)
        rows[:, 0 if kind == "max_first" else c - 1] = 255 - np.arange(n, dtype=np.uint8)
    elif kind == "zero_sum_middle":
        rows[n // 2, :] = 113
    else:
        raise ValueError(kind)


def input_tensor(case: Case, setup: int = 0) -> np.ndarray:
    """the input of setup number `setup`: random bytes (between the rows too), then the rows the case asks for"""
    batch = case.batches()[setup]
    si = case.strides_at(setup)[0]
    rng = np.random.default_rng(_seed(f"{case.name}/{setup}"))
    x = rng.integers(0, 256, size=_span(batch, si, case.channels), dtype=np.uint8)
    if batch:
        _fill_rows(case.rows, _pixels(x, batch, si, case.channels), rng)
    return x


def output_tensor(case: Case, setup: int = 0) -> np.ndarray:
    return np.full(_span(case.batches()[setup], case.strides_at(setup)[1], case.channels), FILL, dtype=np.uint8)


# ---- the model ----------------------------------------------------------------------------------------------------
_TABLES = {}


def table(scale: float, channels: int) -> np.ndarray:
    """reference src/softargmax.c:86-91; `scale` already rounded to float32"""
    key = (scale, channels)
    if key not in _TABLES:
        qscale = min(4294967295.0 / float(channels), 8388607.0)
        t = np.array([int(round(qscale * math.exp(float(i - 255) * scale))) for i in range(256)], dtype=np.int64)
        assert t.min() >= 0 and t.max() < (1 << 23)
        t.setflags(write=False)
        _TABLES[key] = t
    return _TABLES[key]


_CHUNK = 1 << 22   # elements of 64-bit intermediates at a time


def _row_chunks(n: int, channels: int):
    step = max(1, _CHUNK // channels)
    for lo in range(0, n, step):
        yield lo, min(n, lo + step)


def row_sums(case: Case, x: np.ndarray, setup: int = 0) -> np.ndarray:
    """each row's table sum modulo 2^32"""
    n, si = case.batches()[setup], case.strides_at(setup)[0]
    t = table(case.scale, case.channels)
    rows = _pixels(x, n, si, case.channels) if n else np.zeros((0, case.channels), np.uint8)
    sums = np.zeros(n, dtype=np.int64)
    for lo, hi in _row_chunks(n, case.channels):
        xs = rows[lo:hi].astype(np.int64)
        sums[lo:hi] = t[xs + (255 - xs.max(axis=1, keepdims=True))].sum(axis=1) & 0xFFFFFFFF
    return sums


def model(case: Case, x: np.ndarray, setup: int = 0):
    """(the output buffer after one setup + run on input x -- FILL between strided rows, or the input's own bytes in
    place --, each row's table sum modulo 2^32). A row whose sum is 0 gives all 0."""
    n = case.batches()[setup]
    si, so = case.strides_at(setup)
    out = x.copy() if case.in_place_at(setup) else output_tensor(case, setup)
    sums = np.zeros(n, dtype=np.int64)
    if n:
        t = table(case.scale, case.channels)
        rows, dst = _pixels(x, n, si, case.channels), _pixels(out, n, so, case.channels)
        for lo, hi in _row_chunks(n, case.channels):
            xs = rows[lo:hi].astype(np.int64)
            tc = t[xs + (255 - xs.max(axis=1, keepdims=True))]
            vsum = (tc.sum(axis=1) & 0xFFFFFFFF)[:, None]
            q = np.minimum(((tc << 8) + (vsum >> 1)) // np.maximum(vsum, 1), 255)
            dst[lo:hi] = np.where(vsum == 0, 0, q).astype(np.uint8)
            sums[lo:hi] = vsum[:, 0]
    return out, sums


# ---- drivers ------------------------------------------------------------------------------------------------------
class ZeroSumRow(Exception):
    """a row whose table sum is 0 modulo 2^32 was about to be handed to the compiled reference, which would divide by
    zero there and take the process with it"""


def create(lib, case: Case, channels: int = None):
    return lib.create_softargmax_nc_q8_status(case.channels if channels is None else channels, *case.create_args())


def _padded(data: np.ndarray) -> np.ndarray:
    return np.concatenate([np.full(PAD, FILL, np.uint8), data, np.full(PAD, FILL, np.uint8)])


def run(lib, case: Case, inputs=None, to_device=None, from_device=None):
    """Run every setup of the case, each on fresh buffers; returns (the output buffer after each run with its PAD bytes
    on either side, kernel name of the last run). With to_device / from_device (GPU tier) the tensors are device
    buffers offset by the case's misalignment, unless the case asks for host pointers."""
    st, op = create(lib, case)
    if st != 0:
        raise RuntimeError(f"{case.name}: create -> {st!r}")
    outs, kname = [], None
    device = to_device is not None and not case.host
    try:
        for k, n in enumerate(case.batches()):
            x = input_tensor(case, k) if inputs is None else inputs[k]
            in_place = case.in_place_at(k)
            si, so = case.strides_at(k)
            hx = _padded(x)
            hy = hx if in_place else _padded(output_tensor(case, k))
            if device:
                bx = to_device(hx, case.misalign_in)
                by = bx if in_place else to_device(hy, case.misalign_out)
            else:
                bx, by = hx, hy
            st = lib.setup_softargmax_nc_q8_status(op, n, bx[PAD:], si, by[PAD:], so)
            if st != 0:
                raise RuntimeError(f"{case.name}: setup {k} (batch {n}) -> {st!r}")
            lib.run_operator(op)
            outs.append(from_device(by)[:hy.size].copy() if device else by.copy())
        kname = lib.operator_kernel(op) if hasattr(lib, "operator_kernel") else None
    finally:
        lib.delete_operator(op)
    return outs, kname


def run_reference(reference, case: Case, inputs=None) -> List[np.ndarray]:
    """the compiled reference on the case's tensors (host), behind the fence: raises ZeroSumRow, before any call into
    the reference, if a row's table sum is 0 modulo 2^32 or the case is marked as holding such rows"""
    if case.zero_sum:
        raise ZeroSumRow(f"{case.name} is marked zero_sum")
    inputs = [input_tensor(case, k) for k in range(len(case.batches()))] if inputs is None else inputs
    for k, x in enumerate(inputs):
        zero = np.flatnonzero(row_sums(case, x, k) == 0)
        if zero.size:
            raise ZeroSumRow(f"{case.name}: setup {k}, rows {zero[:4]} have a table sum of 0 modulo 2^32")
    return run(reference, case, inputs=inputs)[0]


def expected(case: Case, inputs=None) -> List[np.ndarray]:
    """the model's output buffer of every setup, with the PAD bytes on either side"""
    inputs = [input_tensor(case, k) for k in range(len(case.batches()))] if inputs is None else inputs
    return [_padded(model(case, x, k)[0]) for k, x in enumerate(inputs)]


def _assert_equal(case: Case, what: str, got: List[np.ndarray], want: List[np.ndarray]) -> None:
    assert len(got) == len(want), case.name
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size, (case.name, g.size, w.size)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{case.name} (setup {i}, {what}): {bad.size} bytes differ, first at {bad[:4] - PAD} "
                                 f"(relative to the tensor): got {g[bad[:4]]}, want {w[bad[:4]]}")


def check_model(reference, case: Case) -> None:
    """CPU tier: the model against the compiled reference, byte for byte"""
    inputs = [input_tensor(case, k) for k in range(len(case.batches()))]
    _assert_equal(case, "model against the compiled reference", expected(case, inputs), run_reference(reference, case, inputs))


def check(qnnp, reference, case: Case, to_device, from_device: Optional[object]) -> str:
    """GPU tier: the case on the product (device buffers, or host buffers where the case says so) must give the bytes of
    the compiled reference (host buffers) -- of the model for a zero_sum case --, FILL in front of, between and behind the
    rows included; returns the kernel name of the last run"""
    inputs = [input_tensor(case, k) for k in range(len(case.batches()))]
    want = expected(case, inputs) if case.zero_sum else run_reference(reference, case, inputs)
    got, kname = run(qnnp, case, inputs=inputs, to_device=to_device, from_device=from_device)
    _assert_equal(case, str(kname), got, want)
    return kname
