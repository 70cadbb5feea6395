"""Cases and drivers for the byte lookup-table operators: sigmoid (qnnp_*_sigmoid_nc_q8), leaky ReLU
(qnnp_*_leaky_relu_nc_q8) and the product's table operator under both (qnnp_gfx950_*_lut_nc_x8).

Case lists restate the parameters of the reference's operator tests: test/sigmoid.cc (18 tests) and test/leaky-relu.cc
(13 tests), loop for loop (the float loops in float32, as the C++ runs them), with the testers' defaults
(test/sigmoid-operator-tester.h: input 0.75 / 121, output 1/256 / 0; test/leaky-relu-operator-tester.h: slope 0.5, input
1.25 / 121, output 0.75 / 133; both: batch 1, strides = the channel count, qmin 0, qmax 255). The testers run each case
for a few iterations of fresh random input; here each case runs once, on input seeded by its name.

The truth is the COMPILED REFERENCE on the host. Its table for any create arguments is what it answers on the identity
input arange(256) (reference_table); numpy never builds a table, it only applies one (table[x]) and keeps the FILL bytes
between strided pixels. A sigmoid or leaky ReLU case is also run on the compiled reference with the case's own
tensors. The "table" kind is the product-only operator: its table is a fixed random PERMUTATION of 0..255, so every
wrong index changes a byte (sigmoid tables saturate: a lookup at a neighbouring index can go unseen there).

Beyond the reference's lists (extra_cases): the head and tail of every piece width, flat tensors of one pixel with wide
strides, strided rows of each piece width (adjoining rows that share an aligned piece among them), more than one sweep of
each kernel's loop, in place, host pointers, re-setup.

Input tensors of 256 bytes or more hold every byte value; shorter ones hold distinct values.
Every output buffer starts filled with FILL; the bytes between strided pixels must come back as FILL.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import List

import numpy as np

FILL = 0xA5

# One pass of a flat kernel's grid-stride loop on the MI355X: 256 compute units x 16 workgroups x 256 lanes, one piece
# each (hip/x8lut.hip). tests/test_gpu_lut.py checks the device against it.
FLAT_PASS_PIECES = 256 * 16 * 256
# Row groups one pass of a row kernel's loop covers (gridDim.y)
ROWS_PASS_GROUPS = 65535


def _seed(name: str) -> int:
    return 0x1A7 ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class LutCase:
    kind: str                 # "sigmoid" | "leaky" | "table"
    name: str
    batch: int
    channels: int
    in_stride: int = 0        # 0: the channel count
    out_stride: int = 0
    qmin: int = 0
    qmax: int = 255
    input_scale: float = 0.0  # 0: the tester's default (sigmoid 0.75, leaky ReLU 1.25)
    input_zero_point: int = 121
    slope: float = 0.5        # leaky ReLU
    output_scale: float = 0.75
    output_zero_point: int = 133
    table_seed: int = 1       # table: which permutation
    next_batch: int = 0       # a second setup on new buffers with this batch (0: none)
    misalign_in: int = 0      # GPU tier: device base pointer offsets (bytes)
    misalign_out: int = 0
    host: bool = False        # GPU tier: host pointers (the staged path)
    in_place: bool = False    # output is the input tensor (equal strides)

    @property
    def strides(self):
        si = self.in_stride or self.channels
        return (si, si if self.in_place else (self.out_stride or self.channels))

    def batches(self):
        return [self.batch] + ([self.next_batch] if self.next_batch else [])

    def create_args(self):
        """the arguments of the operator's create after `channels`"""
        if self.kind == "sigmoid":
            return (self.input_zero_point, self.input_scale or 0.75, 0, 1.0 / 256.0, self.qmin, self.qmax)
        if self.kind == "leaky":
            return (self.slope, self.input_zero_point, self.input_scale or 1.25, self.output_zero_point,
                    self.output_scale, self.qmin, self.qmax)
        return (permutation(self.table_seed),)


def permutation(seed: int) -> np.ndarray:
    """a fixed random permutation of 0..255"""
    return np.random.default_rng(0xB17E + seed).permutation(256).astype(np.uint8)


def _float_loop(start, stop, factor):
    """for (float v = start; v < stop; v *= factor), in float32"""
    v, stop, factor = np.float32(start), np.float32(stop), np.float32(factor)
    out = []
    while v < stop:
        out.append(float(v))
        v = np.float32(v * factor)
    return out


ZERO_POINTS = list(range(0, 256, 51))
CHANNELS_15 = list(range(1, 100, 15))


# ---- the reference's test lists (test/sigmoid.cc, test/leaky-relu.cc), loop for loop ------------------------------

def _reference_sigmoid_tests(add):
    scales = _float_loop(1.0e-2, 1.0e+2, 10.0)
    add("zero_batch", batch=0, channels=8)
    for batch, prefix, strides in ((1, "unit_batch", {}), (3, "small_batch", {}),
                                   (3, "strided_batch", dict(in_stride=129, out_stride=117))):
        for c in CHANNELS_15:
            add(prefix, batch=batch, channels=c, **strides)
        if prefix == "small_batch":
            for c in CHANNELS_15:
                add("small_batch_with_input_stride", batch=3, channels=c, in_stride=129)
            for c in CHANNELS_15:
                add("small_batch_with_output_stride", batch=3, channels=c, out_stride=117)
        for c in CHANNELS_15:
            add(f"{prefix}_with_qmin", batch=batch, channels=c, qmin=128, **strides)
        for c in CHANNELS_15:
            add(f"{prefix}_with_qmax", batch=batch, channels=c, qmax=128, **strides)
        for c in CHANNELS_15:
            for s in scales:
                add(f"{prefix}_with_input_scale", batch=batch, channels=c, input_scale=s, **strides)
        for c in CHANNELS_15:
            for zp in ZERO_POINTS:
                add(f"{prefix}_with_input_zero_point", batch=batch, channels=c, input_zero_point=zp, **strides)


def _reference_leaky_relu_tests(add):
    pi = 3.14159265
    add("zero_batch", batch=0, channels=2)
    for c in range(1, 100):
        add("unit_batch", batch=1, channels=c)
    for c in CHANNELS_15:
        add("unit_batch_with_qmin", batch=1, channels=c, qmin=128)
    for c in CHANNELS_15:
        add("unit_batch_with_qmax", batch=1, channels=c, qmax=128)
    for c in CHANNELS_15:
        for slope in _float_loop(1.0e-4, 1.0, pi):
            add("unit_batch_with_negative_slope", batch=1, channels=c, slope=slope)
    for c in CHANNELS_15:
        for s in _float_loop(1.0e-2, 1.0e+2, pi):
            add("unit_batch_with_input_scale", batch=1, channels=c, input_scale=s)
    for c in CHANNELS_15:
        for zp in ZERO_POINTS:
            add("unit_batch_with_input_zero_point", batch=1, channels=c, input_zero_point=zp)
    for c in CHANNELS_15:
        for s in _float_loop(1.0e-2, 1.0e+2, pi):
            add("unit_batch_with_output_scale", batch=1, channels=c, output_scale=s)
    for c in CHANNELS_15:
        for zp in ZERO_POINTS:
            add("unit_batch_with_output_zero_point", batch=1, channels=c, output_zero_point=zp)
    for c in range(1, 100):
        add("small_batch", batch=3, channels=c)
    for c in CHANNELS_15:
        add("small_batch_with_input_stride", batch=3, channels=c, in_stride=129)
    for c in CHANNELS_15:
        add("small_batch_with_output_stride", batch=3, channels=c, out_stride=117)
    for c in CHANNELS_15:
        add("small_batch_with_input_and_output_stride", batch=3, channels=c, in_stride=129, out_stride=117)


def _collect(kind: str, fn) -> List[LutCase]:
    out: List[LutCase] = []
    counts = {}

    def add(test, **kw):
        k = counts.get(test, 0)
        counts[test] = k + 1
        out.append(LutCase(kind, f"{kind}/{test}/{k}", **kw))
    fn(add)
    return out


def reference_sigmoid_cases() -> List[LutCase]:
    return _collect("sigmoid", _reference_sigmoid_tests)


def reference_leaky_relu_cases() -> List[LutCase]:
    return _collect("leaky", _reference_leaky_relu_tests)


# ---- beyond the reference's lists ---------------------------------------------------------------------------------

# input - output (mod 16) -> the piece width the kernels take when the strides allow it too
DELTAS = {16: 0, 4: 4, 1: 1}


def flat_edge_cases(width: int) -> List[LutCase]:
    """flat tensors of 1 .. 49 bytes with the output misaligned by 0 .. 15 and input - output = DELTAS[width] (mod 16):
    every head and tail a piece of `width` bytes can have"""
    d = DELTAS[width]
    return [LutCase("table", f"table/x/flat_x{width}/n{n}_m{mo}", 1, n, misalign_in=mo + d, misalign_out=mo,
                    table_seed=1 + (n + mo) % 2)
            for n in range(1, 50) for mo in range(16)]


def rows_cases() -> List[LutCase]:
    out = []
    for c in (1, 7, 24, 33, 100):
        # (input stride, output stride): differences of 16, 4 and 3 bytes; the last three have adjoining output rows
        # (output stride == channels), where the tail of one row and the head of the next share an aligned piece
        for w, si, so in ((16, c + 32, c + 16), (4, c + 8, c + 4), (1, c + 5, c + 2), (16, c + 16, c), (4, c + 4, c),
                          (1, c + 3, c)):
            for mi, mo in ((0, 0), (3, 3)) if w == 16 else ((0, 0),):
                out.append(LutCase("table", f"table/x/rows_x{w}/c{c}_s{si}_{so}_m{mi}_{mo}", 29, c, in_stride=si,
                                   out_stride=so, misalign_in=mi, misalign_out=mo, table_seed=2))
        out.append(LutCase("sigmoid", f"sigmoid/x/rows/c{c}", 29, c, in_stride=c + 5, out_stride=c + 2, qmin=3, qmax=250))
        out.append(LutCase("leaky", f"leaky/x/rows_adjoining/c{c}", 29, c, in_stride=c + 16, slope=0.1))
    return out


def sweep_cases() -> List[LutCase]:
    """more than one pass of each kernel's loop"""
    p = FLAT_PASS_PIECES
    return [
        # flat: 128 x 112 x 112 x 24 = 38.5 MB, 2.3 passes of 16-byte pieces
        LutCase("sigmoid", "sigmoid/x/sweep_flat_x16", 128 * 112 * 112, 24),
        LutCase("table", "table/x/sweep_flat_x4", 1, 4 * p + 4 * p // 4 + 3, misalign_in=4),
        LutCase("table", "table/x/sweep_flat_x1", 1, p + p // 4 + 1, misalign_in=1),
        # rows: 3 channels are 3 items of 256 lanes, 85 rows per workgroup; a few rows past gridDim.y workgroups
        LutCase("table", "table/x/sweep_rows_x1", ROWS_PASS_GROUPS * 85 + 7, 3, in_stride=5, out_stride=4),
    ]


def extra_cases() -> List[LutCase]:
    out = rows_cases()
    out += [
        # one pixel: flat whatever the strides say (reference operator-run.c:1024)
        LutCase("table", "table/x/one_pixel_wide_strides", 1, 40, in_stride=4096, out_stride=8191),
        LutCase("sigmoid", "sigmoid/x/one_pixel_wide_strides", 1, 77, in_stride=1 << 20, out_stride=(1 << 20) + 1,
                misalign_in=2, misalign_out=2),
        LutCase("leaky", "leaky/x/wide_strides", 7, 50, in_stride=4097, out_stride=8192),
        LutCase("sigmoid", "sigmoid/x/flat_many_blocks", 1000, 96, input_scale=0.05, input_zero_point=128),
        LutCase("leaky", "leaky/x/flat_many_blocks_misaligned", 3, 1 << 18, misalign_in=5, misalign_out=5),
    ]
    for kind in ("table", "sigmoid", "leaky"):
        k = f"{kind}/x"
        for c in (1, 16, 17, 100):
            for stride, mis in ((0, 0), (0, 3), (c + 7, 0), (c + 7, 1), (c + 16, 0)):
                out.append(LutCase(kind, f"{k}/c{c}_in_place_s{stride}_m{mis}", 29, c, in_stride=stride, in_place=True,
                                   misalign_in=mis))
        out += [
            LutCase(kind, f"{k}/host_pointers", 13, 40, host=True),
            LutCase(kind, f"{k}/host_pointers_strided", 13, 40, in_stride=45, out_stride=41, host=True),
            LutCase(kind, f"{k}/host_in_place_strided", 13, 40, in_stride=45, host=True, in_place=True),
            LutCase(kind, f"{k}/resetup_larger", 7, 24, next_batch=31),
            LutCase(kind, f"{k}/resetup_in_place", 31, 24, in_stride=30, next_batch=5, in_place=True),
        ]
    return out


def all_cases() -> List[LutCase]:
    return (reference_sigmoid_cases() + reference_leaky_relu_cases() + extra_cases() + sweep_cases() +
            [c for w in DELTAS for c in flat_edge_cases(w)])


# ---- tensors ------------------------------------------------------------------------------------------------------
def _span(batch: int, stride: int, channels: int) -> int:
    return (batch - 1) * stride + channels if batch else 0


def input_tensor(case: LutCase, batch: int = None) -> np.ndarray:
    """the input of the setup with `batch` pixels (default: the first); the re-setup gets fresh bytes. 256 bytes or
    more: random bytes with every value 0..255 at 256 places spread over the tensor; fewer: distinct values"""
    batch = case.batch if batch is None else batch
    rng = np.random.default_rng(_seed(f"{case.name}/{batch}"))
    n = _span(batch, case.strides[0], case.channels)
    if n < 256:
        return rng.permutation(256).astype(np.uint8)[:n]
    x = rng.integers(0, 256, size=n, dtype=np.uint8)
    x[np.arange(256) * (n // 256) + rng.integers(0, n // 256, size=256)] = rng.permutation(256).astype(np.uint8)
    return x


def output_tensor(case: LutCase, batch: int = None) -> np.ndarray:
    batch = case.batch if batch is None else batch
    return np.full(_span(batch, case.strides[1], case.channels), FILL, dtype=np.uint8)


def _pixels(buf: np.ndarray, n: int, stride: int, channels: int) -> np.ndarray:
    """the [n][channels] view of the pixels of a strided tensor (no copy)"""
    return np.lib.stride_tricks.as_strided(buf, shape=(n, channels), strides=(stride, 1))


def apply_table(case: LutCase, table: np.ndarray, x: np.ndarray, batch: int) -> np.ndarray:
    """the output buffer after one setup + run with `batch` pixels on input x: table[x] per pixel byte, the bytes between
    pixels kept (FILL, or the input's own in place)"""
    si, so = case.strides
    out = x.copy() if case.in_place else output_tensor(case, batch)
    if batch:
        _pixels(out, batch, so, case.channels)[...] = table[_pixels(x, batch, si, case.channels)]
    return out


# ---- drivers ------------------------------------------------------------------------------------------------------
_CREATE = {"sigmoid": "create_sigmoid_nc_q8_status", "leaky": "create_leaky_relu_nc_q8_status",
           "table": "create_lut_nc_x8_status"}
_SETUP = {"sigmoid": "setup_sigmoid_nc_q8_status", "leaky": "setup_leaky_relu_nc_q8_status",
          "table": "setup_lut_nc_x8_status"}


def create(lib, case: LutCase, channels: int = None):
    return getattr(lib, _CREATE[case.kind])(case.channels if channels is None else channels, *case.create_args())


def setup_status(lib, case: LutCase, op, n, x, y):
    si, so = case.strides
    return getattr(lib, _SETUP[case.kind])(op, n, x, si, y, so)


_TABLES = {}


def reference_table(reference, case: LutCase) -> np.ndarray:
    """the 256-byte table behind the case's operator: the COMPILED REFERENCE's answer on the identity input (the
    permutation itself for the product-only table operator)"""
    if case.kind == "table":
        return permutation(case.table_seed)
    key = (case.kind,) + case.create_args()
    if key not in _TABLES:
        st, op = create(reference, case, channels=256)
        if st != 0:
            raise RuntimeError(f"{case.name}: reference create -> {st!r}")
        try:
            x, y = np.arange(256, dtype=np.uint8), np.zeros(256, np.uint8)
            st = getattr(reference, _SETUP[case.kind])(op, 1, x, 256, y, 256)
            assert st == 0, st
            reference.run_operator(op)
        finally:
            reference.delete_operator(op)
        y.setflags(write=False)
        _TABLES[key] = y
    return _TABLES[key]


def run(lib, case: LutCase, to_device=None, from_device=None):
    """Run every setup of the case, each on fresh buffers; returns (the output buffer after each run, kernel name of the
    last run). With to_device / from_device (GPU tier) the tensors are device buffers offset by the case's
    misalignment, unless the case asks for host pointers."""
    st, op = create(lib, case)
    if st != 0:
        raise RuntimeError(f"{case.name}: create -> {st!r}")
    outs, kname = [], None
    one = np.zeros(1, np.uint8)
    device = to_device is not None and not case.host
    try:
        for n in case.batches():
            x = input_tensor(case, n)
            out = x.copy() if case.in_place else output_tensor(case, n)
            if device:
                d_x = to_device(x if x.size else one, case.misalign_in)
                d_y = d_x if case.in_place else to_device(out if out.size else one, case.misalign_out)
            else:
                d_x = x.copy() if x.size else one
                d_y = d_x if case.in_place else (out if out.size else one)
            st = setup_status(lib, case, op, n, d_x, d_y)
            if st != 0:
                raise RuntimeError(f"{case.name}: setup batch {n} -> {st!r}")
            lib.run_operator(op)
            if device:
                outs.append(from_device(d_y)[:out.size].copy())
            else:
                outs.append((d_y if out.size else out)[:out.size].copy())
        kname = lib.operator_kernel(op) if hasattr(lib, "operator_kernel") else None
    finally:
        lib.delete_operator(op)
    return outs, kname


def expected(reference, case: LutCase) -> List[np.ndarray]:
    """the output buffer of every setup of the case: the reference's table applied by numpy"""
    table = reference_table(reference, case)
    return [apply_table(case, table, input_tensor(case, b), b) for b in case.batches()]


def check_reference(reference, case: LutCase, want=None):
    """the compiled reference on the case's own tensors (host) against its table applied by numpy"""
    want = expected(reference, case) if want is None else want
    if case.kind != "table":
        ref_out, _ = run(reference, case)
        assert len(ref_out) == len(want), case.name
        for r, w in zip(ref_out, want):
            assert np.array_equal(r, w), f"{case.name}: the reference's table applied by numpy vs the compiled reference"
    return want


def check(qnnp, reference, case: LutCase, to_device, from_device):
    """GPU tier: the case on the product (device buffers, or host buffers where the case says so) must give the bytes
    of the compiled reference (host buffers), FILL between strided pixels included; returns the kernel name of the last
    run"""
    want = check_reference(reference, case)
    got, kname = run(qnnp, case, to_device=to_device, from_device=from_device)
    assert len(got) == len(want), case.name
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{case.name} (setup {i}, {kname}): {bad.size} bytes differ, first at {bad[:4]}: "
                                 f"got {g[bad[:4]]}, want {w[bad[:4]]}")
    return kname
