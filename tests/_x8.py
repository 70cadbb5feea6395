"""Cases, a numpy model and drivers for channel shuffle (qnnp_*_channel_shuffle_nc_x8) and clamp (qnnp_*_clamp_nc_u8).

Case lists restate the parameters of the reference's operator tests: test/channel-shuffle.cc (21 tests) and
test/clamp.cc (9 tests), loop for loop, with the testers' defaults (test/channel-shuffle-operator-tester.h,
test/clamp-operator-tester.h: batch 1, strides = the channel count, qmin 0, qmax 255). The testers run each case for a
few iterations of fresh random input; here each case runs once, on input seeded by its name. The expectation is
bit-exact: the numpy model below, checked against the compiled reference by the CPU tier.

Beyond those lists: base pointers offset by 1-3 bytes on input and output, wide strides, large G * gc (the LDS
kernel's limit and the gather kernel past it), clamp in place, host-pointer tensors, re-setup with a new batch and new
buffers, and the ShuffleNet shapes of the reference's convolution bench lists (tests/golden/reference_bench_shapes.json)
at batch 1 and 128.

Every output buffer starts filled with FILL; the bytes between strided pixels must come back as FILL.
"""
from __future__ import annotations

import json
import os
import zlib
from dataclasses import dataclass
from typing import List

import numpy as np

FILL = 0xA5


def _seed(name: str) -> int:
    return 0x5F0C ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class X8Case:
    kind: str                 # "shuffle" | "clamp"
    name: str
    batch: int
    groups: int = 0           # channel shuffle
    group_channels: int = 0
    clamp_channels: int = 0   # clamp
    in_stride: int = 0        # 0: the channel count
    out_stride: int = 0
    qmin: int = 0             # clamp
    qmax: int = 255
    next_batch: int = 0       # a second setup on new buffers with this batch (0: none)
    misalign_in: int = 0      # GPU tier: device base pointer offsets (bytes)
    misalign_out: int = 0
    host: bool = False        # GPU tier: host pointers (the staged path)
    in_place: bool = False    # clamp: output is the input tensor (equal strides)

    @property
    def channels(self) -> int:
        return self.groups * self.group_channels if self.kind == "shuffle" else self.clamp_channels

    @property
    def strides(self):
        si = self.in_stride or self.channels
        return (si, si if self.in_place else (self.out_stride or self.channels))

    def batches(self):
        return [self.batch] + ([self.next_batch] if self.next_batch else [])


# ---- the reference's test lists (test/channel-shuffle.cc, test/clamp.cc), loop for loop ---------------------------

def _reference_channel_shuffle_tests(add):
    add("zero_batch", batch=0, groups=2, group_channels=4)
    for batch, suffix in ((1, "unit_batch"), (3, "small_batch")):
        for groups, word in ((2, "two"), (3, "three"), (4, "four")):
            for gc in range(1, 100, 15):
                add(f"{word}_groups_{suffix}", batch=batch, groups=groups, group_channels=gc)
        for groups in range(5, 12, 3):
            for gc in range(1, 100, 15):
                add(f"many_groups_{suffix}", batch=batch, groups=groups, group_channels=gc)
    for what, strides, many in (("input_stride", (511, 0), (1007, 0)), ("output_stride", (0, 513), (0, 1111)),
                                ("input_and_output_stride", (511, 513), (1007, 1111))):
        for groups, word in ((2, "two"), (3, "three"), (4, "four")):
            for gc in range(1, 100, 15):
                add(f"{word}_groups_small_batch_with_{what}", batch=3, groups=groups, group_channels=gc,
                    in_stride=strides[0], out_stride=strides[1])
        for groups in range(5, 12, 3):
            for gc in range(1, 100, 15):
                add(f"many_groups_small_batch_with_{what}", batch=3, groups=groups, group_channels=gc,
                    in_stride=many[0], out_stride=many[1])


def _reference_clamp_tests(add):
    add("zero_batch", batch=0, clamp_channels=2)
    for c in range(1, 100):
        add("unit_batch", batch=1, clamp_channels=c)
    for c in range(1, 100, 15):
        for qmin in range(1, 255):
            add("unit_batch_with_qmin", batch=1, clamp_channels=c, qmin=qmin)
    for c in range(1, 100, 15):
        for qmax in range(1, 255):
            add("unit_batch_with_qmax", batch=1, clamp_channels=c, qmax=qmax)
    for c in range(1, 100):
        add("small_batch", batch=3, clamp_channels=c)
    for c in range(1, 100, 15):
        add("small_batch_with_input_stride", batch=3, clamp_channels=c, in_stride=129)
    for c in range(1, 100, 15):
        add("small_batch_with_output_stride", batch=3, clamp_channels=c, out_stride=117)
    for c in range(1, 100, 15):
        add("small_batch_with_input_and_output_stride", batch=3, clamp_channels=c, in_stride=129, out_stride=117)
    for c in range(1, 100, 15):
        add("qmin_and_qmax_equal_uint8_max", batch=3, clamp_channels=c, qmin=255, qmax=255)


def _collect(kind: str, fn) -> List[X8Case]:
    out: List[X8Case] = []
    counts = {}

    def add(test, **kw):
        k = counts.get(test, 0)
        counts[test] = k + 1
        out.append(X8Case(kind, f"{kind}/{test}/{k}", **kw))
    fn(add)
    return out


def reference_shuffle_cases() -> List[X8Case]:
    return _collect("shuffle", _reference_channel_shuffle_tests)


def reference_clamp_cases() -> List[X8Case]:
    return _collect("clamp", _reference_clamp_tests)


# ---- ShuffleNet shapes of the reference's convolution bench lists ------------------------------------------------
_SHAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_bench_shapes.json")


def shufflenet_shuffles():
    """(list, groups, group_channels, H) of every channel shuffle of the bench lists' ShuffleNet units: v1 shuffles
    after the grouped 1x1 that feeds a depthwise layer (groups = its G, group_channels = its output channels per
    group); v2 shuffles two branches of the branch width (the output channels of the branch's square 1x1 layers)."""
    lists = json.load(open(_SHAPES))["lists"]
    out = set()
    for name, rows in lists.items():
        for i, (h, _w, kh, _kw, _s, _d, g, gci, gco) in enumerate(rows):
            if name.startswith("ShuffleNetV1") and kh == 1 and g > 1 and i + 1 < len(rows) and rows[i + 1][7:9] == [1, 1]:
                out.add((name, g, gco, h))
            if name.startswith("ShuffleNetV2") and kh == 1 and g == 1 and gci == gco:
                out.add((name, 2, gco, h))
    return sorted(out)


# ReLU / ReLU6-style clamps at the activation sizes of those networks: (C, H)
CLAMP_BENCH = [(24, 112), (64, 56), (200, 28), (240, 28), (272, 28), (384, 28), (116, 28), (176, 28), (400, 14),
               (232, 14), (800, 7), (464, 7), (1024, 7)]


def bench_cases(batch: int) -> List[X8Case]:
    out = [X8Case("shuffle", f"shuffle/bench/{n}_g{g}_gc{gc}_{h}x{h}/b{batch}", batch * h * h, g, gc)
           for n, g, gc, h in shufflenet_shuffles()]
    out += [X8Case("clamp", f"clamp/bench/c{c}_{h}x{h}/b{batch}", batch * h * h, clamp_channels=c, qmin=0, qmax=127)
            for c, h in CLAMP_BENCH]
    return out


def extra_cases() -> List[X8Case]:
    out: List[X8Case] = []
    s = "shuffle/x"
    # one case per kernel path and alignment class
    for g, gc in ((2, 16), (2, 64), (2, 8), (2, 100), (4, 16), (4, 68), (4, 32), (2, 25), (3, 20), (8, 12), (5, 7),
                  (2, 58), (2, 122), (11, 3)):
        out.append(X8Case("shuffle", f"{s}/g{g}_gc{gc}", 37, g, gc))
        for mi, mo in ((1, 0), (0, 2), (3, 3), (4, 0), (0, 4), (2, 1)):
            out.append(X8Case("shuffle", f"{s}/g{g}_gc{gc}_misaligned_{mi}_{mo}", 37, g, gc, misalign_in=mi,
                              misalign_out=mo))
        out.append(X8Case("shuffle", f"{s}/g{g}_gc{gc}_strides", 19, g, gc, in_stride=g * gc + 3,
                          out_stride=g * gc + 8))
    out += [
        X8Case("shuffle", f"{s}/wide_strides", 5, 3, 40, in_stride=4096, out_stride=8191),
        X8Case("shuffle", f"{s}/wide_strides_aligned", 5, 2, 64, in_stride=4096, out_stride=1024),
        X8Case("shuffle", f"{s}/lds_longest_row", 3, 8, 4096),            # G * gc = 32768: the lds kernel's limit
        X8Case("shuffle", f"{s}/lds_longest_row_misaligned", 3, 8, 4096, misalign_in=3, misalign_out=1),
        X8Case("shuffle", f"{s}/gather", 3, 3, 11000),                     # 33000 channels: the gather kernel
        X8Case("shuffle", f"{s}/gather_strided", 3, 7, 5001, in_stride=35011, out_stride=35100, misalign_out=1),
        X8Case("shuffle", f"{s}/register_long_row", 3, 2, 20000),          # 40000 channels, register path
        X8Case("shuffle", f"{s}/many_groups_one_channel", 9, 1000, 1),
        X8Case("shuffle", f"{s}/host_pointers", 13, 3, 20, host=True),
        X8Case("shuffle", f"{s}/host_pointers_strided", 13, 2, 24, in_stride=50, out_stride=49, host=True),
        X8Case("shuffle", f"{s}/resetup_larger", 7, 4, 17, next_batch=23),
        X8Case("shuffle", f"{s}/resetup_smaller_strided", 23, 2, 64, in_stride=130, out_stride=129, next_batch=4),
    ]
    c = "clamp/x"
    for ch in (1, 3, 4, 15, 16, 17, 64, 100, 1000):
        out.append(X8Case("clamp", f"{c}/c{ch}", 29, clamp_channels=ch, qmin=30, qmax=200))
        for mi, mo in ((1, 0), (0, 3), (2, 2), (4, 0), (8, 0), (1, 5)):
            out.append(X8Case("clamp", f"{c}/c{ch}_misaligned_{mi}_{mo}", 29, clamp_channels=ch, qmin=30, qmax=200,
                              misalign_in=mi, misalign_out=mo))
        out.append(X8Case("clamp", f"{c}/c{ch}_strides", 29, clamp_channels=ch, in_stride=ch + 16, out_stride=ch + 32,
                          qmin=30, qmax=200))
        out.append(X8Case("clamp", f"{c}/c{ch}_strides_odd", 29, clamp_channels=ch, in_stride=ch + 5,
                          out_stride=ch + 2, qmin=30, qmax=200))
        for stride, mis in ((0, 0), (0, 3), (ch + 7, 0), (ch + 7, 1)):
            out.append(X8Case("clamp", f"{c}/c{ch}_in_place_s{stride}_m{mis}", 29, clamp_channels=ch, in_stride=stride,
                              qmin=30, qmax=200, in_place=True, misalign_in=mis))
    out += [
        X8Case("clamp", f"{c}/relu6_like", 1000, clamp_channels=96, qmin=0, qmax=6),
        X8Case("clamp", f"{c}/identity", 100, clamp_channels=33, qmin=0, qmax=255),
        X8Case("clamp", f"{c}/wide_strides", 7, clamp_channels=50, in_stride=4097, out_stride=8192, qmin=1, qmax=254),
        X8Case("clamp", f"{c}/large_flat", 3, clamp_channels=1 << 20, qmin=7, qmax=99, misalign_in=5, misalign_out=5),
        X8Case("clamp", f"{c}/host_pointers", 13, clamp_channels=40, qmin=20, qmax=100, host=True),
        X8Case("clamp", f"{c}/host_pointers_strided", 13, clamp_channels=40, in_stride=45, out_stride=41, qmin=20,
               qmax=100, host=True),
        X8Case("clamp", f"{c}/host_in_place_strided", 13, clamp_channels=40, in_stride=45, qmin=20, qmax=100,
               host=True, in_place=True),
        X8Case("clamp", f"{c}/resetup_larger", 7, clamp_channels=24, qmin=10, qmax=20, next_batch=31),
        X8Case("clamp", f"{c}/resetup_in_place", 31, clamp_channels=24, in_stride=30, qmin=10, qmax=20, next_batch=5,
               in_place=True),
    ]
    return out


def all_cases() -> List[X8Case]:
    return reference_shuffle_cases() + reference_clamp_cases() + extra_cases() + bench_cases(1)


# ---- tensors ----------------------------------------------------------------------------------------------------
def _span(batch: int, stride: int, channels: int) -> int:
    return (batch - 1) * stride + channels if batch else 0


def input_tensor(case: X8Case, batch: int = None) -> np.ndarray:
    """the input of the setup with `batch` pixels (default: the first); the re-setup gets fresh bytes"""
    batch = case.batch if batch is None else batch
    rng = np.random.default_rng(_seed(f"{case.name}/{batch}"))
    return rng.integers(0, 256, size=_span(batch, case.strides[0], case.channels), dtype=np.uint8)


def output_tensor(case: X8Case, batch: int = None) -> np.ndarray:
    batch = case.batch if batch is None else batch
    return np.full(_span(batch, case.strides[1], case.channels), FILL, dtype=np.uint8)


# ---- numpy model ------------------------------------------------------------------------------------------------
def _rows(n: int, stride: int, channels: int) -> np.ndarray:
    return np.arange(n, dtype=np.int64)[:, None] * stride + np.arange(channels, dtype=np.int64)[None, :]


def channel_shuffle(x: np.ndarray, n: int, groups: int, group_channels: int) -> np.ndarray:
    """[n][groups][group_channels] -> [n][group_channels][groups] (reference src/x8zip/xm-sse2.c)"""
    return x.reshape(n, groups, group_channels).transpose(0, 2, 1).reshape(n, groups * group_channels)


def expected_one(case: X8Case, x: np.ndarray, batch: int) -> np.ndarray:
    """the output buffer after one setup + run with `batch` pixels on input x (the input buffer itself, in place)"""
    si, so = case.strides
    c = case.channels
    out = x.copy() if case.in_place else output_tensor(case, batch)
    if batch:
        px = x[_rows(batch, si, c)]
        if case.kind == "shuffle":
            y = channel_shuffle(px, batch, case.groups, case.group_channels)
        else:
            y = np.minimum(np.maximum(px, np.uint8(case.qmin)), np.uint8(case.qmax))   # reference u8clamp sse2
        out[_rows(batch, so, c)] = y
    return out


def expected(case: X8Case) -> List[np.ndarray]:
    return [expected_one(case, input_tensor(case, b), b) for b in case.batches()]


# ---- drivers ----------------------------------------------------------------------------------------------------
def create(lib, case: X8Case):
    if case.kind == "shuffle":
        return lib.create_channel_shuffle_nc_x8_status(case.groups, case.group_channels, 0)
    return lib.create_clamp_nc_u8_status(case.clamp_channels, case.qmin, case.qmax, 0)


def setup_status(lib, case: X8Case, op, n, x, y):
    si, so = case.strides
    fn = lib.setup_channel_shuffle_nc_x8_status if case.kind == "shuffle" else lib.setup_clamp_nc_u8_status
    return fn(op, n, x, si, y, so)


def run(lib, case: X8Case, to_device=None, from_device=None):
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
                d_x = x if x.size else one
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


def check(qnnp, reference, case: X8Case, to_device, from_device):
    """GPU tier: the case on the product (device buffers, or host buffers where the case says so) must give the bytes
    of the compiled reference (host buffers) and of the numpy model; returns the kernel name of the last run"""
    want = expected(case)
    ref_out, _ = run(reference, case)
    for r, w in zip(ref_out, want):
        assert np.array_equal(r, w), f"{case.name}: numpy model vs compiled reference"
    got, kname = run(qnnp, case, to_device=to_device, from_device=from_device)
    assert len(got) == len(want), case.name
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{case.name} (setup {i}, {kname}): {bad.size} bytes differ, first at {bad[:4]}: "
                                 f"got {g[bad[:4]]}, want {w[bad[:4]]}")
    return kname
