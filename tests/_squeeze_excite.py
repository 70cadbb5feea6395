"""Cases and drivers for the fused squeeze-and-excite operator (qnnp_gfx950_{create,setup}_squeeze_excite).

No reference operator exists, so the expectation of a block is the oracle's, stage by stage on the CPU, exactly as part 6
of tests/test_multiply_gpu.py builds it: oracle.o1.global_average_pooling_q8 -> fc_expected (o1.gemm_acc +
o1.q31_requantize, the ReLU as output_min) -> fc_expected -> the gate's table -> _multiply.expected. A Block computes it
once; every run compares bytes with it, the bytes between strided rows included.

The pooling case takes its pixel count from the kernel's constants (hip/q8segate.hip kSeThreads and kSePoolUnroll,
restated here and held to the source by tests/test_squeeze_excite_host.py).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

import _multiply as mul
from _cases import FcCase
from _runner import fc_expected
from oracle import o1

FILL = mul.FILL
SE_THREADS = 1024        # hip/q8segate.hip kSeThreads: lanes of the one workgroup of an image
SE_POOL_UNROLL = 4       # hip/q8segate.hip kSePoolUnroll: pixels in flight per lane
KERNELS = {1: "q8_se_gate_pool", 2: "q8_se_gate"}
AUTO_IN_FRONT = (1024, 196)       # squeeze-excite.c: above this many channels, from this many pixels per image on


def auto_kernel(case) -> str:
    """what "se_kernel" 0 takes for the case"""
    in_front = case.c > AUTO_IN_FRONT[0] and case.pixels >= AUTO_IN_FRONT[1]
    return KERNELS[2 if in_front else 1]


def _seed(name: str) -> int:
    return 0x5E6A ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class Case:
    name: str
    batch: int
    pixels: int
    c: int
    s: int
    kzp1: int = 127            # kernel zero points of the two fully connected layers
    kzp2: int = 127
    x_zp: int = 121
    pool_zp: int = 119
    gate: str = "hardsigmoid"  # | "sigmoid" | "table"
    constant: Optional[int] = None   # every weight and every input byte (the ends of the accumulator range)


# 72 channels are 18 dwords: 32 lanes per pixel slice, 1024 / 32 = 32 slices, 4 * 32 = 128 pixels per pass of the
# unrolled loop -- 2 passes and a remainder of 27 pixels, which is no whole round of the slices either
_POOL_PIXELS = 2 * SE_POOL_UNROLL * (SE_THREADS // 32) + 27

CASES = [
    Case("mobilenet_se", 3, 49, 24, 8),                                   # the block of tests/test_multiply_gpu.py
    Case("degenerate", 2, 1, 1, 1),
    # (input zero points: the pooled row is about pool_zp + 1.25 * (127.5 - x_zp). Where the first kernel zero point is far
    # from 128 it is kept near pool_zp, so that the hidden row's accumulators straddle zero and the ReLU has work to do)
    Case("nothing_aligned", 2, 5, 33, 9, kzp1=128, kzp2=90, x_zp=40),     # crosses a 32-column block, K % 16 != 0
    Case("k_blocks", 2, 50, 130, 40, kzp1=90, kzp2=128, x_zp=128, pool_zp=60, gate="sigmoid"),   # K crosses 64 and 128, five column blocks, S > 32
    Case("b1_196", 1, 196, 72, 24, kzp1=128, kzp2=128, x_zp=215, gate="table"),
    Case("wide", 1, 2, 2052, 516, gate="table"),                         # more than one pass of every per-channel loop
    Case("pool_passes", 2, _POOL_PIXELS, 72, 24, kzp1=90, kzp2=201, x_zp=126, pool_zp=200, gate="sigmoid"),
    # the automatic rule's threshold (squeeze-excite.c): more than 1024 channels AND 196 pixels or more get the pooling
    # launch in front -- both sides of the pixel bound at 1028 channels, and 1024 channels past it
    Case("auto_in_front", 1, 196, 1028, 8, kzp1=128, x_zp=100),
    Case("auto_inside", 1, 195, 1028, 8, kzp1=128, x_zp=100),
    Case("auto_inside_1024", 1, 197, 1024, 8, kzp1=128, x_zp=100),
    # the ends: the row term at its largest in either sign, accumulators at their bound
    Case("kzp0_all255", 2, 5, 33, 9, kzp1=0, kzp2=0, constant=255),
    Case("kzp255_all0", 2, 5, 33, 9, kzp1=255, kzp2=255, constant=0),
    Case("kzp0_all0", 2, 5, 33, 9, kzp1=0, kzp2=0, constant=0, x_zp=200),
    Case("kzp255_all255", 2, 5, 33, 9, kzp1=255, kzp2=255, constant=255, x_zp=7),
]


def sigmoid_table(izp, iscale, qmin=0, qmax=255) -> np.ndarray:
    """sigmoid.c's table (reference src/sigmoid.c:96-110) in numpy float32, one rounding per operation"""
    f = np.float32
    x = f(iscale) * (np.arange(256, dtype=np.int32) - izp).astype(np.float32)
    y = f(256.0) / (f(1.0) + np.exp(-x))
    assert y.dtype == np.float32
    return np.rint(np.minimum(np.maximum(y, f(qmin)), f(qmax))).astype(np.uint8)


class Block:
    """one case: its tensors, its quantization and the oracle's expectation of every stage (dense rows)"""

    def __init__(self, case: Case):
        self.case = case
        batch, pixels, c, s = case.batch, case.pixels, case.c, case.s
        rng = np.random.default_rng(_seed(case.name))
        draw = (lambda shape: rng.integers(0, 256, size=shape, dtype=np.uint8)) if case.constant is None else \
            (lambda shape: np.full(shape, case.constant, np.uint8))
        self.x = draw(batch * pixels * c)
        self.x_scale, self.pool_scale = 0.05, 0.04
        self.pooled = np.full(batch * c, FILL, np.uint8)
        o1.global_average_pooling_q8(batch, pixels, c, case.x_zp, self.x_scale, case.pool_zp, self.pool_scale, 0, 255,
                                     self.x, c, self.pooled, c)
        self.k1, self.k2 = draw((s, c)), draw((c, s))
        self.b1 = rng.integers(-2000, 2001, size=s, dtype=np.int32)
        self.b2 = rng.integers(-2000, 2001, size=c, dtype=np.int32)
        if case.constant is not None:
            self.b1 = self._centred(self.b1, self.pooled.reshape(batch, c), self.k1, case.pool_zp, case.kzp1)
        fc1 = FcCase(case.name + "_fc1", batch, c, s, izp=case.pool_zp, kzp=case.kzp1)
        _, (_, zp1) = fc_expected(fc1, self.pooled, self.k1, self.b1)
        self.fc1 = FcCase(fc1.name, batch, c, s, izp=case.pool_zp, kzp=case.kzp1, qmin=zp1)   # the ReLU: output_min = the zero point
        self.hidden, (self.scale1, self.zp1) = fc_expected(self.fc1, self.pooled, self.k1, self.b1)
        assert self.zp1 == zp1
        if case.constant is not None:
            self.b2 = self._centred(self.b2, self.hidden.reshape(batch, s), self.k2, zp1, case.kzp2)
        self.fc2 = FcCase(case.name + "_fc2", batch, s, c, izp=zp1, kzp=case.kzp2)
        self.excite, (self.scale2, self.zp2) = fc_expected(self.fc2, self.hidden, self.k2, self.b2)
        if case.gate == "hardsigmoid":
            # 0.011 per step keeps x + 3 inside (0, 6) wherever the zero point lies (255 * 0.011 < 3): not saturated
            self.gate_args = (self.zp2, 0.011, 0, 1.0 / 256, 0, 255)
            self.table = mul.hardsigmoid_table(*self.gate_args)
        elif case.gate == "sigmoid":
            # |x| <= 255 * 0.015 = 3.8: sigmoid inside (0.02, 0.98), the table inside (5, 251)
            self.gate_args = (self.zp2, 0.015, 0, 1.0 / 256, 0, 255)
            self.table = sigmoid_table(self.zp2, 0.015)
        else:
            # any byte function: a permutation of 1 .. 254 and the two ends left out, so the gate stays inside (0, 255)
            perm = np.random.default_rng(_seed(case.name + "/table")).permutation(254).astype(np.uint8) + 1
            self.table = np.concatenate([perm, perm[:2]]).astype(np.uint8)
            self.gate_args = (self.table,)
        self.gate = self.table[self.excite]
        self.q = mul.Quant(case.x_zp, self.x_scale, 0, 1.0 / 256, 133, 0.04)
        self.want = mul.product_rows(self.q, self.x.reshape(batch * pixels, c),
                                     np.repeat(self.gate.reshape(batch, c), pixels, axis=0)).reshape(-1)
        for stage in (self.x, self.pooled, self.hidden, self.excite, self.gate, self.want):
            stage.setflags(write=False)

    @staticmethod
    def _centred(noise, a, k, izp, kzp):
        """the constant cases' bias: minus the products' sum -- the same for every row, the rows being equal -- plus the
        noise. The accumulators then straddle zero and the outputs stay inside their range, while the dot product and the
        row term they are made of are at the end of theirs: an error in either moves every output to a clamp."""
        products = o1.gemm_acc(np.ascontiguousarray(a), k, np.zeros(k.shape[0], np.int32), izp, kzp)
        assert np.all(products == products[0])
        return (noise.astype(np.int64) - products[0]).astype(np.int32)

    @property
    def rows(self):
        return self.case.batch * self.case.pixels

    def stages(self):
        return (("pooling", self.pooled), ("FC C -> S with ReLU", self.hidden), ("FC S -> C", self.excite),
                ("gate", self.gate), ("x * s", self.want))

    def expected_for(self, batch: int, pixels: int) -> np.ndarray:
        """the oracle's output for the first batch * pixels rows of x read as `batch` images of `pixels` pixels, with the
        block's members as they are (their quantization is the one derived for the block's own geometry)"""
        case, c = self.case, self.case.c
        x = self.x[:batch * pixels * c]
        pooled = np.full(batch * c, FILL, np.uint8)
        o1.global_average_pooling_q8(batch, pixels, c, case.x_zp, self.x_scale, case.pool_zp, self.pool_scale, 0, 255, x, c, pooled, c)
        f = np.float32
        acc = o1.gemm_acc(pooled.reshape(batch, c), self.k1, self.b1, self.fc1.izp, self.fc1.kzp)
        hidden = o1.requantize_rows(acc, f(f(1.0) * f(1.0) / self.scale1), self.zp1, self.fc1.qmin, 255)
        acc = o1.gemm_acc(hidden, self.k2, self.b2, self.fc2.izp, self.fc2.kzp)
        gate = self.table[o1.requantize_rows(acc, f(f(1.0) * f(1.0) / self.scale2), self.zp2, 0, 255)]
        return mul.product_rows(self.q, x.reshape(batch * pixels, c), np.repeat(gate, pixels, axis=0)).reshape(-1)

    def strided(self, dense: np.ndarray, stride: int, fill=None) -> np.ndarray:
        """the [rows][c] tensor `dense` with `stride` bytes between rows, the gaps filled (FILL, or a row pattern)"""
        c = self.case.c
        out = np.full(mul.span(self.rows, stride, c), FILL, np.uint8) if fill is None else fill.copy()
        mul.rows_view(out, self.rows, stride, c)[...] = dense.reshape(self.rows, c)
        return out

    # ---- the members and the fused operator ----
    def create_members(self, lib):
        case = self.case
        ops = [lib.create_global_average_pooling_nwc_q8(case.c, case.x_zp, self.x_scale, case.pool_zp, self.pool_scale, 0, 255, 0)]
        try:
            ops.append(lib.create_fully_connected_nc_q8(case.c, case.s, self.fc1.izp, 1.0, self.fc1.kzp, 1.0, self.k1, self.b1,
                                                        self.zp1, float(self.scale1), self.fc1.qmin, 255, 0))
            ops.append(lib.create_fully_connected_nc_q8(case.s, case.c, self.fc2.izp, 1.0, self.fc2.kzp, 1.0, self.k2, self.b2,
                                                        self.zp2, float(self.scale2), 0, 255, 0))
            create_gate = {"hardsigmoid": lib.create_hardsigmoid_nc_q8, "sigmoid": lib.create_sigmoid_nc_q8,
                           "table": lib.create_lut_nc_x8}[case.gate]
            ops.append(create_gate(case.c, *self.gate_args))
            ops.append(lib.create_multiply_nc_q8(case.c, *self.q.args()))
        except Exception:
            delete_all(lib, ops)
            raise
        return ops


_BLOCKS = {}


def block(case: Case) -> Block:
    """the case's block, computed once and shared (its arrays are read-only)"""
    if case.name not in _BLOCKS:
        _BLOCKS[case.name] = Block(case)
    return _BLOCKS[case.name]


def delete_all(lib, ops):
    for op in reversed(ops):
        lib.delete_operator(op)


def assert_not_degenerate(b: Block):
    """a kernel that writes constants, skips the ReLU or saturates the gate cannot produce this expectation. The
    thresholds are the issue's where the tensors are large enough to reach them; the constant cases (every weight and
    every input byte equal) differ through their biases only and are held to more than one value per stage."""
    case = b.case
    if case.constant is not None:
        assert np.unique(b.hidden).size > 1 and np.unique(b.gate).size > 1 and np.unique(b.want).size > 1, case.name
        return
    if b.hidden.size >= 16:
        assert b.hidden.min() == b.zp1 == b.fc1.qmin and np.unique(b.hidden).size > 4, (case.name, np.unique(b.hidden))
    inside = np.unique(b.gate[(b.gate > 0) & (b.gate < 255)])
    if b.gate.size >= 48:
        assert inside.size >= 8, (case.name, inside)
    if b.want.size >= 1024:
        assert np.unique(b.want).size > 64, (case.name, np.unique(b.want).size)
    assert not np.all(b.want == FILL), case.name


def differences(got, want, what):
    if not np.array_equal(got, want):
        assert got.size == want.size, (what, got.size, want.size)
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}")
