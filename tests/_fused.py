"""The fused inverted-residual block (qnnp_gfx950_create_fused_block; hip/q8fusedstrip.hip, hip/q8fused.hip) in every
requantization class: blocks, their oracle chain and the class table (numpy and the scalar oracle only, no GPU).

A `Stage` is one member convolution: kernel, bias, the three zero points, requantization scale and clamp. Members are
created with input scale 1, kernel scale 1 and output scale 1 / scale; a scale that is no float32 reciprocal (the single
largest multiplier, 1 - 2^-24) goes in as the kernel scale against output scale 1, as tests/_worstcase.py does. A
`Block` is [expand ->] depthwise 3x3 (pad 1) -> project [-> + block input].

Class table. `stage_class` restates hip/requant_math.h and hip/requant.hip.h (it calls neither). Four flags:
    shift 0   scale in [0.5, 1)
    folded    shift <= 22, and not (shift 0 with multiplier above 0x7FFFFF00)
    bounded   shift in 1..20, folded, and max|bias| + 65025 K < 2^30
    full      folded and clamp exactly [0, 255]
sequence: 0 shift 0, 1 bounded and full, 2 general;  clamp class: 0 full, 1 nothing to add after the clamp (folded, or
zero point 0), 2 zero point added after the clamp;  the strip kernel's mode is sequence * 3 + clamp class:
    0 shift 0, full                    3 bounded, full                 7 general, narrower clamp, folded
    1 shift 0, narrower clamp          6 general, full (large bias,    8 general, unfolded (scale < 2^-23), zero point != 0
    2 shift 0, unfolded, zp != 0         or shift 21 / 22)
tests/test_fused_classes_host.py holds the table to the library's own decisions.

Recipes. `build_block` makes one stage per requested mode, stage by stage on the ORACLE's bytes of the stage before:
weights are drawn around the kernel zero point as wide (or, at scales >= 0.5, as sparse) as puts the outputs' spread at
some 45 steps, the bias puts each channel's mean at its own spot of the range (as _perchannel._tuned does); a narrowed
clamp sits at the 20 % / 80 % quantiles of the oracle's unclamped outputs. Where no dot product can move an output
(mode 8: scale 1.5 * 2^-24, 24 * 255 * 128 * scale = 0.07 steps) the bias carries the accumulator: spread over +-2^31,
one value per channel. Mode 6 takes two channels with biases of +-(2^30 - 1000), which un-bound the whole stage and
saturate; the other channels stay informative.

Sensitivity conditions, asserted by `Block.check()` on the oracle's tensors before any GPU run -- conditions on the
inputs, not measurements:
  1. in every stage at least a quarter of the outputs lie strictly between that stage's qmin and qmax;
  2. in a stage with a narrowed clamp at least 1/16 of its outputs sit at each bound narrower than 0 / 255;
  3. for each stage under test, each of these oracle mutants changes at least one byte of the block's FINAL output:
     clamp widened to [0, 255] (clamped classes), output zero point + 1 and - 1 (the next stage keeps the true one),
     floor instead of round to nearest in that stage;
  4. with a residual the final output changes when the add's a and b ratios are swapped. Where both ratios are below
     2^-9 no pair of bytes can move the sum (255 * ratio < 1/2): the add's output is the constant y zero point for every
     input and for either order, and check() asserts exactly that instead.
A mixed triple states condition 3 for every stage from which a difference can reach the output (class_triples); the ratio
blocks whose b ratio is below 2^-9 state it for none (ratio_block).

Worst case (bound_block): stage under test with weights at the extreme (255 at kernel zero point 127, 0 at 128) in
tests/_worstcase.py's channel densities and inputs of 255 at zero point 0 in the first four image rows -- carried there
through the stages in front by weights that take a pixel of 255s to 255 -- so that |sum (a - izp)(w - kzp)| reaches
K * 255 * 128; the density-1 channels take the largest bias that keeps the stage bounded, then the smallest that does not.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from _cases import seed_for
from _runner import FILL
from oracle import o1

f32 = np.float32
MODES = (0, 1, 2, 3, 6, 7, 8)
CLAMPED_MODES = (1, 7)
TOP_SCALE = float.fromhex("0x1.FFFFFEp-1")          # multiplier 0x7FFFFF80: the zero point is not folded
MODE_SCALE = {0: 0.75, 1: 0.625, 2: TOP_SCALE, 3: 2.0 ** -9 * 1.25, 6: 2.0 ** -9 * 1.5, 7: 2.0 ** -8 * 1.125, 8: 1.5 * 2.0 ** -24}


# ---- the class table -----------------------------------------------------------------------------------------------
def scale_bits(scale) -> Tuple[int, int]:
    """(Q31 multiplier in [2^30, 2^31), right shift) of a float32 scale in [2^-32, 1)"""
    bits = int(np.array(scale, np.float32).view(np.uint32))
    return ((bits & 0x7FFFFF) | 0x800000) << 7, 126 - (bits >> 23)


def stage_flags(scale, zp, qmin, qmax, bias, reduction) -> dict:
    multiplier, shift = scale_bits(scale)
    folded = shift <= 22 and not (shift == 0 and multiplier > 0x7FFFFF00)
    max_bias = int(np.abs(np.asarray(bias, np.int64)).max()) if np.size(bias) else 0
    bounded = 1 <= shift <= 20 and folded and max_bias + 65025 * int(reduction) < 2 ** 30
    return {"shift0": shift == 0, "folded": folded, "bounded": bounded, "full": folded and (qmin, qmax) == (0, 255), "shift": shift}


def stage_class(scale, zp, qmin, qmax, bias, reduction) -> Tuple[int, int]:
    """(rounding sequence, clamp class) of a stage: see the module docstring"""
    f = stage_flags(scale, zp, qmin, qmax, bias, reduction)
    seq = 0 if f["shift0"] else (1 if f["bounded"] and f["full"] else 2)
    clamp = 0 if f["full"] else (1 if f["folded"] or zp == 0 else 2)
    return seq, clamp


def mode_of(seq_clamp) -> int:
    return seq_clamp[0] * 3 + seq_clamp[1]


def scale_arguments(scale):
    """(kernel scale, output scale, the float32 requantization scale the operator forms from 1.0 * kernel / output)"""
    scale = f32(scale)
    out = f32(1.0) / scale
    if f32(f32(1.0) * f32(1.0) / out) == scale:
        return 1.0, float(out), scale
    assert f32(f32(1.0) * scale / f32(1.0)) == scale
    return float(scale), 1.0, scale


# ---- stages and blocks -----------------------------------------------------------------------------------------------
@dataclass
class Stage:
    kernel: np.ndarray           # [1][n][1][1][k], depthwise [c][1][3][3][1]
    bias: np.ndarray
    izp: int
    kzp: int
    ozp: int
    scale: np.float32            # requantization scale
    qmin: int = 0
    qmax: int = 255
    depthwise: bool = False
    stride: int = 1

    @property
    def channels(self) -> int:
        return self.kernel.shape[0] if self.depthwise else self.kernel.shape[1]

    @property
    def reduction(self) -> int:
        return 9 if self.depthwise else self.kernel.shape[4]

    @property
    def cin(self) -> int:
        return self.kernel.shape[0] if self.depthwise else self.kernel.shape[4]

    def mode(self) -> int:
        return mode_of(stage_class(self.scale, self.ozp, self.qmin, self.qmax, self.bias, self.reduction))

    def shape(self, batch, h, w, in_stride=None):
        if self.depthwise:
            return o1.conv_shape(batch, h, w, (1, 1, 1, 1), (3, 3), (self.stride, self.stride), (1, 1), self.channels, 1, 1, in_stride)
        return o1.conv_shape(batch, h, w, (0, 0, 0, 0), (1, 1), (1, 1), (1, 1), 1, self.cin, self.channels, in_stride)

    def acc(self, x, batch, h, w, in_stride=None, bias=None):
        """oracle accumulators [pixels, channels] on the flat input x"""
        b = self.bias if bias is None else bias
        return o1.conv2d_acc(self.shape(batch, h, w, in_stride), x, self.kernel, b, self.izp, self.kzp).reshape(-1, self.channels)

    def requantize(self, acc, mutant=None) -> np.ndarray:
        """the oracle's bytes of acc; mutant: None | "wide" | "zp+1" | "zp-1" | "floor" (module docstring, condition 3)"""
        qmin, qmax, zp = self.qmin, self.qmax, self.ozp
        if mutant == "wide":
            qmin, qmax = 0, 255
        elif mutant in ("zp+1", "zp-1"):
            zp += 1 if mutant == "zp+1" else -1
            assert 0 <= zp <= 255
        if mutant == "floor":
            multiplier, shift = scale_bits(self.scale)
            y = (acc.astype(np.int64) * multiplier) >> (31 + shift)           # |acc * M| < 2^62; >> floors
            return (np.clip(y, qmin - zp, qmax - zp) + zp).astype(np.uint8)
        return o1.q31_requantize(acc, self.scale, zp, qmin, qmax)

    def mutants(self):
        out = ["floor"] + [m for m, ok in (("zp+1", self.ozp < 255), ("zp-1", self.ozp > 0)) if ok]
        return out + (["wide"] if (self.qmin, self.qmax) != (0, 255) else [])

    def create(self, lib):
        ks, osc, scale = scale_arguments(self.scale)
        assert scale == self.scale
        s = self.stride
        if self.depthwise:
            return lib.create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, s, s, 1, 1, self.channels, 1, 1, self.izp, 1.0, self.kzp, ks,
                                                    self.kernel, self.bias, self.ozp, osc, self.qmin, self.qmax, 0)
        return lib.create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, self.cin, self.channels, self.izp, 1.0, self.kzp, ks,
                                                self.kernel, self.bias, self.ozp, osc, self.qmin, self.qmax, 0)


@dataclass
class Add:
    """the residual add: a = the block input at scale a_scale, b = the project output at b_scale"""
    a_scale: float = 1.0
    b_scale: float = 0.75
    y_scale: float = 1.25
    y_zp: int = 121
    qmin: int = 0
    qmax: int = 255


@dataclass
class Block:
    name: str
    batch: int
    h: int
    w: int
    inp: np.ndarray                      # flat block input, in_stride bytes between pixels (random bytes in the gaps)
    in_stride: int
    stages: List[Optional[Stage]]        # [expand | None, depthwise, project]
    add: Optional[Add] = None
    under_test: Tuple[int, ...] = (0, 1, 2)      # stage positions condition 3 is stated for

    @property
    def cin(self) -> int:
        return (self.stages[0] or self.stages[1]).cin

    @property
    def cout(self) -> int:
        return self.stages[2].channels

    @property
    def stride(self) -> int:
        return self.stages[1].stride

    @property
    def out_hw(self):
        s = self.stride
        return (self.h - 1) // s + 1, (self.w - 1) // s + 1

    def modes(self):
        return tuple(None if s is None else s.mode() for s in self.stages)

    def oracle(self, inp=None, in_stride=None, mutant=None, swap_add=False):
        """The oracle chain: every intermediate tensor, dense [pixels, channels]: [hidden | None, depthwise, project,
        sum | None]. mutant = (stage position, name): that stage requantized by Stage.requantize's mutant."""
        inp = self.inp if inp is None else inp
        in_stride = in_stride or self.in_stride
        out, x, stride, h, w = [], inp, in_stride, self.h, self.w
        for pos, st in enumerate(self.stages):
            if st is None:
                out.append(None)
                continue
            acc = st.acc(x, self.batch, h, w, stride)
            y = st.requantize(acc, mutant[1] if mutant is not None and mutant[0] == pos else None)
            if st.depthwise:
                h, w = self.out_hw
            out.append(y)
            x, stride = y.reshape(-1), None
        if self.add is not None:
            a, rows = self.add, out[2].shape[0]
            y = np.empty((rows, self.cout), np.uint8)
            sa, sb = (a.b_scale, a.a_scale) if swap_add else (a.a_scale, a.b_scale)
            first = self.stages[0] or self.stages[1]
            o1.add_q8(rows, self.cout, first.izp, sa, self.stages[2].ozp, sb, a.y_zp, a.y_scale, a.qmin, a.qmax,
                      np.ascontiguousarray(inp), in_stride, np.ascontiguousarray(out[2]).reshape(-1), self.cout, y.reshape(-1), self.cout)
            out.append(y)
        else:
            out.append(None)
        return out

    def final(self, tensors=None) -> np.ndarray:
        t = self.oracle() if tensors is None else tensors
        return t[3] if t[3] is not None else t[2]

    def expected(self, out_stride=None, out=None) -> np.ndarray:
        """the whole output buffer: the oracle's final bytes, FILL between strided pixels"""
        dense = self.final() if out is None else out
        out_stride = out_stride or self.cout
        rows = dense.shape[0]
        flat = np.full((rows - 1) * out_stride + self.cout, FILL, np.uint8)
        np.lib.stride_tricks.as_strided(flat, shape=(rows, self.cout), strides=(out_stride, 1))[:] = dense
        return flat

    def check(self):
        """conditions 1-4 of the module docstring, on the oracle alone"""
        t = self.oracle()
        final = self.final(t)
        for pos, st in enumerate(self.stages):
            if st is None:
                continue
            y = t[pos]
            inside = np.count_nonzero((y > st.qmin) & (y < st.qmax))
            assert 4 * inside >= y.size, f"{self.name}: condition 1 fails in stage {pos}: {inside} of {y.size} outputs inside ({st.qmin}, {st.qmax})"
            for bound, narrowed in ((st.qmin, st.qmin > 0), (st.qmax, st.qmax < 255)):
                if narrowed:
                    at = np.count_nonzero(y == bound)
                    assert 16 * at >= y.size, f"{self.name}: condition 2 fails in stage {pos}: {at} of {y.size} outputs at {bound}"
            if pos in self.under_test:
                for m in st.mutants():
                    other = self.final(self.oracle(mutant=(pos, m)))
                    assert np.any(other != final), f"{self.name}: condition 3 fails: mutant {m} of stage {pos} (mode {st.mode()}) leaves the output as it is"
        if self.add is not None:
            a = self.add
            if max(a.a_scale, a.b_scale) / a.y_scale < 2.0 ** -9:
                assert np.all(final == min(max(a.y_zp, a.qmin), a.qmax)), f"{self.name}: ratios below 2^-9 must give the constant zero point"
            else:
                swapped = self.final(self.oracle(swap_add=True))
                assert np.any(swapped != final), f"{self.name}: condition 4 fails: swapping the add's ratios leaves the output as it is"
        return self

    # ---- device runs ----
    def _create(self, lib):
        ops = [None if st is None else st.create(lib) for st in self.stages]
        add = None
        if self.add is not None:
            a = self.add
            first = self.stages[0] or self.stages[1]
            add = lib.create_add_nc_q8(self.cout, first.izp, a.a_scale, self.stages[2].ozp, a.b_scale, a.y_zp, a.y_scale, a.qmin, a.qmax, 0)
        return ops, add

    def run_members(self, lib, inp=None, in_stride=None):
        """the stand-alone operators in sequence on the device: the same list as oracle()"""
        from _gpu import from_device, to_device
        import torch
        inp = self.inp if inp is None else inp
        in_stride = in_stride or self.in_stride
        ops, add = self._create(lib)
        try:
            d_in = to_device(inp)
            x, stride, h, w, out, bufs = d_in, in_stride, self.h, self.w, [], []
            for st, op in zip(self.stages, ops):
                if st is None:
                    out.append(None)
                    bufs.append(None)
                    continue
                oh, ow = self.out_hw if st.depthwise else (h, w)
                y = torch.full((self.batch * oh * ow * st.channels,), FILL, dtype=torch.uint8, device="cuda")
                lib.setup_convolution2d_nhwc_q8(op, self.batch, h, w, x, stride, y, st.channels)
                lib.run_operator(op)
                x, stride, h, w = y, st.channels, oh, ow
                bufs.append(y)
            if add is not None:
                rows = self.batch * h * w
                y = torch.full((rows * self.cout,), FILL, dtype=torch.uint8, device="cuda")
                lib.setup_add_nc_q8(add, rows, d_in, in_stride, bufs[2], self.cout, y, self.cout)
                lib.run_operator(add)
                bufs.append(y)
            else:
                bufs.append(None)
            return [None if b is None else from_device(b).reshape(-1, c) for b, c in
                    zip(bufs, [s.channels if s else 0 for s in self.stages] + [self.cout])]
        finally:
            for op in ops + [add]:
                if op is not None:
                    lib.delete_operator(op)

    def run_fused(self, lib, fused_kernel=0, rows=0, in_stride=None, out_stride=None, in_offset=0, out_offset=0, inp=None):
        """The fused operator on guarded device buffers through _runner.placed_run (guards, FILL in the gaps, input
        unchanged, output untouched on refusal): (whole output buffer, kernel name), or (None, status) when refused."""
        from _runner import placed_run
        from qnnpack_amd import QnnpackError
        inp = self.inp if inp is None else inp
        in_stride = in_stride or self.in_stride
        out_stride = out_stride or self.cout
        oh, ow = self.out_hw
        out = np.full((self.batch * oh * ow - 1) * out_stride + self.cout, FILL, np.uint8)
        ops, add = self._create(lib)
        fused = None
        lib.set_option("fused_kernel", fused_kernel)
        lib.set_option("fused_rows", rows)
        try:
            try:
                fused = lib.create_fused_block(ops[0], ops[1], ops[2], add)
                got = placed_run(lib, fused, inp, out, in_offset, out_offset, self.name,
                                 lambda d_in, d_out: lib.setup_fused_block(fused, self.batch, self.h, self.w, d_in, in_stride, d_out, out_stride))
            except QnnpackError as e:
                return None, e.status
            return got, lib.operator_kernel(fused)
        finally:
            lib.set_option("fused_kernel", 0)
            lib.set_option("fused_rows", 0)
            for op in [fused] + ops + [add]:
                if op is not None:
                    lib.delete_operator(op)


# ---- recipes ---------------------------------------------------------------------------------------------------------
def _weights(rng, shape, channel_axis, kzp, sigma_w):
    """zero-mean weights around kzp with standard deviation sigma_w: normal draws, or below 0.6 sparse +-1 (every output
    channel keeps at least one)"""
    if sigma_w >= 0.6:
        d = np.rint(rng.normal(0.0, sigma_w, shape))
    else:
        d = np.where(rng.random(shape) < sigma_w ** 2, rng.choice([-1.0, 1.0], shape), 0.0)
        flat = np.moveaxis(d, channel_axis, 0).reshape(shape[channel_axis], -1)
        for c in np.flatnonzero(~flat.any(axis=1)):
            flat[c, rng.integers(0, flat.shape[1])] = rng.choice([-1.0, 1.0])
        d = np.moveaxis(flat.reshape(np.moveaxis(d, channel_axis, 0).shape), 0, channel_axis)
    return np.clip(kzp + d, 0, 255).astype(np.uint8)


def make_stage(rng, mode, x, in_stride, batch, h, w, cin, channels, izp, kzp, depthwise=False, stride=1, relu6=None) -> Stage:
    """A stage in `mode` tuned on its actual input x (flat, in_stride): module docstring, Recipes. relu6 = k: clamp
    [zp, zp + k] instead of the quantile clamp."""
    scale = scale_arguments(MODE_SCALE[mode])[2]
    reduction = 9 if depthwise else cin
    kshape = (channels, 1, 3, 3, 1) if depthwise else (1, channels, 1, 1, cin)
    axis = 0 if depthwise else 1
    rows = np.lib.stride_tricks.as_strided(x, shape=(batch * h * w, cin), strides=(in_stride or cin, 1))
    sigma_a = max(8.0, float(np.sqrt(np.mean((rows.astype(np.float64) - izp) ** 2))))
    sigma_w = min(60.0, 45.0 / (float(scale) * sigma_a * np.sqrt(reduction)))
    kernel = _weights(rng, kshape, axis, kzp, sigma_w)
    ozp = int(rng.integers(70, 186)) if relu6 is None else int(rng.integers(20, 60))
    st = Stage(kernel, np.zeros(channels, np.int32), izp, kzp, ozp, scale, 0, 255, depthwise, stride)
    if mode == 8:
        # the bias carries the accumulator: one value per channel, outputs spread over [8, 248) at every fraction of a step
        target = rng.uniform(8.0, 248.0, channels)
        bias = np.rint((target - ozp) / float(scale))
        st.bias = np.clip(bias, -2 ** 31 + 2 ** 22, 2 ** 31 - 2 ** 22).astype(np.int32)
    else:
        acc0 = st.acc(x, batch, h, w, in_stride)
        spot = rng.uniform(0.08, 0.25, channels) * rng.choice([-1.0, 1.0], channels) * 255 + (127.5 - ozp)
        if relu6 is not None:
            spot = rng.uniform(0.05, 0.95, channels) * relu6          # the channels' means spread over the clamp's width
        st.bias = np.clip(np.rint(spot / float(scale) - acc0.mean(axis=0)), -2 ** 29, 2 ** 29).astype(np.int32)
        if mode == 6:
            st.bias[[1, channels - 2]] = [2 ** 30 - 1000, -(2 ** 30 - 1000)]
    if mode in CLAMPED_MODES:
        y = st.requantize(st.acc(x, batch, h, w, in_stride))
        if relu6 is not None:
            st.qmin, st.qmax = ozp, min(255, ozp + relu6)
        else:
            st.qmin, st.qmax = int(np.quantile(y, 0.2)), int(np.quantile(y, 0.8))
    assert st.mode() == mode, (mode, st.mode(), stage_flags(st.scale, st.ozp, st.qmin, st.qmax, st.bias, st.reduction))
    return st


def block_input(rng, batch, h, w, cin, in_stride=None) -> np.ndarray:
    in_stride = in_stride or cin
    return rng.integers(0, 256, (batch * h * w - 1) * in_stride + cin, dtype=np.uint8)


def build_block(name, modes, cin=24, hidden=40, cout=24, h=7, w=9, batch=2, stride=1, residual=None, expand=True,
                in_stride=None, kzps=None, add=None, under_test=(0, 1, 2), relu6=None) -> Block:
    """modes = (expand, depthwise, project); without `expand` the first entry is ignored and cin is the hidden width.
    residual defaults to stride 1 with cin == cout and an expand stage. kzps: kernel zero points, drawn from 127 / 128."""
    rng = np.random.default_rng(seed_for(name) ^ 0xF05ED)
    if not expand:
        cin = hidden
    if residual is None:
        residual = expand and stride == 1 and cin == cout
    in_stride = in_stride or cin
    kzps = kzps or [int(z) for z in rng.choice([127, 128], 3)]
    izp = int(rng.integers(60, 196))
    inp = block_input(rng, batch, h, w, cin, in_stride)
    stages, x, xs = [], inp, in_stride
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    if expand:
        st = make_stage(rng, modes[0], x, xs, batch, h, w, cin, hidden, izp, kzps[0], relu6=relu6)
        stages.append(st)
        x, xs, izp = st.requantize(st.acc(x, batch, h, w, xs)).reshape(-1), hidden, st.ozp
    else:
        stages.append(None)
    st = make_stage(rng, modes[1], x, xs, batch, h, w, hidden, hidden, izp, kzps[1], depthwise=True, stride=stride, relu6=relu6)
    stages.append(st)
    x, xs, izp = st.requantize(st.acc(x, batch, h, w, xs)).reshape(-1), hidden, st.ozp
    stages.append(make_stage(rng, modes[2], x, xs, batch, oh, ow, hidden, cout, izp, kzps[2]))
    if residual and add is None:
        add = Add()
    under = tuple(p for p in under_test if stages[p] is not None)
    return Block(name, batch, h, w, inp, in_stride, stages, add if residual else None, under)




# ---- worst-case operands at the accumulator bound (the operand pattern of tests/_worstcase.py) ------------------------
BOUND_SCALE = 1.5 * 2.0 ** -20          # shift 19: bounded while max|bias| + 65025 K < 2^30
BOUND_KZP = (127, 128, 127)             # per position: extreme weight 255 (w - kzp = +128) or 0 (-128)
EXTREME_ROWS = 4                        # image rows 0..3 of the block input hold 255 in every channel (zero point 0)


def _carrier_stage(rng, x, in_stride, batch, h, w, cin, channels, depthwise, stride=1) -> Stage:
    """Takes extreme inputs (255 at zero point 0) to extreme outputs (255 at zero point 0): every weight is 64..128 above
    the kernel zero point 127, so a pixel (window) of 255s saturates while the other pixels stay inside the range."""
    kshape = (channels, 1, 3, 3, 1) if depthwise else (1, channels, 1, 1, cin)
    kernel = (127 + rng.integers(64, 129, kshape)).astype(np.uint8)
    st = Stage(kernel, np.zeros(channels, np.int32), 0, 127, 0, f32(1.0), 0, 255, depthwise, stride)
    acc0 = st.acc(x, batch, h, w, in_stride)
    rest = acc0.reshape(batch, h, w, channels)[:, EXTREME_ROWS + 1:].reshape(-1, channels).astype(np.float64)
    scale = 45.0 / max(1.0, float(rest.std(axis=0).mean()))
    st.scale = scale_arguments(2.0 ** np.floor(np.log2(scale)) * 1.25)[2]
    spot = rng.uniform(100.0, 156.0, channels)
    st.bias = np.rint(spot / float(st.scale) - rest.mean(axis=0)).astype(np.int32)
    assert st.mode() == 3, st.mode()
    return st


def _bound_stage(rng, pos, over, x, in_stride, batch, h, w, cin, channels, depthwise) -> Stage:
    """Weights at the extreme in the densities (1, 1, 7/8, 1/2, 1/8, 0) by channel; the density-1 channels take the
    largest bias that keeps the stage bounded (over: the smallest that does not), the others a bias spread over
    sign * [0, 2^27), inside the clamp at BOUND_SCALE."""
    kzp = BOUND_KZP[pos]
    w_ext, sign = (255, 1) if kzp == 127 else (0, -1)
    reduction = 9 if depthwise else cin
    dens = np.asarray((1.0, 1.0, 7 / 8, 1 / 2, 1 / 8, 0.0))[np.arange(channels) % 6]
    kshape = (channels, 1, 3, 3, 1) if depthwise else (1, channels, 1, 1, cin)
    d = dens.reshape((channels, 1, 1, 1, 1) if depthwise else (1, channels, 1, 1, 1))
    kernel = np.where(rng.random(kshape) < d, np.uint8(w_ext), np.uint8(kzp)).astype(np.uint8)
    bias = sign * rng.integers(0, 2 ** 27, channels).astype(np.int64)
    bias[dens == 1.0] = sign * ((2 ** 30 + (1 if over else 0)) - 1 - 65025 * reduction)
    st = Stage(kernel, bias.astype(np.int32), 0, kzp, 0 if sign > 0 else 255, scale_arguments(BOUND_SCALE)[2], 0, 255, depthwise, 1)
    assert st.mode() == (6 if over else 3), (st.mode(), over)
    return st


@functools.lru_cache(maxsize=None)
def bound_block(pos, over, cin=160, hidden=256, cout=32, h=7, w=9, batch=2) -> Block:
    """Stage `pos` at the accumulator bound; the stages in front of it carry the extremes to it, those behind are mode 3 / 0"""
    name = f"fb_bound_s{pos}_{'over' if over else 'at'}"
    rng = np.random.default_rng(seed_for(f"fb_bound_s{pos}") ^ 0xB0D)        # (both biases share every other draw)
    inp = block_input(rng, batch, h, w, cin).reshape(batch, h, w, cin)
    inp[:, :EXTREME_ROWS] = 255
    inp = inp.reshape(-1)
    stages, x, izp = [], inp, 0
    geometry = [(cin, hidden, False), (hidden, hidden, True), (hidden, cout, False)]
    for p, (k, n, dwise) in enumerate(geometry):
        if p < pos:
            st = _carrier_stage(rng, x, k, batch, h, w, k, n, dwise)
        elif p == pos:
            st = _bound_stage(rng, pos, over, x, k, batch, h, w, k, n, dwise)
        else:
            st = make_stage(rng, OTHER[p], x, k, batch, h, w, k, n, izp, int(rng.choice([127, 128])), depthwise=dwise)
        stages.append(st)
        x, izp = st.requantize(st.acc(x, batch, h, w, k)).reshape(-1), st.ozp
    return Block(name, batch, h, w, inp, cin, stages, None, (pos,))


# ---- the parametrisation of tests/test_requant_classes_fused_gpu.py (tests/test_fused_classes_host.py checks every block) ----
OTHER = (3, 0, 3)        # the stages not under test: bounded / shift 0 with the full clamp, so that they pass a difference on
MIXED = [(1, 7, 1), (7, 1, 7), (2, 6, 8), (8, 3, 2)]
UNIFORM = [(0, 0, 0), (3, 3, 3)]
FIXED = (7, 1, 6)        # the mixed triple of the layout, geometry, zero-point and ratio families


def class_triples():
    """(id, triple, positions condition 3 is stated for). A single-mode case states it for its own stage. A mixed or
    uniform triple states it for every stage from which a difference can reach the output: not for the stages in front
    of a mode-8 stage, whose bytes no dot product moves (module docstring); those stages are under test in their own
    single-mode cases."""
    out = []
    for pos in range(3):
        for mode in MODES:
            triple = list(OTHER)
            triple[pos] = mode
            out.append((f"s{pos}_m{mode}", tuple(triple), (pos,)))
    for tag, triples in (("mixed", MIXED), ("uniform", UNIFORM)):
        for t in triples:
            last8 = max([p for p in range(3) if t[p] == 8], default=0)
            out.append((tag + "_" + "".join(map(str, t)), t, tuple(p for p in range(3) if p >= last8)))
    return out


@functools.lru_cache(maxsize=None)
def class_block(ident, triple, under, hidden=40, expand=True) -> Block:
    return build_block(f"fb_{ident}_h{hidden}" + ("" if expand else "_noexpand"), triple, hidden=hidden, expand=expand,
                       under_test=under)


KZP_OUTSIDE = [(pos, kzp) for pos in range(3) for kzp in (3, 200)]


@functools.lru_cache(maxsize=None)
def kzp_block(pos, kzp) -> Block:
    kzps = [127, 128, 127]
    kzps[pos] = kzp
    return build_block(f"fb_kzp_s{pos}_{kzp}", FIXED, hidden=48, kzps=kzps)


RELU6_K = 96          # the clamp [zp, zp + 96] at zero points 20..59


@functools.lru_cache(maxsize=None)
def relu6_block(stride) -> Block:
    return build_block(f"fb_relu6_s{stride}", (7, 7, 3), hidden=48, stride=stride, relu6=RELU6_K)


# (tag, a ratio, b ratio) with the sum at scale 1: tests/test_pointwise_range_gpu.FOLDED_RATIOS (restated: that module
# is GPU-marked), below, at and above the add's 2^-10 seam, and top against bottom
TOP_RATIO = float(np.nextafter(f32(2.0 ** 8), f32(0)))
RATIOS = [("both_below_seam", 2.0 ** -12, 2.0 ** -13), ("at_seam", 2.0 ** -10, 2.0 ** -14), ("top_and_bottom", TOP_RATIO, 2.0 ** -14),
          ("mid", 0.75, 1.25)]


@functools.lru_cache(maxsize=None)
def ratio_block(tag) -> Block:
    ra, rb = next((a, b) for t, a, b in RATIOS if t == tag)
    # (condition 3 needs the project output to reach the sum: 255 * rb >= 1/2. Below that the family is about the add
    #  alone, and the stages' classes are under test in the other families)
    under = (0, 1, 2) if 255 * rb >= 0.5 else ()
    return build_block(f"fb_ratio_{tag}", FIXED, hidden=48, add=Add(a_scale=ra, b_scale=rb, y_scale=1.0), under_test=under)


# layout: (cin, input stride, input base offset) -> bytes per input staging piece; (cout, output stride, base) -> store mode
INPUT_LAYOUTS = [(32, 48, 0, 16), (24, 32, 8, 8), (24, 28, 4, 4)]
OUTPUT_LAYOUTS = [(32, 48, 0, 2), (32, 48, 16, 2), (24, 28, 4, 1), (24, 29, 1, 0), (32, 33, 0, 0)]
REFUSED_LAYOUTS = [(24, 24, 2), (24, 26, 0), (24, 28, 3)]          # (cin, input stride, base): not multiples of 4


@functools.lru_cache(maxsize=None)
def layout_block(channels, in_stride) -> Block:
    return build_block(f"fb_layout_c{channels}_s{in_stride}", FIXED, cin=channels, cout=channels, in_stride=in_stride)


GEOMETRY_IMAGES = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 7)]


@functools.lru_cache(maxsize=None)
def geometry_block(h, w, stride, hidden=40) -> Block:
    # (tiny images: more of them, so that the conditions have a few hundred outputs to hold on)
    return build_block(f"fb_geo_{h}x{w}_s{stride}_h{hidden}", FIXED, hidden=hidden, h=h, w=w, stride=stride,
                       batch=2 if h * w >= 30 else 6)


def blocks_used():
    """every block of tests/test_requant_classes_fused_gpu.py, as (id, block)"""
    for ident, triple, under in class_triples():
        yield f"strip/{ident}", class_block(ident, triple, under)
        yield f"strip/{ident}/noexpand", class_block(ident, triple, under, 40, False)
        yield f"tile/{ident}", class_block(ident, triple, under, 48)
        yield f"tile/{ident}/noexpand", class_block(ident, triple, under, 48, False)
    for pos, kzp in KZP_OUTSIDE:
        yield f"kzp/{pos}/{kzp}", kzp_block(pos, kzp)
    for stride in (1, 2):
        yield f"relu6/{stride}", relu6_block(stride)
    for tag, _, _ in RATIOS:
        yield f"ratio/{tag}", ratio_block(tag)
    for c, s in sorted({(c, s) for c, s, _, _ in INPUT_LAYOUTS} | {(c, c) for c, _, _, _ in OUTPUT_LAYOUTS} | {(c, s) for c, s, _ in REFUSED_LAYOUTS}):
        yield f"layout/{c}/{s}", layout_block(c, s)
    for h, w in GEOMETRY_IMAGES:
        for stride in (1, 2):
            yield f"geometry/{h}x{w}/s{stride}", geometry_block(h, w, stride)
    yield "geometry/6x5/s2", geometry_block(6, 5, 2)
    yield "geometry/hidden272", geometry_block(7, 9, 1, 272)
    for pos in range(3):
        for over in (False, True):
            yield f"bound/{pos}/{'over' if over else 'at'}", bound_block(pos, over)


def stride_tricks_rows(flat, rows, channels, stride):
    """[rows, channels] view of a flat buffer with `stride` bytes between rows"""
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, channels), strides=(stride, 1))
