"""GPU tier: the fused inverted-residual block (qnnp_gfx950_create_fused_block; hip/q8fusedstrip.hip and
hip/q8fused.hip) against the scalar oracle's chain in every requantization class, layout and geometry it accepts.

Blocks, recipes, the oracle chain and the sensitivity conditions are those of tests/_fused.py;
tests/test_fused_classes_host.py establishes the conditions on the oracle alone, holds the class table to the library
and asserts that the mode families below contain all seven modes in each stage position. Every case asserts that the
fused output equals the ORACLE chain byte for byte (whole output buffers, the bytes between strided pixels included,
through _runner.placed_run: guards, input unchanged), that it equals the members' device chain, and the kernel's name.

Unless stated otherwise a block is 24 -> 40 -> 24 channels (partial 32-blocks), 7 x 9 pixels, batch 2, stride 1 with the
residual add, kernel zero points drawn from 127 / 128 per member. Families:
  modes     every mode in every stage on the strip kernel (3 x 7), four mixed triples and the two uniform controls, each
            also without an expand stage (40 -> 40 -> 24, no residual); the same on the tile kernel at 48 hidden channels;
  kzp       one member at a time at kernel zero point 3 / 200: the tile kernel takes the block, the strip kernel refuses;
  relu6     expand and depthwise clamped to [zp, zp + 96] at a scale below 0.5, project unclamped; stride 1 with the
            residual, stride 2 without (a residual needs stride 1);
  ratios    the add's (a, b) ratios of tests/test_pointwise_range_gpu.FOLDED_RATIOS on both kernels;
  layout    strip kernel: input pieces of 16 / 8 / 4 bytes, store modes 2 / 1 / 0, unaligned inputs refused at setup;
  geometry  images of 1 and 2 pixels, forced strip heights with a shorter last strip, nine hidden blocks (two chunks);
  bound     worst-case operands with the bias at and just over the accumulator bound, 160 -> 256 -> 32 channels;
  network   the whole MobileNetV2 with ReLU6-style clamps at the smallest input, all 17 blocks on the strip kernel.

Run time on an MI355X: the whole file (161 ids) takes about 3 s; the slowest id is
test_nine_hidden_blocks_take_a_second_chunk, 0.12 s, and no other id takes more than 0.02 s.
"""
import numpy as np
import pytest

import _fused as F
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

STRIP, TILE = "q8_fused_strip", "q8_fused_block"


def _dense(flat, block, out_stride):
    oh, ow = block.out_hw
    return F.stride_tricks_rows(flat, block.batch * oh * ow, block.cout, out_stride or block.cout)


def _hold(qnnp, block, fused_kernel, want, may_refuse=False, **placement):
    """Run the fused block and hold it to the oracle chain and to the members' device chain. Returns the kernel name, or
    None when setup refused with unsupported_parameter and may_refuse allows it."""
    what = f"{block.name} modes {block.modes()} fused_kernel {fused_kernel} {placement}"
    expected = block.expected(placement.get("out_stride"))
    got, name = block.run_fused(qnnp, fused_kernel, **placement)
    if got is None:
        assert may_refuse, f"{what}: refused ({name.name})"
        assert name == Status.unsupported_parameter, f"{what}: refused with {name.name}"
        return None
    assert name == want, f"{what}: ran {name}"
    members = block.run_members(qnnp)
    member_out = members[3] if members[3] is not None else members[2]
    oracle = block.oracle()
    fused_out = _dense(got, block, placement.get("out_stride"))
    vs_oracle = np.array_equal(got, expected)
    vs_members = np.array_equal(fused_out, member_out)
    if not (vs_oracle and vs_members):
        # which side disagrees with the oracle, and from which stage on the members do
        first = next((pos for pos in range(4) if oracle[pos] is not None and not np.array_equal(oracle[pos], members[pos])), None)
        side = ("the members' chain agrees with the oracle: the fused kernel is wrong" if first is None else
                f"the members' chain leaves the oracle at tensor {first} (0 hidden, 1 depthwise, 2 project, 3 sum)")
        bad = np.flatnonzero(fused_out != block.final(oracle))
        where = np.unravel_index(bad[:4], fused_out.shape) if bad.size else ()
        raise AssertionError(f"{what} [{name}]: fused == oracle: {vs_oracle}, fused == members: {vs_members}; {side}; "
                             f"{bad.size} of {fused_out.size} pixel bytes differ from the oracle, first at (pixel, channel) "
                             f"{[(int(p), int(c)) for p, c in zip(*where)] if bad.size else []}")
    return name


CLASS_IDS = [ident for ident, _, _ in F.class_triples()]
CLASS_ARGS = {ident: (triple, under) for ident, triple, under in F.class_triples()}


# ---- every mode in every stage ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("expand", [True, False], ids=["expand", "noexpand"])
@pytest.mark.parametrize("ident", CLASS_IDS)
def test_every_class_on_the_strip_kernel(qnnp, ident, expand):
    block = F.class_block(ident, *CLASS_ARGS[ident], 40, expand)
    assert _hold(qnnp, block, 2, STRIP) == STRIP


@pytest.mark.parametrize("expand", [True, False], ids=["expand", "noexpand"])
@pytest.mark.parametrize("ident", CLASS_IDS)
def test_every_class_on_the_tile_kernel(qnnp, ident, expand):
    """runs as q8_fused_block or is refused at setup, never under another name; the uniform control and a clamped triple
    must be accepted"""
    block = F.class_block(ident, *CLASS_ARGS[ident], 48, expand)
    name = _hold(qnnp, block, 1, TILE, may_refuse=ident not in ("uniform_000", "mixed_171"))
    assert name in (TILE, None)


# ---- kernel zero points outside 127 / 128 ------------------------------------------------------------------------------
@pytest.mark.parametrize("pos,kzp", F.KZP_OUTSIDE)
def test_kernel_zero_points_outside_the_centred_pair(qnnp, pos, kzp):
    block = F.kzp_block(pos, kzp)
    assert _hold(qnnp, block, 0, TILE) == TILE                   # the tile kernel is the block's only fused path
    got, status = block.run_fused(qnnp, 2)
    assert got is None and status == Status.unsupported_parameter, (got is None, status)


# ---- a ReLU6-style block end to end ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_kernel,want", [(2, STRIP), (1, TILE), (0, STRIP)], ids=["strip", "tile", "auto"])
@pytest.mark.parametrize("stride", [1, 2])
def test_relu6_block(qnnp, stride, fused_kernel, want):
    block = F.relu6_block(stride)
    assert block.modes() == (7, 7, 3) and (block.add is not None) == (stride == 1)
    for st in block.stages[:2]:
        assert (st.qmin, st.qmax) == (st.ozp, st.ozp + F.RELU6_K) and float(st.scale) < 0.5
    assert _hold(qnnp, block, fused_kernel, want) == want


# ---- the residual add over its ratio range -----------------------------------------------------------------------------
def test_ratios_are_those_of_the_folded_add():
    from test_pointwise_range_gpu import FOLDED_RATIOS
    assert [(t, float(np.float32(a)), float(np.float32(b))) for t, a, b in FOLDED_RATIOS] == \
           [(t, float(np.float32(a)), float(np.float32(b))) for t, a, b in F.RATIOS]


@pytest.mark.parametrize("fused_kernel,want", [(2, STRIP), (1, TILE)], ids=["strip", "tile"])
@pytest.mark.parametrize("tag", [t for t, _, _ in F.RATIOS])
def test_residual_ratios(qnnp, tag, fused_kernel, want):
    assert _hold(qnnp, F.ratio_block(tag), fused_kernel, want) == want


# ---- layout, on the strip kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,in_stride,in_offset,piece", F.INPUT_LAYOUTS)
def test_input_pieces(qnnp, channels, in_stride, in_offset, piece):
    """the staging piece follows from the channel count, the pixel stride and the base address (q8fusedstrip.hip, in_piece)"""
    assert max(p for p in (16, 8, 4) if channels % p == 0 and in_stride % p == 0 and in_offset % p == 0) == piece
    block = F.layout_block(channels, in_stride)
    assert _hold(qnnp, block, 2, STRIP, in_offset=in_offset) == STRIP


@pytest.mark.parametrize("channels,out_stride,out_offset,mode", F.OUTPUT_LAYOUTS)
def test_store_modes(qnnp, channels, out_stride, out_offset, mode):
    """16-byte, dword and byte stores follow from the channel count, the pixel stride and the base address"""
    fits = lambda n: channels % n == 0 and out_stride % n == 0 and out_offset % n == 0
    assert (2 if fits(16) else (1 if fits(4) else 0)) == mode
    block = F.layout_block(channels, channels)
    assert _hold(qnnp, block, 2, STRIP, out_stride=out_stride, out_offset=out_offset) == STRIP


@pytest.mark.parametrize("channels,in_stride,in_offset", F.REFUSED_LAYOUTS)
def test_unaligned_input_is_refused_at_setup(qnnp, channels, in_stride, in_offset):
    got, status = F.layout_block(channels, in_stride).run_fused(qnnp, 2, in_offset=in_offset)
    assert got is None and status == Status.unsupported_parameter, (got is None, status)


# ---- geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("h,w", F.GEOMETRY_IMAGES)
def test_images_of_one_and_two_pixels(qnnp, h, w, stride):
    assert _hold(qnnp, F.geometry_block(h, w, stride), 2, STRIP) == STRIP


@pytest.mark.parametrize("rows", [0, 1, 2])
def test_forced_strip_heights_with_a_shorter_last_strip(qnnp, rows):
    block = F.geometry_block(6, 5, 2)              # 3 x 3 outputs: strips of 2 leave a last strip of 1
    assert _hold(qnnp, block, 2, STRIP, rows=rows) == STRIP


def test_nine_hidden_blocks_take_a_second_chunk(qnnp):
    assert _hold(qnnp, F.geometry_block(7, 9, 1, 272), 2, STRIP) == STRIP


# ---- worst-case operands at the accumulator bound ----------------------------------------------------------------------
@pytest.mark.parametrize("over", [False, True], ids=["largest_bounded_bias", "smallest_unbounded_bias"])
@pytest.mark.parametrize("pos", [0, 1, 2], ids=["expand", "depthwise", "project"])
def test_accumulator_bound(qnnp, pos, over):
    """the offset forms wrap by design: bias + 2^31 at the largest bias that keeps the stage bounded (mode 3), and the
    general sequence one step over it (mode 6)"""
    block = F.bound_block(pos, over)
    assert block.modes()[pos] == (6 if over else 3)
    assert _hold(qnnp, block, 2, STRIP) == STRIP


# ---- the whole network with ReLU6-style clamps -------------------------------------------------------------------------
RELU6_STEPS = 96


def relu6_clamp(op, ozp):
    """ReLU6-style: every expand and depthwise output clamped to [zp, zp + 96]; project, first, last: unclamped"""
    if op.name.endswith(("_expand", "_dw")):
        return ozp, min(255, ozp + RELU6_STEPS)
    return 0, 255


def test_fused_network_with_relu6_clamps_matches_oracle(qnnp):
    """The whole network with a narrowed clamp on every expand and depthwise stage (mode 7 of the strip kernel's
    per-stage switch beside mode 3 in the project stage), automatic kernel choice: all 17 blocks on q8_fused_strip,
    tensor by tensor against the oracle. 33 x 33 is the smallest input whose last block still has 2 x 2 pixels
    (33 -> 17 -> 9 -> 5 -> 3 -> 2), so every block has an odd or tiny image."""
    import torch
    from _gpu import from_device
    from examples import mobilenetv2 as mnv2
    from test_gpu_network import oracle_forward
    input_hw, batch = 33, 1
    plan = mnv2.build_plan(input_hw=input_hw, classes=1000, seed=0x51A0 + input_hw)
    assert plan.shapes[plan.ops[-3].dst][:2] == (2, 2)
    rng = np.random.default_rng(1000 + input_hw)
    image = rng.integers(0, 256, size=batch * input_hw * input_hw * 3, dtype=np.uint8)
    expected, quant = oracle_forward(plan, image, batch, clamp=relu6_clamp)
    clamped = [q for name, q in quant.items() if name.endswith(("_expand", "_dw"))]
    assert len(clamped) == 33 and all((q.qmin, q.qmax) == (q.out_zp, min(255, q.out_zp + RELU6_STEPS)) for q in clamped)
    for op in plan.ops:                                      # the clamp bites and leaves room
        if op.name.endswith(("_expand", "_dw")):
            t, q = expected[op.dst], quant[op.name]
            assert np.any(t == q.qmin) and np.any((t > q.qmin) & (t < q.qmax)), op.name
    net = mnv2.DeviceNetwork(qnnp, torch, plan, batch, quant, fuse=True)
    try:
        assert len(net.fused) == 17, (len(net.fused), sorted(net.fused))
        net.buffers[0].copy_(torch.from_numpy(image))
        net.run()
        assert {net.kernels[name] for name in net.fused} == {"q8_fused_strip"}
        hidden = set()
        for first, last in net.fused.values():
            hidden.update(plan.ops[i].dst for i in range(first, last))       # tensors the fused blocks never write
        for op in plan.ops:
            if op.dst in hidden:
                continue
            got = from_device(net.buffers[op.dst])
            bad = np.flatnonzero(got != expected[op.dst])
            assert bad.size == 0, f"{op.name}: {bad.size} of {got.size} bytes differ (first at {bad[:4].tolist()})"
    finally:
        net.close()
