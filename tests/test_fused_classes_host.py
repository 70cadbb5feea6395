"""CPU tier: what tests/test_requant_classes_fused_gpu.py rests on, without a GPU.

 1. The class table of tests/_fused.py (stage_class: rounding sequence and clamp class of a stage, hence the strip
    kernel's mode) against what the library decides, through the debug hooks: qnnp_debug_accumulator_bits, the kind_out
    of qnnp_debug_requant_fast_offset (1 shift 0, 2 bounded, 0 general) and the bounded_out of
    qnnp_debug_requant_fast_bits -- for every stage of every block the GPU file uses and over a grid of scales, zero
    points, clamps and bias bounds. Whether a shift-0 zero point is folded shows in qnnp_debug_requant_lane's kind. The
    hooks do not show the fold at shifts 22 / 23 nor the full-range flag: those two rules are pinned by the table of
    known classes below, and the GPU file asserts the bytes.
 2. Block.check() -- the sensitivity conditions 1-4 of tests/_fused.py, the mutant oracles of condition 3 and the
    swapped ratios of condition 4 among them -- passes for every block the GPU file uses: its expected bytes cannot be
    reached by a kernel that drops a clamp, misplaces a zero point, truncates, or confuses the add's operands.
 3. The mode families of the GPU file hold every one of the seven modes in each of the three stage positions, on the
    strip shape and on the tile shape, judged by the blocks as built (a recipe that drifts into another class fails)."""
import ctypes

import numpy as np
import pytest

import _fused as F
from oracle import o1


def _hooks(debug_hooks):
    L = debug_hooks.lib
    L.qnnp_debug_accumulator_bits.restype = ctypes.c_uint32
    L.qnnp_debug_accumulator_bits.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t]
    for fn in (L.qnnp_debug_requant_fast_offset, L.qnnp_debug_requant_fast_bits):
        fn.restype = None
        fn.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8,
                       ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    L.qnnp_debug_requant_lane.restype = None
    L.qnnp_debug_requant_lane.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint8,
                                          ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    return L


ACC = np.array([0, 1, -1, 77, -77, 12345, -12345, 2 ** 20 + 3, -(2 ** 20) - 3, 2 ** 29, -(2 ** 29)], np.int32)


def _library_decides(L, scale, zp, qmin, qmax, bias, reduction):
    """(accumulator bits, offset kind, bounded, lane kind at a stated bound of 30 bits) as the library's host code decides"""
    bias = np.ascontiguousarray(bias, np.int32)
    bits = int(L.qnnp_debug_accumulator_bits(bias.ctypes.data, bias.size, reduction))
    out = np.empty(ACC.size, np.uint8)
    kind, bounded, lane = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    L.qnnp_debug_requant_fast_offset(ACC.size, ACC.ctypes.data, np.float32(scale), zp, qmin, qmax, bits, out.ctypes.data, ctypes.byref(kind))
    assert np.array_equal(out, o1.q31_requantize(ACC, scale, zp, qmin, qmax))
    L.qnnp_debug_requant_fast_bits(ACC.size, ACC.ctypes.data, np.float32(scale), zp, qmin, qmax, bits, out.ctypes.data, ctypes.byref(bounded))
    assert np.array_equal(out, o1.q31_requantize(ACC, scale, zp, qmin, qmax))
    zeros = np.zeros(ACC.size, np.int32)
    L.qnnp_debug_requant_lane(ACC.size, ACC.ctypes.data, zeros.ctypes.data, np.float32(scale), zp, qmin, qmax, 30, out.ctypes.data, ctypes.byref(lane))
    return bits, kind.value, bounded.value, lane.value


def _assert_agrees(L, scale, zp, qmin, qmax, bias, reduction, what):
    flags = F.stage_flags(scale, zp, qmin, qmax, bias, reduction)
    bits, kind, bounded, lane = _library_decides(L, scale, zp, qmin, qmax, bias, reduction)
    multiplier, shift = F.scale_bits(scale)
    params = o1.q31_params(scale, zp, qmin, qmax)
    assert (multiplier, shift) == (params.multiplier, params.shift), (what, multiplier, shift)
    max_bias = int(np.abs(np.asarray(bias, np.int64)).max())
    assert (1 <= bits <= 30) == (max_bias + 65025 * reduction < 2 ** 30), (what, bits)
    assert flags["shift0"] == (kind == 1), (what, flags, kind)
    assert flags["bounded"] == (bounded == 1) == (kind == 2), (what, flags, bounded, kind)
    if shift == 0:
        assert flags["folded"] == (lane == 1), (what, flags, lane)       # (a stated bound of 30 bits: the fold alone decides)
    seq, clamp = F.stage_class(scale, zp, qmin, qmax, bias, reduction)
    assert seq == (0 if kind == 1 else (1 if kind == 2 and flags["full"] else 2)), (what, seq, kind)
    assert F.mode_of((seq, clamp)) in F.MODES, (what, seq, clamp)         # modes 4 and 5 do not exist


@pytest.fixture(scope="module")
def blocks():
    return list(F.blocks_used())


def test_class_table_agrees_with_the_library_on_every_recipe(debug_hooks, blocks):
    L = _hooks(debug_hooks)
    stages = 0
    for ident, block in blocks:
        for pos, st in enumerate(block.stages):
            if st is not None:
                _assert_agrees(L, st.scale, st.ozp, st.qmin, st.qmax, st.bias, st.reduction, f"{ident} stage {pos}")
                stages += 1
    assert stages > 300


GRID_SCALES = [0.5, 0.75, float.fromhex("0x1.FFFFFCp-1"), F.TOP_SCALE, 0.49999997, 0.25, 2.0 ** -9, 1.5 * 2.0 ** -20, 1.5 * 2.0 ** -21,
               2.0 ** -21, 1.5 * 2.0 ** -22, 1.5 * 2.0 ** -23, 2.0 ** -23, 1.5 * 2.0 ** -24, 2.0 ** -31]


def test_class_table_agrees_with_the_library_on_a_grid(debug_hooks):
    L = _hooks(debug_hooks)
    for reduction in (9, 24, 256, 16512):
        edge = 2 ** 30 - 65025 * reduction
        for max_bias in (0, 10000, edge - 1, edge, 2 ** 31 - 1):
            for sign in (1, -1):
                bias = np.array([3, sign * max_bias, -7], np.int64).astype(np.int32)
                for scale in GRID_SCALES:
                    for zp in (0, 1, 128, 255):
                        for qmin, qmax in ((0, 255), (1, 254), (0, 254), (10, 10)):
                            _assert_agrees(L, np.float32(scale), zp, qmin, qmax, bias, reduction, (reduction, max_bias * sign, scale, zp, qmin, qmax))


# (scale, zero point, clamp, max |bias|, reduction) -> mode: the table of the issue, by hand
KNOWN = [((0.75, 5, 0, 255, 100, 24), 0), ((0.5, 0, 0, 255, 2 ** 31 - 1, 24), 0),
         ((0.75, 5, 1, 255, 100, 24), 1), ((F.TOP_SCALE, 0, 0, 255, 100, 24), 1), ((F.TOP_SCALE, 0, 3, 200, 100, 24), 1),
         ((F.TOP_SCALE, 5, 0, 255, 100, 24), 2), ((F.TOP_SCALE, 255, 9, 250, 100, 24), 2),
         ((2.0 ** -9, 5, 0, 255, 100, 24), 3), ((0.49999997, 0, 0, 255, 2 ** 30 - 65025 * 24 - 1, 24), 3), ((1.5 * 2.0 ** -21, 255, 0, 255, 0, 9), 3),
         ((2.0 ** -9, 5, 0, 255, 2 ** 30 - 65025 * 24, 24), 6), ((1.5 * 2.0 ** -22, 5, 0, 255, 0, 9), 6), ((1.5 * 2.0 ** -23, 5, 0, 255, 0, 9), 6),
         ((2.0 ** -9, 5, 0, 254, 100, 24), 7), ((1.5 * 2.0 ** -23, 5, 5, 255, 0, 9), 7), ((1.5 * 2.0 ** -24, 0, 0, 255, 0, 9), 7),
         ((1.5 * 2.0 ** -24, 5, 0, 255, 0, 9), 8), ((2.0 ** -31, 200, 7, 201, 0, 9), 8)]


@pytest.mark.parametrize("args,mode", KNOWN)
def test_known_classes(args, mode):
    scale, zp, qmin, qmax, max_bias, reduction = args
    assert F.mode_of(F.stage_class(np.float32(scale), zp, qmin, qmax, np.array([max_bias, -1], np.int64), reduction)) == mode


FAMILIES = ["strip", "tile", "kzp", "relu6", "ratio", "layout", "geometry", "bound"]


@pytest.mark.parametrize("family", FAMILIES)
def test_conditions_hold_on_the_oracle_alone(blocks, family):
    """conditions 1-4, the mutants and the swapped ratios included; the counts say that no family is empty and how many
    mutants each single-mode case has been held to"""
    mine = [(ident, block) for ident, block in blocks if ident.split("/")[0] == family]
    assert mine
    for ident, block in mine:
        block.check()
        if family in ("strip", "tile") and "/s" in ident:                 # a single-mode case: its own stage, where it exists
            pos, mode = int(ident.split("/")[1][1]), int(ident.split("_m")[1].split("/")[0])
            st = block.stages[pos]
            if st is not None:
                assert block.under_test == (pos,) and st.mode() == mode, (ident, block.under_test, st.mode())
                assert "floor" in st.mutants() and (("wide" in st.mutants()) == (mode in F.CLAMPED_MODES)), (ident, st.mutants())
                assert "zp+1" in st.mutants() and "zp-1" in st.mutants(), (ident, st.mutants())
        if block.add is not None and family != "ratio":
            assert block.add.a_scale != block.add.b_scale


def test_every_block_the_gpu_file_uses_was_checked(blocks):
    assert {ident.split("/")[0] for ident, _ in blocks} == set(FAMILIES)
    assert len({ident for ident, _ in blocks}) == len(blocks)


@pytest.mark.parametrize("shape", ["strip", "tile"])
def test_every_mode_in_every_stage_position(blocks, shape):
    seen = {pos: set() for pos in range(3)}
    for ident, block in blocks:
        if ident.startswith(shape + "/") and not ident.endswith("/noexpand"):
            for pos, mode in enumerate(block.modes()):
                seen[pos].add(mode)
            triple = next(t for i, t, _ in F.class_triples() if i == ident.split("/")[1])
            assert block.modes() == triple, (ident, block.modes(), triple)     # the block as built is in the classes asked for
    for pos in range(3):
        assert seen[pos] == set(F.MODES), (shape, pos, sorted(seen[pos]))
    # without an expand stage: the two stages that remain
    seen = {1: set(), 2: set()}
    for ident, block in blocks:
        if ident.startswith(shape + "/") and ident.endswith("/noexpand"):
            assert block.stages[0] is None and block.add is None
            seen[1].add(block.modes()[1])
            seen[2].add(block.modes()[2])
    assert seen[1] == seen[2] == set(F.MODES), (shape, seen)


def test_bound_blocks_sit_at_the_bound(blocks):
    """the stage under test of each accumulator-bound block: the largest bias that keeps it bounded (mode 3), then the
    smallest that does not (mode 6); the same operands otherwise; extreme operands meet in it"""
    for pos in range(3):
        at, over = F.bound_block(pos, False), F.bound_block(pos, True)
        a, o = at.stages[pos], over.stages[pos]
        k = a.reduction
        assert int(np.abs(a.bias.astype(np.int64)).max()) + 65025 * k == 2 ** 30 - 1 and a.mode() == 3
        assert int(np.abs(o.bias.astype(np.int64)).max()) + 65025 * k == 2 ** 30 and o.mode() == 6
        assert np.array_equal(a.kernel, o.kernel) and np.array_equal(at.inp, over.inp)
        # a whole extreme window meets a whole extreme channel: |sum (a - izp)(w - kzp)| = K * 255 * 128 somewhere
        x = at.inp if pos == 0 else at.oracle()[pos - 1].reshape(-1)
        h, w = at.h, at.w
        dot = a.acc(x, at.batch, h, w, None, bias=np.zeros(a.channels, np.int32))
        assert int(np.abs(dot.astype(np.int64)).max()) == k * 255 * 128, (pos, int(np.abs(dot).max()), k * 255 * 128)


def test_floor_mutant_is_the_truncated_oracle():
    """the floor mutant of Stage.requantize never exceeds the oracle's byte, is at most one step below it, and differs"""
    rng = np.random.default_rng(5)
    acc = rng.integers(-2 ** 18, 2 ** 18, 4096).astype(np.int32)          # +-83 steps around zero point 100
    st = F.Stage(np.zeros((1, 1, 1, 1, 4), np.uint8), np.zeros(1, np.int32), 0, 127, 100, np.float32(2.0 ** -12 * 1.3))
    a, b = st.requantize(acc).astype(int), st.requantize(acc, "floor").astype(int)
    assert np.all((a - b >= 0) & (a - b <= 1)) and 0.3 < np.mean(a != b) < 0.7
