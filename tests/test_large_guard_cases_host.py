"""CPU tier: the cases of tests/test_large_guards_gpu.py sit where that file says they sit. For every pair of
tests/_large_guards.py: the spans its guard computes (restated there, beside the case) lie below every bound at the last
accepted size; at the first refused size the intended term, and no other, is at or past its bound; both sizes pass the
operator's setup limits (convolution.c / deconvolution.c: rows at most (2^32 - 1) / 2 and at most 2^31 - 1 bytes per input
image; fully-connected.c: the same row limit); and the peak device memory of the case is within _large.BUDGET. These are
conditions on the inputs: nothing here runs a kernel."""
import dataclasses

import numpy as np
import pytest

import _fused as fb
import _large as lg
import _large_guards as G
import _perchannel as pc
from _cases import FcCase


@pytest.mark.parametrize("pair", G.PAIRS, ids=G.PAIR_IDS)
def test_pair_sits_on_its_bound(pair):
    last, refused = pair.guard(pair.case), pair.guard(pair.refused)
    assert pair.term in last, (pair.name, sorted(last))
    assert G.crossed(last) == set(), f"{pair.name}: the last accepted size crosses {sorted(G.crossed(last))}: {last}"
    assert G.crossed(refused) == {pair.term}, f"{pair.name}: the first refused size crosses {sorted(G.crossed(refused))}, not {pair.term} alone: {refused}"
    assert refused[pair.term][0] - last[pair.term][0] > 0
    assert pair.refused.batch == pair.case.batch + 1


@pytest.mark.parametrize("pair", G.PAIRS, ids=G.PAIR_IDS)
def test_pair_passes_setup_and_fits_the_budget(pair):
    for case in (pair.case, pair.refused):
        for limit, (value, most) in G.setup_limits(case).items():
            assert value <= most, f"{case.name}: {limit} {value} is past the setup limit {most}"
        assert G.nbytes(case) <= lg.BUDGET, f"{case.name}: {G.nbytes(case) / lg.GiB:.2f} GiB"


def test_batch_counts_are_the_ones_the_guards_give():
    """the counts the cases were chosen by, from the bounds (none is written down in _large_guards.py)"""
    assert (G.C3_OUT_LAST, G.C3_IN_LAST, G.C3_DIV_LAST) == (65535, 174762, 16383)
    assert (G.C3_32_OUT_LAST, G.C3_32_IN_LAST, G.C3_GRID_LAST) == (131071, 699050, (1 << 24) - 1)
    assert (G.GW_LAST, G.GWK_LAST, G.M16_LAST, G.UP_LAST) == ((1 << 25) - 1, 64, 21399, 131071)
    assert (65 * G.M16_WAVES_LAST + 8) * 65 < G.B32 <= (65 * (G.M16_WAVES_LAST + 1) + 8) * 65
    assert (35 * G.M16_GRID_LAST + 3) // 4 < (1 << 24) <= (35 * (G.M16_GRID_LAST + 1) + 3) // 4


C3_PAIRS = [p for p in G.PAIRS if p.guard is G.c3rows_guard]


@pytest.mark.parametrize("pair", C3_PAIRS, ids=[p.name for p in C3_PAIRS])
def test_lds_flavour_plan_of_the_first_layer_cases(pair):
    """code 30 is listed exactly where c3lds_plan takes the shape, on both sides of the bound -- so that its refusal past the
    bound is conv_c3rows*_supported's; and the plan's own batch term lies inside units*pairs (bands <= pairs)"""
    for case in (pair.case, pair.refused):
        plan = G.c3lds_plan(case)
        assert (plan is not None) == (30 in pair.forced), (case.name, plan)
        if plan is not None:
            assert plan["bands"] <= plan["pairs"] and plan["wgs*bands"] < G.B32 and plan["grid"] < G.B32
            assert plan["wgs*bands"] <= G.c3rows_guard(case)["units*pairs"][0]
    assert pair.case.batch * int(np.prod(G.output_hw(pair.case))) >= 2048          # q8igemm.hip:make_plan's row rule


M16_PAIRS = [p for p in G.PAIRS if p.guard is G.dwmfma16_guard]


@pytest.mark.parametrize("pair", M16_PAIRS, ids=[p.name for p in M16_PAIRS])
def test_dwmfma16_plan_does_not_depend_on_the_device(pair):
    """the row segments -- and with them the third term -- follow the CU count only below 12 waves per CU"""
    for case in (pair.case, pair.refused):
        terms, per_seg = G.dwmfma16_plan(case)
        assert per_seg >= 12 * 1024
        assert terms == G.dwmfma16_plan(case, cu_count=8)[0] == G.dwmfma16_plan(case, cu_count=1024)[0]


def test_stream_c3_cases_sit_on_both_sides_of_the_staged_flavour():
    staged, unstaged, past = G.STREAM_C3
    assert G.crossed(G.stream_c3_guard(staged)) == set()
    assert G.crossed(G.stream_c3_guard(unstaged)) == {"input"} and unstaged.batch == staged.batch + 1
    assert G.crossed(G.stream_c3_guard(past)) == set() and G.spans(past)[1] > G.B32
    for case in G.STREAM_C3:
        assert case.goc % 16 == 0                      # the staged flavour's other condition
        assert all(v <= most for v, most in G.setup_limits(case).values()) and G.nbytes(case) <= lg.BUDGET


def test_gwk_rows_sit_on_both_sides_of_the_span():
    last, refused = G.GWK_CASE, dataclasses.replace(G.GWK_CASE, batch=G.GWK_CASE.batch + 1)
    assert G.crossed(G.gw_guard(last)) == set() and G.crossed(G.gw_guard(refused)) == {"input"}
    # the split-K flavour: K >= 256 and at most two blocks per CU (q8pwconv.hip:pwstream_gw_plan), on any device of 4 CUs or more
    assert last.input_channels >= 256 and G.gw_guard(refused)["units"][0] <= 8
    assert G.spans(refused)[0] + refused.batch * 64 <= lg.BUDGET


def test_cases_past_4g_are_past_4g_and_fit():
    for case in G.LONGK_CASES + [G.D2S_CASE]:
        assert max(G.spans(case)) > G.B32, case.name
        assert all(v <= most for v, most in G.setup_limits(case).values()), case.name
        assert G.nbytes(case) <= lg.BUDGET, case.name
        if isinstance(case, FcCase):           # pwstream_longk_plan's K conditions: 256 < K <= 1024 in whole 16-byte pieces
            assert 256 < case.input_channels <= 1024 and case.input_channels % 16 == 0 and case.output_channels % 16 == 0
    assert G.spans(G.LONGK_CASES[0])[0] > G.B32 and G.spans(G.LONGK_CASES[1])[1] > G.B32
    # residual: input + residual + output; per-channel: 64 -> 40 rows and 58-channel images; multiply: three tensors
    assert G.RESIDUAL_ROWS * 64 > G.B32 and G.RESIDUAL_ROWS * (16 + 64 + 64) + 2 * lg.CHUNK <= lg.BUDGET
    assert G.PC_FC_ROWS * 64 > G.B32 and G.PC_FC_ROWS * (64 + 40) + 2 * lg.CHUNK <= lg.BUDGET
    assert G.PC_DW_BATCH * 28 * 28 * 58 > G.B32 and 2 * G.PC_DW_BATCH * 28 * 28 * 58 + 2 * lg.CHUNK <= lg.BUDGET
    for stride, channels in ((G.MUL_STRIDE_X16, 1024), (G.MUL_STRIDE_X1, 1021)):
        assert 2 * stride > G.B32 and 3 * (2 * stride + channels) <= lg.BUDGET
    assert G.MUL_STRIDE_X16 % 16 == 0 and G.MUL_STRIDE_X1 % 4 == 1


def test_fused_block_limit_batch():
    """fused-block.c: input pixels x input stride at most 2^32 - 1; the contract's block is 28 x 28 x 24 in and out"""
    batch = (G.B32 - 1) // (28 * 28 * 24)
    assert batch * 28 * 28 * 24 <= G.B32 - 1 < (batch + 1) * 28 * 28 * 24
    assert batch * 28 * 28 <= (G.B32 - 1) // 2
    assert 2 * batch * 28 * 28 * 24 + 2 * lg.CHUNK <= lg.BUDGET


def test_small_problems_hold_their_sensitivity_conditions():
    """the fused block and the per-channel problems of the GPU file, at a marker count the GPU cases have: Block.check and
    Problem.check state conditions on the inputs, so they can fail here first"""
    n = lg.PERIOD + 5
    fb.build_block("fused_block_at_limit", fb.FIXED, cin=24, hidden=144, cout=24, h=28, w=28, batch=n, residual=False).check()
    pc.fc_problem("pc_fc_64_40_past_4g", n * G.ROWS, 64, 40).check()
    pc.conv_problem("pc_dw_58_past_4g", n, (28, 28), (3, 3), (1, 1, 1, 1), groups=58).check()
