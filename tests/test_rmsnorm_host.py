"""CPU tier of the normalized (residual add + RMSNorm) input of the dynamic fully connected operators: the header and
DYNAMIC_API agree, the numpy restatement of the definition (tests/_rmsnorm.py), which the GPU tier takes as its expectation,
against float64 and at the properties the definition claims, and the built library without a GPU."""
import ctypes

import numpy as np
import pytest

from _headers import prototypes
from _rmsnorm import F32, rmsnorm, square_sum
from qnnpack_amd import binding
from test_kernel_resources import kernels     # noqa: F401  (the fixture: the gfx950 code objects' metadata)

SETUPS = ("qnnp_gfx950_setup_fully_connected_nc_f32_qd8_rmsnorm", "qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_rmsnorm")


def test_the_two_setups_are_the_image_of_their_prototypes_and_api_is_untouched():
    declared = prototypes("qnnpack_gfx950_dynamic.h")
    table = {f.symbol: f for f in binding.DYNAMIC_API}
    assert set(table) == set(declared) and len(binding.API) == 65 and not set(SETUPS) & set(binding.API)
    for symbol in SETUPS:
        ret, params = declared[symbol]
        f = table[symbol]
        assert ret == "enum qnnp_status" and f.bound == binding.IF_PRESENT and f.methods
        assert [p.name for p in f.params][1:] == [name for _, name in params][1:]
        for (c_type, _), p in zip(params, f.params):
            assert (p.kind == "tensor") == (c_type in ("float*", "int32_t*")), (symbol, p.name, c_type)


@pytest.mark.parametrize("k", [1, 17, 1040, 2880, 16384])
def test_restatement_against_float64(k):
    """relative 2^-20 on h: the sum has 15 roundings, squares included, which the root halves; five more from the division by
    K, the add, the root, the reciprocal and the two products: about 12.5 * 2^-24"""
    rng = np.random.default_rng(k)
    x_in, residual = (rng.normal(0, 3, (4, k)).astype(F32) for _ in range(2))
    gamma = rng.uniform(0.5, 2, k).astype(F32)
    for res in (None, residual):
        h, x = rmsnorm(x_in, gamma, 1e-5, res)
        assert np.array_equal(x, x_in if res is None else x_in + res)
        x64 = x.astype(np.float64)
        want = x64 / np.sqrt((x64 * x64).mean(axis=1, keepdims=True) + np.float64(F32(1e-5))) * gamma
        worst = float(np.max(np.abs(h - want) / np.abs(want)))
        print(f"K = {k}: largest relative error {worst * 2 ** 24:.2f} * 2^-24")
        assert worst <= 2.0 ** -20


@pytest.mark.parametrize("k,pieces", [(1, 1), (16, 1), (17, 2), (1040, 128), (2880, 256), (4097, 512), (16384, 1024)])
def test_the_tree_over_1024_pieces_is_the_tree_over_the_pieces_that_cover_the_row(k, pieces):
    x = np.random.default_rng(k).normal(0, 3, (3, k)).astype(F32)
    x[1, ::7] = 1e-30                               # squares that are flushed
    assert np.array_equal(square_sum(x).view(np.uint32), square_sum(x, pieces).view(np.uint32))


def test_a_row_whose_sequential_sum_differs_from_the_tree():
    """1 and thirty-one 2^-12: one after the other every 2^-24 is half a last place of 1 and is rounded away; the tree adds
    them to each other first. The GPU tier runs this row."""
    x = fixed_row()
    sequential = F32(0)
    for v in x[0]:
        sequential = F32(sequential + F32(v * v))
    tree = square_sum(x)[0]
    assert sequential == 1 and tree == F32(1 + 30 * 2.0 ** -24) and tree.view(np.uint32) != sequential.view(np.uint32)


def fixed_row():
    x = np.full((1, 32), 2.0 ** -12, F32)
    x[0, 0] = 1
    return x


def test_special_rows_of_the_restatement():
    gamma = np.ones(16, F32)
    x = np.zeros((4, 16), F32)
    x[0, 3], x[1, 3], x[2, :] = np.nan, np.inf, 3e19       # NaN; an infinite element; a finite row whose S overflows
    x[3, :4] = [2.0 ** -140, -2.0 ** -140, 2.0 ** -70, 0]  # denormals square to zero, 2^-70 to 2^-140: flushed too
    h, _ = rmsnorm(x, gamma, 2.0 ** -40)
    assert np.isnan(h[0]).all() and np.isnan(h[1, 3]) and (np.delete(h[1], 3) == 0).all() and (h[2] == 0).all()
    assert h[3, 0] == F32(2.0 ** -140) * F32(2.0 ** 20) and h[3, 2] == F32(2.0 ** -50)       # S = 0: r = 2^20 exactly
    _, s = rmsnorm(np.array([[2.0 ** -127, -2.0 ** -126, 2.0 ** -126]], F32), gamma[:3], 1.0,
                   np.array([[1.0, 2.0 ** -127, -1.5 * 2.0 ** -126]], F32))
    assert np.array_equal(s.view(np.uint32), np.array([[1.0, -2.0 ** -126, -0.0]], F32).view(np.uint32))


# ---- the built library, without a GPU ----
def test_the_rmsnorm_kernels_use_no_scratch_memory(kernels):
    found = {name: k for name, k in kernels.items() if "f32_qd8_rmsnorm_rows_" in name}
    assert len(found) == 8, sorted(found)           # wave and block, each with or without a residual, each with its _x4 flavour
    for name, k in found.items():
        assert k["scratch"] == 0 and k["spill"] == 0, (name, k)


@pytest.mark.parametrize("change,want", [
    ({}, 0), ({"residual": 0x5000, "residual_out": 0x5000, "residual_stride": 80}, 0), ({"input": 0x1004}, 0),
    ({"gamma": 0}, -4), ({"residual_out": 0x5000}, -4), ({"residual": 0x5000, "residual_stride": 79}, -4),
    ({"input_stride": 79}, -4), ({"k": 0}, -4), ({"k": 16385, "k_pad": 16448, "input_stride": 16385}, -4), ({"k_pad": 80}, -4),
    ({"gamma": 0x4002}, -4), ({"residual": 0x5001, "residual_stride": 80}, -4), ({"input": 0x1002}, -4), ({"quantized": 0x2008}, -4)],
    ids=lambda v: "_".join(f"{key}{value}" for key, value in v.items()) if isinstance(v, dict) else str(v))
def test_the_row_launch_validates_its_arguments(product, change, want):
    """qnnp_hip_qd8_rmsnorm_rows_run answers from its arguments alone before it touches a device: rows = 0 launches nothing"""
    class Args(ctypes.Structure):
        _fields_ = [("input", ctypes.c_void_p), ("quantized", ctypes.c_void_p), ("row_table", ctypes.c_void_p),
                    ("rows", ctypes.c_uint32), ("k", ctypes.c_uint32), ("k_pad", ctypes.c_uint32), ("input_stride", ctypes.c_uint64),
                    ("gamma", ctypes.c_void_p), ("residual", ctypes.c_void_p), ("residual_out", ctypes.c_void_p),
                    ("residual_stride", ctypes.c_uint64), ("epsilon", ctypes.c_float)]
    values = dict(input=0x1000, quantized=0x2000, row_table=0x3000, rows=0, k=80, k_pad=128, input_stride=80, gamma=0x4000,
                  residual=0, residual_out=0, residual_stride=0, epsilon=1e-5)
    values.update(change)
    assert all(hasattr(product.lib, symbol) for symbol in SETUPS)
    run = product.lib.qnnp_hip_qd8_rmsnorm_rows_run
    run.argtypes, run.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    assert run(ctypes.byref(Args(**values)), None) == want
