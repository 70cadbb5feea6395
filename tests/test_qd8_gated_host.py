"""CPU tier of the gated input of the dynamic fully connected operators: the numpy restatement of the header's definition
(tests/_gated.py), which the GPU tier takes as its expectation, against float64 and at the special values."""
import numpy as np
import pytest

from _gated import F32, gated, sigmoid

INF, NAN = float("inf"), float("nan")
DEN = 2.0 ** -140
SIGMOID_BOUND = 2.0 ** -21      # 4.46 * 2^-24 measured, rounded up to the next power of two


def sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-z.astype(np.float64)))


def test_sigmoid_against_float64():
    rng = np.random.default_rng(7)
    z = np.concatenate([np.linspace(-100, 100, 4_000_001), rng.normal(0, 3, 2_000_000)]).astype(F32)
    z = z[z > -80]
    want = sigmoid64(z)
    worst = float(np.max(np.abs(sigmoid(z).astype(np.float64) - want) / want))
    print(f"largest relative error {worst * 2 ** 24:.2f} * 2^-24")
    assert worst <= SIGMOID_BOUND
    below = sigmoid(np.array([-80, -81, -1e30, -INF], F32))
    assert (below == below[0]).all() and 1.8e-35 < below[0] < 1.81e-35       # exp(-80), about 1.5 * 2^-116


@pytest.mark.parametrize("alpha,limit,up_shift", [(1.0, INF, 0.0), (1.702, 7.0, 1.0)], ids=["silu", "clamped"])
def test_common_parameter_sets_against_float64(alpha, limit, up_shift):
    rng = np.random.default_rng(11)
    x = rng.normal(0, 4, (64, 512)).astype(F32)
    x[0, :8] = [100, 3, -100, 3, 3, 100, 3, -100]
    g, u = x[:, 0::2].astype(np.float64), x[:, 1::2].astype(np.float64)
    gc, uc = np.minimum(g, limit), np.clip(u, -limit, limit)
    z = (F32(alpha) * gc.astype(F32)).astype(F32)               # the definition's z: its rounding is not the sigmoid's error
    want = gc * sigmoid64(np.maximum(z, F32(-80))) * (uc + up_shift)
    got = gated(x, alpha, limit, up_shift).astype(np.float64)
    assert limit == INF or ((g > limit).any() and (u < -limit).any() and (z < -80).any())
    assert np.all(np.abs(got - want) <= SIGMOID_BOUND * np.abs(want))
    if limit == INF:
        assert np.array_equal(z, x[:, 0::2])                    # alpha = 1: h is g * sigmoid(g) * u itself


@pytest.mark.parametrize("g,u,params,want", [
    (NAN, 1.0, (1.0, INF, 0.0), NAN), (1.0, NAN, (1.0, INF, 0.0), NAN), (NAN, NAN, (1.702, 7.0, 1.0), NAN),
    (INF, 2.0, (1.0, INF, 0.0), INF), (INF, 2.0, (1.702, 7.0, 1.0), None),      # clamped to 7: finite, checked below
    (-INF, 2.0, (1.0, INF, 0.0), -INF), (-INF, 0.0, (1.0, INF, 0.0), NAN), (-INF, -1.0, (1.702, 7.0, 1.0), NAN),
    (1.0, INF, (1.0, INF, 0.0), INF), (1.0, -INF, (1.0, INF, 0.0), -INF),
    (DEN, 3.0, (1.0, INF, 0.0), 0.0), (-DEN, 3.0, (1.0, INF, 0.0), -0.0), (-DEN, -3.0, (64.0, INF, 0.0), 0.0),
    (0.0, 3.0, (1.0, INF, 0.0), 0.0), (-0.0, 3.0, (1.0, INF, 0.0), -0.0),
    (2.0, DEN, (1.0, INF, 0.0), 0.0), (2.0, -DEN, (1.0, INF, 0.0), -0.0), (-2.0, -0.0, (1.0, INF, 0.0), -0.0),   # -0 + 0 = +0
    (2.0, -1.0, (1.702, 7.0, 1.0), 0.0), (-2.0, -1.0, (1.702, 7.0, 1.0), -0.0),   # b = -1 + 1 = +0
    (2.0 ** -126, 1.0, (1.0, INF, 0.0), 0.0),                                     # a = 2^-127: flushed
    (-2.0 ** -125, 1e30, (1.0, INF, 0.0), -0.0), (2.0 ** -124, 1.0, (1.0, INF, 0.0), 2.0 ** -125),   # a = -2^-126 exactly: flushed too
])
def test_special_values(g, u, params, want):
    h = gated(np.array([[g, u]], F32), *params)
    if want is None:
        seven = gated(np.array([[7.0, 2.0]], F32), *params)
        assert h.view(np.uint32) == seven.view(np.uint32) and 20.9 < h[0, 0] < 21.0
    elif np.isnan(want):
        assert np.isnan(h[0, 0])
    else:
        assert h.view(np.uint32)[0, 0] == np.array(want, F32).view(np.uint32), (h, want)


# ---- the built library, without a GPU ----
from test_kernel_resources import kernels     # noqa: E402,F401  (the fixture: the gfx950 code objects' metadata)

SETUPS = ("qnnp_gfx950_setup_fully_connected_nc_f32_qd8_gated", "qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_gated")


def test_the_gated_kernels_use_no_scratch_memory(kernels):
    gated = {name: k for name, k in kernels.items() if "f32_qd8_gated_rows_" in name}
    assert len(gated) == 6, sorted(gated)             # wave, block, twopass, each with its _x4 flavour
    for name, k in gated.items():
        assert k["scratch"] == 0 and k["spill"] == 0, (name, k)


@pytest.mark.parametrize("change,want", [({}, 0), ({"input_stride": 2 * 80 - 1}, -4), ({"k": 0}, -4), ({"k": 32769, "k_pad": 32832}, -4),
                                         ({"k_pad": 80}, -4), ({"input": 0x1004}, 0), ({"input": 0x1002}, -4), ({"quantized": 0x2008}, -4)],
                         ids=lambda v: "_".join(f"{key}{value}" for key, value in v.items()) if isinstance(v, dict) else str(v))
def test_the_row_launch_validates_like_the_plain_one(product, change, want):
    """qnnp_hip_qd8_gated_rows_run answers from its arguments alone before it touches a device: rows = 0 launches nothing"""
    import ctypes

    class Args(ctypes.Structure):
        _fields_ = [("input", ctypes.c_void_p), ("quantized", ctypes.c_void_p), ("row_table", ctypes.c_void_p),
                    ("rows", ctypes.c_uint32), ("k", ctypes.c_uint32), ("k_pad", ctypes.c_uint32), ("input_stride", ctypes.c_uint64),
                    ("alpha", ctypes.c_float), ("limit", ctypes.c_float), ("up_shift", ctypes.c_float)]
    values = dict(input=0x1000, quantized=0x2000, row_table=0x3000, rows=0, k=80, k_pad=128, input_stride=160,
                  alpha=1.0, limit=INF, up_shift=0.0)
    values.update(change)
    assert all(hasattr(product.lib, symbol) for symbol in SETUPS)
    run = product.lib.qnnp_hip_qd8_gated_rows_run
    run.argtypes, run.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    assert run(ctypes.byref(Args(**values)), None) == want
