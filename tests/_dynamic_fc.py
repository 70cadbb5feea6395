"""The dynamically quantized fully connected operator, restated in numpy (include/qnnpack_gfx950_dynamic.h has the
definition). Every float operation is a np.float32 operation, rounded once by IEEE; np.rint is ties to even; the
accumulator is int64 and asserted to fit int32."""
import numpy as np

F32 = np.float32


def quantize_rows(x):
    """x [rows][K] float32 -> (q [rows][K] int32 in [0, 255], scale [rows] float32, zp [rows] int32)"""
    assert x.dtype == np.float32 and x.ndim == 2
    with np.errstate(all="ignore"):
        lo = np.fmin.reduce(x, axis=1, initial=F32(0))          # fmin / fmax ignore NaN
        hi = np.fmax.reduce(x, axis=1, initial=F32(0))
        scale = (hi - lo) / F32(255)
        scale = np.where((scale >= F32(2.0 ** -60)) & (scale <= F32(2.0 ** 60)), scale, F32(1)).astype(F32)
        inv = F32(1) / scale
        zp = np.rint(np.minimum(-lo * inv, F32(255))).astype(np.int32)
        t = x * inv[:, None]
        t = np.where(np.isnan(t), F32(0), t)
        t = np.minimum(np.maximum(t, (-zp).astype(F32)[:, None]), (255 - zp).astype(F32)[:, None])
        q = np.rint(t).astype(np.int32) + zp[:, None]
    assert t.dtype == np.float32 and inv.dtype == np.float32 and q.min() >= 0 and q.max() <= 255
    return q, scale, zp


def expected(x, kernel, kernel_scales, bias, output_min=-np.inf, output_max=np.inf):
    """y [rows][N] float32 of x [rows][K], kernel [N][K] int8, kernel_scales [N], bias [N] or None"""
    q, scale, zp = quantize_rows(x)
    acc = (q.astype(np.int64) - zp[:, None]) @ kernel.astype(np.int64).T
    assert np.abs(acc).max() < 2 ** 31, "the accumulator must fit int32 by itself"
    s = scale[:, None] * kernel_scales.astype(F32)[None, :]
    y = acc.astype(F32) * s
    y = y + (np.zeros(kernel.shape[0], F32) if bias is None else bias.astype(F32))[None, :]
    y = np.minimum(np.maximum(y, F32(output_min)), F32(output_max))
    assert s.dtype == np.float32 and y.dtype == np.float32
    return y


def rows_kernel(k, batch, input_address, input_stride):
    """the row kernel the header's dispatch rule names"""
    name = "f32_qd8_rows_wave" if k <= 1024 else ("f32_qd8_rows_block" if k <= 16384 else "f32_qd8_rows_twopass")
    wide = input_address % 16 == 0 and (batch == 1 or input_stride % 4 == 0)
    return name if wide else name + "_x4"


def gemm_kernel(batch):
    return "qd8_f32_gemv_mfma_16" if batch <= 16 else "qd8_f32_gemm_mfma_128x128"


def problem(name, batch, k, n):
    """(x, kernel, kernel_scales, bias) of a case, from its name"""
    rng = np.random.default_rng(sum(name.encode()) * 7919 + batch * 31 + k * 17 + n)
    x = (rng.standard_normal((batch, k)) * rng.uniform(0.1, 4.0, size=(batch, 1))).astype(F32)
    kernel = rng.integers(-128, 128, size=(n, k), dtype=np.int8)
    kernel_scales = rng.uniform(0.002, 0.05, size=n).astype(F32)
    bias = rng.standard_normal(n).astype(F32)
    return x, kernel, kernel_scales, bias
