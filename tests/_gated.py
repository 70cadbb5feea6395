"""The gated input of the dynamically quantized fully connected operator, restated in numpy line for line
(include/qnnpack_gfx950_dynamic.h has the definition): every operation on float32 arrays, rounded once by IEEE."""
import numpy as np

F32 = np.float32
TINY = F32(2.0 ** -126)


def _c(text):
    return F32(float.fromhex(text))


def sigmoid(z):
    """the definition's s for float32 z (NaN where z is NaN)"""
    assert z.dtype == np.float32
    with np.errstate(all="ignore"):
        y = -np.abs(z)
        y = np.where(y < F32(-80), F32(-80), y)
        n = np.rint(y * _c("0x1.715476p+0"))
        r1 = y - n * _c("0x1.62E400p-1")
        r2 = r1 - n * _c("0x1.7F7D1Cp-20")
        p = np.full_like(z, _c("0x1.0F9F9Cp-7"))
        for c in ("0x1.573A1Ap-5", "0x1.555A80p-3", "0x1.FFFDC6p-2", "0x1.FFFFF6p-1", "0x1p+0"):
            p = p * r2
            p = p + _c(c)
        n_int = np.where(np.isnan(n), F32(0), n).astype(np.int32)          # a NaN is never converted
        e = p * ((n_int + 127) << 23).astype(np.int32).view(F32)
        d = F32(1) + e
        q = e / d
        s = np.where(z > 0, F32(1) - q, q)
    assert s.dtype == np.float32
    return s


def gated(x, alpha, limit, up_shift):
    """h [rows][K] float32 of x [rows][2 K]: gate at even, up at odd elements"""
    assert x.dtype == np.float32 and x.shape[-1] % 2 == 0
    alpha, limit, up_shift = F32(alpha), F32(limit), F32(up_shift)
    g, u = x[..., 0::2], x[..., 1::2]
    with np.errstate(all="ignore"):
        gc = np.where(g > limit, limit, g)
        uc = np.where(u > limit, limit, np.where(u < -limit, -limit, u))
        z = alpha * gc
        a = gc * sigmoid(z)
        a = np.where(np.abs(a) <= TINY, np.copysign(F32(0), a), a)
        b = uc + up_shift
        b = np.where(np.abs(b) < TINY, np.copysign(F32(0), b), b)
        h = a * b
    assert z.dtype == np.float32 and h.dtype == np.float32
    return h
