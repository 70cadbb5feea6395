"""The normalized input of the dynamically quantized fully connected operator (the _rmsnorm setups), restated in numpy line
for line from include/qnnpack_gfx950_dynamic.h. Every array is float32 and every operation one IEEE operation, rounded once;
numpy keeps denormals, so the flushes are the explicit ones of the definition."""
import numpy as np

F32 = np.float32
TINY = F32(2.0 ** -126)


def flush(v):
    return np.where(np.abs(v) <= TINY, np.copysign(F32(0), v), v).astype(F32)


def flush_lt(v):
    return np.where(np.abs(v) < TINY, np.copysign(F32(0), v), v).astype(F32)


def square_sum(x, pieces=1024):
    """S [rows] of x [rows][K]: the in-piece tree over sixteen, then the tree over `pieces` zero-padded pieces"""
    rows, k = x.shape
    assert x.dtype == F32 and k <= 16 * pieces and pieces & (pieces - 1) == 0
    with np.errstate(all="ignore"):
        sq = np.zeros((rows, 16 * pieces), F32)
        sq[:, :k] = flush(x * x)
        u = sq.reshape(rows, pieces, 16)
        for half in (8, 4, 2, 1):
            u = u[:, :, :half] + u[:, :, half:2 * half]
        s = u.reshape(rows, pieces)
        while s.shape[1] > 1:
            s = s.reshape(rows, 2, s.shape[1] // 2)           # s[j] + s[j + h], h = half of what is left
            s = s[:, 0, :] + s[:, 1, :]
    assert s.dtype == F32
    return s[:, 0]


def rmsnorm(x_in, gamma, epsilon, residual=None):
    """(h, x) of input rows x_in [rows][K], gamma [K] and an optional residual [rows][K]"""
    assert x_in.dtype == F32 and gamma.dtype == F32
    with np.errstate(all="ignore"):
        x = x_in if residual is None else flush_lt(flush_lt(x_in) + flush_lt(residual))
        m = square_sum(x) / F32(x.shape[1])
        v = m + F32(epsilon)
        r = F32(1) / np.sqrt(v)
        t = flush(x * r[:, None])
        h = flush(t * gamma[None, :])
    assert r.dtype == F32 and h.dtype == F32 and x.dtype == F32
    return h, x
