"""The top-k softmax router and the weighted combine of include/qnnpack_gfx950_moe.h, restated in numpy line for line: every
float operation on float32 arrays, rounded once by IEEE; clamp and selection on integer keys."""
import numpy as np

F32, U32 = np.float32, np.uint32
TINY = F32(2.0 ** -126)


def _c(text):
    return F32(float.fromhex(text))


def exp_of(y):
    """the definition's e for float32 y in [-80, 0]"""
    assert y.dtype == np.float32
    n = np.rint(y * _c("0x1.715476p+0"))
    r1 = y - n * _c("0x1.62E400p-1")
    r2 = r1 - n * _c("0x1.7F7D1Cp-20")
    p = np.full_like(y, _c("0x1.0F9F9Cp-7"))
    for c in ("0x1.573A1Ap-5", "0x1.555A80p-3", "0x1.FFFDC6p-2", "0x1.FFFFF6p-1", "0x1p+0"):
        p = p * r2
        p = p + _c(c)
    e = p * ((n.astype(np.int32) + 127) << 23).astype(np.int32).view(F32)
    assert e.dtype == np.float32
    return e


def router(logits, a, first_group=0):
    """ids int32 [T][A] and weights float32 [T][A] of logits float32 [T][E]"""
    assert logits.dtype == np.float32 and logits.ndim == 2 and 1 <= a <= logits.shape[1]
    bits = np.ascontiguousarray(logits).view(U32)
    magnitude = bits & U32(0x7FFFFFFF)
    c = np.where(magnitude == 0x7F800000, (bits & U32(0x80000000)) | U32(0x7F7FFFFF), bits)
    c = np.where(magnitude > 0x7F800000, U32(0xFF7FFFFF), c).astype(U32)
    key = c ^ np.where(c >> 31 != 0, U32(0xFFFFFFFF), U32(0x80000000))
    # descending key, ascending e among equals: a stable sort of the keys' complements
    sel = np.argsort(0xFFFFFFFF - key.astype(np.int64), axis=1, kind="stable")[:, :a]
    with np.errstate(all="ignore"):
        l = np.take_along_axis(c.view(F32), sel, axis=1)
        d = l - l[:, :1]
        e = exp_of(np.where(d < F32(-80), F32(-80), d))
        s = e[:, 0]
        for i in range(1, a):
            s = s + e[:, i]
        w = e / s[:, None]
    assert w.dtype == np.float32
    return sel.astype(np.int32) - np.int32(first_group), w


def flush(v):
    return np.where(np.abs(v) <= TINY, np.copysign(F32(0), v), v)


def combine(x, w, ids, a, groups, backwards=False):
    """output float32 [T][N] of x float32 [T A][N], w float32 [T A], ids int32 [T A]; rows that do not count are not used"""
    assert x.dtype == np.float32 and w.dtype == np.float32 and ids.dtype == np.int32 and len(x) == len(w) == len(ids)
    tokens = len(ids) // a
    acc = np.zeros((tokens, x.shape[1]), F32)
    with np.errstate(all="ignore"):
        for i in (reversed(range(a)) if backwards else range(a)):
            j = np.arange(tokens) * a + i
            counts = ((ids[j] >= 0) & (ids[j] < groups))[:, None]
            p = flush(w[j][:, None] * np.where(counts, x[j], F32(0)))
            acc = np.where(counts, flush(acc + p), acc)
    assert acc.dtype == np.float32
    return acc
