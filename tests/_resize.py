"""The definition of the bilinear resize operator (qnnp_gfx950_*_resize_bilinear2d_nhwc_u8, include/qnnpack_gfx950.h)
restated in numpy and Python integers, the kernel selection rule of hip/u8resize.hip, and the case lists the CPU and GPU
tiers share. No reference operator exists: the header's definition is integers only, so this restatement IS the
expectation, byte for byte.

Per axis, with n_in input and n_out output positions and output index o (uint64 arithmetic, divisions round down):
  half-pixel centres: num = max((2o + 1) n_in - n_out, 0);  f = (4096 num + 2 n_out) / (4 n_out)
  align corners:      f = 0 if n_out == 1 else (4096 o (n_in - 1) + (n_out - 1)) / (2 (n_out - 1))
  i0 = min(f >> 11, n_in - 1), i1 = min(i0 + 1, n_in - 1), w = 0 if i0 == i1 else f & 2047
and every output byte is (top (2048 - wy) + bot wy + 2^21) >> 22 with top / bot the two row blends in Q11.
"""
import zlib

import numpy as np

FILL = 0xA5
ALIGN_CORNERS = 1          # QNNP_GFX950_RESIZE_ALIGN_CORNERS
SIZE_LIMIT = 1 << 24       # sizes are below it


def _seed(name: str) -> int:
    return 0x5E51 ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


def axis_entry(n_in: int, n_out: int, align: bool, o: int):
    """(i0, i1, w) of one output index, in Python integers"""
    if align:
        f = 0 if n_out == 1 else (4096 * o * (n_in - 1) + (n_out - 1)) // (2 * (n_out - 1))
    else:
        num = max((2 * o + 1) * n_in - n_out, 0)
        f = (4096 * num + 2 * n_out) // (4 * n_out)
    i0 = min(f >> 11, n_in - 1)
    i1 = min(i0 + 1, n_in - 1)
    return i0, i1, 0 if i0 == i1 else f & 2047


def axis(n_in: int, n_out: int, align: bool):
    """(i0, i1, w) for every output index, as three int64 arrays (every intermediate is below 2^62)"""
    assert 0 < n_in < SIZE_LIMIT and 0 < n_out < SIZE_LIMIT
    o = np.arange(n_out, dtype=np.int64)
    if align:
        f = np.zeros(n_out, np.int64) if n_out == 1 else (4096 * o * (n_in - 1) + (n_out - 1)) // (2 * (n_out - 1))
    else:
        num = np.maximum((2 * o + 1) * n_in - n_out, 0)
        f = (4096 * num + 2 * n_out) // (4 * n_out)
    i0 = np.minimum(f >> 11, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, np.where(i0 == i1, 0, f & 2047)


def blend(t00, t01, t10, t11, wx, wy) -> np.ndarray:
    """the four taps of every output byte and the two Q11 weights (broadcastable arrays) -> the output bytes"""
    t00, t01, t10, t11 = (t.astype(np.uint32) for t in (t00, t01, t10, t11))
    wx, wy = np.asarray(wx).astype(np.uint32), np.asarray(wy).astype(np.uint32)
    top = t00 * (2048 - wx) + t01 * wx
    bot = t10 * (2048 - wx) + t11 * wx
    acc = top * (2048 - wy) + bot * wy + (1 << 21)
    assert acc.dtype == np.uint32 and int(acc.max()) < 2 ** 31
    return (acc >> 22).astype(np.uint8)


def resize(x: np.ndarray, out_h: int, out_w: int, align: bool, rows=None) -> np.ndarray:
    """x [batch][in_h][in_w][channels] uint8 -> [batch][out_h][out_w][channels] uint8; with `rows` (output row
    indices) only those output rows: [batch][len(rows)][out_w][channels]"""
    assert x.dtype == np.uint8 and x.ndim == 4
    y0, y1, wy = axis(x.shape[1], out_h, align)
    if rows is not None:
        y0, y1, wy = y0[rows], y1[rows], wy[rows]
    x0, x1, wx = axis(x.shape[2], out_w, align)
    return blend(x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1],
                 wx[None, None, :, None], wy[None, :, None, None])


def taps(x: np.ndarray, out_h: int, out_w: int, align: bool):
    """the four taps of every output byte, as four [batch][out_h][out_w][channels] arrays"""
    y0, y1, _ = axis(x.shape[1], out_h, align)
    x0, x1, _ = axis(x.shape[2], out_w, align)
    return x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]


def ideal(x: np.ndarray, out_h: int, out_w: int, align: bool) -> np.ndarray:
    """the real-valued bilinear interpolation in float64 (source coordinates clamped to the image, as PyTorch's)"""
    def coords(n_in, n_out):
        o = np.arange(n_out, dtype=np.float64)
        if align:
            s = np.zeros(n_out) if n_out == 1 else o * (n_in - 1) / (n_out - 1)
        else:
            s = np.maximum((o + 0.5) * n_in / n_out - 0.5, 0.0)
        s = np.minimum(s, n_in - 1)
        i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0
    y0, y1, fy = coords(x.shape[1], out_h)
    x0, x1, fx = coords(x.shape[2], out_w)
    v = x.astype(np.float64)
    fx = fx[None, None, :, None]
    fy = fy[None, :, None, None]
    top = v[:, y0][:, :, x0] * (1 - fx) + v[:, y0][:, :, x1] * fx
    bot = v[:, y1][:, :, x0] * (1 - fx) + v[:, y1][:, :, x1] * fx
    return top * (1 - fy) + bot * fy


def span(pixels: int, stride: int, channels: int) -> int:
    return (pixels - 1) * stride + channels if pixels else 0


def pixels_view(buf: np.ndarray, batch: int, h: int, w: int, stride: int, channels: int) -> np.ndarray:
    """the [batch][h][w][channels] view of a strided NHWC tensor (no copy)"""
    return np.lib.stride_tricks.as_strided(buf, shape=(batch, h, w, channels),
                                           strides=(h * w * stride, w * stride, stride, 1))


class Case:
    """one setup: geometry, channels, pixel strides (0 = dense) and the mode"""

    def __init__(self, batch, in_h, in_w, out_h, out_w, channels, in_stride=0, out_stride=0, align=False):
        self.batch, self.in_h, self.in_w, self.out_h, self.out_w, self.channels = batch, in_h, in_w, out_h, out_w, channels
        self.in_stride, self.out_stride, self.align = in_stride or channels, out_stride or channels, bool(align)

    @property
    def flags(self):
        return ALIGN_CORNERS if self.align else 0

    @property
    def in_pixels(self):
        return self.batch * self.in_h * self.in_w

    @property
    def out_pixels(self):
        return self.batch * self.out_h * self.out_w

    @property
    def in_span(self):
        return span(self.in_pixels, self.in_stride, self.channels)

    @property
    def out_span(self):
        return span(self.out_pixels, self.out_stride, self.channels)

    def setup_args(self, x, y):
        return (self.batch, self.in_h, self.in_w, self.out_h, self.out_w, x, self.in_stride, y, self.out_stride)

    def __repr__(self):
        return (f"{self.batch}x{self.in_h}x{self.in_w}x{self.channels}->{self.out_h}x{self.out_w}"
                f"_s{self.in_stride}_{self.out_stride}{'_ac' if self.align else ''}")


def tensors(name: str, c: Case):
    """random input bytes with ONE channel drawn from {0, 255} only -- rounding ties and the 255 * 2^22 top of the
    accumulator both occur -- and the FILL-ed output buffer. In that channel the first 2 x 2 pixels of the first image
    are 0 and the last 2 x 2 pixels of the last image 255, so the expectation holds both values wherever the first output
    pixel blends only the former and the last only the latter (has_extremes)."""
    rng = np.random.default_rng(_seed(name))
    x = rng.integers(0, 256, size=c.in_span, dtype=np.uint8)
    view = pixels_view(x, c.batch, c.in_h, c.in_w, c.in_stride, c.channels)
    view[..., c.channels // 2] = rng.integers(0, 2, size=view.shape[:3], dtype=np.uint8) * 255
    view[0, :2, :2, c.channels // 2] = 0
    view[-1, -2:, -2:, c.channels // 2] = 255
    return x, np.full(c.out_span, FILL, np.uint8)


def has_extremes(c: Case) -> bool:
    """whether the 0 block and the 255 block of tensors() are disjoint, all taps of the first output pixel lie in the
    former and all taps of the last output pixel in the latter (by the axis tables of the definition)"""
    if c.batch == 1 and max(c.in_h, c.in_w) < 4:
        return False
    for n_in, n_out in ((c.in_h, c.out_h), (c.in_w, c.out_w)):
        i0, i1, _ = axis(n_in, n_out, c.align)
        if i1[0] > 1 or i0[-1] < n_in - 2:
            return False
    return True


def expected(c: Case, x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """the output buffer after the run: the pixels' bytes resized, every byte between strided pixels kept"""
    out = y.copy()
    src = pixels_view(x, c.batch, c.in_h, c.in_w, c.in_stride, c.channels)
    pixels_view(out, c.batch, c.out_h, c.out_w, c.out_stride, c.channels)[...] = resize(src, c.out_h, c.out_w, c.align)
    return out


def kernel_for(channels: int, bases, strides) -> str:
    """hip/u8resize.hip's selection rule: bases = (input, output) addresses, strides = the two pixel strides"""
    if channels % 16 == 0 and all(v % 16 == 0 for v in tuple(bases) + tuple(strides)):
        return "u8_resize_x16"
    return "u8_resize_x4" if channels >= 4 else "u8_resize_x1"


# ---- case lists ------------------------------------------------------------------------------------------------------
PROPERTY_IN = (1, 2, 3, 5, 7, 8, 13)
PROPERTY_OUT = (1, 2, 3, 4, 7, 10, 16, 29)
TABLE_IN = (1, 2, 3, 5, 7, 8, 13, 224, 513)
TABLE_OUT = (1, 2, 3, 4, 7, 10, 16, 29, 224, 513)
TABLE_EDGES = ((SIZE_LIMIT - 1, 1), (1, SIZE_LIMIT - 1), (SIZE_LIMIT - 1, SIZE_LIMIT - 1))
GEOMETRY_IN = (1, 2, 3, 5, 7)
GEOMETRY_OUT = (1, 2, 3, 4, 7, 10)
CHANNELS = (1, 2, 3, 4, 5, 15, 16, 17, 21, 32, 33, 64)
