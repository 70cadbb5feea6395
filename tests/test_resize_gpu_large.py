"""GPU tier: the bilinear resize operator on tensors past 2^31 and 2^32 bytes, against the definition of tests/_resize.py.

A pixel index times a pixel stride passes 2^32 in both tensors of a segmentation-sized upsampling, so hip/u8resize.hip
forms every byte offset in 64 bits; a 32-bit product anywhere would land in another image of the same tensor -- plausible
uint8. Two cases, one per tensor:

 * the OUTPUT past 2^32 bytes (4 images of 64 x 64 x 64 -> 4099 x 4099 x 64): the pixel rows that hold output bytes
   2^31 - 1, 2^31, 2^32 - 1 and 2^32 and the first and last row of every image are compared with the definition;
 * the INPUT past 2^31 bytes (3 images of 8200 x 8200 x 16 -> 7 x 7 x 16): the input is filled on the device from a
   per-byte formula, only the tap rows the axis tables name are read back, and the expectation is computed from them.

Conventions of tests/test_gpu_large_tensors.py / tests/_large.py: the memory requirement fails, never skips; both ends of
every tensor carry guards; nothing of gigabyte size is copied to the host."""
import numpy as np
import pytest

import _large as lg
import _resize as rs
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_after_each():
    yield
    lg.free_memory()


def _read(t, lo, hi):
    import torch
    torch.cuda.synchronize()
    return t.view[lo:hi].cpu().numpy()


def test_output_past_4_gib(qnnp):
    c = rs.Case(4, 64, 64, 4099, 4099, 64)
    row_bytes = c.out_w * c.out_stride
    assert c.out_span > lg.BOUNDS[-1] and c.out_pixels < 2 ** 31
    lg.require_memory(c.out_span + c.in_span, "resize, output past 4 GiB")
    x, _ = rs.tensors("large/output", c)
    d_x, d_y = lg.Tensor(c.in_span, 1), lg.Tensor(c.out_span, 2)
    import torch
    d_x.view.copy_(torch.from_numpy(x).cuda())
    d_y.fill(rs.FILL)
    op = qnnp.create_resize_bilinear2d_nhwc_u8(c.channels)
    try:
        assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(d_x.view, d_y.view)) == Status.success
        qnnp.run_operator(op)
        assert qnnp.operator_kernel(op) == "u8_resize_x16"
    finally:
        qnnp.delete_operator(op)
    rows = {b // row_bytes for b in lg.BOUNDS}
    for n in range(c.batch):
        rows.update((n * c.out_h, (n + 1) * c.out_h - 1))
    assert len(rows) >= 10
    src = rs.pixels_view(x, c.batch, c.in_h, c.in_w, c.in_stride, c.channels)
    for r in sorted(rows):
        n, oy = divmod(r, c.out_h)
        want = rs.resize(src[n:n + 1], c.out_h, c.out_w, False, rows=[oy]).reshape(-1)
        got = _read(d_y, r * row_bytes, (r + 1) * row_bytes)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"output row {r} (image {n}, row {oy}, from byte {r * row_bytes}): {bad.size} bytes differ, "
                               f"first at {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}")
    # a coarse look at the whole tensor, in chunks on the device: an unwritten stretch would be all FILL, while written
    # bytes of a random image are FILL about once in 256
    for lo in range(0, c.out_span, lg.CHUNK):
        part = d_y.view[lo:lo + lg.CHUNK]
        assert int((part == rs.FILL).sum()) < part.numel() // 16, f"bytes {lo} .. {lo + part.numel()} look unwritten"
    d_y.assert_guards("resize, output past 4 GiB")
    d_x.assert_guards("resize, output past 4 GiB (input)")
    assert np.array_equal(_read(d_x, 0, c.in_span), x)


def _formula(b):
    """the input byte at byte offset b (int64 numpy array or torch tensor)"""
    return (b * 131 + (b >> 8) * 7 + (b >> 16) * 13 + (b >> 24) * 29) & 0xFF


def test_input_past_2_gib(qnnp):
    import torch
    c = rs.Case(3, 8200, 8200, 7, 7, 16)
    row_bytes = c.in_w * c.in_stride
    image_bytes = c.in_h * row_bytes
    assert c.in_span > lg.BOUNDS[1] and c.in_pixels < 2 ** 31
    lg.require_memory(c.in_span + 2 * lg.CHUNK, "resize, input past 2 GiB")
    d_x, d_y = lg.Tensor(c.in_span, 3), lg.Tensor(c.out_span, 4)
    step = lg.CHUNK // 8                                     # int64 temporaries of CHUNK bytes
    for lo in range(0, c.in_span, step):
        hi = min(lo + step, c.in_span)
        d_x.view[lo:hi].copy_(_formula(torch.arange(lo, hi, dtype=torch.int64, device="cuda")).to(torch.uint8))
    d_y.fill(rs.FILL)
    for align in (False, True):
        op = qnnp.create_resize_bilinear2d_nhwc_u8(c.channels, rs.ALIGN_CORNERS if align else 0)
        try:
            assert qnnp.setup_resize_bilinear2d_nhwc_u8_status(op, *c.setup_args(d_x.view, d_y.view)) == Status.success
            qnnp.run_operator(op)
            assert qnnp.operator_kernel(op) == "u8_resize_x16"
        finally:
            qnnp.delete_operator(op)
        y0, y1, wy = rs.axis(c.in_h, c.out_h, align)
        x0, x1, wx = rs.axis(c.in_w, c.out_w, align)
        got = _read(d_y, 0, c.out_span).reshape(c.batch, c.out_h, c.out_w, c.channels)
        beyond = 0
        for n in range(c.batch):
            rows = {}
            for y in sorted(set(y0.tolist()) | set(y1.tolist())):
                lo = n * image_bytes + y * row_bytes
                rows[y] = _read(d_x, lo, lo + row_bytes).reshape(c.in_w, c.channels)
                # the fill is what the formula says, here as on the device
                assert np.array_equal(rows[y].reshape(-1), _formula(np.arange(lo, lo + row_bytes, dtype=np.int64)).astype(np.uint8))
                assert np.unique(rows[y]).size > 100
                beyond += lo + row_bytes > lg.BOUNDS[1]
            top = np.stack([rows[y] for y in y0.tolist()])   # [out_h][in_w][channels]
            bot = np.stack([rows[y] for y in y1.tolist()])
            want = rs.blend(top[:, x0], top[:, x1], bot[:, x0], bot[:, x1], wx[None, :, None], wy[:, None, None])
            bad = np.flatnonzero(got[n] != want)
            assert bad.size == 0, (f"image {n}, align corners {align}: {bad.size} bytes differ, first at {bad[:4]}: "
                                   f"got {got[n].reshape(-1)[bad[:4]]}, want {want.reshape(-1)[bad[:4]]}")
        assert beyond >= 7, "some taps lie beyond byte 2^31"
        assert np.unique(got).size > 100
        d_y.assert_guards("resize, input past 2 GiB (output)")
        d_y.fill(rs.FILL)
    d_x.assert_guards("resize, input past 2 GiB")
