/*
 * resize-table.h -- the axis table of the bilinear resize operator (resize-bilinear.c, hip/u8resize.hip): for every output
 * index of one axis, the two input indices it blends and the Q11 weight of the second. Integer arithmetic only, all of it
 * in uint64_t, so the C builder, the numpy restatement of the tests and the header's definition agree bit for bit.
 *
 * With n_in input and n_out output positions (both in [1, 2^24), which keeps every product below 2^62), output index o:
 *   half-pixel centres (the default):  num = max((2o + 1) * n_in - n_out, 0)       [the signed value, clamped]
 *                                      f   = (4096 * num + 2 * n_out) / (4 * n_out)
 *   align corners:                     f   = n_out == 1 ? 0 : (4096 * o * (n_in - 1) + (n_out - 1)) / (2 * (n_out - 1))
 * f is the source coordinate in Q11, rounded to nearest; divisions round down. Then
 *   i0 = min(f >> 11, n_in - 1),  i1 = min(i0 + 1, n_in - 1),  w = i0 == i1 ? 0 : f & 2047
 * and the output is x[i0] * (2048 - w) + x[i1] * w (in Q11).
 *
 * One 8-byte entry per output index: `i0`, and `w_step` = w | (i1 - i0) << 11 -- the weight in bits 0..10 and, in bit 11,
 * whether the second tap is the next input position (1) or the same one (0: the weight is 0 then).
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

struct qnnp_resize_entry {
  uint32_t i0;
  uint32_t w_step;
};

#define QNNP_RESIZE_SIZE_LIMIT ((size_t) 1 << 24)   /* sizes are below it */

static inline struct qnnp_resize_entry qnnp_resize_axis_entry(uint64_t n_in, uint64_t n_out, int align_corners, uint64_t o)
{
  uint64_t f;
  if (align_corners) {
    f = n_out == 1 ? 0 : (UINT64_C(4096) * o * (n_in - 1) + (n_out - 1)) / (2 * (n_out - 1));
  } else {
    const uint64_t centre = (2 * o + 1) * n_in;
    const uint64_t num = centre > n_out ? centre - n_out : 0;
    f = (UINT64_C(4096) * num + 2 * n_out) / (4 * n_out);
  }
  uint64_t i0 = f >> 11;
  if (i0 > n_in - 1) i0 = n_in - 1;
  const uint64_t i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
  const struct qnnp_resize_entry e = {
    .i0 = (uint32_t) i0,
    .w_step = i0 == i1 ? 0u : ((uint32_t) (f & 2047u) | UINT32_C(1) << 11),
  };
  return e;
}

/* table[o] for o < n_out */
static inline void qnnp_resize_axis_table(size_t n_in, size_t n_out, int align_corners, struct qnnp_resize_entry* table)
{
  for (size_t o = 0; o < n_out; o++) {
    table[o] = qnnp_resize_axis_entry(n_in, n_out, align_corners, o);
  }
}
