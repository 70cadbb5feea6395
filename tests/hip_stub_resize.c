/*
 * hip_stub_resize.c -- TEST INFRASTRUCTURE: the bilinear resize launch of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/u8resize.hip) for the host-sanitizer build of the resize operator (Makefile target asan-resize), beside
 * tests/hip_stub.c. It validates the argument block as the device launcher does, checks what resize-bilinear.c is to hand
 * over (table entries that stay inside the input, weights below 2048, a zero weight where both taps are one) and then
 * computes every byte on the host FROM THE UPLOADED TABLES, in the two-step form of the definition (top and bottom row
 * blends, then the blend of the two), so ASan sees an undersized table or staging buffer and the test can check the
 * bytes that come back through the staging round trip.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "hip/qnnp_hip.h"

/* what the last launch was handed (tests/host_asan_resize_test.c reads them) */
struct qnnp_hip_resize_args qnnp_stub_resize_last;
unsigned qnnp_stub_resize_launches;

struct entry {
  uint32_t i0;
  uint32_t w_step;
};

int qnnp_hip_resize_run(const struct qnnp_hip_resize_args* a, const char** kernel_name)
{
  const uint32_t limit = UINT32_C(1) << 24;
  if (a == NULL || a->input == NULL || a->output == NULL || a->table == NULL || (uintptr_t) a->table % 8 != 0 ||
      a->channels == 0 || a->channels > 0x7FFFFFFFu || a->input_stride < a->channels || a->output_stride < a->channels ||
      a->input_height == 0 || a->input_width == 0 || a->output_height == 0 || a->output_width == 0 ||
      a->input_height >= limit || a->input_width >= limit || a->output_height >= limit || a->output_width >= limit) {
    return QNNP_HIP_EINVAL;
  }
  const uint64_t in_image = (uint64_t) a->input_height * a->input_width;
  const uint64_t out_image = (uint64_t) a->output_height * a->output_width;
  if (a->batch > 0x7FFFFFFFu || a->batch * in_image > 0x7FFFFFFFu || a->batch * out_image > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;
  if (a->streaming_mode > 2) abort();
  qnnp_stub_resize_last = *a;
  qnnp_stub_resize_launches++;
  if (kernel_name != NULL) *kernel_name = "stub_resize";
  /* a copy of the table: ASan checks that all output_height + output_width entries are there */
  const size_t entries = (size_t) a->output_height + a->output_width;
  struct entry* table = (struct entry*) malloc(entries * sizeof(struct entry));
  if (table == NULL) abort();
  memcpy(table, a->table, entries * sizeof(struct entry));
  const struct entry* rows = table;
  const struct entry* cols = table + a->output_height;
  /* resize-bilinear.c's side of the contract */
  for (size_t i = 0; i < entries; i++) {
    const uint32_t n_in = i < a->output_height ? a->input_height : a->input_width;
    const uint32_t step = table[i].w_step >> 11, w = table[i].w_step & 2047u;
    if (step > 1 || table[i].i0 + step >= n_in || (step == 0 && w != 0)) abort();
  }
  for (uint64_t n = 0; n < a->batch; n++) {
    for (uint32_t oy = 0; oy < a->output_height; oy++) {
      const uint64_t y0 = rows[oy].i0, y1 = y0 + (rows[oy].w_step >> 11);
      const uint32_t wy = rows[oy].w_step & 2047u;
      for (uint32_t ox = 0; ox < a->output_width; ox++) {
        const uint64_t x0 = cols[ox].i0, x1 = x0 + (cols[ox].w_step >> 11);
        const uint32_t wx = cols[ox].w_step & 2047u;
        const uint8_t* p00 = a->input + (n * in_image + y0 * a->input_width + x0) * a->input_stride;
        const uint8_t* p01 = a->input + (n * in_image + y0 * a->input_width + x1) * a->input_stride;
        const uint8_t* p10 = a->input + (n * in_image + y1 * a->input_width + x0) * a->input_stride;
        const uint8_t* p11 = a->input + (n * in_image + y1 * a->input_width + x1) * a->input_stride;
        uint8_t* po = a->output + (n * out_image + (uint64_t) oy * a->output_width + ox) * a->output_stride;
        for (uint32_t c = 0; c < a->channels; c++) {
          const uint32_t top = p00[c] * (2048u - wx) + p01[c] * wx;
          const uint32_t bot = p10[c] * (2048u - wx) + p11[c] * wx;
          po[c] = (uint8_t) ((top * (2048u - wy) + bot * wy + (UINT32_C(1) << 21)) >> 22);
        }
      }
    }
  }
  free(table);
  return QNNP_HIP_OK;
}
