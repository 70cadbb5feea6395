/*
 * hip_stub_mul.c -- TEST INFRASTRUCTURE: the multiply launch of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/q8mul.hip) for the host-sanitizer build of the multiply operator (Makefile target asan-mul), beside tests/hip_stub.c
 * and tests/hip_stub_lut.c. It validates the argument block as the device launcher does, checks what multiply.c is to
 * hand over (the accumulator bound of one product, a Q31 multiplier, zero points that are bytes) and then computes every
 * byte on the host from the definition of the down-convert (the stub's "device" memory is host memory), so ASan sees
 * any undersized staging buffer and the test can check the bytes that come back through the staging round trip.
 */
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

/* what the last launch was handed (tests/host_asan_mul_test.c reads them) */
struct qnnp_hip_mul_args qnnp_stub_mul_last;
unsigned qnnp_stub_mul_launches;

/* the scalar definition: Q31 product rounded half up, then a shift that rounds half away from zero, clamp, zero point */
static uint8_t requantize(int32_t n, const struct qnnp_hip_requant* rq)
{
  const int64_t product = (int64_t) n * (int64_t) rq->multiplier;
  const int32_t q = (int32_t) (uint32_t) ((uint64_t) (product + INT64_C(0x40000000)) >> 31);
  const int32_t remainder = (q & rq->remainder_mask) - (int32_t) (n < 0);
  /* arithmetic shift of a negative value, spelled out */
  const int32_t shifted = q >= 0 ? (int32_t) ((uint32_t) q >> rq->shift) : -(int32_t) (((uint32_t) -(q + 1)) >> rq->shift) - 1;
  int32_t y = shifted + (int32_t) (remainder > rq->remainder_threshold);
  if (y < rq->output_min_less_zero_point) y = rq->output_min_less_zero_point;
  if (y > rq->output_max_less_zero_point) y = rq->output_max_less_zero_point;
  return (uint8_t) (y + rq->output_zero_point);
}

int qnnp_hip_mul_run(const struct qnnp_hip_mul_args* a, const char** kernel_name)
{
  if (a == NULL || a->a == NULL || a->b == NULL || a->product == NULL || a->channels == 0 ||
      a->channels > 0x7FFFFFFFu || a->a_stride < a->channels || a->b_stride < a->channels ||
      a->product_stride < a->channels) {
    return QNNP_HIP_EINVAL;
  }
  const uint64_t rows = (uint64_t) a->b_rows * a->a_rows_per_b_row;
  if (rows > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;
  /* multiply.c's side of the contract */
  if (a->rq.accumulator_bits != 16 || a->rq.multiplier < 0x40000000 || a->rq.shift > 31 ||
      a->rq.remainder_mask != (int32_t) ((UINT32_C(1) << a->rq.shift) - 1) ||
      a->rq.remainder_threshold != (a->rq.remainder_mask >> 1) ||
      a->a_zero_point < 0 || a->a_zero_point > 255 || a->b_zero_point < 0 || a->b_zero_point > 255 ||
      a->rq.output_zero_point < 0 || a->rq.output_zero_point > 255 || a->streaming_mode > 2) {
    abort();
  }
  qnnp_stub_mul_last = *a;
  qnnp_stub_mul_launches++;
  if (kernel_name != NULL) *kernel_name = "stub_mul";
  for (uint64_t r = 0; r < rows; r++) {
    const uint8_t* pa = a->a + r * a->a_stride;
    const uint8_t* pb = a->b + (r / a->a_rows_per_b_row) * a->b_stride;
    uint8_t* pp = a->product + r * a->product_stride;
    for (uint32_t c = 0; c < a->channels; c++) {
      pp[c] = requantize(((int32_t) pa[c] - a->a_zero_point) * ((int32_t) pb[c] - a->b_zero_point), &a->rq);
    }
  }
  return QNNP_HIP_OK;
}
