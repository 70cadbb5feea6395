/*
 * requantization.h -- host-side builder for the fused Q31 down-convert
 * parameters. Restates the scalar branch of
 * qnnp_compute_conv_quantization_params (reference src/qnnpack/requantization.h:122-198,
 * scalar members :183-196): a float scale in [2^-32, 1) becomes a Q31 multiplier
 * in [2^30, 2^31) and a right shift in [0, 31].
 *
 * The arithmetic that consumes these parameters (the normative rounding of
 * qnnp_q31_requantize, requantization.h:464-480) lives in hip/requant.hip.h.
 */
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hip/qnnp_hip.h"

static inline struct qnnp_hip_requant qnnp_compute_requant(
    float scale, uint8_t output_zero_point, uint8_t output_min, uint8_t output_max)
{
  uint32_t bits;
  memcpy(&bits, &scale, sizeof(bits));
  struct qnnp_hip_requant rq;
  /* mantissa with the implicit one restored, moved up to bit 30 */
  rq.multiplier = (int32_t) (((bits & UINT32_C(0x007FFFFF)) | UINT32_C(0x00800000)) << 7);
  /* 2^-shift * multiplier * 2^-31 == scale */
  const uint32_t shift = 127 + 31 - 32 - (bits >> 23);
  const uint32_t mask = (UINT32_C(1) << shift) - UINT32_C(1);
  rq.shift = shift;
  rq.remainder_mask = (int32_t) mask;
  rq.remainder_threshold = (int32_t) (mask >> 1);
  rq.output_min_less_zero_point = (int32_t) output_min - (int32_t) output_zero_point;
  rq.output_max_less_zero_point = (int32_t) output_max - (int32_t) output_zero_point;
  rq.output_zero_point = (int32_t) output_zero_point;
  rq.accumulator_bits = 0;      /* unknown until the operator says otherwise (qnnp_accumulator_bits) */
  return rq;
}

/*
 * Smallest b with |bias[i] + sum_k (a - izp)(w - kzp)| < 2^b for every uint8 a, w: the value the fused epilogue
 * requantizes is exactly this accumulator (the zero-point algebra of the kernels cancels), and each of the
 * `reduction_length` products is at most 255 * 255 in magnitude. 0 = more than 31 bits (bound unusable).
 * Lets the device use the cheaper bounded rounding sequence (hip/requant_math.h).
 */
static inline uint32_t qnnp_accumulator_bits(const int32_t* bias, size_t count, size_t reduction_length)
{
  uint64_t max_bias = 0;
  for (size_t i = 0; i < count; i++) {
    const int64_t b = bias[i];
    const uint64_t mag = (uint64_t) (b < 0 ? -b : b);
    if (mag > max_bias) max_bias = mag;
  }
  const uint64_t bound = max_bias + (uint64_t) reduction_length * UINT64_C(65025) + 1;
  uint32_t bits = 0;
  while (bits < 40 && (UINT64_C(1) << bits) < bound) bits++;
  return bits <= 31 ? bits : 0;
}

/*
 * Scalar member of qnnp_compute_avgpool_quantization_params (reference src/qnnpack/requantization.h:200-222, :252-265):
 * a scale in [2^-32, 256) becomes a 24-bit multiplier in [2^23, 2^24) and a right shift in [16, 55]. Consumed by
 * avgpool_quantize (hip/avgpool_math.hip.h): global average pooling and windowed average pooling.
 */
static inline struct qnnp_hip_avgpool_params qnnp_compute_avgpool_params(
    int32_t bias, float scale, uint8_t output_zero_point, uint8_t output_min, uint8_t output_max)
{
  uint32_t scale_bits;
  memcpy(&scale_bits, &scale, sizeof(scale_bits));
  struct qnnp_hip_avgpool_params p;
  p.bias = bias;
  p.multiplier = ((int32_t) scale_bits & INT32_C(0x007FFFFF)) | INT32_C(0x00800000);   /* [2^23, 2^24) */
  const int32_t shift = 127 + 23 - (int32_t) (scale_bits >> 23);                        /* [16, 55] */
  p.right_shift = (uint32_t) shift;
  p.rounding = INT64_C(1) << (p.right_shift - 1);
  p.output_min_less_zero_point = (int32_t) (uint32_t) output_min - (int32_t) (uint32_t) output_zero_point;
  p.output_max_less_zero_point = (int32_t) (uint32_t) output_max - (int32_t) (uint32_t) output_zero_point;
  p.output_zero_point = (int32_t) (uint32_t) output_zero_point;
  return p;
}

/*
 * Scalar member of qnnp_compute_add_quantization_params (reference src/qnnpack/requantization.h:327-360, :400-413):
 * the two input-to-output scale ratios, each in [2^-14, 2^8), become multipliers in [0, 2^22] -- the larger one in
 * [2^21, 2^22] -- and a right shift of 21 - exponent(larger ratio). Consumed by add_quantize (hip/add_math.hip.h): the
 * stand-alone add, the residual add folded into a convolution (residual.c) and the fused block (fused-block.c).
 *
 * The shift is in [14, 31] while the larger ratio is at least 2^-10. Below that it would be 32 ... 35, which neither a
 * 32-bit shift nor the 32-bit remainder mask can express (the reference is undefined there: its asserts and its
 * comment contradict each other, requantization.h:336-347). The accumulator a * a_multiplier + b * b_multiplier +
 * zero_point_product is below 2^31 in magnitude, that is below half of 2^shift, so the correctly rounded quotient is 0
 * for every input: both multipliers and the zero-point product are 0 there and the shift is 31, and every output is
 * clamp(output_zero_point).
 */
static inline struct qnnp_hip_add_params qnnp_compute_add_params(
    uint8_t a_zero_point, uint8_t b_zero_point, uint8_t output_zero_point,
    float a_output_scale, float b_output_scale, uint8_t output_min, uint8_t output_max)
{
  const float max_output_scale = a_output_scale > b_output_scale ? a_output_scale : b_output_scale;
  uint32_t max_scale_bits;
  memcpy(&max_scale_bits, &max_output_scale, sizeof(max_scale_bits));
  const int32_t max_scale_exponent = (int32_t) (max_scale_bits >> 23) - 127;
  uint32_t shift = (uint32_t) (21 - max_scale_exponent);                /* in [14, 35] */
  uint32_t a_multiplier = 0, b_multiplier = 0;
  if (shift <= 31) {
    const uint32_t multiplier_bits = (uint32_t) (21 - max_scale_exponent + 127) << 23;
    float scale_multiplier;
    memcpy(&scale_multiplier, &multiplier_bits, sizeof(scale_multiplier));
    /* multipliers in [0, 2^22], the larger one in [2^21, 2^22] (2^22: a mantissa of 24 ones, rounded to 22 bits);
     * lrintf = round to nearest even */
    a_multiplier = (uint32_t) (int32_t) lrintf(a_output_scale * scale_multiplier);
    b_multiplier = (uint32_t) (int32_t) lrintf(b_output_scale * scale_multiplier);
  } else {
    shift = 31;                                                         /* the quotient is 0 for every input */
  }
  const uint32_t remainder_mask = (UINT32_C(1) << shift) - UINT32_C(1);

  struct qnnp_hip_add_params p;
  p.a_multiplier = a_multiplier;
  p.b_multiplier = b_multiplier;
  p.zero_point_product =
      (int32_t) -(a_multiplier * (uint32_t) a_zero_point + b_multiplier * (uint32_t) b_zero_point);
  p.shift = shift;                                                      /* in [14, 31] */
  p.remainder_mask = (int32_t) remainder_mask;
  p.remainder_threshold = (int32_t) (remainder_mask >> 1);
  p.y_zero_point = (int32_t) (uint32_t) output_zero_point;
  p.y_min = (int32_t) (uint32_t) output_min;
  p.y_max = (int32_t) (uint32_t) output_max;
  return p;
}
