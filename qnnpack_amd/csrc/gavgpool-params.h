/*
 * gavgpool-params.h -- what a global average pooling operator derives from the pooled width at setup: the range check
 * and the quantization parameters (reference src/global-average-pooling.c:133-145). Shared by
 * qnnp_setup_global_average_pooling_nwc_q8 (global-average-pooling.c) and the fused squeeze-and-excite block
 * (squeeze-excite.c), whose pooling stage must be that operator's bit for bit.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "hip/qnnp_hip.h"
#include "operator.h"
#include "requantization.h"

/* 1 and *params for `width` pixels per image, or 0: the accumulator of one output is width * 255 at most; the scale
 * must stay inside the parameter builder's range [2^-32, 256) (asserted by the reference, requantization.h:208-209) */
static inline int qnnp_gavgpool_params_for_width(
    const struct qnnp_operator* pool, size_t width, struct qnnp_hip_avgpool_params* params)
{
  const float scale = pool->input_scale / (pool->output_scale * (float) width);
  if (width > (size_t) INT32_MAX / 255 || !(scale >= 0x1.0p-32f) || !(scale < 256.0f)) {
    return 0;
  }
  *params = qnnp_compute_avgpool_params(
      -(int32_t) width * (int32_t) (uint32_t) pool->input_zero_point, scale,
      pool->output_zero_point, pool->output_min, pool->output_max);
  return 1;
}
