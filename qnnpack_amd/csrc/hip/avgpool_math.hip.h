/*
 * avgpool_math.hip.h -- the scalar average-pooling quantizer, shared by global average pooling (q8pointwise.hip) and
 * windowed average pooling (q8pool.hip). Restates qnnp_avgpool_quantize (reference src/qnnpack/requantization.h:482-498);
 * the parameters come from qnnp_compute_avgpool_params (requantization.h of this tree).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qnnp_hip.h"

namespace qnnp {

/* src/qnnpack/requantization.h:482-498 */
__device__ __forceinline__ uint32_t avgpool_quantize(int32_t n, const qnnp_hip_avgpool_params& q)
{
  const int64_t product = static_cast<int64_t>(n) * static_cast<int64_t>(q.multiplier);
  const int64_t adjusted = product - static_cast<int64_t>(n < 0);
  int32_t y = static_cast<int32_t>((adjusted + q.rounding) >> q.right_shift);
  y = y < q.output_min_less_zero_point ? q.output_min_less_zero_point : y;
  y = y > q.output_max_less_zero_point ? q.output_max_less_zero_point : y;
  return static_cast<uint32_t>(y + q.output_zero_point) & 0xFFu;
}

}  // namespace qnnp
