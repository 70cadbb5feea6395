/*
 * qd8_mxfp4.hip.h -- what the kernels of the MXFP4 dynamically quantized fully connected operators share (qd8f32gemm4m.hip:
 * one weight set; qd8f32gemm4g.hip: one per group): the decode of E2M1 codes to int8 w2 in registers and the forms of one
 * term of the ordered float chain. qd8f32gemm4m.hip's header has the account of the decode and of the weight image.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

/* four E2M1 codes, one in the low nibble of each byte of `codes` (the high nibbles may hold anything), to four int8 w2 */
__device__ __forceinline__ int mx_decode(uint32_t codes)
{
  const uint32_t index = codes & 0x07070707u;
  const uint32_t plus = __builtin_amdgcn_perm(0x0C080604u, 0x03020100u, index);           // 0 1 2 3 | 4 6 8 12
  const uint32_t minus = __builtin_amdgcn_perm(0xF4F8FAFCu, 0xFDFEFF00u, index);          // 0 -1 -2 -3 | -4 -6 -8 -12
  const uint32_t pick = ((codes >> 1) & 0x04040404u) | 0x03020100u;                       // byte i: i, or 4 + i where bit 3 is set
  return static_cast<int>(__builtin_amdgcn_perm(minus, plus, pick));
}
/* the MFMA operand of block b (0 .. 3, K order) of a pair fragment: eight bytes w2 */
__device__ __forceinline__ long mx_operand(const v4i& codes, int b)
{
  const int lo = (b & 1) * 2, shift = (b >> 1) * 4;
  typedef int v2i __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(long, v2i{mx_decode(static_cast<uint32_t>(codes[lo]) >> shift),
                                      mx_decode(static_cast<uint32_t>(codes[lo + 1]) >> shift)});
}
/* one term of the ordered sum: sum = the block's MFMA result, |sum + zero_offset * wsum2| = |acc_b| < 2^17; exact */
__device__ __forceinline__ float mx_term(int32_t sum, int32_t zero_offset, int32_t wsum2, int32_t exponent)
{
  return __builtin_amdgcn_ldexpf(static_cast<float>(sum + zero_offset * wsum2), exponent);
}
/* The tile kernel's form of ysum = ysum + t_b, one operation shorter: the float 2^(e - 128) of a table value (its biased
 * exponent is e - 1, in [110, 142]) and ONE v_fma_f32. The product (float) acc_b * 2^(e - 128) is exact -- at most 17
 * significant bits, far inside the normal range -- so the fused operation rounds the very real number ysum + t_b that the
 * definition's separate addition rounds: the same bits, though the definition has no fused multiply-add. That holds for a
 * power-of-two scale alone, which is why no sibling kernel can do it. */
__device__ __forceinline__ float mx_scale(int32_t entry)
{
  return __builtin_bit_cast(float, ((entry & 255) - 1) << 23);
}
__device__ __forceinline__ float mx_add_term(float ysum, int32_t sum, int32_t zero_offset, int32_t wsum2, float scale)
{
  return __builtin_fmaf(static_cast<float>(sum + zero_offset * wsum2), scale, ysum);
}

}  // namespace

}  // namespace qnnp
