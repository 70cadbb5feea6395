/*
 * u8_bytewise.hip.h -- bytewise uint8 max / clamp on packed dwords, shared by the max-pooling kernels (q8pool.hip) and
 * the clamp kernels (x8shuffle.hip).
 *
 * gfx950 has no packed 8-bit max or min. The 16-bit packed forms stand in: in each 16-bit lane the high byte decides
 * the comparison, so v_pk_max_u16 on the raw dwords keeps the max of the odd bytes in the high halves, and on the dwords
 * shifted left by 8 in each lane (v_pk_lshlrev_b16) the max of the even bytes; one v_perm_b32 joins the two.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace qnnp {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 as_u16x2(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ uint32_t as_u32(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }

/* running bytewise max of one dword: odd bytes in the high halves of `odd`, even bytes in the high halves of `even` */
__device__ __forceinline__ void max_step(uint32_t& odd, uint32_t& even, uint32_t x)
{
  odd = as_u32(__builtin_elementwise_max(as_u16x2(odd), as_u16x2(x)));
  even = as_u32(__builtin_elementwise_max(as_u16x2(even), as_u16x2(x) << static_cast<unsigned short>(8)));
}

/* clamp both halves' high bytes to [lo, hi] (their low bytes only break ties) and join the bytes */
__device__ __forceinline__ uint32_t max_finish(uint32_t odd, uint32_t even, uint32_t clamp_hi, uint32_t clamp_lo)
{
  odd = as_u32(__builtin_elementwise_max(__builtin_elementwise_min(as_u16x2(odd), as_u16x2(clamp_hi)), as_u16x2(clamp_lo)));
  even = as_u32(__builtin_elementwise_max(__builtin_elementwise_min(as_u16x2(even), as_u16x2(clamp_hi)), as_u16x2(clamp_lo)));
  return __builtin_amdgcn_perm(odd, even, 0x07030501u);    // bytes: even.1, odd.1, even.3, odd.3
}

/* the clamp bounds in the 16-bit-lane form of max_finish: the bound in the high byte, the low byte 0xFF / 0x00 */
__host__ __device__ __forceinline__ uint32_t clamp_hi_bound(uint32_t output_max) { return (output_max << 8 | 0xFFu) * 0x00010001u; }
__host__ __device__ __forceinline__ uint32_t clamp_lo_bound(uint32_t output_min) { return (output_min << 8) * 0x00010001u; }

/* min(max(x, lo), hi) of each byte of x, with the bounds of clamp_hi_bound / clamp_lo_bound (5 VALU) */
__device__ __forceinline__ uint32_t clamp_u8x4(uint32_t x, uint32_t clamp_hi, uint32_t clamp_lo)
{
  return max_finish(x, as_u32(as_u16x2(x) << static_cast<unsigned short>(8)), clamp_hi, clamp_lo);
}

}  // namespace qnnp
