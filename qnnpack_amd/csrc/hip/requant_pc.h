/*
 * requant_pc.h -- the Q31 down-convert with ONE (multiplier, shift) PER OUTPUT CHANNEL (per-channel weight scales,
 * include/qnnpack_gfx950_perchannel.h), written once and compiled both for the device (igemm_epilogue.hip.h,
 * q8dwconv_pc.hip) and for the host (debug-hooks.c exports it as qnnp_debug_requant_pc, so the CPU test tier checks it
 * against the oracle for every shift without a GPU).
 *
 * It is the normative sequence of qnnp_q31_requantize itself (reference src/qnnpack/requantization.h:464-480), one
 * branch-free form for every shift 0 ... 31:
 *     P   = (int64) n * M + 2^30                       M in [2^30, 2^31)
 *     q   = (int32) (P >> 31)
 *     rem = (q & (2^s - 1)) - (n < 0)
 *     y   = (q >> s) + (rem > ((2^s - 1) >> 1))         s == 0: mask 0, rem <= 0, nothing added
 *     out = min(max(y, qmin - zp), qmax - zp) + zp
 * The per-tensor kernels fold (M, s) into per-OPERATOR constants and pick an instruction sequence per operator
 * (requant_math.h); with the constants changing from channel to channel there is nothing to pick, so the sequence is
 * the definition. The zero point and the clamp stay per operator.
 */
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define QNNP_PC_HD __host__ __device__ __forceinline__
#else
#define QNNP_PC_HD static inline
#endif

/* one entry of an operator's device table: entry c belongs to output channel c. 8 bytes, so the four consecutive
 * channels a lane owns are two 16-byte loads. Pad entries are {2^30, 0}: valid, and no lane ever shifts by garbage. */
struct qnnp_requant_pc_entry {
  int32_t multiplier;   /* [0x40000000, 0x7FFFFF80] */
  uint32_t shift;       /* [0, 31] */
};

#define QNNP_REQUANT_PC_PAD_MULTIPLIER INT32_C(0x40000000)

/* y before the clamp */
QNNP_PC_HD int32_t qnnp_requant_pc_scale(int32_t n, int32_t multiplier, uint32_t shift)
{
  const int64_t product = (int64_t) n * (int64_t) multiplier + (INT64_C(1) << 30);
  const int32_t q = (int32_t) (uint32_t) ((uint64_t) product >> 31);
  const int32_t mask = (int32_t) ((UINT32_C(1) << shift) - UINT32_C(1));
  const int32_t remainder = (q & mask) - (int32_t) (n < 0);
  return (q >> shift) + (int32_t) (remainder > (mask >> 1));
}

/* the output byte, in an int32: lo / hi are output_min / output_max less the zero point */
QNNP_PC_HD int32_t qnnp_requant_pc(int32_t n, int32_t multiplier, uint32_t shift, int32_t lo, int32_t hi, int32_t zero_point)
{
  int32_t y = qnnp_requant_pc_scale(n, multiplier, shift);
  y = y < lo ? lo : y;
  y = y > hi ? hi : y;
  return y + zero_point;
}
