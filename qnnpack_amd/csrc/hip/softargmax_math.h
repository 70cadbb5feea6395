/*
 * softargmax_math.h -- the integer arithmetic of the softargmax operator's normalisation, written once and compiled both
 * for the device (q8softargmax.hip) and for the host (tests/host_asan_softargmax_test.c checks it against the plain
 * division over the whole 32-bit range of divisors without a GPU).
 *
 * Normative definition (reference src/u8lut32norm/scalar.c:39-50), all in uint32_t:
 *     y = min(((t << 8) + (vsum >> 1)) / vsum, 255)                 t < 2^23, so the numerator never wraps
 * The division is exact. The reference divides by a per-row magic number (fxdiv_init_uint32_t / fxdiv_quotient_uint32_t);
 * so does this: the round-up method of Granlund and Montgomery, "Division by Invariant Integers using Multiplication"
 * (PLDI 1994), figure 4.1, which is exact for EVERY 32-bit numerator and EVERY divisor d >= 1:
 *     l = ceil(log2 d),   m = floor(2^32 * (2^l - d) / d) + 1,   t = mulhi(n, m),
 *     n / d = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0)
 * t <= n, and t + ((n - t) >> 1) <= n: no intermediate wraps. One 64-by-32-bit division per row (for m), then one
 * multiply-high, one subtraction, one addition and two shifts per byte.
 */
#pragma once

#include <stdint.h>

#ifndef QNNP_HD
#ifdef __HIPCC__
#define QNNP_HD __host__ __device__ __forceinline__
#else
#define QNNP_HD static inline
#endif
#endif

struct qnnp_softargmax_divisor {
  uint32_t m;
  uint32_t s1;   /* min(l, 1) */
  uint32_t s2;   /* max(l - 1, 0) */
};

/* d >= 1 */
QNNP_HD struct qnnp_softargmax_divisor qnnp_softargmax_divisor_init(uint32_t d)
{
  struct qnnp_softargmax_divisor r;
  if (d == 1) {
    r.m = 1;
    r.s1 = 0;
    r.s2 = 0;
  } else {
    const uint32_t l_minus_1 = 31u - (uint32_t) __builtin_clz(d - 1);
    /* 2^l - d; for l == 32 the power wraps to 0 and the difference is still right modulo 2^32 (it is below d) */
    const uint32_t u_hi = (UINT32_C(2) << l_minus_1) - d;
    r.m = (uint32_t) (((uint64_t) u_hi << 32) / d) + 1;
    r.s1 = 1;
    r.s2 = l_minus_1;
  }
  return r;
}

/* n / d for the d of qnnp_softargmax_divisor_init */
QNNP_HD uint32_t qnnp_softargmax_divide(uint32_t n, struct qnnp_softargmax_divisor d)
{
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t t = __umulhi(n, d.m);
#else
  const uint32_t t = (uint32_t) (((uint64_t) n * d.m) >> 32);
#endif
  return (t + ((n - t) >> d.s1)) >> d.s2;
}

/* the output byte of table entry t in a row whose (wrapped, nonzero) table sum has the divisor d and the rounding term
 * vsum >> 1 */
QNNP_HD uint32_t qnnp_softargmax_normalize(uint32_t t, uint32_t rounding, struct qnnp_softargmax_divisor d)
{
  const uint32_t q = qnnp_softargmax_divide((t << 8) + rounding, d);
  return q > 255u ? 255u : q;
}
