/*
 * qnnpack_gfx950_moe.h -- the two ends of a MIXTURE-OF-EXPERTS layer, around the grouped operator of
 * qnnpack_gfx950_dynamic.h: a TOP-K SOFTMAX ROUTER in front of it and a WEIGHTED COMBINE behind it. No reference
 * counterpart. Operators behind qnnp_run_operator / qnnp_delete_operator like every other one: they run on the library
 * stream, record into the library's hipGraph capture (one launch each), and qnnp_gfx950_operator_kernel names the kernel a
 * handle last ran. With them a layer is five operators on device pointers and nothing comes back to the host in between:
 *
 *   router            logits [T][E]            -> group_ids [T A], weights [T A]
 *   grouped layer 1   x [T][K], group_ids      -> {gate, up} rows [T A][2 H]            (setup_grouped_..._qd8)
 *   grouped layer 2   those rows, group_ids    -> expert rows [T A][N]                  (setup_grouped_..._qd8_gated, A = 1
 *                                                                                        over T A input rows)
 *   combine           expert rows, weights, group_ids -> y [T][N]
 *
 * (the fifth is whatever produces the logits: a dense fully connected operator of qnnpack_gfx950_dynamic.h, say). Both the
 * logit operator and grouped layer 1 read rmsnorm(x + residual) * gamma in a pre-norm block: set them up with
 * setup_..._qd8_rmsnorm and setup_grouped_..._qd8_rmsnorm of that header on x itself, and no norm launch stands in front.
 *
 * ---- The router ----
 * create(groups = E in 1 .. 1024, assignments = A in 1 .. 8 and at most E, first_group, flags)
 * setup(router, batch_size = T, logits, logits_stride in ELEMENTS (>= E), group_ids [T A], weights [T A])
 *
 * Definition (bit-exact, no tolerance). Float operations are float32, each rounded once, nothing fused. Per token t:
 *   c[e]    the logit with NaN replaced by -FLT_MAX, +inf by FLT_MAX and -inf by -FLT_MAX, decided on the bit pattern; every
 *           other value, denormals and both zeros included, is kept as it is
 *   key(c)  = bits(c) ^ (bits(c) >> 31 ? 0xFFFFFFFF : 0x80000000) as uint32: monotone in c, and -0 ranks below +0
 *   for a = 0 .. A - 1:  sel_a = the not yet selected e with the largest key; among equal keys the smallest e
 *           (clamp and selection are defined on bits: they are integer instructions and no denormal mode enters them)
 *   l_a = c[sel_a];  m = l_0;  d_a = l_a - m           both operands are finite: never NaN; d_a may overflow to -inf
 *   y  = d_a < -80.0f ? -80.0f : d_a
 *   n  = rintf(y * 0x1.715476p+0f)
 *   r1 = y - n * 0x1.62E400p-1f                        the product is exact: |n| <= 116 and the constant has 15 significant bits
 *   r2 = r1 - n * 0x1.7F7D1Cp-20f
 *   p  = 0x1.0F9F9Cp-7f
 *   p  = p * r2;  p = p + 0x1.573A1Ap-5f
 *   p  = p * r2;  p = p + 0x1.555A80p-3f
 *   p  = p * r2;  p = p + 0x1.FFFDC6p-2f
 *   p  = p * r2;  p = p + 0x1.FFFFF6p-1f
 *   p  = p * r2;  p = p + 1.0f
 *   e_a = p * 2^n                                      2^n from the bits (n + 127) << 23; the exp lines of the gated definition
 *                                                      of qnnpack_gfx950_dynamic.h, constant for constant; e_0 is exactly 1
 *   S = e_0;  for a = 1 .. A - 1 IN THIS ORDER:  S = S + e_a
 *   w_a = e_a / S                                      an IEEE division
 *   group_ids[t A + a] = (int32) sel_a - (int32) first_group;   weights[t A + a] = w_a
 * Slots come out in descending logit order. This is the softmax over the selected logits: gpt-oss's form, and in real
 * arithmetic equal to "softmax over all, top-k, renormalize" (Mixtral; Qwen3 with norm_topk_prob). first_group serves
 * expert-parallel sharding: ids below it come out negative, and the grouped operator and the combine skip those, as they
 * skip ids at or above their `groups`.
 *
 * No result depends on the denormal mode. Clamp, keys and selection are integer work. d_a = l_a - m:
 *   - If |m| and |l_a| are both below 2^-100, then |d_a| < 2^-99 in either mode, denormal, flushed or neither:
 *     y * 0x1.715476p+0f rounds to n = -0 whatever it was, r2 = y, every p * r2 is far below the last place of the constant
 *     added to it, so p = 1 and e_a = 1 (step "s" of the gated argument).
 *   - Otherwise one of the two is at least 2^-100 in magnitude. If the other is a denormal, it lies below 2^-126, a quarter
 *     of the larger one's last place (at least 2^-123): the difference rounds to the same number whether that operand is read
 *     as itself or as zero -- if m >= 2^-100, a denormal l_a lies below half a last place of m. If both are normal, d_a is
 *     at least 2^-101 in magnitude, or the two are within a factor of two of each other and d_a is zero or a multiple of
 *     2^-124. Either way d_a is zero or a normal number, the same in both modes.
 *   - For such a d_a: y is zero or a normal number in [-80, -2^-124]; with n = 0, r2 = y; with n != 0, r1 and r2 are zero or
 *     differences of multiples of 2^-44, far above 2^-126; a p * r2 below 2^-126 is absorbed by its constant flushed or not.
 *   - Every e_a >= 2^-116 is normal, S lies in [1, 8], and w_a >= 2^-116 / 8 = 2^-119 is normal.
 *
 * Create answers, in this order: uninitialized; invalid_parameter for groups == 0, assignments == 0, assignments > groups;
 * unsupported_parameter for groups > 1024, assignments > 8, first_group >= 2^31; invalid_parameter inside a graph capture;
 * out_of_memory. A refused create writes no handle. `flags` is accepted and ignored.
 *
 * Setup answers, in this order: uninitialized; invalid_parameter for a NULL handle, inside a graph capture, for a handle of
 * another kind. batch_size == 0 then succeeds and the run does nothing. invalid_parameter: a NULL tensor, a pointer that is not
 * 4-byte aligned, a stride below E. unsupported_parameter: batch_size * A >= 2^20, the grouped operator's limit on its output
 * rows -- whatever the router produces the grouped setup accepts; it is answered from the sizes alone, before a span is formed
 * or a pointer looked at. invalid_parameter: any two of the three byte spans sharing a byte; a tensor that is not memory of
 * the operator's device, host memory included (the grouped operator needs the ids on the device anyway). A refused setup leaves
 * the previous one runnable.
 *
 * Kernel (hip/f32topk.hip). One launch. A token's logits live in the registers of a group of L lanes, V per lane; each of the
 * A rounds is a per-lane maximum, log2(L) cross-lane exchange steps, and the winner struck out. L and V follow from E alone:
 *     f32_topk_l8_v4     E <=   32    eight tokens per wave
 *     f32_topk_l16_v4    E <=   64    four
 *     f32_topk_l32_v4    E <=  128    two
 *     f32_topk_l64_v4    E <=  256    one wave per token
 *     f32_topk_l64_v8    E <=  512
 *     f32_topk_l64_v16   E <= 1024
 * each with _x4 behind its name where the logits' base or, with more than one token, their stride is no multiple of 16
 * bytes: 4-byte loads. No scratch memory, no LDS.
 *
 * ---- The combine ----
 * create(channels = N < 2^24, assignments = A in 1 .. 8, groups in 1 .. 1024: ids in [0, groups) count, flags)
 * setup(combine, batch_size = T, input [T A] rows of N, input_stride, weights [T A], group_ids [T A], output [T] rows of N,
 *       output_stride); both strides in ELEMENTS
 *
 * Definition (bit-exact, no tolerance). flush(v) = |v| <= 0x1p-126f ? copysignf(0, v) : v. Per token t and column c, float32,
 * each operation rounded once, nothing fused:
 *   acc = +0.0f
 *   for a = 0 .. A - 1 IN THIS ORDER, j = t A + a:
 *       if 0 <= group_ids[j] < groups:
 *           p   = flush(weights[j] * input[j][c])
 *           acc = flush(acc + p)
 *   output[t][c] = acc
 * A row whose id is outside [0, groups) contributes nothing and NO BYTE OF IT IS READ: the grouped operator never wrote it.
 * If all A rows are skipped the output is +0. NaN and infinities in rows that count, and in their weights, follow the
 * formulas. group_ids and weights are read when the operator runs: overwriting them and running again, or replaying a
 * graph, combines the new way with no setup in between. They must not change while a run is in flight.
 *
 * No result depends on the denormal mode. A product or a sum whose exact value is below 2^-126 in magnitude is, rounded, a
 * denormal or exactly 2^-126 in one mode and either of those or a zero of the same sign in the other, whichever way a mode
 * decides that a result within one rounding of 2^-126 is tiny; flush, with <= (step "a" of the gated argument), makes all
 * of them that zero. What passes flush is a normal number above 2^-126, the same in both modes, so every operand of the next
 * operation is the same. A denormal weight or input element is read as itself or as a zero of its sign; either way its
 * product with a finite value below 2^126 is at most 2^-126 in magnitude and flushed to the same zero -- a denormal times a
 * value of 2^126 or more, or times infinity, is the one place the modes part: weights are the router's, in [2^-119, 1], and
 * the expert rows are the grouped operator's, which are zero or normal (qnnpack_gfx950_dynamic.h).
 *
 * Create answers, in this order: uninitialized; invalid_parameter for zero channels, assignments or groups;
 * unsupported_parameter for assignments > 8, groups > 1024, channels >= 2^24; invalid_parameter inside a graph capture;
 * out_of_memory. A refused create writes no handle.
 *
 * Setup follows the grouped setup's pattern: uninitialized; invalid_parameter for a NULL handle, inside a graph capture, for a
 * handle of another kind. batch_size == 0 then succeeds and the run does nothing. invalid_parameter: a NULL tensor, weights or
 * group_ids; one of the four that is not 4-byte aligned; a stride below N. unsupported_parameter: batch_size * A >= 2^20, from
 * the sizes alone. invalid_parameter: an output whose byte span shares a byte with that of the input, the weights or the
 * group_ids; one of the four that is not memory of the operator's device, host memory included. A refused setup leaves the
 * previous one runnable.
 *
 * Kernel (hip/f32combine.hip). One launch, streaming. A workgroup owns one token and a run of columns, four per lane: the
 * token's ids and weights are uniform, fetched once, and whether a row counts is one branch for the whole workgroup. The
 * loads of all rows that count are issued before the first multiply.
 *     f32_combine_wave    N <= 256    one wave per token
 *     f32_combine_block   beyond      256 lanes per token and 1024 columns
 * each with _x4 behind its name where a base or, with more than one row, a stride of the input or the output is no
 * multiple of 16 bytes: 4-byte loads and stores. Columns past N are never touched. No scratch memory, no LDS.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack.h"

#ifdef __cplusplus
extern "C" {
#endif

enum qnnp_status qnnp_gfx950_create_topk_router_nc_f32(
    size_t groups,                       /* E, 1 .. 1024 */
    size_t assignments,                  /* A, 1 .. 8, <= E */
    uint32_t first_group,                /* subtracted from every id; < 2^31 */
    uint32_t flags,
    qnnp_operator_t* router);

enum qnnp_status qnnp_gfx950_setup_topk_router_nc_f32(
    qnnp_operator_t router,
    size_t batch_size,                   /* T */
    const float* logits,                 /* [T] rows of E floats, device */
    size_t logits_stride,                /* in elements, >= E */
    int32_t* group_ids,                  /* [T * A], device */
    float* weights);                     /* [T * A], device */

enum qnnp_status qnnp_gfx950_create_weighted_combine_nc_f32(
    size_t channels,                     /* N, < 2^24 */
    size_t assignments,                  /* A, 1 .. 8 */
    size_t groups,                       /* ids in [0, groups) count; 1 .. 1024 */
    uint32_t flags,
    qnnp_operator_t* combine);

enum qnnp_status qnnp_gfx950_setup_weighted_combine_nc_f32(
    qnnp_operator_t combine,
    size_t batch_size,                   /* T */
    const float* input,                  /* [T * A] rows of N floats, device */
    size_t input_stride,                 /* in elements, >= N */
    const float* weights,                /* [T * A], device; read when the operator runs */
    const int32_t* group_ids,            /* [T * A], device; read when the operator runs */
    float* output,                       /* [T] rows of N floats, device */
    size_t output_stride);

#ifdef __cplusplus
}
#endif
