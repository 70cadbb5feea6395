/*
 * qnnpack_gfx950_dynamic.h -- a DYNAMICALLY QUANTIZED fully connected operator: float32 in, float32 out, int8 on the
 * matrix cores in between (W8A8 with one activation scale per row -- per token --, one weight scale per output channel).
 * The caller needs no calibrated activation range: every input row is quantized to its own range inside the operator.
 * This is the shape of PyTorch's quantized::linear_dynamic, of transformer and recommender MLPs, LSTM / GRU gates and
 * the classifier head of a float model. No reference counterpart. An operator behind qnnp_run_operator /
 * qnnp_delete_operator like every other one: it records into the library's hipGraph capture (as its two launches), runs
 * on the library stream, and takes host tensors through the device staging.
 *
 * Definition (bit-exact, no tolerance). All arithmetic is float32, every operation rounded once (no fused multiply-add),
 * in this order. Per input row r, with K = input_channels:
 *   lo = min(0, min_k x[r][k]);  hi = max(0, max_k x[r][k])           NaN elements are ignored by the min and the max
 *   scale_r = (hi - lo) / 255.0f                                        an IEEE division
 *   if !(scale_r >= 0x1p-60f && scale_r <= 0x1p60f)  scale_r = 1.0f    all-zero rows, overflowed and denormal ranges
 *   inv = 1.0f / scale_r;  zp_r = (int32) rintf(min(-lo * inv, 255.0f))          ties to even
 *   t = x * inv;  t = isnan(t) ? 0 : t;  t = min(max(t, (float) -zp_r), (float) (255 - zp_r))
 *   q = (int32) rintf(t) + zp_r                                         in [0, 255]
 * Per output (r, c):
 *   acc = sum_k (q[r][k] - zp_r) * kernel[c][k]                         exact in int32
 *   s = scale_r * kernel_scales[c]
 *   y = (float) acc * s;  y = y + bias[c];  y = min(max(y, output_min), output_max)      (float) acc: to nearest even
 * The bytes are THIS definition's, not PyTorch's: quantized::linear_dynamic nudges its zero point differently.
 *
 * No result depends on the denormal mode. Output side: kernel_scales lie in [2^-20, 2^20], a row scale that passes the
 * test above is at least 2^-60 and a bias is zero or a normal number. So s >= 2^-80 is normal, a nonzero product
 * (float) acc * s is at least 2^-80, and a sum y + bias that cancels is zero or a multiple of about 2^-103 (the last
 * place of a product of that size): never a denormal. Input side: a denormal x gives |x * inv| < 2^-126 * 2^60, which
 * rounds to the zero point flushed or not; and a range hi - lo that is denormal or flushed to zero fails the test above
 * either way and takes scale 1.
 *
 * The accumulator cannot wrap: |q - zp_r| <= 255, |kernel| <= 128, K <= 32768 give |acc| <= 255 * 128 * 32768 < 2^31.
 * The kernels compute it as sum_k (q - 128) * kernel[c][k] + (128 - zp_r) * wsum[c] with wsum[c] = sum_k kernel[c][k]:
 * either part is at most 2^29 in magnitude.
 *
 * Create answers, in this order: uninitialized; invalid_parameter for a zero channel count, a NULL kernel or
 * kernel_scales, a scale that is not a normal number above zero, a bias that is NaN, infinite or denormal, an
 * output_min or output_max that is NaN, output_min > output_max; unsupported_parameter for a scale outside
 * [2^-20, 2^20], input_channels > 32768, output_channels >= 2^24; out_of_memory. A refused create writes no handle.
 * kernel, kernel_scales and bias are host memory, read during the call and not kept. bias == NULL means all zero;
 * -INFINITY / +INFINITY as output_min / output_max mean no clamp. `flags` is accepted and ignored.
 *
 * Setup follows qnnpack_gfx950_float.h: both strides count ELEMENTS. batch_size == 0 succeeds and the run does nothing.
 * invalid_parameter: a NULL tensor, a pointer that is not 4-byte aligned, a stride below the channel count of its side,
 * input and output byte spans that share a byte, memory of another GPU, a call inside a graph capture.
 * unsupported_parameter: batch_size >= 2^31. Every check comes before the operator changes: a refused setup leaves the
 * previous one runnable. Setup grows the one device scratch the operator owns (the quantized rows, k_pad = K rounded up
 * to 64 bytes each, and eight bytes per row of scale and zero point); it never shrinks and is freed with the operator.
 *
 * Kernels. A run is two launches, chosen by batch_size and K alone (and the input's alignment for the load width):
 *   rows (hip/f32qd8rows.hip; qnnp_gfx950_dynamic_rows_kernel names it)
 *     f32_qd8_rows_wave      K <= 1024       one wave per row
 *     f32_qd8_rows_block     K <= 16384      one workgroup per row, the row read once and kept in registers
 *     f32_qd8_rows_twopass   K <= 32768      the row is read twice
 *     each with _x4 behind its name where the input base or, with more than one row, the input stride is no multiple of
 *     16 bytes: 4-byte loads
 *   matrix product and float epilogue (hip/qd8f32gemm.hip; qnnp_gfx950_operator_kernel names it)
 *     qd8_f32_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_gemm_mfma_128x128   batch_size > 16
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8(
    size_t input_channels,
    size_t output_channels,
    const int8_t* kernel,          /* [output_channels][input_channels], symmetric int8, host */
    const float* kernel_scales,    /* [output_channels], host */
    const float* bias,             /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

/*
 * The same operator with 4-BIT weights (qd8-f32-qc4w: one scale per output channel, no block-wise scales). Byte k / 2 of
 * row c of `kernel` holds weight (c, k) in bits 4 (k % 2) .. 4 (k % 2) + 3, a two's-complement signed nibble in [-8, 7];
 * with an odd input_channels the high nibble of a row's last byte is ignored, whatever it holds. The definition above
 * holds with kernel[c][k] read as that nibble, and nothing else changes: |acc| <= 255 * 8 * 32768 < 2^31. The kernels
 * feed the matrix cores 16 * kernel[c][k] (the nibble in the top half of an int8), so their loop sums
 * 16 * sum_k (q - 128) * kernel[c][k], at most 128 * 128 * 32768 = 2^29 in magnitude, and shift it right by four: exact.
 *
 * Statuses and their order are those of qnnp_gfx950_create_fully_connected_nc_f32_qd8, the limits
 * input_channels <= 32768 and output_channels < 2^24 included. The handle is set up with
 * qnnp_gfx950_setup_fully_connected_nc_f32_qd8 and is run, captured, named and deleted like the int8 one: the row launch and
 * the scratch are the same, only the weight image (half the bytes, K rounded up to 128) and the second launch differ
 * (hip/qd8f32gemm4.hip; qnnp_gfx950_operator_kernel names it):
 *     qd8_f32_qc4w_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_qc4w_gemm_mfma_128x128   batch_size > 16
 */
enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qc4w(
    size_t input_channels,
    size_t output_channels,
    const uint8_t* kernel,         /* [output_channels][(input_channels + 1) / 2], two signed nibbles per byte, host */
    const float* kernel_scales,    /* [output_channels], host */
    const float* bias,             /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

/*
 * The 4-bit operator with BLOCK-WISE weight scales (qd8-f32-qb4w: what symmetric GPTQ and GGUF weights carry; AWQ and
 * asymmetric GPTQ weights also carry a zero point per block: _qb4w_zp below): one scale per
 * output channel and per block of B = block_size consecutive K positions. `kernel` is the _qc4w layout,
 * [output_channels][input_channels / 2] bytes (K is even here: no spare nibble); `kernel_scales` is
 * [output_channels][input_channels / block_size].
 *
 * Definition (bit-exact, no tolerance). Per input row, q, zp_r and scale_r are exactly those above. With nb = K / B, all
 * float operations float32, each rounded once, no fused multiply-add; per output (r, c):
 *   acc_b = sum_{k in [b B, (b + 1) B)} (q[r][k] - zp_r) * kernel[c][k]      exact in int32, b = 0 .. nb - 1
 *   t_b   = (float) acc_b * kernel_scales[c][b]                 the conversion is exact: |acc_b| <= 255 * 8 * 256 < 2^19
 *   ysum  = 0.0f;  for b = 0, 1, ..., nb - 1 IN THIS ORDER:  ysum = ysum + t_b
 *   y     = ysum * scale_r;  y = y + bias[c];  y = min(max(y, output_min), output_max)
 * The acc_b are exact integers and every t_b depends on its own block alone, so the kernels split K between waves, passes
 * and matrix instructions at any block boundary, in any order. Only the chain ysum = ysum + t_b is ordered: it has ONE
 * owner per output, which walks b upward.
 *
 * The block table. Per (channel, block) the device holds s16 = kernel_scales[c][b] / 16 and
 * wsum16 = 16 * sum_{k in block} kernel[c][k]. The kernels' loop sum is L = 16 * sum (q - 128) * kernel[c][k] (the nibble
 * in the top half of an int8), at most 128 * 128 * 256 = 2^22 per block, and L + (128 - zp_r) * wsum16 = 16 * acc_b exactly,
 * below 2^24. They compute t_b = (float) (16 acc_b) * s16 without the shift of _qc4w: both conversions are exact, s16 is
 * exact, and (16 acc_b) * (s / 16) is the same real number as acc_b * s with no underflow in between, so the one rounding
 * gives the same bits.
 *
 * Block scales lie in [2^-16, 2^16], narrower than the [2^-20, 2^20] of the other creates, and each is a normal number
 * above zero: that keeps the results independent of the denormal mode here too. A nonzero t_b is at least 2^-16 in
 * magnitude and, |acc_b| < 2^19 having at most 19 significant bits, a multiple of 2^-39 (the last place of a scale of
 * 2^-16 is 2^-39). So every partial ysum is zero or a multiple of 2^-39, never a denormal, and below 2^9 * 2^19 * 2^16 <
 * 2^44. ysum * scale_r is zero or at least 2^-39 * 2^-60 = 2^-99 in magnitude, and a sum with a normal bias that cancels
 * is zero or a multiple of the product's last place, at least 2^-99 * 2^-24 = 2^-123: still normal. With scales down to
 * 2^-20 the same chain would end at 2^-127, a denormal.
 *
 * Create answers, in the order of the other creates: uninitialized; invalid_parameter as above and for block_size == 0 (the
 * scale checks read input_channels / block_size scales per channel, rounded down); unsupported_parameter for a
 * block_size other than 64, 128 and 256, an input_channels that is no multiple of block_size, a scale outside
 * [2^-16, 2^16], input_channels > 32768, output_channels >= 2^24; out_of_memory. An argument set that is both invalid and
 * unsupported answers invalid_parameter. Block size 32 is refused here and by _qb4w_zp: one v_mfma_i32_16x16x64_i8 sums 64
 * consecutive K positions, so a 32-wide block needs the 16x16x32 instruction and a different fragment image. Those are
 * qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_b32's, below.
 *
 * The handle is set up with qnnp_gfx950_setup_fully_connected_nc_f32_qd8 and run, captured, named and deleted like the
 * others: the row launch, the scratch and the weight image (the _qc4w one) are the same, the second launch is
 * hip/qd8f32gemm4b.hip's (qnnp_gfx950_operator_kernel names it):
 *     qd8_f32_qb4w_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_qb4w_gemm_mfma_128x128   batch_size > 16    (128 x 128 tiles fit the register file without scratch memory)
 * The block table adds 8 bytes per channel and block to the device image: 25 %, 12.5 % and 6.25 % of the weight bytes at
 * B = 64, 128 and 256.
 */
enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w(
    size_t input_channels,
    size_t output_channels,
    size_t block_size,             /* 64, 128 or 256; divides input_channels */
    const uint8_t* kernel,         /* [output_channels][input_channels / 2], two signed nibbles per byte as _qc4w, host */
    const float* kernel_scales,    /* [output_channels][input_channels / block_size], host */
    const float* bias,             /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

/*
 * The block-wise 4-bit operator with one integer ZERO POINT per output channel and block (w = (u - z) * scale: the form of
 * AWQ weights, of GPTQ weights with sym=False, of torchao's int4 and HQQ's integer mode). `kernel` has the _qb4w layout,
 * [output_channels][input_channels / 2] bytes with weight k in bits 4 (k % 2) .. 4 (k % 2) + 3 of byte k / 2, but each
 * nibble is UNSIGNED, u in [0, 15]; `kernel_scales` and `kernel_zero_points` are [output_channels][input_channels /
 * block_size], every zero point in [0, 15]. The zero point cannot be folded into the nibbles: u - z spans [-15, 15].
 *
 * Definition (bit-exact, no tolerance). Per input row, q, zp_r and scale_r are exactly those above. With B = block_size,
 * nb = K / B, u[c][k] the nibble and z[c][b] the zero point, all float operations float32, each rounded once, no fused
 * multiply-add; per output (r, c):
 *   acc_b = sum_{k in [b B, (b + 1) B)} (q[r][k] - zp_r) * (u[c][k] - z[c][b])     exact in int32, b = 0 .. nb - 1
 *   t_b   = (float) acc_b * kernel_scales[c][b]                 the conversion is exact: |acc_b| <= 255 * 15 * 256 < 2^20
 *   ysum  = 0.0f;  for b = 0, 1, ..., nb - 1 IN THIS ORDER:  ysum = ysum + t_b
 *   y     = ysum * scale_r;  y = y + bias[c];  y = min(max(y, output_min), output_max)
 * The chain and the finish are _qb4w's: ONE owner per output walks b upward, everything else may happen anywhere.
 *
 * Consequence: with every zero point 8 and u = w + 8 (the signed nibble w of _qb4w with bit 3 flipped, byte ^ 0x88), the
 * acc_b are those of _qb4w, and the result equals the _qb4w operator's bit for bit on equal scales.
 *
 * Where the zero point enters. The kernels subtract it while they unpack the nibbles, so that the matrix cores multiply
 * (q - 128) with the int8 u - z itself; their loop sum is L = sum (q - 128) * (u - z), at most 128 * 15 * 256 per block. Per
 * (channel, block) the device holds the scale as given and wsum = sum_{k in block} (u - z), at most 15 * 256 in magnitude,
 * and L + (128 - zp_r) * wsum = acc_b exactly. There is no factor 16 as in _qb4w: t_b is computed as the definition writes it.
 * The zero points themselves travel in a second table of one uint16 per channel and 128 K positions (both 64-wide halves'
 * zero points), 1 / 32 of the weight bytes, next to the 8 bytes per channel and block of the block table.
 *
 * Block scales lie in [2^-16, 2^16] and each is a normal number above zero, as for _qb4w, and no result depends on the
 * denormal mode: a nonzero t_b is at least 2^-16 in magnitude and, |acc_b| < 2^20 having at most 20 significant bits, a
 * multiple of 2^-39 (the last place of a scale of 2^-16 is 2^-39). So every partial ysum is zero or a multiple of 2^-39, never
 * a denormal, and below 2^9 * 2^20 * 2^16 = 2^45. ysum * scale_r is zero or at least 2^-39 * 2^-60 = 2^-99 in magnitude, and
 * a sum with a normal bias that cancels is zero or a multiple of the product's last place, at least 2^-99 * 2^-24 = 2^-123:
 * still normal.
 *
 * Create answers in _qb4w's order, with two additions: a NULL kernel_zero_points is invalid_parameter with the other NULL
 * pointers, and a zero point above 15 is invalid_parameter, checked behind the scales' validity (a normal number above
 * zero) and in front of the bias, over input_channels / block_size entries per channel, rounded down, like the scale
 * checks. An argument set that is both invalid and unsupported answers invalid_parameter; a refused create writes no
 * handle; block size 32 stays refused; input_channels <= 32768 and output_channels < 2^24 as before.
 *
 * The handle is set up with qnnp_gfx950_setup_fully_connected_nc_f32_qd8 and run, captured, named and deleted like the
 * others: the row launch and the scratch are the same, the second launch is hip/qd8f32gemm4z.hip's
 * (qnnp_gfx950_operator_kernel names it):
 *     qd8_f32_qb4w_zp_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_qb4w_zp_gemm_mfma_128x128   batch_size > 16    (no scratch memory at any block size)
 */
enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_zp(
    size_t input_channels,
    size_t output_channels,
    size_t block_size,                   /* 64, 128 or 256; divides input_channels */
    const uint8_t* kernel,               /* [output_channels][input_channels / 2], two UNSIGNED nibbles per byte, host */
    const float* kernel_scales,          /* [output_channels][input_channels / block_size], host */
    const uint8_t* kernel_zero_points,   /* [output_channels][input_channels / block_size], each in [0, 15], host */
    const float* bias,                   /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

/*
 * The block-wise 4-bit operator with BLOCKS OF 32 K positions: the block of GGUF Q4_0 and Q4_1 and of GPTQ, AWQ and torchao
 * checkpoints made with group_size = 32. `kernel` has the _qb4w nibble layout, `kernel_scales` and `kernel_zero_points` are
 * [output_channels][input_channels / 32].
 *
 * Definition (bit-exact, no tolerance): _qb4w_zp's with B = 32. Per input row, q, zp_r and scale_r are those above; all float
 * operations float32, each rounded once, no fused multiply-add; per output (r, c), with nb = K / 32:
 *   acc_b = sum_{k in [32 b, 32 b + 32)} (q[r][k] - zp_r) * (u[c][k] - z[c][b])     exact in int32, b = 0 .. nb - 1
 *   t_b   = (float) acc_b * kernel_scales[c][b]                 the conversion is exact: |acc_b| <= 255 * 15 * 32 < 2^17
 *   ysum  = 0.0f;  for b = 0, 1, ..., nb - 1 IN THIS ORDER:  ysum = ysum + t_b
 *   y     = ysum * scale_r;  y = y + bias[c];  y = min(max(y, output_min), output_max)
 * With kernel_zero_points == NULL the nibbles are SIGNED, w in [-8, 7] as in _qb4w, and the definition holds with u - z read
 * as w. The create turns that form into the other while it packs: u = w ^ 8 and z = 8 give the same acc_b, hence the same
 * bits, and one kernel pair serves both forms.
 *
 * Block scales lie in [2^-16, 2^16] and each is a normal number above zero, and no result depends on the denormal mode: a
 * nonzero t_b is at least 2^-16 in magnitude and, |acc_b| < 2^17 having at most 17 significant bits, a multiple of 2^-39 (the
 * last place of a scale of 2^-16). There are at most 32768 / 32 = 2^10 blocks, so every partial ysum is zero or a multiple of
 * 2^-39, never a denormal, and below 2^10 * 2^17 * 2^16 = 2^43. ysum * scale_r is zero or at least 2^-39 * 2^-60 = 2^-99 in
 * magnitude, and a sum with a normal bias that cancels is zero or a multiple of the product's last place, at least
 * 2^-99 * 2^-24 = 2^-123: still normal.
 *
 * Create answers in _qb4w_zp's order: uninitialized; invalid_parameter for a zero channel count, a NULL kernel or
 * kernel_scales, a scale that is not a normal number above zero, a zero point above 15 (checked only where zero points are
 * given), a bad bias, a bad clamp; unsupported_parameter for an input_channels that is no multiple of 32, a scale outside
 * [2^-16, 2^16], input_channels > 32768, output_channels >= 2^24; out_of_memory. The scale and zero-point checks read
 * input_channels / 32 entries per channel, rounded down. An argument set that is both invalid and unsupported answers
 * invalid_parameter; a refused create writes no handle.
 *
 * The handle is set up with qnnp_gfx950_setup_fully_connected_nc_f32_qd8 and run, captured, named and deleted like the
 * others: the row launch and the scratch are the same (K rounded up to 64 per row, so K may be an odd multiple of 32), the
 * weight image and the second launch are hip/qd8f32gemm4s.hip's (qnnp_gfx950_operator_kernel names it), on
 * v_mfma_i32_16x16x32_i8, one instruction per block and 16 x 16 outputs:
 *     qd8_f32_qb4w_b32_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_qb4w_b32_gemm_mfma_128x128   batch_size > 16    (no scratch memory)
 * Scales, weight sums and zero points add 6 bytes per channel and block to the device image: 37.5 % of the weight bytes.
 */
enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_b32(
    size_t input_channels,               /* a multiple of 32 */
    size_t output_channels,
    const uint8_t* kernel,               /* [output_channels][input_channels / 2], the _qb4w nibble layout, host */
    const float* kernel_scales,          /* [output_channels][input_channels / 32], host */
    const uint8_t* kernel_zero_points,   /* [output_channels][input_channels / 32], each in [0, 15]; NULL: signed nibbles */
    const float* bias,                   /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

/*
 * The operator with MXFP4 weights (OCP Microscaling: what FP4 checkpoints for this hardware generation carry): 4-bit
 * FLOATING-POINT codes, E2M1, two per byte in the _qb4w nibble layout, and one E8M0 power-of-two scale per output channel and
 * block of 32 consecutive K positions, `kernel_scales` [output_channels][input_channels / 32] bytes e, scale = 2^(e - 127).
 *
 * Definition (bit-exact, no tolerance). An E2M1 code c has its sign in bit 3 and a magnitude index c & 7 into
 * {0, 0.5, 1, 1.5, 2, 3, 4, 6}. Let w2[c][k] be TWICE that value, an integer in {0, +-1, +-2, +-3, +-4, +-6, +-8, +-12}; code
 * 8 (-0) is 0. Per input row, q, zp_r and scale_r are those of the first definition above; all float operations float32, each
 * rounded once, no fused multiply-add; per output (r, c), with nb = K / 32 and e[c][b] the block's scale byte:
 *   acc_b = sum_{k in [32 b, 32 b + 32)} (q[r][k] - zp_r) * w2[c][k]     exact; |acc_b| <= 255 * 12 * 32 = 97920 < 2^17
 *   t_b   = (float) acc_b * 2^(e[c][b] - 128)                            exact: a 17-bit integer times a power of two
 *   ysum  = 0.0f;  for b = 0, 1, ..., nb - 1 IN THIS ORDER:  ysum = ysum + t_b
 *   y     = ysum * scale_r;  y = y + bias[c];  y = min(max(y, output_min), output_max)
 * The halving of w2 is the 128 in the exponent where the scale has 127. Twice an E2M1 value being an integer is what puts
 * the format on the INTEGER matrix cores: a block is one v_mfma_i32_16x16x32_i8 as in _qb4w_b32, the term is exact, and the
 * only roundings are those of the chain and the finish, which are _qb4w's: ONE owner per output walks b upward.
 *
 * Scales are restricted to 2^-16 .. 2^16 (e in [111, 143]), the range of the other block-wise creates, and no result depends
 * on the denormal mode: a nonzero t_b is a nonzero integer times 2^(e - 128), so a multiple of 2^-17 and at least that large.
 * There are at most 32768 / 32 = 2^10 blocks, so every partial ysum is zero or a multiple of 2^-17, never a denormal, and
 * below 2^10 * 2^17 * 2^15 = 2^42. ysum * scale_r is zero or at least 2^-17 * 2^-60 = 2^-77 in magnitude, and a sum with a
 * normal bias that cancels is zero or a multiple of the product's last place, at least 2^-77 * 2^-24 = 2^-101: still normal.
 *
 * Consequence: where every code's w2 lies in [-8, 7] (no +4, no +-6) and e is in [112, 143], the _qb4w_b32 operator on the
 * signed nibbles w2, kernel_zero_points == NULL and block scales 2^(e - 128) has the same acc_b and the same t_b, hence the
 * same bits. At e = 111 that scale would be 2^-17, below _qb4w_b32's range.
 *
 * Create answers, in the order of the other creates: uninitialized; invalid_parameter for a zero channel count, a NULL kernel
 * or kernel_scales, a scale byte of 255 (E8M0's NaN; checked where the other creates check for a normal number above zero,
 * over input_channels / 32 entries per channel, rounded down), a bad bias, a bad clamp; unsupported_parameter for an
 * input_channels that is no multiple of 32, a scale byte outside [111, 143] (refused, not clamped), input_channels > 32768,
 * output_channels >= 2^24; out_of_memory. An argument set that is both invalid and unsupported answers invalid_parameter; a
 * refused create writes no handle.
 *
 * The handle is set up with qnnp_gfx950_setup_fully_connected_nc_f32_qd8 and run, captured, named and deleted like the
 * others: the row launch and the scratch are the same, the weight image is _qb4w_b32's holding the raw codes, and the second
 * launch is hip/qd8f32gemm4m.hip's (qnnp_gfx950_operator_kernel names it), which decodes the codes to w2 in registers:
 *     qd8_f32_mxfp4w_gemv_mfma_16        batch_size <= 16
 *     qd8_f32_mxfp4w_gemm_mfma_128x128   batch_size > 16    (no scratch memory)
 * Scale and weight sum share one 32-bit word per block: 4 bytes per block, 25 % of the weight bytes (_qb4w_b32: 6 and 37.5 %).
 */
enum qnnp_status qnnp_gfx950_create_fully_connected_nc_f32_qd8_mxfp4w(
    size_t input_channels,               /* a multiple of 32, <= 32768 */
    size_t output_channels,              /* < 2^24 */
    const uint8_t* kernel,               /* [output_channels][input_channels / 2]: E2M1 code of weight k in bits 4 (k % 2) .. + 3 of byte k / 2, host */
    const uint8_t* kernel_scales,        /* [output_channels][input_channels / 32]: E8M0, scale = 2^(e - 127), host */
    const float* bias,                   /* [output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

enum qnnp_status qnnp_gfx950_setup_fully_connected_nc_f32_qd8(
    qnnp_operator_t fully_connected,
    size_t batch_size,
    const float* input,
    size_t input_stride,
    float* output,
    size_t output_stride);

/*
 * The GROUPED operator with MXFP4 weights, for the expert matrices of a mixture-of-experts layer: `groups` weight sets of
 * the _mxfp4w kind in ONE operator, and per output row an id that says which set multiplies it. The ids live in device
 * memory and are read BY THE DEVICE WHEN THE OPERATOR RUNS: a router's choice needs no read-back, no gather, no launch per
 * expert, and the run can be captured in a graph.
 *
 * `kernel`, `kernel_scales` and `bias` are those of the _mxfp4w create, `groups` of them one behind the other. Setup takes
 * batch_size input rows (tokens), `assignments` = A output rows per input row (the router's top-k) and group_ids
 * [batch_size * A]; the output has R = batch_size * A rows, row j belonging to input row j / A.
 *
 * Definition (bit-exact, no tolerance). For j in [0, R) let g = group_ids[j], read at run time.
 *   0 <= g < groups: output row j is what the _mxfp4w definition above gives for input row j / A with group g's codes, scales
 *       and bias: the row quantization, the exact block sums acc_b, the terms t_b, the float32 chain over b in ascending order
 *       and the finish, all unchanged. It equals the stand-alone _mxfp4w operator's result on that group's weights bit for bit.
 *   any other g: the row is SKIPPED, no byte of output row j is written. Negative ids are the masked rows of a padded batch,
 *       ids at or above `groups` the experts that live on another device.
 * Only the bytes of group_ids at the moment of the run count: overwriting them and running again (or replaying a graph)
 * routes the new way with no setup in between. They must not change WHILE a run is in flight.
 *
 * Create answers in the _mxfp4w order: invalid_parameter also for groups == 0 (with the zero channel counts),
 * unsupported_parameter also for groups > 1024 (with the other limits, so behind the scale checks, which run over every
 * group, as the bias check does).
 *
 * Setup follows qnnp_gfx950_setup_fully_connected_nc_f32_qd8, which refuses a grouped handle as this one refuses any other
 * (invalid_parameter). batch_size == 0 succeeds and the run does nothing. invalid_parameter: a NULL tensor or group_ids,
 * assignments == 0, a tensor or group_ids that is not 4-byte aligned, a stride below the channel count, an output whose byte
 * span shares a byte with the input's or with that of group_ids, a tensor or group_ids that is not memory of the operator's
 * device (host memory included: the device reads the ids, and a staged output could not leave skipped rows alone), a call
 * inside a capture. unsupported_parameter: assignments > 8, R >= 2^20, more than 2^31 bytes of quantized input rows
 * (batch_size * K rounded up to 64: a gathered row is addressed by a 32-bit offset), a launch grid beyond 2^31 - 1
 * workgroups; these are answered from the sizes alone, before the spans are formed or a pointer is looked at. A refused setup
 * leaves the previous one runnable.
 *
 * A run is three launches (hip/qd8f32gemm4g.hip). The row kernel above over the batch_size INPUT rows: a token routed to
 * four experts is quantized once. qd8_grouped_plan, one workgroup: a histogram of the ids, a prefix sum, the permutation of
 * the rows bucketed by group, one tile entry per H rows of a group, and the number of tiles. The product kernel, on a grid
 * fixed at setup from T = floor(R / H) + min(groups, R) row tiles, which is at least the number any routing needs (every
 * group with a row adds at most one partial tile); workgroups past the device's tile count leave at once. Its rows are
 * gathered through the permutation and its results scattered to their output rows. qnnp_gfx950_operator_kernel names it:
 *     qd8_f32_mxfp4w_grouped_mfma_16        R <= 16 * groups   (H = 16)
 *     qd8_f32_mxfp4w_grouped_mfma_128x128   otherwise          (H = 128; no scratch memory)
 * At a mean of 16 rows per group or fewer a 128-row tile is at least 7 / 8 padding. The handle is run, captured, named
 * (qnnp_gfx950_dynamic_rows_kernel too) and deleted like the others. The scratch grows by 4 bytes per output row and 16 per tile.
 */
enum qnnp_status qnnp_gfx950_create_grouped_fully_connected_nc_f32_qd8_mxfp4w(
    size_t groups,                       /* 1 .. 1024 */
    size_t input_channels,               /* a multiple of 32, <= 32768 */
    size_t output_channels,              /* < 2^24 */
    const uint8_t* kernel,               /* [groups][output_channels][input_channels / 2], the _mxfp4w code layout, host */
    const uint8_t* kernel_scales,        /* [groups][output_channels][input_channels / 32]: E8M0, e in [111, 143], host */
    const float* bias,                   /* [groups][output_channels] float32, host; NULL means all zero */
    float output_min,
    float output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

enum qnnp_status qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8(
    qnnp_operator_t fully_connected,
    size_t batch_size,                   /* input rows */
    size_t assignments,                  /* A = groups per input row, 1 .. 8 */
    const float* input,                  /* [batch_size] rows of input_channels floats, device */
    size_t input_stride,                 /* in elements */
    const int32_t* group_ids,            /* [batch_size * A], device; read when the operator runs */
    float* output,                       /* [batch_size * A] rows of output_channels floats, device */
    size_t output_stride);

/*
 * A GATED input (SwiGLU) for every handle above. A gated MLP, dense or expert, is two layers: the first produces gate and up
 * columns, the second consumes act(gate) * up. These two setups are the second layer's: they take the first layer's output as
 * it is, and the row kernel computes the product h while it reads, in registers, so that h is never written as floats and no
 * element-wise launch stands between the two matrix products. No new create: the first setup takes a handle of any of the
 * six plain creates, the second a handle of the grouped create.
 *
 * Input layout. With K = input_channels an input row holds 2 K floats: element 2 k is the gate g and element 2 k + 1 the up
 * value u of position k -- interleaved, not two halves (the column order of the MXFP4 mixture-of-experts checkpoints; a caller
 * with separate gate and up matrices interleaves their ROWS when creating the first layer). input_stride >= 2 K.
 *   SiLU-gated (Llama, Mixtral, Qwen):          alpha = 1,      limit = +INFINITY, up_shift = 0
 *   the clamped form of the MXFP4 checkpoints:  alpha = 1.702f, limit = 7,         up_shift = 1
 *
 * Definition (bit-exact, no tolerance). All arithmetic is float32, every operation rounded once, nothing fused. Per row r and
 * position k:
 *   gc = g > limit ? limit : g
 *   uc = u > limit ? limit : (u < -limit ? -limit : u)
 *   z  = alpha * gc
 *   y  = (-|z| < -80.0f) ? -80.0f : -|z|
 *   n  = rintf(y * 0x1.715476p+0f)
 *   r1 = y - n * 0x1.62E400p-1f            the product is exact: |n| <= 116 and the constant has 15 significant bits
 *   r2 = r1 - n * 0x1.7F7D1Cp-20f
 *   p  = 0x1.0F9F9Cp-7f
 *   p  = p * r2;  p = p + 0x1.573A1Ap-5f
 *   p  = p * r2;  p = p + 0x1.555A80p-3f
 *   p  = p * r2;  p = p + 0x1.FFFDC6p-2f
 *   p  = p * r2;  p = p + 0x1.FFFFF6p-1f
 *   p  = p * r2;  p = p + 1.0f
 *   e  = p * 2^n                           2^n from the bits (n + 127) << 23; n >= -116, so e is a normal number
 *   d  = 1.0f + e;  q = e / d              an IEEE division
 *   s  = z > 0 ? 1.0f - q : q              the sigmoid of z
 *   a  = gc * s;          if |a| <= 0x1p-126f: a = copysignf(0, a)      (<=, not <: step a of the denormal argument)
 *   b  = uc + up_shift;   if |b| < 0x1p-126f:  b = copysignf(0, b)
 *   h[r][k] = a * b
 * If g or u is NaN, h is NaN (NaN compares false, so gc or uc is that NaN; an implementation must not convert a NaN n to an
 * integer: any n serves, a = gc * s is NaN whatever s is). Infinite g and u follow the formulas: g = -inf gives z = -inf,
 * y = -80, a = -inf. Everything after that is the first definition of this header with h[r] as the input row x[r]: the
 * range, scale_r, zp_r, q, and the product and the finish of the handle's weight format, unchanged. A gated run equals, bit
 * for bit, the same handle's plain run on a float tensor holding h.
 *
 * The sigmoid's accuracy: against 1 / (1 + exp(-z)) in float64 the lines above have a largest relative error of
 * 4.46 * 2^-24 (4 000 001 points of linspace(-100, 100) and 2 000 000 samples of normal(0, 3), those with z > -80; measured
 * with their numpy restatement on a CPU). For z <= -80 the clamp pins the sigmoid at about exp(-80) = 1.8e-35 (1.5 * 2^-116): no claim there.
 *
 * No result depends on the denormal mode. alpha and limit lie in [2^-6, 2^6] (or limit is +INFINITY) and up_shift is zero or a
 * normal number. The steps, written out:
 *   s.  A |z| below 2^-100, denormal or flushed (a denormal g, or a small normal g times a small alpha): y * 0x1.715476p+0f rounds
 *       to n = -0 whatever it was, r2 = y, every p * r2 is far below the last place of the constant added to it, so p = 1, e = 1,
 *       q = 0.5 and s = 0.5 -- on EITHER branch of z > 0, which a denormal z takes differently in the two modes. For every other
 *       z: y is normal; with n = 0, r2 = y; with n != 0, r1 and r2 are zero or differences of multiples of 2^-44, far above
 *       2^-126; a p * r2 below 2^-126 is absorbed by its constant flushed or not; e >= 2^-116, d >= 1 and q >= 2^-117 are normal:
 *       s is the same normal number in both modes.
 *   a.  gc * s with an exact magnitude below 2^-126 (only a |g| below 2^-124 gets there: s < 1 / 4 needs |z| > 1, hence |g| > 2^-6)
 *       is, rounded, a denormal or exactly 2^-126 in one mode and either of those or a zero of the same sign in the other,
 *       whichever way a mode decides that a result within one rounding of 2^-126 is tiny. The explicit test is therefore
 *       |a| <= 2^-126, not <: it makes all of them that zero. With < an a of 2^-126 in one mode and 0 in the other would meet
 *       a b that limit = +INFINITY leaves unbounded, and h could be anything against 0. An exact product of 2^-126 or more is
 *       no denormal in either mode.
 *   b.  Two normal numbers that cancel leave zero or a multiple of 2^-149: the same, and a denormal one becomes a zero of its sign
 *       by the mode or by the explicit test. A denormal u with up_shift = 0 is that denormal in one mode, then flushed to a zero
 *       of u's sign, and 0 + 0 = +0 in the other: b can differ in the SIGN OF A ZERO, nothing else.
 *   h.  So a is the same in both modes and b is the same but for the sign of a zero; h = a * b is the same in both modes, or a
 *       zero of either sign, or a product of two equal normal operands that is a denormal (or within a rounding of 2^-126) in
 *       one mode and a zero in the other. The "input side" argument above covers all of these: any |x| <= 2^-126 enters the
 *       range like a zero of either sign -- a range of nothing larger fails the scale test and takes scale 1, -lo * inv and
 *       x * inv stay at or below 2^-126 * 2^60 and round to zero -- and quantizes to the zero point.
 *
 * Statuses: those of the plain setup of the same handle, in its order, with 2 * input_channels wherever the input's channel
 * count enters (the stride check, the input's byte span for the overlap and device checks, the host-pointer staging of the
 * plain form; the grouped form's size limits count quantized rows, still K rounded up to 64 bytes each). One check is added,
 * behind the alignment check and in front of the stride check: invalid_parameter for an alpha that is not a normal number in
 * [2^-6, 2^6], a limit that is NaN or neither in [2^-6, 2^6] nor +INFINITY, an up_shift that is NaN, infinite, denormal or
 * above 2^6 in magnitude. A refused setup leaves the previous one runnable, gated or not; a plain setup after a gated one, or
 * the reverse, replaces it. The scratch has the plain setup's size. Each of the two refuses the other's handles.
 *
 * Kernels. Only the first launch differs (hip/f32qd8gatedrows.hip; qnnp_gfx950_dynamic_rows_kernel names it), by K, the number
 * of positions, as above:
 *     f32_qd8_gated_rows_wave      K <= 1024       one wave per row; a lane reads 128 contiguous bytes for 16 positions
 *     f32_qd8_gated_rows_block     K <= 16384      one workgroup per row, the row read once, up to 64 h per lane in registers
 *     f32_qd8_gated_rows_twopass   K <= 32768      the row is read twice and h computed twice, to the same bits
 * each with _x4 behind its name where the input base or, with more than one row, the input stride is no multiple of 16 bytes.
 * No scratch memory. qnnp_gfx950_operator_kernel is unaffected.
 */
enum qnnp_status qnnp_gfx950_setup_fully_connected_nc_f32_qd8_gated(
    qnnp_operator_t fully_connected,     /* of any of the six plain creates */
    size_t batch_size,
    const float* input,                  /* [batch_size] rows of 2 * input_channels floats: {gate, up} per position */
    size_t input_stride,                 /* in elements, >= 2 * input_channels */
    float alpha,
    float limit,
    float up_shift,
    float* output,
    size_t output_stride);

enum qnnp_status qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_gated(
    qnnp_operator_t fully_connected,     /* of the grouped create */
    size_t batch_size,                   /* input rows */
    size_t assignments,                  /* A = groups per input row, 1 .. 8 */
    const float* input,                  /* [batch_size] rows of 2 * input_channels floats, device */
    size_t input_stride,                 /* in elements, >= 2 * input_channels */
    float alpha,
    float limit,
    float up_shift,
    const int32_t* group_ids,            /* [batch_size * A], device; read when the operator runs */
    float* output,                       /* [batch_size * A] rows of output_channels floats, device */
    size_t output_stride);

/*
 * A NORMALIZED input (residual add + RMSNorm) for every handle above with input_channels <= 16384. The gated setups are a
 * second layer's; these two are the FIRST layer's: in a pre-norm transformer block the router's logit FC, the first expert
 * layer and every dense QKV or MLP-up projection read rmsnorm(x + residual) * gamma. The row kernel computes that row h in
 * registers while it reads, so that h is never written as floats and the add, square, mean, rsqrt and multiply launches in
 * front of the operator disappear; where asked, it writes the sum x back as the next block's residual stream. No new create:
 * the first setup takes a handle of any of the six plain creates, the second a handle of the grouped create.
 *
 * Definition (bit-exact, no tolerance). All arithmetic is float32, every operation rounded once, nothing fused. Two flushes:
 *   flush(v)   = |v| <= 0x1p-126f ? copysignf(0, v) : v          behind a product
 *   flush_lt(v) = |v| <  0x1p-126f ? copysignf(0, v) : v          on a loaded element and behind a sum of two of them
 * With K = input_channels (K <= 16384), per row r:
 *   x[k]  = residual ? flush_lt(flush_lt(input[r][k]) + flush_lt(residual[r][k])) : input[r][k]          k < K
 *           if residual_out: residual_out[r][k] = x[k]                  the bits of x
 *   sq[k] = flush(x[k] * x[k]) for k < K;  +0 for K <= k < 16384
 *   piece sums, j = 0 .. 1023, over u = sq[16 j .. 16 j + 15]:
 *           u[i] = u[i] + u[i + 8] (i < 8);  then u[i] + u[i + 4] (i < 4);  then i + 2 (i < 2);  then u[0] + u[1];   s[j] = u[0]
 *   across pieces, for h = 512, 256, 128, 64, 32, 16, 8, 4, 2, 1 IN THIS ORDER:  s[j] = s[j] + s[j + h]  for j < h
 *   S  = s[0]
 *   m  = S / (float) K                       an IEEE division; (float) K is exact
 *   v  = m + epsilon
 *   r  = 1.0f / sqrtf(v)                     the correctly rounded square root, then an IEEE division
 *   t  = flush(x[k] * r);   h[r][k] = flush(t * gamma[k])
 * Everything after that is the first definition of this header with h[r] as the input row x[r]: the range, scale_r, zp_r, q,
 * and the product and the finish of the handle's weight format, unchanged. An rmsnorm run equals, bit for bit, the same
 * handle's plain run on a float tensor holding h.
 *
 * Why this order. Every sq is +0 or a positive normal number (or +inf, or NaN), and v + (+0) == v in every bit for those: the
 * tree over 1024 zero-padded pieces gives the bits of the tree over any smaller power-of-two count of pieces that covers the
 * row. So S is a function of x and K alone -- not of the kernel that ran, its load width or the batch --, and the tree maps
 * onto the piece layout of the row kernels (piece j = i * 256 + wave * 64 + lane): steps 512 and 256 pair a lane's own
 * pieces, 128 and 64 pair the waves of a workgroup, 32 to 1 are an xor butterfly inside a wave, in which both partners form
 * s[j] + s[j ^ h]: float addition is commutative in every bit but a NaN's payload.
 *
 * NaN and infinity. A NaN among the x makes S, r and every h NaN; the row definition quantizes NaN to the zero point and an
 * all-NaN row has scale 1: no payload reaches an output. Only residual_out shows a payload: it is that of the one NaN
 * operand of the sum where there is one (quieted), unspecified otherwise. An infinite x, or a finite row whose S overflows,
 * gives v = +inf, sqrtf(v) = +inf and r = +0: t is a zero of x's sign (NaN for the infinite x itself).
 *
 * No result depends on the denormal mode. epsilon is a normal number in [2^-40, 1] (checked); gamma is zero or normal with
 * magnitude at most 2^20 (a precondition, not checked: it lives in device memory). The steps, written out:
 *   x.  THIS STEP FAILED as first written, x = input + residual: a denormal operand counts as zero in one mode and as itself in
 *       the other, and a sum of two normal numbers that cancel can be a denormal; residual_out would show either. Hence the
 *       three flush_lt, which are not needed for h (steps t and h below absorb any |x| < 2^-126) but make residual_out the
 *       same bits in both modes. flush_lt of a loaded element: a denormal becomes the zero that the other mode reads. The sum
 *       of two numbers that are each zero or normal is exact whenever it is below 2^-125 in magnitude (both are multiples of
 *       2^-149), so it is a denormal only as an exact value, which both the mode and flush_lt turn into the same signed zero:
 *       < suffices, there is no rounding to straddle 2^-126. Without a residual x is the input's bits, denormals included.
 *   sq. x * x of a normal x with an exact value below 2^-126 is, rounded, a denormal or exactly 2^-126 in one mode and either
 *       of those or +0 in the other, whichever way a mode decides that a result within one rounding of 2^-126 is tiny; flush
 *       with <= makes all of them +0. A denormal x squares to less than 2^-252: +0 in either mode.
 *   S.  The sums run over +0 and positive normal numbers: nothing cancels, every partial sum is +0 or at least 2^-126.
 *   m.  S / K can be a denormal (K up to 2^14). An m below 2^-100, denormal or flushed, is absorbed by epsilon >= 2^-40, whose
 *       last place is at least 2^-63: v is the same. Any other m is normal.
 *   r.  v >= 2^-40 is normal or +inf; sqrtf(v) lies in [2^-20, 2^64] or is +inf; r lies in [2^-64, 2^20] or is +0.
 *   t.  A normal x times r: as step sq, <= makes a product within a rounding of 2^-126 a zero in either mode. A denormal x
 *       (no residual) gives |x * r| < 2^-126 * 2^20 = 2^-106 in one mode and a zero in the other.
 *   h.  t is zero, normal, or that mode-dependent value below 2^-106; gamma is zero or normal, at most 2^20. A product of two
 *       normal numbers is settled by <= as before. What remains is an h that is below 2^-86 in magnitude in one mode and a
 *       zero in the other. The "input side" argument of the first definition covers it with 2^-86 in the place of 2^-126:
 *       a row whose range passes the scale test has hi - lo >= 255 * 2^-60 > 2^-53, whose half last place, 2^-77, absorbs such
 *       an h at either end of the range; a range of nothing larger fails the test and takes scale 1; and h * inv is below
 *       2^-86 * 2^60 = 2^-26, which rounds to the zero point like a zero.
 *
 * Statuses: those of the plain setup of the same handle, in its order; K is the channel count of input, gamma and both
 * residual tensors. Added: unsupported_parameter for a handle with input_channels > 16384, answered from the handle alone,
 * directly behind the check of the handle's kind and before batch_size or any pointer is looked at (there is no three-pass
 * regime: the norm runs over a model's hidden size, and the in-place residual update is safe because the row stays in
 * registers). invalid_parameter: a NULL gamma, or a residual_out without a residual (with the NULL tensors); gamma, residual or
 * residual_out not 4-byte aligned (with the alignment check); an epsilon that is not a normal number in [2^-40, 1] (behind the
 * alignment check and in front of the stride check, where the gated setups check their parameters); residual_stride < K
 * where a residual is given (with the stride check); an overlap (with the overlap check): output shares no byte with any
 * other tensor, residual_out shares none with input, gamma or group_ids, and residual_out is either residual itself, the
 * same base pointer (in place), or disjoint from it; a tensor -- input, output, gamma, residual, residual_out -- that is not
 * memory of the operator's device, in the plain form too (host memory included: nothing of these setups is staged).
 * batch_size == 0 succeeds and the run does nothing. A refused setup leaves the previous one runnable; a plain, gated or
 * rmsnorm setup replaces whichever came before. Each of the two refuses the other's handles. The scratch has the plain
 * setup's size. gamma, like group_ids, is read WHEN THE OPERATOR RUNS: overwriting it between runs or between replays of a
 * graph needs no new setup; so are input and residual, and residual_out is written by every run.
 *
 * Kernels. Only the first launch differs (hip/f32qd8rmsnormrows.hip; qnnp_gfx950_dynamic_rows_kernel names it):
 *     f32_qd8_rmsnorm_rows_wave     K <= 1024     one wave per row; loads, lane exchanges, stores: no LDS memory, no barrier
 *     f32_qd8_rmsnorm_rows_block    K <= 16384    one workgroup per row, the row read once and kept in registers as x
 * each with _x4 behind its name where a base of input, residual, residual_out or gamma or, with more than one row,
 * input_stride or residual_stride is no multiple of 16 bytes. Nothing at or past K is read or written in any float tensor.
 * No scratch memory. qnnp_gfx950_operator_kernel is unaffected.
 */
enum qnnp_status qnnp_gfx950_setup_fully_connected_nc_f32_qd8_rmsnorm(
    qnnp_operator_t fully_connected,     /* of any of the six plain creates, input_channels <= 16384 */
    size_t batch_size,
    const float* input,                  /* [batch_size] rows of input_channels floats, device */
    size_t input_stride,                 /* in elements */
    const float* gamma,                  /* [input_channels], device; read when the operator runs */
    float epsilon,                       /* a normal number in [2^-40, 1] */
    const float* residual,               /* rows of input_channels floats, device; or NULL */
    float* residual_out,                 /* rows of input_channels floats, device; NULL, or == residual (in place) */
    size_t residual_stride,              /* of both residual tensors, in elements */
    float* output,                       /* device */
    size_t output_stride);

enum qnnp_status qnnp_gfx950_setup_grouped_fully_connected_nc_f32_qd8_rmsnorm(
    qnnp_operator_t fully_connected,     /* of the grouped create, input_channels <= 16384 */
    size_t batch_size,                   /* input rows */
    size_t assignments,                  /* A = groups per input row, 1 .. 8 */
    const float* input,                  /* [batch_size] rows of input_channels floats, device */
    size_t input_stride,                 /* in elements */
    const float* gamma,                  /* [input_channels], device; read when the operator runs */
    float epsilon,
    const float* residual,
    float* residual_out,
    size_t residual_stride,
    const int32_t* group_ids,            /* [batch_size * A], device; read when the operator runs */
    float* output,                       /* [batch_size * A] rows of output_channels floats, device */
    size_t output_stride);

/* Name of the row kernel the operator's last run launched in front of the kernel qnnp_gfx950_operator_kernel names
 * (static string), or NULL: before the first run, or for a handle of another kind. */
const char* qnnp_gfx950_dynamic_rows_kernel(qnnp_operator_t fully_connected);

#ifdef __cplusplus
}
#endif
