/*
 * qnnpack_gfx950_perchannel.h -- convolution and fully connected operators whose weights carry ONE SCALE PER OUTPUT
 * CHANNEL: PyTorch's default weight observer for convolution and linear, TFLite's int8 convolution, and what makes
 * depthwise filter banks (MobileNet, EfficientNet-lite) quantizable at all. No reference counterpart.
 *
 * Definition (bit-exact, no tolerance). For output channel c, counted over all groups
 * (c = g * group_output_channels + oc), with the accumulator
 *   acc[c] = bias[c] + sum (a - input_zero_point) * (w - kernel_zero_point)
 * of the per-tensor operators:
 *   scale_c = (input_scale * kernel_scales[c]) / output_scale       float32, each operation rounded once, this order
 *   (multiplier_c, shift_c) from scale_c as qnnp_compute_conv_quantization_params forms them (a Q31 multiplier in
 *                                                                    [2^30, 2^31) and a right shift in [0, 31])
 *   y[c] = qnnp_q31_requantize(acc[c], multiplier_c, shift_c, output_zero_point, output_min, output_max)
 * With every kernel_scales[c] equal to s the result is byte for byte that of the per-tensor create with
 * kernel_scale = s.
 *
 * The kernel zero point stays ONE value per operator: symmetric per-channel int8 weights moved to uint8 (w + 128) have
 * zero point 128 in every channel, which is the PyTorch and the TFLite case. Per-channel kernel zero points are out of
 * scope. The output zero point and the clamp are per operator too. Deconvolution has no per-channel create.
 *
 * The two creates take the parameters of qnnp_create_convolution2d_nhwc_q8 and qnnp_create_fully_connected_nc_q8 in
 * their order, with `float kernel_scale` replaced by `const float* kernel_scales`: host memory, groups *
 * group_output_channels (output_channels) floats, read during the call and not kept. Everything else is the existing
 * interface: qnnp_setup_convolution2d_nhwc_q8, qnnp_setup_fully_connected_nc_q8, qnnp_run_operator,
 * qnnp_delete_operator, qnnp_gfx950_operator_kernel, hipGraph capture, host tensors staged through the device.
 *
 * Create answers, in the order of the per-tensor create:
 *   uninitialized;
 *   invalid_parameter        everything that is invalid_parameter there; kernel_scales == NULL; any kernel_scales[c] that
 *                            is not a finite (normal) number above zero;
 *   unsupported_parameter    any scale_c outside [2^-32, 1) -- the log names the first such channel -- and everything
 *                            that is unsupported_parameter there;
 *   out_of_memory.
 * A refused create writes no handle.
 *
 * Kernels (qnnp_gfx950_operator_kernel names the one that ran). Per-channel operators run on kernels of their own and
 * on nothing else:
 *   dense, grouped, 1x1, KxK, 3-channel and fully connected   q8_igemm_pc_mfma_128x32 / _128x64 / _128x128, with _c3 for
 *                                                              3-channel inputs: the generic implicit-GEMM kernel with
 *                                                              a per-channel epilogue (hip/q8igemm.hip)
 *   depthwise                                                  q8_dwconv_pc_w3s1 / _w3s2 / _w5s1 / _w5s2 (windows 3 or 5
 *                                                              wide, column stride 1 or 2, no column dilation) and
 *                                                              q8_dwconv_pc_any (hip/q8dwconv_pc.hip)
 * The specialised per-tensor kernels have no per-channel flavour yet.
 *
 * What does not combine with a per-channel operator is REFUSED with unsupported_parameter, never run per tensor:
 *   qnnp_gfx950_create_fused_block with a per-channel member;
 *   qnnp_gfx950_attach_residual_add on a per-channel convolution (run the add operator behind it);
 *   at run, a forced "gemm_kernel" code other than 0 and 1, or a forced "dwconv_kernel" code other than 0
 *   (include/qnnpack_gfx950_test.h: a forced kernel that does not take the operator fails the run).
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

enum qnnp_status qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t kernel_height,
    uint32_t kernel_width,
    uint32_t subsampling_height,
    uint32_t subsampling_width,
    uint32_t dilation_height,
    uint32_t dilation_width,
    uint32_t groups,
    size_t group_input_channels,
    size_t group_output_channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t kernel_zero_point,
    const float* kernel_scales,
    const uint8_t* kernel,
    const int32_t* bias,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* convolution);

enum qnnp_status qnnp_gfx950_create_fully_connected_nc_q8_per_channel(
    size_t input_channels,
    size_t output_channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t kernel_zero_point,
    const float* kernel_scales,
    const uint8_t* kernel,
    const int32_t* bias,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* fully_connected);

#ifdef __cplusplus
}
#endif
