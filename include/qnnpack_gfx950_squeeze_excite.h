/*
 * qnnpack_gfx950_squeeze_excite.h -- the fused squeeze-and-excite block of libqnnpack_gfx950.so. Part of the interface of
 * qnnpack_gfx950.h, which includes it, beside the fused inverted-residual block; a header of its own as
 * qnnpack_gfx950_float.h and qnnpack_gfx950_perchannel.h are.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fused squeeze-and-excite block (no reference counterpart), the block of MobileNetV3, EfficientNet and RegNet-Y:
 *     global average pooling -> fully connected C -> S (its ReLU is its output_min) -> fully connected S -> C ->
 *     table gate (sigmoid, hardsigmoid, ...) -> x * s, the gate broadcast over the pixels of its image
 * as ONE operator of two kernel launches instead of five: the squeeze path -- pooling, both fully connected layers and
 * the gate -- is one kernel that keeps its rows on the chip (kernel q8_se_gate_pool; for large images the pooling stays a
 * launch of its own in front of q8_se_gate), followed by the multiply kernel. It pays for blocks of up to about 400 000
 * weights per fully connected layer (MobileNetV3's, EfficientNet's); beyond that the five stand-alone operators are
 * faster, because one workgroup per image reads both weight images whole.
 *
 * Definition. The operator is built FROM five stand-alone operators, and for `batch_size` images of `pixels` pixels of C
 * bytes its output y is, byte for byte, what these five setups give when run in order on private intermediates p, h, e, s:
 *     qnnp_setup_global_average_pooling_nwc_q8(pool, batch_size, pixels, x, input_pixel_stride, p, C)
 *     qnnp_setup_fully_connected_nc_q8(fc1, batch_size, p, C, h, S)
 *     qnnp_setup_fully_connected_nc_q8(fc2, batch_size, h, S, e, C)
 *     qnnp_gfx950_setup_lut_nc_x8(gate, batch_size, e, C, s, C)
 *     qnnp_gfx950_setup_multiply_nc_q8(multiply, batch_size, pixels, x, input_pixel_stride, s, C, y, output_pixel_stride)
 * No consistency of scales or zero points between the members is checked, exactly as that chain checks none.
 *
 * Members: `pool` a global average pooling operator; `fc1` and `fc2` fully connected operators or 1x1 convolutions
 * (stride 1, no padding, one group); `gate` any table operator (qnnp_create_sigmoid_nc_q8, qnnp_create_leaky_relu_nc_q8,
 * qnnp_gfx950_create_hardsigmoid_nc_q8, qnnp_gfx950_create_hardswish_nc_q8, qnnp_gfx950_create_lut_nc_x8); `multiply` a
 * multiply operator. The fused operator BORROWS their device images -- the two weight images and folded biases, the
 * gate's table -- and their quantization parameters: the members must outlive it, are not changed by it and stay usable
 * on their own. It owns one grow-only device scratch for the gate rows.
 *
 * Create, in this order: uninitialized; invalid_parameter for a NULL member or a NULL result pointer, a member of the
 * wrong kind, a channel chain that does not close (pool channels == fc1 inputs == fc2 outputs == gate channels ==
 * multiply channels == C and fc1 outputs == fc2 inputs == S), members on different devices, a create inside a graph
 * capture; unsupported_parameter for a fully connected member with per-channel weight scales
 * (qnnpack_gfx950_perchannel.h; the fused inverted-residual block refuses them too) and for C or S above
 * QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS -- keep using the stand-alone operators for such a block.
 * Setup: batch_size == 0 succeeds and run then does nothing. Then, in this order: invalid_parameter for pixels == 0, a NULL
 * tensor, a pixel stride below C; unsupported_parameter for a pixel count the pooling setup refuses (pixels > INT32_MAX /
 * 255, or input_scale / (output_scale * pixels) outside [2^-32, 256)) and for batch_size * pixels >= 2^31;
 * invalid_parameter for input and output byte spans that share a byte other than exactly in place (output == input with
 * equal strides, as multiply allows on `a`) and for memory of another GPU; out_of_memory for the scratch. Inside a graph
 * capture setup answers invalid_parameter. A setup refused by these checks leaves the previous valid setup runnable.
 * Tensors are host or device memory; the operator records into a hipGraph capture with device pointers, runs in async
 * mode, and hands qnnp_gfx950_operator_set_streaming_stores on to its multiply launch. qnnp_gfx950_operator_kernel
 * answers the gate kernel's name. Run and delete are qnnp_run_operator / qnnp_delete_operator. */
#define QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS 4096

enum qnnp_status qnnp_gfx950_create_squeeze_excite(
    qnnp_operator_t pool, qnnp_operator_t fc1, qnnp_operator_t fc2, qnnp_operator_t gate, qnnp_operator_t multiply,
    qnnp_operator_t* squeeze_excite);
enum qnnp_status qnnp_gfx950_setup_squeeze_excite(
    qnnp_operator_t squeeze_excite, size_t batch_size, size_t pixels,
    const uint8_t* input, size_t input_pixel_stride, uint8_t* output, size_t output_pixel_stride);

#ifdef __cplusplus
}
#endif
