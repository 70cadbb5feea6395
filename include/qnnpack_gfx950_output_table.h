/*
 * qnnpack_gfx950_output_table.h -- a byte table folded behind a convolution of libqnnpack_gfx950.so. Part of the
 * interface of qnnpack_gfx950.h, which includes it, beside the residual add folded into a convolution; a header of its
 * own as qnnpack_gfx950_squeeze_excite.h is.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Output table (no reference counterpart): an activation that is not a clamp -- hardswish, swish, sigmoid, leaky ReLU,
 * any 256-byte table -- behind a convolution, without the table operator's launch and its pass over the tensor. ReLU and
 * ReLU6 are the convolution's output_min / output_max already; this is the same for every other activation.
 *
 * Definition. From the attach on, qnnp_run_operator(convolution) writes table[b] for every output byte b the convolution
 * would have written: byte for byte what the convolution followed by
 *     qnnp_gfx950_setup_lut_nc_x8(table, pixels, output, output_pixel_stride, output, output_pixel_stride)
 * in place gives (pixels = batch * output height * output width). The lookup comes after the requantization and its
 * clamp. Bytes between strided pixels are not written.
 *
 * `convolution`: a convolution, fully connected or depthwise operator, per-tensor or per-channel
 * (qnnpack_gfx950_perchannel.h); not a deconvolution, not a fused operator. `table`: any table operator
 * (qnnp_create_sigmoid_nc_q8, qnnp_create_leaky_relu_nc_q8, qnnp_gfx950_create_hardswish_nc_q8,
 * qnnp_gfx950_create_hardsigmoid_nc_q8, qnnp_gfx950_create_lut_nc_x8) whose channel count equals the convolution's output
 * channel count (groups * group_output_channels).
 *
 * Lifetime. The table names no tensor: attach it any time after create, with or without a valid setup; it stays attached
 * across later setups. The 256 bytes are copied into a device table the convolution owns (freed by
 * qnnp_delete_operator), so the table operator may be deleted afterwards. Attaching again replaces the table;
 * table == NULL detaches it and the operator writes its plain bytes again.
 *
 * Folding. The attachment never changes which kernel runs the convolution; it selects that kernel's table flavour where
 * one exists (the pointwise streaming kernels and the 3x3 / 5x5 depthwise column walks: DESIGN.md section 4.6k). Everywhere
 * else the table kernel is launched in place on the output behind the convolution. Both forms record into a hipGraph
 * capture, run in async mode and work with host endpoints. qnnp_gfx950_operator_table_folded answers, after a run:
 * 1 = epilogue, 0 = separate launch, -1 = nothing attached. qnnp_gfx950_operator_kernel keeps answering the convolution
 * kernel's name.
 *
 * Attach, in this order: uninitialized; invalid_parameter for a NULL `convolution`; invalid_parameter for an operator of
 * the wrong kind on either side, a channel mismatch, operators on different devices, or a call inside a graph capture;
 * unsupported_parameter when a residual add is attached to `convolution` (the order of add and table would be a second
 * definition); out_of_memory for the device table. A refused attach leaves the previous state as it was.
 *
 * Combinations are refused with unsupported_parameter, never silently dropped: qnnp_gfx950_attach_residual_add on an
 * operator that has a table, and qnnp_gfx950_create_fused_block / qnnp_gfx950_create_squeeze_excite with a member that has
 * one (those operators borrow the members' parameters and would lose the table). */
enum qnnp_status qnnp_gfx950_attach_output_table(qnnp_operator_t convolution, qnnp_operator_t table);
int qnnp_gfx950_operator_table_folded(qnnp_operator_t op);

#ifdef __cplusplus
}
#endif
