/*
 * squeeze-excite.c -- qnnp_gfx950_create_squeeze_excite / qnnp_gfx950_setup_squeeze_excite
 * (include/qnnpack_gfx950_squeeze_excite.h): a squeeze-and-excite block -- global average pooling -> fully connected C -> S
 * -> fully connected S -> C -> table gate -> x * s -- as ONE operator of two launches instead of five. No reference
 * counterpart: the reference has none of the block's last two operators.
 *
 * Like the fused inverted-residual block (fused-block.c) the operator is BUILT FROM the stand-alone operators, created
 * through the regular API: it borrows their device images (the two standard weight images and bias pair tables, the
 * gate's 256-byte table) and their parameters, so its result is the bytes those five produce in sequence by construction
 * of the arithmetic. The members must outlive the fused operator; nothing of theirs is changed, so they stay usable on
 * their own.
 *
 * The squeeze path is the kernel of hip/q8segate.hip; it writes the gate rows s [batch][C] into a grow-only device
 * scratch the operator owns (as resize-bilinear.c owns its tables; freed by qnnp_delete_operator), and the multiply
 * member's own launch (hip/q8mul.hip) reads them. Flavour 2 runs the pooling as the pooling operator's own launch into a
 * second part of the scratch, p [batch][C], in front of the gate kernel.
 *
 * Setup follows lut.c / multiply.c / resize-bilinear.c: every check comes before the operator changes, so a refused setup
 * leaves the previous one runnable. What can still fail afterwards is an allocation (the scratch, the staging of host
 * tensors); the operator is then not runnable until the next successful setup.
 *
 * Not part of the seam library (oracle/Makefile).
 */
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>
#include <qnnpack_gfx950_squeeze_excite.h>

#include "gavgpool-params.h"
#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "state.h"

_Static_assert(QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS == QNNP_HIP_SE_MAX_CHANNELS,
    "the header states the limit of the kernel");

/* The automatic rule, from the tables in profiles/squeeze_excite/README.md. The pooling runs
 * inside the gate kernel: measured faster than the pooling launch in front for every image of up to 1024 channels, 3.2 MB
 * images included -- there the pooling launch gives an image ONE workgroup of 256 lanes (q8pointwise.hip), the gate kernel
 * one of 1024. Above 1024 channels the pooling launch deals an image over several workgroups, while a lane of the gate
 * kernel walks all the pixels of its channels alone; the launch in front then wins from some pixel count on: measured
 * slower at 49 pixels (1280, 1536, 3840 channels; a tie at 4096), faster at 196 (1152 channels), 784 and 3136 (2048
 * channels). The bound is the smallest measured win; between 49 and 196 pixels nothing was measured. */
#define QNNP_SE_POOL_IN_FRONT_MIN_CHANNELS ((size_t) 1024)
#define QNNP_SE_POOL_IN_FRONT_MIN_PIXELS ((size_t) 196)

static int is_fully_connected(const struct qnnp_operator* op)
{
  return op->ukernel_type == qnnp_ukernel_type_gemm && !op->transposed && op->groups == 1 &&
      op->kernel_height == 1 && op->kernel_width == 1 && op->kc_slot == op->group_input_channels;
}

static struct qnnp_hip_se_fc se_fc(const struct qnnp_operator* fc)
{
  return (struct qnnp_hip_se_fc) {
    .w = (const int8_t*) fc->d_weights,
    .bias2 = fc->d_bias,              /* the first n_pad entries of the pair table (bias-pair.h) */
    .k_pad = fc->k_pad,
    .n_pad = fc->n_pad,
    .row_coeff = 128 - (int32_t) fc->kernel_zero_point,
    .rq = fc->requant,
  };
}

/* the gate kernel (behind a pooling launch in flavour 2), then the multiply member's launch over the gate rows */
static int launch_squeeze_excite(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  const struct qnnp_operator* mul = op->se_multiply;
  const uint32_t channels = (uint32_t) op->channels;
  uint8_t* gate = (uint8_t*) op->d_se_scratch;
  const uint8_t* gate_input = (const uint8_t*) input;
  const char* name = NULL;
  if (op->se_flavour == 2) {
    uint8_t* pooled = gate + op->se_pooled_offset;
    const struct qnnp_hip_gavgpool_args pool_args = {
      .input = (const uint8_t*) input,
      .output = pooled,
      .batch = op->batch_size,
      .width = op->input_width,
      .channels = channels,
      .input_stride = op->input_pixel_stride,
      .output_stride = channels,
      .params = op->avgpool_params,
    };
    const int rc = qnnp_hip_gavgpool_run(&pool_args, &name);
    if (rc != QNNP_HIP_OK) {
      return rc;
    }
    gate_input = pooled;
  }
  const struct qnnp_hip_se_gate_args gate_args = {
    .input = gate_input,
    .gate = gate,
    .batch = (uint32_t) op->batch_size,
    .pixels = (uint32_t) op->input_width,
    .channels = channels,
    .squeeze = (uint32_t) op->se_fc1->group_output_channels,
    .input_stride = op->input_pixel_stride,
    .pool = op->se_flavour != 2,
    .pool_params = op->avgpool_params,
    .fc1 = se_fc(op->se_fc1),
    .fc2 = se_fc(op->se_fc2),
    .table = (const uint8_t*) op->se_gate->d_weights,
  };
  int rc = qnnp_hip_se_gate_run(&gate_args, &op->kernel_name);
  if (rc != QNNP_HIP_OK) {
    return rc;
  }
  const struct qnnp_hip_mul_args mul_args = {
    .a = (const uint8_t*) input,
    .b = gate,
    .product = (uint8_t*) output,
    .b_rows = (uint32_t) op->batch_size,
    .a_rows_per_b_row = (uint32_t) op->input_width,
    .channels = channels,
    .a_stride = op->input_pixel_stride,
    .b_stride = channels,
    .product_stride = op->output_pixel_stride,
    .a_zero_point = (int32_t) (uint32_t) mul->mul_a_zero_point,
    .b_zero_point = (int32_t) (uint32_t) mul->mul_b_zero_point,
    .rq = mul->requant,
    .streaming_mode = op->streaming_mode,
  };
  return qnnp_hip_mul_run(&mul_args, &name);
}

/* what create checks before it enters the members' device: NULL handles, kinds, the channel chain, one device */
static enum qnnp_status validate_members(
    qnnp_operator_t pool, qnnp_operator_t fc1, qnnp_operator_t fc2, qnnp_operator_t gate, qnnp_operator_t multiply,
    qnnp_operator_t* squeeze_excite)
{
  if (pool == NULL || fc1 == NULL || fc2 == NULL || gate == NULL || multiply == NULL || squeeze_excite == NULL) {
    qnnp_log_error("cannot create squeeze-and-excite operator: NULL member or NULL result pointer");
    return qnnp_status_invalid_parameter;
  }
  if (pool->ukernel_type != qnnp_ukernel_type_global_average_pooling || !is_fully_connected(fc1) ||
      !is_fully_connected(fc2) || gate->ukernel_type != qnnp_ukernel_type_lut ||
      multiply->ukernel_type != qnnp_ukernel_type_multiply) {
    qnnp_log_error("cannot create squeeze-and-excite operator: the members are not a global average pooling, two fully "
        "connected (or 1x1 convolution), a table and a multiply operator");
    return qnnp_status_invalid_parameter;
  }
  const size_t channels = pool->channels, squeeze = fc1->group_output_channels;
  if (fc1->group_input_channels != channels || fc2->group_output_channels != channels || gate->channels != channels ||
      multiply->channels != channels || fc2->group_input_channels != squeeze) {
    qnnp_log_error("cannot create squeeze-and-excite operator: the members' channel counts do not chain");
    return qnnp_status_invalid_parameter;
  }
  if (fc1->device != pool->device || fc2->device != pool->device || gate->device != pool->device ||
      multiply->device != pool->device) {
    qnnp_log_error("cannot create squeeze-and-excite operator: the members live on different devices");
    return qnnp_status_invalid_parameter;
  }
  return qnnp_status_success;
}

/* inside the members' device */
static enum qnnp_status create_squeeze_excite(
    qnnp_operator_t pool, qnnp_operator_t fc1, qnnp_operator_t fc2, qnnp_operator_t gate, qnnp_operator_t multiply,
    qnnp_operator_t* squeeze_excite)
{
  /* the gate kernel requantizes per tensor (qnnpack_gfx950_perchannel.h), as the fused block's kernels do */
  if (fc1->per_channel || fc2->per_channel) {
    qnnp_log_error("cannot create squeeze-and-excite operator: a fully connected member has per-channel weight scales");
    return qnnp_status_unsupported_parameter;
  }
  /* the gate kernel borrows the members' parameters and would lose an attached output table (output-table.c) */
  if (fc1->d_output_table != NULL || fc2->d_output_table != NULL) {
    qnnp_log_error("cannot create squeeze-and-excite operator: a fully connected member has an output table attached");
    return qnnp_status_unsupported_parameter;
  }
  if (pool->channels > QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS ||
      fc1->group_output_channels > QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS) {
    qnnp_log_error("cannot create squeeze-and-excite operator with %zu channels squeezed to %zu: the gate kernel takes %u "
        "of each at most", pool->channels, fc1->group_output_channels, (unsigned) QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS);
    return qnnp_status_unsupported_parameter;
  }
  qnnp_operator_t op = qnnp_allocate_operator(qnnp_ukernel_type_squeeze_excite, launch_squeeze_excite);
  if (op == NULL) {
    return qnnp_status_out_of_memory;
  }
  op->device = pool->device;   /* not the calling thread's: it borrows their device images */
  op->se_pool = pool;
  op->se_fc1 = fc1;
  op->se_fc2 = fc2;
  op->se_gate = gate;
  op->se_multiply = multiply;
  op->channels = pool->channels;
  *squeeze_excite = op;
  return qnnp_status_success;
}

static enum qnnp_status setup_squeeze_excite(
    qnnp_operator_t op, size_t batch_size, size_t pixels, const uint8_t* input, size_t input_stride, uint8_t* output,
    size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_squeeze_excite) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (pixels == 0) {
    qnnp_log_error("cannot set up squeeze-and-excite operator with %zu pixels: the pixel count may not be zero", pixels);
    return qnnp_status_invalid_parameter;
  }
  if (input == NULL || output == NULL || input_stride < channels || output_stride < channels) {
    qnnp_log_error("cannot set up squeeze-and-excite operator: NULL tensor or pixel stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  /* the pooling member's range for this pixel count, and its parameters (gavgpool-params.h) */
  struct qnnp_hip_avgpool_params pool_params;
  if (!qnnp_gavgpool_params_for_width(op->se_pool, pixels, &pool_params)) {
    qnnp_log_error("cannot set up squeeze-and-excite operator with %zu pixels: outside the pooling's supported range", pixels);
    return qnnp_status_unsupported_parameter;
  }
  /* (pixels is INT32_MAX / 255 at most by now; the batch is checked first, so the product cannot wrap) */
  if (batch_size > (size_t) INT32_MAX || (uint64_t) batch_size * (uint64_t) pixels > (uint64_t) INT32_MAX) {
    qnnp_log_error("cannot set up squeeze-and-excite operator with batch %zu of %zu pixels: outside the device kernels' "
        "index range", batch_size, pixels);
    return qnnp_status_unsupported_parameter;
  }
  const size_t rows = batch_size * pixels;
  const size_t input_span = (rows - 1) * input_stride + channels;
  const size_t output_span = (rows - 1) * output_stride + channels;
  /* the gate is complete before the multiply starts, and a lane of the multiply reads its own piece of x before it
   * writes that piece of y: y may BE x, as multiply allows on `a` */
  const int in_place = (const void*) output == (const void*) input && output_stride == input_stride;
  if (!in_place && qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("cannot set up squeeze-and-excite operator: the output overlaps the input without being that tensor");
    return qnnp_status_invalid_parameter;
  }
  if (qnnp_hip_is_device_pointer(input) < 0 || qnnp_hip_is_device_pointer(output) < 0) {
    qnnp_log_error("cannot set up squeeze-and-excite operator: a tensor lives on a different device than the operator");
    return qnnp_status_invalid_parameter;
  }
  uint32_t flavour = (uint32_t) qnnp_state.opt_se_kernel;
  if (flavour == 0) {
    flavour = channels > QNNP_SE_POOL_IN_FRONT_MIN_CHANNELS && pixels >= QNNP_SE_POOL_IN_FRONT_MIN_PIXELS ? 2 : 1;
  }
  /* s [batch][C]; flavour 2: then p [batch][C], on a 256-byte boundary so that the pooling kernel's dword stores apply */
  const size_t gate_bytes = batch_size * channels;
  const size_t pooled_offset = (gate_bytes + 255) & ~(size_t) 255;
  const size_t scratch_bytes = flavour == 2 ? pooled_offset + gate_bytes : gate_bytes;

  op->setup_valid = 0;   /* from here on the operator changes: until every allocation below has succeeded */
  if (op->se_scratch_capacity < scratch_bytes) {
    qnnp_hip_free(op->d_se_scratch);
    op->se_scratch_capacity = 0;
    op->d_se_scratch = qnnp_hip_alloc(scratch_bytes);
    if (op->d_se_scratch == NULL) {
      qnnp_log_error("failed to allocate %zu bytes of device scratch for the squeeze-and-excite gate", scratch_bytes);
      return qnnp_status_out_of_memory;
    }
    op->se_scratch_capacity = scratch_bytes;
  }
  op->se_flavour = flavour;
  op->se_pooled_offset = pooled_offset;
  op->avgpool_params = pool_params;
  op->batch_size = batch_size;
  op->input_width = pixels;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->input_span = input_span;
  op->output_span = output_span;
  return qnnp_bind_tensors(op, "qnnp_gfx950_setup_squeeze_excite");
}

/* ---- public entry points: the implementations above inside the device guards of lifecycle.h ---- */

enum qnnp_status qnnp_gfx950_create_squeeze_excite(
    qnnp_operator_t pool, qnnp_operator_t fc1, qnnp_operator_t fc2, qnnp_operator_t gate, qnnp_operator_t multiply,
    qnnp_operator_t* squeeze_excite)
{
  enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_squeeze_excite");
  if (status != qnnp_status_success) {
    return status;
  }
  status = validate_members(pool, fc1, fc2, gate, multiply, squeeze_excite);
  if (status != qnnp_status_success) {
    return status;
  }
  /* on THEIR device, not on whichever one the calling thread has selected (as fused-block.c) */
  int token;
  status = qnnp_enter_for_update(pool->device, qnnp_status_invalid_parameter, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_create(token, create_squeeze_excite(pool, fc1, fc2, gate, multiply, squeeze_excite));
}

enum qnnp_status qnnp_gfx950_setup_squeeze_excite(
    qnnp_operator_t squeeze_excite, size_t batch_size, size_t pixels,
    const uint8_t* input, size_t input_pixel_stride, uint8_t* output, size_t output_pixel_stride)
{
  int token;
  const enum qnnp_status status = qnnp_enter_setup("qnnp_gfx950_setup_squeeze_excite", squeeze_excite, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(squeeze_excite, token,
      setup_squeeze_excite(squeeze_excite, batch_size, pixels, input, input_pixel_stride, output, output_pixel_stride));
}
