/*
 * moe.c -- the two ends of a mixture-of-experts layer (include/qnnpack_gfx950_moe.h has the arithmetic and the statuses):
 *   qnnp_gfx950_create_topk_router_nc_f32 / qnnp_gfx950_setup_topk_router_nc_f32          router logits -> the group_ids
 *       the grouped operator of dynamic-fully-connected.c reads, and the routing weights (hip/f32topk.hip)
 *   qnnp_gfx950_create_weighted_combine_nc_f32 / qnnp_gfx950_setup_weighted_combine_nc_f32   the grouped operator's
 *       batch_size * A rows -> one row per token (hip/f32combine.hip)
 *
 * No reference counterpart. Neither operator owns device memory: a create validates and remembers its sizes, a setup
 * follows the grouped setup of dynamic-fully-connected.c -- validation in the documented order, every check before the
 * operator changes, device memory only -- and the run is one launch, reached through op->launch, so it records into a
 * graph capture like any other. In both, op->input and op->output are the tensors a run reads first and writes: the logits
 * and the ids of the router, the expert rows and the token rows of the combine.
 *
 * Not part of the seam library (oracle/Makefile).
 */
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950_moe.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "state.h"

#define QNNP_MOE_MAX_GROUPS ((size_t) 1024)
#define QNNP_MOE_MAX_ASSIGNMENTS ((size_t) 8)
#define QNNP_MOE_MAX_ROWS ((size_t) 1 << 20)              /* exclusive: the grouped operator's limit on its output rows */
#define QNNP_MOE_MAX_CHANNELS ((size_t) 1 << 24)          /* exclusive */

static int launch_topk_router(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  const struct qnnp_hip_topk_router_args args = {
    .logits = (const float*) input,
    .group_ids = (int32_t*) output,
    .weights = (float*) op->moe_weights,
    .logits_stride = op->input_pixel_stride,
    .tokens = (uint32_t) op->batch_size,
    .groups = op->moe_groups,
    .assignments = op->moe_assignments,
    .first_group = op->moe_first_group,
  };
  return qnnp_hip_topk_router_run(&args, &op->kernel_name);
}

static int launch_weighted_combine(struct qnnp_operator* op, const void* input, const void* input2, void* output)
{
  (void) input2;
  const struct qnnp_hip_weighted_combine_args args = {
    .input = (const float*) input,
    .weights = (const float*) op->moe_weights,
    .group_ids = op->moe_group_ids,
    .output = (float*) output,
    .input_stride = op->input_pixel_stride,
    .output_stride = op->output_pixel_stride,
    .tokens = (uint32_t) op->batch_size,
    .assignments = op->moe_assignments,
    .groups = op->moe_groups,
    .channels = (uint32_t) op->channels,
  };
  return qnnp_hip_weighted_combine_run(&args, &op->kernel_name);
}

/* both creates behind their checks: enter the device, allocate, remember the sizes */
static enum qnnp_status create_moe_operator(
    enum qnnp_ukernel_type type, int (*launch)(struct qnnp_operator*, const void*, const void*, void*), size_t channels,
    size_t groups, size_t assignments, uint32_t first_group, qnnp_operator_t* handle)
{
  int token;
  const enum qnnp_status status = qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  qnnp_operator_t op = qnnp_allocate_operator(type, launch);
  if (op == NULL) {
    return qnnp_leave_create(token, qnnp_status_out_of_memory);
  }
  op->channels = channels;          /* of the output: what operator-run.c compares the output stride with */
  op->moe_groups = (uint32_t) groups;
  op->moe_assignments = (uint32_t) assignments;
  op->moe_first_group = first_group;
  *handle = op;
  return qnnp_leave_create(token, qnnp_status_success);
}

enum qnnp_status qnnp_gfx950_create_topk_router_nc_f32(
    size_t groups,
    size_t assignments,
    uint32_t first_group,
    uint32_t flags,
    qnnp_operator_t* router)
{
  (void) flags;
  const enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_topk_router_nc_f32");
  if (status != qnnp_status_success) {
    return status;
  }
  if (groups == 0 || assignments == 0 || assignments > groups) {
    qnnp_log_error("cannot create top-k router with %zu groups and %zu assignments: neither may be zero and a token cannot "
        "be assigned to more groups than there are", groups, assignments);
    return qnnp_status_invalid_parameter;
  }
  if (groups > QNNP_MOE_MAX_GROUPS || assignments > QNNP_MOE_MAX_ASSIGNMENTS || first_group > (uint32_t) INT32_MAX) {
    qnnp_log_error("cannot create top-k router with %zu groups, %zu assignments and first group %u: at most %zu groups, at "
        "most %zu assignments and a first group below 2^31", groups, assignments, (unsigned) first_group,
        QNNP_MOE_MAX_GROUPS, QNNP_MOE_MAX_ASSIGNMENTS);
    return qnnp_status_unsupported_parameter;
  }
  return create_moe_operator(qnnp_ukernel_type_topk_router, launch_topk_router, assignments, groups, assignments,
      first_group, router);
}

enum qnnp_status qnnp_gfx950_create_weighted_combine_nc_f32(
    size_t channels,
    size_t assignments,
    size_t groups,
    uint32_t flags,
    qnnp_operator_t* combine)
{
  (void) flags;
  const enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_create_weighted_combine_nc_f32");
  if (status != qnnp_status_success) {
    return status;
  }
  if (channels == 0 || assignments == 0 || groups == 0) {
    qnnp_log_error("cannot create weighted combine with %zu channels, %zu assignments and %zu groups: none may be zero",
        channels, assignments, groups);
    return qnnp_status_invalid_parameter;
  }
  if (assignments > QNNP_MOE_MAX_ASSIGNMENTS || groups > QNNP_MOE_MAX_GROUPS || channels >= QNNP_MOE_MAX_CHANNELS) {
    qnnp_log_error("cannot create weighted combine with %zu channels, %zu assignments and %zu groups: fewer than %zu "
        "channels, at most %zu assignments and at most %zu groups", channels, assignments, groups, QNNP_MOE_MAX_CHANNELS,
        QNNP_MOE_MAX_ASSIGNMENTS, QNNP_MOE_MAX_GROUPS);
    return qnnp_status_unsupported_parameter;
  }
  return create_moe_operator(qnnp_ukernel_type_weighted_combine, launch_weighted_combine, channels, groups, assignments, 0,
      combine);
}

/* the limit on batch_size * A, from the sizes alone and before their product is formed */
static int too_many_rows(size_t batch_size, size_t assignments)
{
  return batch_size >= QNNP_MOE_MAX_ROWS || batch_size * assignments >= QNNP_MOE_MAX_ROWS;
}

static enum qnnp_status setup_topk_router(
    const char* function, qnnp_operator_t op, size_t batch_size, const float* logits, size_t logits_stride,
    int32_t* group_ids, float* weights)
{
  if (op->ukernel_type != qnnp_ukernel_type_topk_router) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t groups = op->moe_groups, assignments = op->moe_assignments;
  if (logits == NULL || group_ids == NULL || weights == NULL) {
    qnnp_log_error("cannot set up top-k router: NULL tensor");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) logits % sizeof(float) != 0 || (uintptr_t) group_ids % sizeof(int32_t) != 0 ||
      (uintptr_t) weights % sizeof(float) != 0) {
    qnnp_log_error("cannot set up top-k router: a tensor is not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (logits_stride < groups) {
    qnnp_log_error("cannot set up top-k router: row stride %zu smaller than the %zu groups", logits_stride, groups);
    return qnnp_status_invalid_parameter;
  }
  if (too_many_rows(batch_size, assignments)) {
    qnnp_log_error("cannot set up top-k router with batch %zu and %zu assignments: fewer than %zu assignments in all",
        batch_size, assignments, QNNP_MOE_MAX_ROWS);
    return qnnp_status_unsupported_parameter;
  }
  const size_t logits_span = ((batch_size - 1) * logits_stride + groups) * sizeof(float);
  const size_t ids_span = batch_size * assignments * sizeof(int32_t);
  const size_t weights_span = batch_size * assignments * sizeof(float);
  if (qnnp_spans_overlap(logits, logits_span, group_ids, ids_span) || qnnp_spans_overlap(logits, logits_span, weights, weights_span) ||
      qnnp_spans_overlap(group_ids, ids_span, weights, weights_span)) {
    qnnp_log_error("cannot set up top-k router: two of the logits, the group ids and the weights overlap");
    return qnnp_status_invalid_parameter;
  }
  /* all three in device memory: the grouped operator reads the ids there */
  if (qnnp_hip_is_device_pointer(logits) != 1 || qnnp_hip_is_device_pointer(group_ids) != 1 ||
      qnnp_hip_is_device_pointer(weights) != 1) {
    qnnp_log_error("cannot set up top-k router: the logits, the group ids and the weights have to be memory of the "
        "operator's device");
    return qnnp_status_invalid_parameter;
  }

  op->setup_valid = 0;
  op->batch_size = batch_size;
  op->input = logits;
  op->input_pixel_stride = logits_stride;
  op->output = group_ids;
  op->output_pixel_stride = assignments;
  op->moe_weights = weights;
  op->input_span = logits_span;
  op->output_span = ids_span;
  return qnnp_bind_tensors(op, function);
}

enum qnnp_status qnnp_gfx950_setup_topk_router_nc_f32(
    qnnp_operator_t router,
    size_t batch_size,
    const float* logits,
    size_t logits_stride,
    int32_t* group_ids,
    float* weights)
{
  const char* function = "qnnp_gfx950_setup_topk_router_nc_f32";
  int token;
  const enum qnnp_status status = qnnp_enter_setup(function, router, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(router, token, setup_topk_router(function, router, batch_size, logits, logits_stride, group_ids,
      weights));
}

static enum qnnp_status setup_weighted_combine(
    const char* function, qnnp_operator_t op, size_t batch_size, const float* input, size_t input_stride,
    const float* weights, const int32_t* group_ids, float* output, size_t output_stride)
{
  if (op->ukernel_type != qnnp_ukernel_type_weighted_combine) {
    return qnnp_status_invalid_parameter;
  }
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels, assignments = op->moe_assignments;
  if (input == NULL || weights == NULL || group_ids == NULL || output == NULL) {
    qnnp_log_error("cannot set up weighted combine: NULL tensor, weights or group ids");
    return qnnp_status_invalid_parameter;
  }
  if ((uintptr_t) input % sizeof(float) != 0 || (uintptr_t) weights % sizeof(float) != 0 ||
      (uintptr_t) group_ids % sizeof(int32_t) != 0 || (uintptr_t) output % sizeof(float) != 0) {
    qnnp_log_error("cannot set up weighted combine: a tensor, the weights or the group ids are not 4-byte aligned");
    return qnnp_status_invalid_parameter;
  }
  if (input_stride < channels || output_stride < channels) {
    qnnp_log_error("cannot set up weighted combine: row stride smaller than the channel count");
    return qnnp_status_invalid_parameter;
  }
  if (too_many_rows(batch_size, assignments)) {
    qnnp_log_error("cannot set up weighted combine with batch %zu and %zu assignments: fewer than %zu input rows",
        batch_size, assignments, QNNP_MOE_MAX_ROWS);
    return qnnp_status_unsupported_parameter;
  }
  const size_t rows = batch_size * assignments;
  const size_t input_span = ((rows - 1) * input_stride + channels) * sizeof(float);
  const size_t output_span = ((batch_size - 1) * output_stride + channels) * sizeof(float);
  const size_t weights_span = rows * sizeof(float);
  const size_t ids_span = rows * sizeof(int32_t);
  if (qnnp_spans_overlap(input, input_span, output, output_span) || qnnp_spans_overlap(weights, weights_span, output, output_span) ||
      qnnp_spans_overlap(group_ids, ids_span, output, output_span)) {
    qnnp_log_error("cannot set up weighted combine: the output overlaps the input, the weights or the group ids");
    return qnnp_status_invalid_parameter;
  }
  /* all four in device memory: the launch reads the ids and the weights there */
  if (qnnp_hip_is_device_pointer(input) != 1 || qnnp_hip_is_device_pointer(weights) != 1 ||
      qnnp_hip_is_device_pointer(group_ids) != 1 || qnnp_hip_is_device_pointer(output) != 1) {
    qnnp_log_error("cannot set up weighted combine: the tensors, the weights and the group ids have to be memory of the "
        "operator's device");
    return qnnp_status_invalid_parameter;
  }

  op->setup_valid = 0;
  op->batch_size = batch_size;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->moe_weights = (void*) (uintptr_t) weights;
  op->moe_group_ids = group_ids;
  op->input_span = input_span;
  op->output_span = output_span;
  return qnnp_bind_tensors(op, function);
}

enum qnnp_status qnnp_gfx950_setup_weighted_combine_nc_f32(
    qnnp_operator_t combine,
    size_t batch_size,
    const float* input,
    size_t input_stride,
    const float* weights,
    const int32_t* group_ids,
    float* output,
    size_t output_stride)
{
  const char* function = "qnnp_gfx950_setup_weighted_combine_nc_f32";
  int token;
  const enum qnnp_status status = qnnp_enter_setup(function, combine, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_leave_setup(combine, token, setup_weighted_combine(function, combine, batch_size, input, input_stride, weights,
      group_ids, output, output_stride));
}
