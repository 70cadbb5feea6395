/*
 * lifecycle.h -- what every operator's create and setup share, so that an operator file is validation plus geometry:
 *
 *   entry guards   A public create runs on the calling thread's selected device (qnnp_gfx950_set_device, default = the
 *                  primary one), which becomes the operator's device; a public setup runs on the operator's device. The
 *                  guards refuse before qnnp_initialize, enter that device and refuse inside a graph capture; the
 *                  leave functions restore the thread's previous HIP device and hand the status through. Entry points
 *                  that validate before they enter call qnnp_check_initialized first and enter when they are done.
 *   allocation     qnnp_allocate_operator: the zeroed operator, owned by the device the create runs in.
 *   binding        qnnp_bind_tensors: where the tensors of a setup live, and device staging for those in host memory.
 *   NC setup       qnnp_setup_nc: the whole setup of the operators that map `batch_size` rows of `channels` bytes to as
 *                  many rows of the same size.
 *
 * A setup clears op->setup_valid where it begins to change the operator and qnnp_leave_setup sets it again on success, so
 * a failed setup leaves the operator unrunnable instead of half updated (qnnp_run_operator answers invalid_parameter),
 * while a setup refused by a check that comes earlier leaves the previous one runnable.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <qnnpack.h>

#include "hip/qnnp_hip.h"
#include "log.h"
#include "operator.h"
#include "state.h"

/* Enters `device` (qnnp_hip_leave(*token) undoes it) and answers success, or `no_device` when that device cannot be
 * entered, or invalid_parameter inside a graph capture on it (qnnp_gfx950_graph_begin ... graph_end: only operator
 * launches are recordable there -- an upload would become a graph node reading host memory that is freed right after the
 * call). Nothing is left entered on a refusal. */
static inline enum qnnp_status qnnp_enter_for_update(int device, enum qnnp_status no_device, int* token)
{
  *token = qnnp_hip_enter(device);
  if (*token < 0) {
    return no_device;
  }
  if (qnnp_hip_graph_capturing()) {
    qnnp_hip_leave(*token);
    return qnnp_status_invalid_parameter;
  }
  return qnnp_status_success;
}

/* the first check of every public entry point; `function` is its name, for the log */
static inline enum qnnp_status qnnp_check_initialized(const char* function)
{
  if (!qnnp_state.initialized) {
    qnnp_log_error("%s called before qnnp_initialize succeeded", function);
    return qnnp_status_uninitialized;
  }
  return qnnp_status_success;
}

/* create guard: initialized, then inside the calling thread's device; undone by qnnp_leave_create */
static inline enum qnnp_status qnnp_enter_create(const char* function, int* token)
{
  const enum qnnp_status status = qnnp_check_initialized(function);
  if (status != qnnp_status_success) {
    return status;
  }
  return qnnp_enter_for_update(qnnp_hip_device(), qnnp_status_unsupported_hardware, token);
}

static inline enum qnnp_status qnnp_leave_create(int token, enum qnnp_status status)
{
  qnnp_hip_leave(token);
  return status;
}

/* setup guard: initialized, a handle, then inside the handle's device; undone by qnnp_leave_setup. Whether the handle is
 * of the caller's operator type is the caller's check, inside the entered region. */
static inline enum qnnp_status qnnp_enter_setup(const char* function, qnnp_operator_t op, int* token)
{
  const enum qnnp_status status = qnnp_check_initialized(function);
  if (status != qnnp_status_success) {
    return status;
  }
  if (op == NULL) {
    return qnnp_status_invalid_parameter;
  }
  return qnnp_enter_for_update(op->device, qnnp_status_invalid_parameter, token);
}

/* setup epilogue: a successful setup makes the operator runnable */
static inline enum qnnp_status qnnp_leave_setup(qnnp_operator_t op, int token, enum qnnp_status status)
{
  if (status == qnnp_status_success) {
    op->setup_valid = 1;
  }
  qnnp_hip_leave(token);
  return status;
}

/* A zeroed operator of the given type on the device the create runs in, or NULL (logged: out of host memory). `launch`
 * is the operator's launch function (operator.h), which every create passes. */
static inline qnnp_operator_t qnnp_allocate_operator(
    enum qnnp_ukernel_type type,
    int (*launch)(struct qnnp_operator* op, const void* input, const void* input2, void* output))
{
  qnnp_operator_t op = calloc(1, sizeof(struct qnnp_operator));
  if (op == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for qnnp_operator structure", sizeof(struct qnnp_operator));
    return NULL;
  }
  op->device = qnnp_hip_device();
  op->ukernel_type = type;
  op->launch = launch;
  return op;
}

/* Binds op->input, then op->input2 where the operator has a second operand (add, multiply: the others leave it NULL),
 * then op->output, over the byte spans the setup has stored: decides where each tensor lives and sizes the device staging
 * of those in host memory. Stops at the first failure: out_of_memory (staging) or invalid_parameter (memory of a GPU
 * other than the operator's). `what` names the entry point in the log. */
static inline enum qnnp_status qnnp_bind_tensors(qnnp_operator_t op, const char* what)
{
  enum qnnp_status bound =
      qnnp_bind_endpoint(op->input, op->input_span, &op->input_on_device, &op->d_stage_in, &op->stage_in_capacity);
  if (bound == qnnp_status_success && op->input2 != NULL) {
    bound = qnnp_bind_endpoint(op->input2, op->input2_span, &op->input2_on_device, &op->d_stage_in2, &op->stage_in2_capacity);
  }
  if (bound == qnnp_status_success) {
    bound = qnnp_bind_endpoint(op->output, op->output_span, &op->output_on_device, &op->d_stage_out, &op->stage_out_capacity);
  }
  if (bound != qnnp_status_success) {
    qnnp_log_error("%s: failed to bind the tensors: device staging for host memory could not be allocated, or a tensor "
        "lives on a different device than the operator", what);
  }
  return bound;
}

/* The setup of an operator over `batch_size` rows of op->channels bytes in and as many out (clamp, the table operators,
 * softargmax, channel shuffle), called inside the operator's device. Batch 0 succeeds and the run then does nothing.
 * invalid_parameter: NULL tensors, row strides below the channel count, input and output byte spans that overlap --
 * other than exactly in place (input == output with equal strides) where `in_place_allowed`; unsupported_parameter: a
 * batch beyond the kernels' index range. Every check comes before the operator changes. */
static inline enum qnnp_status qnnp_setup_nc(
    qnnp_operator_t op, const char* what, int in_place_allowed, size_t batch_size, const uint8_t* input,
    size_t input_stride, uint8_t* output, size_t output_stride)
{
  if (batch_size == 0) {
    op->batch_size = 0;
    return qnnp_status_success;
  }
  const size_t channels = op->channels;
  if (input == NULL || output == NULL || input_stride < channels || output_stride < channels) {
    qnnp_log_error("%s: NULL tensor or row stride smaller than the channel count", what);
    return qnnp_status_invalid_parameter;
  }
  if (batch_size > (size_t) INT32_MAX) {
    qnnp_log_error("%s with batch %zu: outside the device kernel's index range", what, batch_size);
    return qnnp_status_unsupported_parameter;
  }
  const size_t input_span = (batch_size - 1) * input_stride + channels;
  const size_t output_span = (batch_size - 1) * output_stride + channels;
  const int in_place = in_place_allowed && (const void*) input == (const void*) output && input_stride == output_stride;
  if (!in_place && qnnp_spans_overlap(input, input_span, output, output_span)) {
    qnnp_log_error("%s: the input and output tensors overlap%s", what,
        in_place_allowed ? " without being the same tensor" : "");
    return qnnp_status_invalid_parameter;
  }

  op->setup_valid = 0;   /* until the allocations below have succeeded */
  op->batch_size = batch_size;
  op->input = input;
  op->input_pixel_stride = input_stride;
  op->output = output;
  op->output_pixel_stride = output_stride;
  op->input_span = input_span;
  op->output_span = output_span;
  return qnnp_bind_tensors(op, what);
}
