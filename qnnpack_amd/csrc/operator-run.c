/*
 * operator-run.c -- qnnp_run_operator for the gfx950 build.
 *
 * Replaces reference src/operator-run.c:639-844. The reference switches on the
 * operator's type, builds a stack context and fans MRxNR microkernel calls out
 * over a pthreadpool (:675 dwconv, :797 gemm, :837 conv). Here every operator
 * carries its launch function (op->launch, operator.h), which builds a POD
 * argument block and makes a whole-operator kernel launch on the library stream
 * through the C-ABI HIP shim (hip/qnnp_hip.h); it lives beside the operator's
 * create and setup. This file is what all operators share around that call:
 * status mapping, staging of host tensors, the synchronisation rule, the timing
 * helpers and graph capture. It refers to no kernel, so it links into every
 * build whichever operators that build has. `threadpool` is ignored.
 *
 * Like the reference, nothing is allocated and nothing is logged on this path
 * (device pointers). Host pointers given to setup are staged through device
 * scratch sized at setup.
 *
 * Threading: as in the reference (run contexts are stack-local, src/operator-run.c:783-795), distinct operators
 * may be run from different threads at the same time. Nothing on this path is process-global mutable state: the
 * operator names its device, the launch stream / asynchrony flag belong to that device's context, and a hipGraph
 * capture belongs to the capturing thread (hip/runtime.hip).
 */
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "operator.h"
#include "state.h"

#define QNNP_TIMING_SAMPLES 5

static enum qnnp_status status_from_hip(int rc)
{
  switch (rc) {
    case QNNP_HIP_OK: return qnnp_status_success;
    case QNNP_HIP_ENOMEM: return qnnp_status_out_of_memory;
    case QNNP_HIP_EINVAL: return qnnp_status_unsupported_parameter;
    default: return qnnp_status_unsupported_hardware;
  }
}

enum qnnp_status qnnp_bind_endpoint(const void* ptr, size_t span, int* on_device, void** stage, size_t* capacity)
{
  const int where = qnnp_hip_is_device_pointer(ptr);
  if (where < 0) {
    return qnnp_status_invalid_parameter;   /* memory of a GPU other than the operator's */
  }
  *on_device = where;
  if (where) return qnnp_status_success;
  if (*capacity < span) {
    qnnp_hip_free(*stage);
    *capacity = 0;
    *stage = qnnp_hip_alloc(span);
    if (*stage == NULL) return qnnp_status_out_of_memory;
    *capacity = span;
  }
  return qnnp_status_success;
}

static enum qnnp_status run_operator(qnnp_operator_t op)
{
  if (!op->setup_valid) {
    return qnnp_status_invalid_parameter;  /* run before setup, or after a setup that failed */
  }
  /* reference operator-run.c:642-644: nothing to do for an empty batch */
  if (op->batch_size == 0) {
    return qnnp_status_success;
  }
  if (op->input == NULL || op->output == NULL) {
    return qnnp_status_invalid_parameter;
  }

  const void* input = op->input;
  const void* input2 = op->input2;
  void* output = op->output;
  const int staged = !op->input_on_device || !op->output_on_device || (op->input2 != NULL && !op->input2_on_device);
  const int capturing = qnnp_hip_graph_capturing();
  if (capturing && staged) {
    return qnnp_status_invalid_parameter;  /* a graph can only hold device-pointer launches */
  }

  if (!op->input_on_device) {
    if (qnnp_hip_h2d(op->d_stage_in, op->input, op->input_span, 1) != QNNP_HIP_OK) {
      return qnnp_status_invalid_parameter;
    }
    input = op->d_stage_in;
  }
  if (op->input2 != NULL && !op->input2_on_device) {
    if (qnnp_hip_h2d(op->d_stage_in2, op->input2, op->input2_span, 1) != QNNP_HIP_OK) {
      return qnnp_status_invalid_parameter;
    }
    input2 = op->d_stage_in2;
  }
  if (!op->output_on_device) {
    const size_t out_channels = op->channels != 0 ? op->channels : (size_t) op->groups * op->group_output_channels;
    if (op->output_pixel_stride != out_channels) {
      /* keep the caller's bytes between pixels intact across the round trip */
      if (qnnp_hip_h2d(op->d_stage_out, op->output, op->output_span, 1) != QNNP_HIP_OK) {
        return qnnp_status_invalid_parameter;
      }
    }
    output = op->d_stage_out;
  }

  const int rc = op->launch(op, input, input2, output);
  if (rc != QNNP_HIP_OK) {
    return status_from_hip(rc);
  }

  if (!op->output_on_device) {
    if (qnnp_hip_d2h(op->output, op->d_stage_out, op->output_span, 1) != QNNP_HIP_OK) {
      return qnnp_status_invalid_parameter;
    }
  }
  if (capturing) {
    return qnnp_status_success;            /* recorded into the graph; nothing has run yet */
  }
  if (staged || !qnnp_hip_get_async()) {
    /* reference semantics: outputs are complete when run returns */
    return status_from_hip(qnnp_hip_stream_sync());
  }
  return qnnp_status_success;
}

enum qnnp_status qnnp_run_operator(qnnp_operator_t op, pthreadpool_t threadpool)
{
  (void) threadpool;
  if (op == NULL) {
    return qnnp_status_invalid_parameter;
  }
  if (!qnnp_state.initialized) {
    return qnnp_status_uninitialized;
  }
  const int token = qnnp_hip_enter(op->device);
  if (token < 0) {
    return qnnp_status_invalid_parameter;
  }
  const enum qnnp_status status = run_operator(op);
  qnnp_hip_leave(token);
  return status;
}

/* ---- qnnpack_gfx950.h timing helpers ---------------------------------- */

static enum qnnp_status time_operator_rotating(
    qnnp_operator_t op, size_t nsets, const void* const* inputs, void* const* outputs,
    int warmup, int iters, float* avg_ms_out)
{
  if (!op->setup_valid) {
    return qnnp_status_invalid_parameter;
  }
  if (op->batch_size == 0) {
    *avg_ms_out = 0.0f;
    return qnnp_status_success;
  }
  for (size_t s = 0; s < nsets; s++) {
    if (qnnp_hip_is_device_pointer(inputs[s]) != 1 || qnnp_hip_is_device_pointer(outputs[s]) != 1) {
      return qnnp_status_invalid_parameter;
    }
  }
  if (op->input2 != NULL && !op->input2_on_device) {
    return qnnp_status_invalid_parameter;   /* add: the second operand is not rotated and must be device memory */
  }
  /* Preferred: record the `iters` launches into a hipGraph and time its replay -- one submission, so the
   * figure is kernel time, not the host's per-launch dispatch gap (5-8 us, as large as the small layers).
   * The replay is timed QNNP_TIMING_SAMPLES times, each sample its own event pair, and the MEDIAN sample is
   * reported (one sample is at the mercy of the clock state of the moment). Falls back to a plain launch loop
   * if the capture is refused. */
  if (qnnp_state.opt_timing_graph && !qnnp_hip_graph_capturing() && qnnp_hip_graph_begin() == QNNP_HIP_OK) {
    int rc = QNNP_HIP_OK;
    size_t gset = 0;
    for (int i = 0; i < iters && rc == QNNP_HIP_OK; i++) {
      rc = op->launch(op, inputs[gset], op->input2, outputs[gset]);
      gset = (gset + 1) % nsets;
    }
    void* graph = NULL;
    const int rc_end = qnnp_hip_graph_end(&graph);
    if (rc == QNNP_HIP_OK && rc_end == QNNP_HIP_OK) {
      float ms = 0.0f;
      const int reps = warmup > 0 ? 1 : 0;
      rc = qnnp_hip_graph_time_median(graph, reps, 1, QNNP_TIMING_SAMPLES, &ms);
      qnnp_hip_graph_destroy(graph);
      if (rc == QNNP_HIP_OK) {
        *avg_ms_out = ms / (float) iters;
        return qnnp_status_success;
      }
    } else if (rc_end == QNNP_HIP_OK) {
      qnnp_hip_graph_destroy(graph);
    }
  }
  void* timer = NULL;
  if (qnnp_hip_timer_create(&timer) != QNNP_HIP_OK) {
    return qnnp_status_out_of_memory;
  }
  enum qnnp_status status = qnnp_status_success;
  size_t set = 0;
  for (int i = 0; i < warmup && status == qnnp_status_success; i++) {
    status = status_from_hip(op->launch(op, inputs[set], op->input2, outputs[set]));
    set = (set + 1) % nsets;
  }
  if (status == qnnp_status_success) {
    qnnp_hip_timer_start(timer);
    for (int i = 0; i < iters && status == qnnp_status_success; i++) {
      status = status_from_hip(op->launch(op, inputs[set], op->input2, outputs[set]));
      set = (set + 1) % nsets;
    }
    float ms = 0.0f;
    const int rc = qnnp_hip_timer_stop_ms(timer, &ms);
    if (status == qnnp_status_success) status = status_from_hip(rc);
    *avg_ms_out = ms / (float) iters;
  }
  qnnp_hip_timer_destroy(timer);
  return status;
}

enum qnnp_status qnnp_gfx950_time_operator_rotating(
    qnnp_operator_t op, size_t nsets, const void* const* inputs, void* const* outputs,
    int warmup, int iters, float* avg_ms_out)
{
  if (op == NULL || avg_ms_out == NULL || iters <= 0 || nsets == 0 || inputs == NULL || outputs == NULL) {
    return qnnp_status_invalid_parameter;
  }
  if (!qnnp_state.initialized) {
    return qnnp_status_uninitialized;
  }
  const int token = qnnp_hip_enter(op->device);
  if (token < 0) {
    return qnnp_status_invalid_parameter;
  }
  const enum qnnp_status status = time_operator_rotating(op, nsets, inputs, outputs, warmup, iters, avg_ms_out);
  qnnp_hip_leave(token);
  return status;
}

enum qnnp_status qnnp_gfx950_time_operator(
    qnnp_operator_t op, int warmup, int iters, float* avg_ms_out)
{
  if (op == NULL) {
    return qnnp_status_invalid_parameter;
  }
  const void* in = op->input;
  void* out = op->output;
  return qnnp_gfx950_time_operator_rotating(op, 1, &in, &out, warmup, iters, avg_ms_out);
}

/* ---- qnnpack_gfx950.h graph capture ------------------------------------ */

enum qnnp_status qnnp_gfx950_graph_begin(void)
{
  if (!qnnp_state.initialized) return qnnp_status_uninitialized;
  /* the calling thread records launches on its selected device until graph_end */
  const int token = qnnp_hip_enter(qnnp_hip_device());
  if (token < 0) return qnnp_status_unsupported_hardware;
  const enum qnnp_status status = status_from_hip(qnnp_hip_graph_begin());
  qnnp_hip_leave(token);
  return status;
}

enum qnnp_status qnnp_gfx950_graph_end(void** graph_out)
{
  if (graph_out == NULL) return qnnp_status_invalid_parameter;
  if (!qnnp_state.initialized) return qnnp_status_uninitialized;
  return status_from_hip(qnnp_hip_graph_end(graph_out));
}

enum qnnp_status qnnp_gfx950_graph_launch(void* graph)
{
  if (graph == NULL) return qnnp_status_invalid_parameter;
  const int rc = qnnp_hip_graph_launch(graph);
  if (rc != QNNP_HIP_OK) return status_from_hip(rc);
  const int token = qnnp_hip_enter(qnnp_hip_graph_device(graph));
  const int async = token >= 0 ? qnnp_hip_get_async() : 0;
  qnnp_hip_leave(token);
  return async ? qnnp_status_success : status_from_hip(qnnp_hip_graph_sync(graph));
}

enum qnnp_status qnnp_gfx950_graph_time(void* graph, int warmup, int iters, float* avg_ms_out)
{
  if (graph == NULL || avg_ms_out == NULL || iters <= 0) return qnnp_status_invalid_parameter;
  /* QNNP_TIMING_SAMPLES event-bracketed batches of `iters` replays each; the median batch / iters */
  return status_from_hip(qnnp_hip_graph_time_median(graph, warmup, iters, QNNP_TIMING_SAMPLES, avg_ms_out));
}

enum qnnp_status qnnp_gfx950_graph_synchronize(void* graph)
{
  if (graph == NULL) return qnnp_status_invalid_parameter;
  return status_from_hip(qnnp_hip_graph_sync(graph));
}

void qnnp_gfx950_graph_destroy(void* graph)
{
  qnnp_hip_graph_destroy(graph);
}
