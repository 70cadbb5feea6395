/*
 * hip_stub_pool.c -- TEST INFRASTRUCTURE: the windowed-pooling launches of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/q8pool.hip) for the host-sanitizer build of the pooling operators (Makefile target asan-pool), beside
 * tests/hip_stub.c. Like the launches there, they validate the argument block and touch the first and last byte of each
 * tensor the kernel would read or write (so ASan sees an undersized staging buffer); nothing is computed.
 */
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

static volatile uint8_t g_pool_sink;

static void touch_span(const void* p, uint64_t pixels, uint64_t stride, uint32_t channels)
{
  const volatile uint8_t* b = (const volatile uint8_t*) p;
  g_pool_sink ^= b[0];
  g_pool_sink ^= b[(pixels - 1) * stride + channels - 1];
}

static int pool_run(const struct qnnp_hip_pool_args* a, const char** kernel_name, const char* name)
{
  if (a == NULL || a->input == NULL || a->output == NULL || a->channels == 0 || a->batch == 0 ||
      a->input_height == 0 || a->input_width == 0 || a->output_height == 0 || a->output_width == 0 ||
      a->kernel_height == 0 || a->kernel_width == 0 || a->stride_height == 0 || a->stride_width == 0 ||
      a->dilation_height == 0 || a->dilation_width == 0 ||
      a->input_stride < a->channels || a->output_stride < a->channels) {
    return QNNP_HIP_EINVAL;
  }
  /* the last output row's window must start inside the padded input (setup's output-size rule) */
  const uint64_t last_y = (uint64_t) (a->output_height - 1) * a->stride_height +
      (uint64_t) (a->kernel_height - 1) * a->dilation_height;
  const uint64_t last_x = (uint64_t) (a->output_width - 1) * a->stride_width +
      (uint64_t) (a->kernel_width - 1) * a->dilation_width;
  if (last_y >= (uint64_t) a->pad_top + a->input_height + 0x7FFFFFFFu || last_x >= (uint64_t) a->pad_left + a->input_width + 0x7FFFFFFFu) {
    abort();
  }
  if (kernel_name != NULL) *kernel_name = name;
  touch_span(a->input, (uint64_t) a->batch * a->input_height * a->input_width, a->input_stride, a->channels);
  touch_span(a->output, (uint64_t) a->batch * a->output_height * a->output_width, a->output_stride, a->channels);
  return QNNP_HIP_OK;
}

int qnnp_hip_maxpool_run(const struct qnnp_hip_pool_args* a, const char** kernel_name)
{
  return pool_run(a, kernel_name, "stub_maxpool");
}

int qnnp_hip_avgpool_run(const struct qnnp_hip_pool_args* a, const char** kernel_name)
{
  if (a != NULL && (a->dilation_height != 1 || a->dilation_width != 1)) return QNNP_HIP_EINVAL;
  return pool_run(a, kernel_name, "stub_avgpool");
}
