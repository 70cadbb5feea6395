/*
 * hip_stub_x8.c -- TEST INFRASTRUCTURE: the channel-shuffle and clamp launches of the HIP seam
 * (qnnpack_amd/csrc/hip/qnnp_hip.h, hip/x8shuffle.hip) for the host-sanitizer build of those operators (Makefile target
 * asan-x8), beside tests/hip_stub.c. They validate the argument block as the device launchers do and then compute the
 * result byte by byte on the host, so ASan sees any undersized staging buffer and the test can check the bytes that come
 * back through the staging round trip.
 */
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

int qnnp_hip_channel_shuffle_run(const struct qnnp_hip_x8_args* a, const char** kernel_name)
{
  if (a == NULL || a->input == NULL || a->output == NULL || a->groups < 2 || a->group_channels == 0 ||
      (uint64_t) a->groups * a->group_channels != a->channels || a->input_stride < a->channels ||
      a->output_stride < a->channels || a->pixels > 0x7FFFFFFFu) {
    return QNNP_HIP_EINVAL;
  }
  if (kernel_name != NULL) *kernel_name = "stub_channel_shuffle";
  for (uint64_t p = 0; p < a->pixels; p++) {
    const uint8_t* x = a->input + p * a->input_stride;
    uint8_t* y = a->output + p * a->output_stride;
    for (uint32_t g = 0; g < a->groups; g++) {
      for (uint32_t c = 0; c < a->group_channels; c++) {
        y[(uint64_t) c * a->groups + g] = x[(uint64_t) g * a->group_channels + c];
      }
    }
  }
  return QNNP_HIP_OK;
}

int qnnp_hip_clamp_run(const struct qnnp_hip_x8_args* a, const char** kernel_name)
{
  if (a == NULL || a->input == NULL || a->output == NULL || a->channels == 0 || a->input_stride < a->channels ||
      a->output_stride < a->channels || a->output_min > a->output_max || a->output_max > 255u ||
      a->pixels > 0x7FFFFFFFu) {
    return QNNP_HIP_EINVAL;
  }
  if (kernel_name != NULL) *kernel_name = "stub_clamp";
  for (uint64_t p = 0; p < a->pixels; p++) {
    const uint8_t* x = a->input + p * a->input_stride;
    uint8_t* y = a->output + p * a->output_stride;
    for (uint32_t c = 0; c < a->channels; c++) {
      const uint32_t v = x[c];
      y[c] = (uint8_t) (v < a->output_min ? a->output_min : (v > a->output_max ? a->output_max : v));
    }
  }
  return QNNP_HIP_OK;
}
