/*
 * hip_stub_softargmax.c -- TEST INFRASTRUCTURE: the softargmax launch of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/q8softargmax.hip) for the host-sanitizer build of the operator (Makefile target asan-softargmax), beside
 * tests/hip_stub.c. It validates the argument block as the device launcher does, keeps a copy of it for the test to
 * look at, and computes nothing: the launch is a no-op.
 */
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

struct qnnp_hip_softargmax_args qnnp_stub_softargmax_last;   /* the argument block of the last accepted launch */
long qnnp_stub_softargmax_launches;

int qnnp_hip_softargmax_run(const struct qnnp_hip_softargmax_args* a, const char** kernel_name)
{
  if (a == NULL || a->input == NULL || a->output == NULL || a->table == NULL || a->channels == 0 ||
      a->channels > 0x7FFFFFFFu || a->input_stride < a->channels || a->output_stride < a->channels ||
      a->rows > 0x7FFFFFFFu || (uintptr_t) a->table % 4 != 0) {
    return QNNP_HIP_EINVAL;
  }
  qnnp_stub_softargmax_last = *a;
  qnnp_stub_softargmax_launches++;
  if (kernel_name != NULL) *kernel_name = "stub_softargmax";
  return QNNP_HIP_OK;
}
