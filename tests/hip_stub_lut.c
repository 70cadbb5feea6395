/*
 * hip_stub_lut.c -- TEST INFRASTRUCTURE: the lookup-table launch of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/x8lut.hip) for the host-sanitizer build of the table operators (Makefile target asan-lut), beside tests/hip_stub.c.
 * It validates the argument block as the device launcher does and then looks every byte up on the host (the stub's
 * "device" memory is host memory), so ASan sees any undersized staging buffer or table and the test can check the bytes
 * that come back through the staging round trip.
 */
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

int qnnp_hip_lut_run(const struct qnnp_hip_lut_args* a, const char** kernel_name)
{
  if (a == NULL || a->input == NULL || a->output == NULL || a->table == NULL || a->channels == 0 ||
      a->channels > 0x7FFFFFFFu || a->input_stride < a->channels || a->output_stride < a->channels ||
      a->pixels > 0x7FFFFFFFu || (uintptr_t) a->table % 4 != 0) {
    return QNNP_HIP_EINVAL;
  }
  if (kernel_name != NULL) *kernel_name = "stub_lut";
  for (uint64_t p = 0; p < a->pixels; p++) {
    const uint8_t* x = a->input + p * a->input_stride;
    uint8_t* y = a->output + p * a->output_stride;
    for (uint32_t c = 0; c < a->channels; c++) {
      y[c] = a->table[x[c]];
    }
  }
  return QNNP_HIP_OK;
}
