/*
 * hip_stub_table.c -- TEST INFRASTRUCTURE: the lookup-table launch of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/x8lut.hip) for the host-sanitizer build of the output table (Makefile target asan-table), beside tests/hip_stub.c and
 * in the place of tests/hip_stub_lut.c. Like that file it validates the argument block as the device launcher does and
 * looks every byte up on the host; it also counts the launches and keeps the last argument block, so that
 * tests/host_asan_table_test.c can see the in-place launch behind a convolution: which tensor it walked, with which strides,
 * through which table. tests/hip_stub.c's convolution launches compute nothing and carry no table in their "epilogue", so
 * every attached table arrives here.
 */
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

struct qnnp_hip_lut_args qnnp_stub_lut_last;
unsigned qnnp_stub_lut_launches = 0;

int qnnp_hip_lut_run(const struct qnnp_hip_lut_args* a, const char** kernel_name)
{
  if (a == NULL || a->input == NULL || a->output == NULL || a->table == NULL || a->channels == 0 ||
      a->channels > 0x7FFFFFFFu || a->input_stride < a->channels || a->output_stride < a->channels ||
      a->pixels > 0x7FFFFFFFu || (uintptr_t) a->table % 4 != 0) {
    return QNNP_HIP_EINVAL;
  }
  qnnp_stub_lut_last = *a;
  qnnp_stub_lut_launches++;
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
