/*
 * hip_stub_quantize.c -- TEST INFRASTRUCTURE: the quantize and dequantize launches of the HIP seam
 * (qnnpack_amd/csrc/hip/qnnp_hip.h, hip/f32q8.hip) for the host-sanitizer build of the two operators (Makefile target
 * asan-quantize), beside tests/hip_stub.c. It validates the argument block as the device launcher does, checks what
 * quantize.c and dequantize.c are to hand over (a normal reciprocal, clamp bounds that are integers around zero, a zero
 * point that is a byte) and then computes every element on the host from the definition (the stub's "device" memory is
 * host memory), so ASan sees any undersized staging buffer and the test can check what comes back through the staging
 * round trip.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

/* what the last launches were handed (tests/host_asan_quantize_test.c reads them) */
struct qnnp_hip_quantize_args qnnp_stub_quantize_last;
struct qnnp_hip_dequantize_args qnnp_stub_dequantize_last;
unsigned qnnp_stub_quantize_launches;
unsigned qnnp_stub_dequantize_launches;

static int shape_ok(const void* f, const void* q, uint32_t planar, uint32_t rows, uint32_t pixels, uint32_t channels,
                    uint64_t f_stride, uint64_t q_stride)
{
  if (f == NULL || q == NULL || (uintptr_t) f % 4 != 0 || channels == 0 || channels > 0x7FFFFFFFu || rows > 0x7FFFFFFFu ||
      q_stride < channels) {
    return 0;
  }
  if (planar != 0) {
    return pixels != 0 && (uint64_t) rows * pixels <= 0x7FFFFFFFu && (uint64_t) channels * pixels <= 0x7FFFFFFFu;
  }
  return f_stride >= channels;
}

static uint8_t quantize_one(float x, const struct qnnp_hip_quantize_args* a)
{
  volatile float t = x * a->inv_scale;   /* volatile: rounded to float32 here, whatever the compiler's evaluation method */
  float u = isnan(t) ? 0.0f : t;
  u = u < a->clamp_lo ? a->clamp_lo : u;
  u = u > a->clamp_hi ? a->clamp_hi : u;
  return (uint8_t) ((int32_t) rintf(u) + a->zero_point);
}

int qnnp_hip_quantize_run(const struct qnnp_hip_quantize_args* a, const char** kernel_name)
{
  if (a == NULL || !shape_ok(a->input, a->output, a->planar, a->rows, a->pixels, a->channels, a->input_stride, a->output_stride)) {
    return QNNP_HIP_EINVAL;
  }
  /* quantize.c's side of the contract */
  if (!isnormal(a->inv_scale) || a->inv_scale <= 0.0f || a->zero_point < 0 || a->zero_point > 255 ||
      a->clamp_lo != rintf(a->clamp_lo) || a->clamp_hi != rintf(a->clamp_hi) || a->clamp_lo >= a->clamp_hi ||
      a->clamp_lo + (float) a->zero_point < 0.0f || a->clamp_hi + (float) a->zero_point > 255.0f ||
      a->streaming_mode > 2 || a->planar > 1) {
    abort();
  }
  qnnp_stub_quantize_last = *a;
  qnnp_stub_quantize_launches++;
  if (kernel_name != NULL) *kernel_name = "stub_quantize";
  if (a->planar) {
    for (uint64_t n = 0; n < a->rows; n++) {
      for (uint64_t c = 0; c < a->channels; c++) {
        for (uint64_t p = 0; p < a->pixels; p++) {
          a->output[(n * a->pixels + p) * a->output_stride + c] = quantize_one(a->input[(n * a->channels + c) * a->pixels + p], a);
        }
      }
    }
  } else {
    for (uint64_t r = 0; r < a->rows; r++) {
      for (uint64_t c = 0; c < a->channels; c++) {
        a->output[r * a->output_stride + c] = quantize_one(a->input[r * a->input_stride + c], a);
      }
    }
  }
  return QNNP_HIP_OK;
}

int qnnp_hip_dequantize_run(const struct qnnp_hip_dequantize_args* a, const char** kernel_name)
{
  if (a == NULL || !shape_ok(a->output, a->input, a->planar, a->rows, a->pixels, a->channels, a->output_stride, a->input_stride)) {
    return QNNP_HIP_EINVAL;
  }
  /* dequantize.c's side of the contract */
  if (!isnormal(a->scale) || a->scale <= 0.0f || a->zero_point < 0 || a->zero_point > 255 || a->streaming_mode > 2 ||
      a->planar > 1) {
    abort();
  }
  qnnp_stub_dequantize_last = *a;
  qnnp_stub_dequantize_launches++;
  if (kernel_name != NULL) *kernel_name = "stub_dequantize";
  if (a->planar) {
    for (uint64_t n = 0; n < a->rows; n++) {
      for (uint64_t c = 0; c < a->channels; c++) {
        for (uint64_t p = 0; p < a->pixels; p++) {
          a->output[(n * a->channels + c) * a->pixels + p] =
              (float) ((int32_t) a->input[(n * a->pixels + p) * a->input_stride + c] - a->zero_point) * a->scale;
        }
      }
    }
  } else {
    for (uint64_t r = 0; r < a->rows; r++) {
      for (uint64_t c = 0; c < a->channels; c++) {
        a->output[r * a->output_stride + c] = (float) ((int32_t) a->input[r * a->input_stride + c] - a->zero_point) * a->scale;
      }
    }
  }
  return QNNP_HIP_OK;
}
