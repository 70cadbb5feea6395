/*
 * hip_stub_se.c -- TEST INFRASTRUCTURE: the squeeze-and-excite gate launch of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/q8segate.hip) for the host-sanitizer build of the fused operator (Makefile target asan-se), beside tests/hip_stub.c,
 * tests/hip_stub_lut.c and tests/hip_stub_mul.c. It validates the argument block as the device launcher does and then
 * computes the gate rows on the host, in plain C FROM THE ARGUMENT BLOCK ALONE: a scalar restatement of how the kernel
 * addresses the members' standard weight image (the fragment panels of pack.h qnnp_pack_igemm_w), the folded bias and
 * the row term -- under tests/hip_stub.c "device" memory is host memory, so the images squeeze-excite.c hands over are
 * the ones fully-connected.c packed. A misread of that layout shows here, against values the test program computes from
 * the raw weights, before any GPU run; and ASan sees any read outside the images, the scratch or the input.
 */
#include <stdint.h>
#include <stdlib.h>

#include "hip/qnnp_hip.h"

/* what the last launch was handed (tests/host_asan_se_test.c reads them) */
struct qnnp_hip_se_gate_args qnnp_stub_se_last;
unsigned qnnp_stub_se_launches;

/* the scalar definition (reference src/qnnpack/requantization.h:464-480), as tests/hip_stub_mul.c spells it */
static uint8_t requantize(int32_t n, const struct qnnp_hip_requant* rq)
{
  const int64_t product = (int64_t) n * (int64_t) rq->multiplier;
  const int32_t q = (int32_t) (uint32_t) ((uint64_t) (product + INT64_C(0x40000000)) >> 31);
  const int32_t remainder = (q & rq->remainder_mask) - (int32_t) (n < 0);
  const int32_t shifted = q >= 0 ? (int32_t) ((uint32_t) q >> rq->shift) : -(int32_t) (((uint32_t) -(q + 1)) >> rq->shift) - 1;
  int32_t y = shifted + (int32_t) (remainder > rq->remainder_threshold);
  if (y < rq->output_min_less_zero_point) y = rq->output_min_less_zero_point;
  if (y > rq->output_max_less_zero_point) y = rq->output_max_less_zero_point;
  return (uint8_t) (y + rq->output_zero_point);
}

/* reference src/qnnpack/requantization.h:482-498 */
static uint8_t avgpool_quantize(int32_t n, const struct qnnp_hip_avgpool_params* q)
{
  const int64_t product = (int64_t) n * (int64_t) q->multiplier;
  const int64_t adjusted = product - (int64_t) (n < 0);
  const int64_t rounded = adjusted + q->rounding;
  /* arithmetic shift of a negative value, spelled out */
  int64_t y = rounded >= 0 ? (int64_t) ((uint64_t) rounded >> q->right_shift) : -(int64_t) (((uint64_t) -(rounded + 1)) >> q->right_shift) - 1;
  if (y < q->output_min_less_zero_point) y = q->output_min_less_zero_point;
  if (y > q->output_max_less_zero_point) y = q->output_max_less_zero_point;
  return (uint8_t) (y + q->output_zero_point);
}

static int fc_valid(const struct qnnp_hip_se_fc* f, uint32_t k, uint32_t n)
{
  return f->w != NULL && f->bias2 != NULL && f->k_pad % 64 == 0 && f->n_pad % 32 == 0 && f->k_pad >= k &&
      f->k_pad <= (QNNP_HIP_SE_MAX_CHANNELS + 63u) / 64u * 64u && f->n_pad >= n;
}

/* out[n] = requantize(bias2[n] + sum_k a'[k] w'(n, k) + row_coeff * sum_k a'[k]) over the fragment image */
static void fully_connected(const struct qnnp_hip_se_fc* f, const uint8_t* a, uint32_t k_total, uint32_t n_total, uint8_t* out)
{
  const uint32_t kblocks = f->k_pad / 32;
  int32_t row_sum = 0;
  for (uint32_t k = 0; k < k_total; k++) row_sum += (int32_t) (int8_t) (a[k] ^ 0x80);
  for (uint32_t n = 0; n < n_total; n++) {
    uint32_t acc = (uint32_t) f->bias2[n] + (uint32_t) f->row_coeff * (uint32_t) row_sum;
    for (uint32_t k = 0; k < k_total; k++) {
      const uint32_t lane = n % 32 + 32 * ((k % 32) / 16);
      const int32_t w = f->w[((((size_t) (n / 32)) * kblocks + k / 32) * 64 + lane) * 16 + k % 16];
      acc += (uint32_t) ((int32_t) (int8_t) (a[k] ^ 0x80) * w);
    }
    out[n] = requantize((int32_t) acc, &f->rq);
  }
}

int qnnp_hip_se_gate_run(const struct qnnp_hip_se_gate_args* a, const char** kernel_name)
{
  if (a == NULL || a->input == NULL || a->gate == NULL || a->table == NULL || (uintptr_t) a->table % 4 != 0 ||
      a->channels == 0 || a->squeeze == 0 || a->channels > QNNP_HIP_SE_MAX_CHANNELS ||
      a->squeeze > QNNP_HIP_SE_MAX_CHANNELS || a->batch > 0x7FFFFFFFu ||
      !fc_valid(&a->fc1, a->channels, a->squeeze) || !fc_valid(&a->fc2, a->squeeze, a->channels)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->pool != 0 && (a->pixels == 0 || a->pixels > 0x7FFFFFFFu / 255u || a->input_stride < a->channels ||
                       (uint64_t) a->batch * a->pixels > 0x7FFFFFFFu)) {
    return QNNP_HIP_EINVAL;
  }
  qnnp_stub_se_last = *a;
  qnnp_stub_se_launches++;
  if (kernel_name != NULL) *kernel_name = a->pool != 0 ? "stub_se_gate_pool" : "stub_se_gate";
  uint8_t* pooled = (uint8_t*) malloc(a->channels);
  uint8_t* hidden = (uint8_t*) malloc(a->squeeze);
  uint8_t* excite = (uint8_t*) malloc(a->channels);
  if (pooled == NULL || hidden == NULL || excite == NULL) abort();
  for (uint64_t i = 0; i < a->batch; i++) {
    for (uint32_t c = 0; c < a->channels; c++) {
      if (a->pool != 0) {
        int32_t sum = a->pool_params.bias;
        for (uint64_t w = 0; w < a->pixels; w++) sum += a->input[(i * a->pixels + w) * a->input_stride + c];
        pooled[c] = avgpool_quantize(sum, &a->pool_params);
      } else {
        pooled[c] = a->input[i * a->channels + c];
      }
    }
    fully_connected(&a->fc1, pooled, a->channels, a->squeeze, hidden);
    fully_connected(&a->fc2, hidden, a->squeeze, a->channels, excite);
    for (uint32_t c = 0; c < a->channels; c++) a->gate[i * a->channels + c] = a->table[excite[c]];
  }
  free(pooled);
  free(hidden);
  free(excite);
  return QNNP_HIP_OK;
}
