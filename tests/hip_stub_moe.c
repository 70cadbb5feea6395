/*
 * hip_stub_moe.c -- TEST INFRASTRUCTURE: the router and combine launches of the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h,
 * hip/f32topk.hip, hip/f32combine.hip) for the host-sanitizer build of moe.c (Makefile target asan-moe), beside
 * tests/hip_stub.c. Each validates its argument block as the device launcher does, keeps it for the test to read, and writes
 * the first and the last element of everything the kernel would write and reads those of everything it would read (the stub's
 * "device" memory is host memory), so ASan sees a span that moe.c got wrong. Nothing is computed.
 */
#include <stdint.h>

#include "hip/qnnp_hip.h"

struct qnnp_hip_topk_router_args qnnp_stub_router_last;
struct qnnp_hip_weighted_combine_args qnnp_stub_combine_last;
unsigned qnnp_stub_router_launches;
unsigned qnnp_stub_combine_launches;
static volatile float g_sink;

int qnnp_hip_topk_router_run(const struct qnnp_hip_topk_router_args* a, const char** kernel_name)
{
  if (a == NULL || a->logits == NULL || a->group_ids == NULL || a->weights == NULL || a->groups == 0 || a->groups > 1024 ||
      a->assignments == 0 || a->assignments > 8 || a->assignments > a->groups || a->first_group >= 0x80000000u ||
      a->logits_stride < a->groups || (uint64_t) a->tokens * a->assignments >= (1u << 20) || a->tokens == 0) {
    return QNNP_HIP_EINVAL;
  }
  qnnp_stub_router_last = *a;
  qnnp_stub_router_launches++;
  if (kernel_name != NULL) *kernel_name = "stub_topk_router";
  const uint64_t slots = (uint64_t) a->tokens * a->assignments;
  g_sink = a->logits[0] + a->logits[(a->tokens - 1) * a->logits_stride + a->groups - 1];
  a->group_ids[0] = a->group_ids[slots - 1] = -(int32_t) a->first_group;
  a->weights[0] = a->weights[slots - 1] = 1.0f;
  return QNNP_HIP_OK;
}

int qnnp_hip_weighted_combine_run(const struct qnnp_hip_weighted_combine_args* a, const char** kernel_name)
{
  if (a == NULL || a->input == NULL || a->weights == NULL || a->group_ids == NULL || a->output == NULL || a->channels == 0 ||
      a->channels >= (1u << 24) || a->assignments == 0 || a->assignments > 8 || a->groups == 0 || a->groups > 1024 ||
      a->input_stride < a->channels || a->output_stride < a->channels ||
      (uint64_t) a->tokens * a->assignments >= (1u << 20) || a->tokens == 0) {
    return QNNP_HIP_EINVAL;
  }
  qnnp_stub_combine_last = *a;
  qnnp_stub_combine_launches++;
  if (kernel_name != NULL) *kernel_name = "stub_weighted_combine";
  const uint64_t rows = (uint64_t) a->tokens * a->assignments;
  g_sink = a->input[0] + a->input[(rows - 1) * a->input_stride + a->channels - 1] + a->weights[0] + a->weights[rows - 1] +
      (float) a->group_ids[0] + (float) a->group_ids[rows - 1];
  a->output[0] = a->output[(a->tokens - 1) * a->output_stride + a->channels - 1] = 0.0f;
  return QNNP_HIP_OK;
}
