/*
 * perchannel_stub_probe.c -- TEST INFRASTRUCTURE: linked with the product's host code and tests/hip_stub.c into
 * libqnnpack_perchannel_stub.so (Makefile target stub-perchannel) for tests/test_perchannel_host.py. The stub's "device"
 * memory is host memory, so the table a per-channel create uploaded can be read back as the stub received it.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <qnnpack.h>

#include "hip/requant_pc.h"
#include "operator.h"

/* 1 and the operator's facts, or 0 for an operator without per-channel scales. `pad`: entries per group (n_pad), or the
 * whole table's (c_pad) for a depthwise operator, whose table is one run. */
int qnnp_stub_per_channel_info(qnnp_operator_t op, uint32_t* runs, uint32_t* pad, int32_t* multiplier_shift_pairs, size_t capacity)
{
  if (op == NULL || !op->per_channel || op->d_requant_pc == NULL) return 0;
  const int depthwise = op->ukernel_type == qnnp_ukernel_type_dwconv;
  *runs = depthwise ? 1u : op->groups;
  *pad = depthwise ? op->c_pad : op->n_pad;
  const size_t entries = (size_t) *runs * *pad;
  if (entries <= capacity) memcpy(multiplier_shift_pairs, op->d_requant_pc, entries * sizeof(struct qnnp_requant_pc_entry));
  return 1;
}

/* the requantization block the operator keeps beside the table: zero point and clamp */
void qnnp_stub_operator_clamp(qnnp_operator_t op, int32_t* zero_point, int32_t* min_less_zp, int32_t* max_less_zp)
{
  *zero_point = op->requant.output_zero_point;
  *min_less_zp = op->requant.output_min_less_zero_point;
  *max_less_zp = op->requant.output_max_less_zero_point;
}
