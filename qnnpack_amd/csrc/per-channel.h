/*
 * per-channel.h -- what the two per-channel creates (include/qnnpack_gfx950_perchannel.h; convolution.c,
 * fully-connected.c) share: the scale of an output channel, the checks on the caller's array, and the device table of
 * (multiplier, shift) entries the kernels read (hip/requant_pc.h).
 */
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "hip/requant_pc.h"
#include "log.h"
#include "requantization.h"
#include "upload.h"

/* scale_c = (input_scale * kernel_scales[c]) / output_scale: float32, each operation rounded once, this order -- the
 * expression of the per-tensor creates, so equal scales give the per-tensor operator's multiplier and shift */
static inline float qnnp_per_channel_scale(float input_scale, float kernel_scale, float output_scale)
{
  return input_scale * kernel_scale / output_scale;
}

/* index of the first kernel scale that is not a finite number above zero, or `count` */
static inline size_t qnnp_per_channel_first_invalid(const float* kernel_scales, size_t count)
{
  for (size_t c = 0; c < count; c++) {
    if (!(kernel_scales[c] > 0.0f && isnormal(kernel_scales[c]))) return c;
  }
  return count;
}

/* index of the first channel whose scale_c lies outside [2^-32, 1), or `count` */
static inline size_t qnnp_per_channel_first_unsupported(
    float input_scale, const float* kernel_scales, float output_scale, size_t count)
{
  for (size_t c = 0; c < count; c++) {
    const float scale = qnnp_per_channel_scale(input_scale, kernel_scales[c], output_scale);
    if (!(scale >= 0x1.0p-32f && scale < 1.0f)) return c;
  }
  return count;
}

/* The table as the kernels index it: `groups` runs of `group_pad` entries, entry g * group_pad + oc for output channel
 * g * group_channels + oc, the rest of each run a harmless valid entry (multiplier 2^30, shift 0). `table` holds
 * groups * group_pad entries. */
static inline void qnnp_per_channel_fill_table(
    struct qnnp_requant_pc_entry* table, uint32_t groups, size_t group_channels, uint32_t group_pad,
    float input_scale, const float* kernel_scales, float output_scale)
{
  for (uint32_t g = 0; g < groups; g++) {
    for (uint32_t oc = 0; oc < group_pad; oc++) {
      struct qnnp_requant_pc_entry* e = &table[(size_t) g * group_pad + oc];
      e->multiplier = QNNP_REQUANT_PC_PAD_MULTIPLIER;
      e->shift = 0;
      if (oc < group_channels) {
        const struct qnnp_hip_requant rq = qnnp_compute_requant(
            qnnp_per_channel_scale(input_scale, kernel_scales[g * group_channels + oc], output_scale), 0, 0, 255);
        e->multiplier = rq.multiplier;
        e->shift = rq.shift;
      }
    }
  }
}

/* the device copy of that table, or NULL (logged) */
static inline void* qnnp_per_channel_upload_table(
    uint32_t groups, size_t group_channels, uint32_t group_pad, float input_scale, const float* kernel_scales,
    float output_scale)
{
  const size_t bytes = sizeof(struct qnnp_requant_pc_entry) * groups * group_pad;
  struct qnnp_requant_pc_entry* host = (struct qnnp_requant_pc_entry*) malloc(bytes);
  if (host == NULL) {
    qnnp_log_error("out of host memory: %zu bytes for the per-channel requantization table", bytes);
    return NULL;
  }
  qnnp_per_channel_fill_table(host, groups, group_channels, group_pad, input_scale, kernel_scales, output_scale);
  void* device = qnnp_upload(host, bytes);
  free(host);
  if (device == NULL) {
    qnnp_log_error("device allocation or upload failed: %zu bytes of per-channel requantization table", bytes);
  }
  return device;
}
