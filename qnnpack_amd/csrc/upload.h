/*
 * upload.h -- host-to-device copies of the images and tables an operator owns. Every create-time image goes through
 * qnnp_upload, every grow-only setup-time table through qnnp_upload_table; both leave nothing allocated that the
 * operator does not hold, so a failure needs no clean-up beyond what qnnp_delete_operator does.
 */
#pragma once

#include <stddef.h>

#include "hip/qnnp_hip.h"

/* device copy of `bytes` of host memory; NULL, with nothing allocated, on failure */
static inline void* qnnp_upload(const void* host, size_t bytes)
{
  void* d = qnnp_hip_alloc(bytes);
  if (d != NULL && qnnp_hip_h2d(d, host, bytes, 0) != QNNP_HIP_OK) {
    qnnp_hip_free(d);
    d = NULL;
  }
  return d;
}

/* Uploads `bytes` of `host` into the grow-only device table *table, which is first replaced by `alloc_bytes` of fresh
 * device memory when *capacity is below `entries` (*capacity then becomes `entries`). Returns 0 on failure; *table
 * is NULL (and *capacity 0) when it was the allocation that failed. */
static inline int qnnp_upload_table(void** table, size_t* capacity, size_t entries, size_t alloc_bytes, const void* host,
                                    size_t bytes)
{
  if (*capacity < entries) {
    qnnp_hip_free(*table);
    *capacity = 0;
    *table = qnnp_hip_alloc(alloc_bytes);
    if (*table == NULL) return 0;
    *capacity = entries;
  }
  return qnnp_hip_h2d(*table, host, bytes, 0) == QNNP_HIP_OK;
}
