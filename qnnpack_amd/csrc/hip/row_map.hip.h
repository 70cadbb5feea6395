/*
 * row_map.hip.h -- the row-to-item map of the byte-moving row kernels, shared by channel shuffle and clamp
 * (x8shuffle.hip) and the byte lookup table (x8lut.hip).
 *
 * Several lanes serve one pixel row when it is short, several workgroups when it is long: a lane's row and item come
 * from one magic-reciprocal divide of its thread index, no per-element division.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"

namespace qnnp {

constexpr int kThreads = 256;
constexpr uint32_t kMaxGridY = 65535;

/* `items` work items in each of `rows` rows. items <= kThreads: rows_per_block rows share a workgroup (lane ->
 * (row, item) by one magic divide); otherwise one row spans gridDim.x workgroups. Grid y walks the row groups. */
struct RowMap {
  uint32_t rows;
  uint32_t items;
  uint32_t items_inv;       // reciprocal_ceil(items) when items <= kThreads
  uint32_t rows_per_block;
  uint32_t groups;          // ceil(rows / rows_per_block)
};

inline RowMap row_map(uint32_t rows, uint32_t items, dim3& grid)
{
  RowMap m;
  m.rows = rows;
  m.items = items;
  const bool shared = items <= static_cast<uint32_t>(kThreads);
  m.items_inv = shared ? reciprocal_ceil(items) : 0u;
  m.rows_per_block = shared ? kThreads / items : 1u;
  m.groups = static_cast<uint32_t>((static_cast<uint64_t>(rows) + m.rows_per_block - 1) / m.rows_per_block);
  const uint32_t gx = shared ? 1u : (items + kThreads - 1) / kThreads;
  grid = dim3(gx, m.groups < kMaxGridY ? m.groups : kMaxGridY);
  return m;
}

/* this lane's row within its group and item within the row; false: the lane has none */
__device__ __forceinline__ bool row_item(const RowMap& m, uint32_t& rl, uint32_t& k)
{
  if (m.items <= static_cast<uint32_t>(kThreads)) {
    rl = div_magic(threadIdx.x, m.items_inv);
    k = threadIdx.x - rl * m.items;
    return rl < m.rows_per_block;
  }
  rl = 0;
  k = blockIdx.x * kThreads + threadIdx.x;
  return k < m.items;
}

inline bool aligned(uint64_t v, uint64_t a) { return v % a == 0; }
inline uint64_t address(const void* p) { return static_cast<uint64_t>(reinterpret_cast<uintptr_t>(p)); }

}  // namespace qnnp
