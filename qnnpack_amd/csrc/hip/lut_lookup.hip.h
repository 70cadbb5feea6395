/*
 * lut_lookup.hip.h -- the byte lookup of the table kernels (x8lut.hip) and of the table flavours of the convolution
 * kernels (qnnpack_gfx950_output_table.h: q8pwconv.hip's kernel units, q8dwcol.hip, q8dwcol5.hip): the 256-byte table in LDS, one LDS
 * byte read (ds_read_u8) per byte, four of them packed into each dword.
 *
 * Two ways to stage the table:
 *   stage_table       one copy per workgroup and ONE workgroup barrier: every lane of the workgroup must call it.
 *   stage_table_wave  no barrier: for kernels whose waves leave early or never meet (the depthwise column walks, the
 *                     one-wave-per-block pointwise kernel). EVERY wave writes the whole table -- 64 lanes, one dword each
 *                     -- and reads it only behind its own writes. A wave's LDS operations are performed in the order it
 *                     issues them, so a wavefront-scope fence -- no instruction, only an order the compiler has to keep --
 *                     is all that stands between its 64 dword writes and its byte reads. The waves of a workgroup write
 *                     the SAME 256 bytes to the SAME place: whichever wave's write a byte read meets, behind the reader's
 *                     own, it finds the value the reader wrote. One copy per workgroup therefore serves as a copy per wave
 *                     would, at a constant LDS address (no per-wave base in a register) and a quarter of the LDS.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace qnnp {

/* the workgroup's copy of the table; every lane of the workgroup must call this (one barrier) */
__device__ __forceinline__ void stage_table(uint8_t (&lds)[256], const uint8_t* table)
{
  if (threadIdx.x < 64u) {
    reinterpret_cast<uint32_t*>(lds)[threadIdx.x] = reinterpret_cast<const uint32_t*>(table)[threadIdx.x];
  }
  __syncthreads();
}

/* the calling wave's writes of the whole table: `dword` is lane l's dword l of the table, requested by the caller as early
 * as it likes (table_dword); every lane of the wave must call this, and every wave that reads `lds` must have called it */
__device__ __forceinline__ uint32_t table_dword(const uint8_t* table)
{
  return reinterpret_cast<const uint32_t*>(table)[threadIdx.x & 63u];
}
__device__ __forceinline__ void stage_table_wave(uint8_t (&lds)[256], uint32_t dword)
{
  reinterpret_cast<uint32_t*>(lds)[threadIdx.x & 63u] = dword;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

/* table[b] for each of the four bytes b of v */
__device__ __forceinline__ uint32_t lut_u8x4(const uint8_t (&lds)[256], uint32_t v)
{
  const uint32_t b0 = lds[v & 0xFFu], b1 = lds[(v >> 8) & 0xFFu], b2 = lds[(v >> 16) & 0xFFu], b3 = lds[v >> 24];
  return b0 | b1 << 8 | b2 << 16 | b3 << 24;
}

/* the same through a pointer to the copy (the epilogues shared by several kernels take it that way) */
__device__ __forceinline__ uint32_t lut_u8x4_at(const uint8_t* lds, uint32_t v)
{
  return lut_u8x4(*reinterpret_cast<const uint8_t (*)[256]>(lds), v);
}

}  // namespace qnnp
