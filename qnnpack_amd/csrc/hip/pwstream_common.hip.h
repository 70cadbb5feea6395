/*
 * pwstream_common.hip.h -- what the streaming kernel units share (q8pwstream.hip, q8pwstaged.hip, q8pwlongk.hip, q8pwgw.hip,
 * q8convc3s.hip) and what their planner (q8pwconv.hip) sizes launches with: the workgroup shape and LDS budgets, the
 * residency the kernels are compiled for, the write-once store, the staged kernels' copy-out, and the launch helpers.
 * HIP-internal; everything here has internal linkage.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "device_ops.hip.h"
#include "igemm_epilogue.hip.h"
#include "igemm_params.h"
#include "per_device.h"
#include "requant.hip.h"

namespace qnnp {

namespace {

/* A store of whole lines that are written exactly once (a wave's contiguous run of an output block) carries the
 * streaming hint: layer 4 (112x112x16 -> 96, 154 MB of output) 39 -> 30.5 us, layer 7 17.6 -> 13.9, same box. The hint
 * on anything that is touched again -- activation loads with column overlaps or re-read per channel column, 4-byte
 * stores that complete a line over several instructions -- costs 25-120 %.
 * `streaming` = IgemmParams::stream_out (wave-uniform): callers that chain operators turn the hint off -- the consumer of
 * a streamed tensor finds none of it in the last-level cache (whole network 214 k -> 212 k images/s with it, the
 * per-layer sweep 300 k -> 313 k). */
__device__ __forceinline__ void store16_once(uint8_t* dst, const uint4& v, uint32_t streaming)
{
  typedef int nt_v4i __attribute__((ext_vector_type(4)));
  const nt_v4i x = {static_cast<int>(v.x), static_cast<int>(v.y), static_cast<int>(v.z), static_cast<int>(v.w)};
  if (streaming) {
    // (as an instruction: with the builtin, hipcc hoists / sinks the two stores of this branch into one and drops the hint)
    asm volatile("global_store_dwordx4 %0, %1, off nt" : : "v"(dst), "v"(x) : "memory");
  } else {
    *reinterpret_cast<nt_v4i*>(dst) = x;
  }
}

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr uint32_t kFlip = 0x80808080u;
constexpr uint32_t kMaxLds = 64 * 1024;     // weights + bias: two workgroups per CU

/* A wave's staged 32-row output block (LDS image `stage`) -> global memory. Dense rows and the whole N: the block
 * is one contiguous run, 1 KiB per store instruction. Otherwise row chunks: the image has 2^log_cpr 16-byte pieces
 * per row (pitch 16 << log_cpr), of which the first cw bytes exist; consecutive lanes take consecutive pieces of a
 * row. c0 = first channel of the chunk. */
/* dense8 (round 4): dense rows whose length is a multiple of 8 but not of 16 bytes (24-channel MobileNet layers): the
 * block is still ONE contiguous, 16-byte aligned run in memory (32 rows x n bytes), only the image keeps its 16-byte
 * pitch; a lane gathers its 16 output bytes as two 8-byte halves, which may sit in two image rows. Those layers took the
 * direct-store kernel before: 4-byte stores, 3.9-4.3 TB/s where their 16-channel neighbours stream 4.9. */
/* TAB: every piece goes through the LDS copy `lut` of the output table (igemm_params.h, lut_lookup.hip.h) on its way out,
 * in all three modes. */
__device__ __forceinline__ uint4 lut_u8x16(const uint8_t* lut, const uint4& v)
{
  return make_uint4(lut_u8x4_at(lut, v.x), lut_u8x4_at(lut, v.y), lut_u8x4_at(lut, v.z), lut_u8x4_at(lut, v.w));
}

template <bool RES = false, bool TAB = false>
__device__ __forceinline__ void stream_copy_out(
    const uint8_t* stage, bool whole_dense, uint32_t log_cpr, uint32_t unit, uint32_t c0, uint32_t cw,
    const IgemmParams& p, uint32_t lane, bool dense8 = false, const uint8_t* lut = nullptr)
{
  static_assert(!(RES && TAB), "a residual add and an output table are never attached together");
  const uint32_t rows_here = min(32u, p.rows - unit * 32u);
  if (dense8) {
    const uint32_t bytes = rows_here * p.n;                  // a multiple of 8
    const uint64_t block_ofs = static_cast<uint64_t>(unit) * 32u * p.n;
    uint8_t* blk = p.output + block_ofs;
    const uint32_t pitch = 16u << log_cpr;
    for (uint32_t o = lane * 16; o < bytes; o += 1024) {
      const uint32_t r = __umulhi(o, p.tiles_n_magic);       // o / n (launcher: reciprocal_floor_plus1(n); o < 2^13)
      const uint32_t c = o - r * p.n;                        // multiple of 8
      const uint2 lo = *reinterpret_cast<const uint2*>(stage + r * pitch + c);
      const bool wrap = c + 8 >= p.n;                        // the second half starts the next row
      const uint2 hi = *reinterpret_cast<const uint2*>(stage + (wrap ? (r + 1) * pitch : r * pitch + c + 8));
      uint4 v = make_uint4(lo.x, lo.y, hi.x, hi.y);
      if constexpr (TAB) v = lut_u8x16(lut, v);
      if constexpr (RES) {
        const uint8_t* res = p.residual + block_ofs + o;
        if (o + 16 <= bytes) {
          const uint4 q = *reinterpret_cast<const uint4*>(res);
          v = make_uint4(add_quantize4(q.x, v.x, p.add), add_quantize4(q.y, v.y, p.add), add_quantize4(q.z, v.z, p.add), add_quantize4(q.w, v.w, p.add));
        } else {
          const uint2 q = *reinterpret_cast<const uint2*>(res);
          v.x = add_quantize4(q.x, v.x, p.add);
          v.y = add_quantize4(q.y, v.y, p.add);
        }
      }
      if (o + 16 <= bytes) store16_once(blk + o, v, p.stream_out);
      else *reinterpret_cast<uint2*>(blk + o) = make_uint2(v.x, v.y);       // (an odd number of rows: the last 8 bytes)
    }
    return;
  }
  if constexpr (RES) {
    // fused residual add: the same walk, each 16-byte piece summed with the residual's bytes of the same pixel and
    // channels (launcher: residual rows are laid out like the output rows, 16-byte aligned)
    const uint64_t block_ofs = static_cast<uint64_t>(unit) * 32u * p.output_stride + c0;
    const uint8_t* res = p.residual + block_ofs;
    uint8_t* blk = p.output + block_ofs;
    if (whole_dense) {
      const uint32_t bytes = rows_here * p.n;
      for (uint32_t o = lane * 16; o < bytes; o += 1024) {
        const uint4 r = *reinterpret_cast<const uint4*>(res + o);
        const uint4 v = *reinterpret_cast<const uint4*>(stage + o);
        store16_once(blk + o, make_uint4(add_quantize4(r.x, v.x, p.add), add_quantize4(r.y, v.y, p.add),
                                         add_quantize4(r.z, v.z, p.add), add_quantize4(r.w, v.w, p.add)), p.stream_out);
      }
    } else {
      const uint32_t pieces = 32u << log_cpr;
      for (uint32_t q = lane; q < pieces; q += 64) {
        const uint32_t rr = q >> log_cpr;
        const uint32_t cb = (q - (rr << log_cpr)) * 16u;
        if (rr < rows_here && cb < cw) {
          const uint64_t o = static_cast<uint64_t>(rr) * p.output_stride + cb;
          const uint4 r = *reinterpret_cast<const uint4*>(res + o);
          const uint4 v = *reinterpret_cast<const uint4*>(stage + q * 16u);
          store16_once(blk + o, make_uint4(add_quantize4(r.x, v.x, p.add), add_quantize4(r.y, v.y, p.add),
                                           add_quantize4(r.z, v.z, p.add), add_quantize4(r.w, v.w, p.add)), p.stream_out);
        }
      }
    }
    return;
  }
  if (whole_dense) {
    const uint32_t bytes = rows_here * p.n;
    uint8_t* blk = p.output + static_cast<uint64_t>(unit) * 32u * p.n;
    for (uint32_t o = lane * 16; o < bytes; o += 2048) {
      uint4 v0 = *reinterpret_cast<const uint4*>(stage + o);
      const bool two = o + 1024 < bytes;
      uint4 v1 = *reinterpret_cast<const uint4*>(stage + (two ? o + 1024 : o));
      if constexpr (TAB) { v0 = lut_u8x16(lut, v0); v1 = lut_u8x16(lut, v1); }
      store16_once(blk + o, v0, p.stream_out);
      if (two) store16_once(blk + o + 1024, v1, p.stream_out);
    }
  } else {
    const uint32_t pieces = 32u << log_cpr;
    uint8_t* blk = p.output + static_cast<uint64_t>(unit) * 32u * p.output_stride + c0;
    for (uint32_t q = lane; q < pieces; q += 64) {
      const uint32_t r = q >> log_cpr;
      const uint32_t cb = (q - (r << log_cpr)) * 16u;
      uint4 v = *reinterpret_cast<const uint4*>(stage + q * 16u);
      if constexpr (TAB) v = lut_u8x16(lut, v);
      if (r < rows_here && cb < cw) {
        store16_once(blk + static_cast<uint64_t>(r) * p.output_stride + cb, v, p.stream_out);
      }
    }
  }
}

/* resident workgroups per CU (= waves per SIMD) the staged kernel is compiled for, i.e. what its register need
 * allows (54 / 66 / 74 / 79 / 88 / 98 / 107 / 118 VGPRs for 1..8 K blocks, per requantization flavour, since the bias
 * is no longer carried from block to block; 72 ... 134 before -- one more resident wave per SIMD, which the
 * registers would now allow, measured level or slightly behind: layer 3 17.2 -> 17.7 us, layer 21 9.9 -> 10.7). A wave of
 * this kernel spends most of a unit's time waiting -- the next rows, the previous unit's store acknowledgements --
 * and residency is what hides that. */
constexpr int staged_waves(int kb) { return kb <= 1 ? 7 : (kb == 2 ? 6 : (kb <= 4 ? 5 : (kb <= 7 ? 4 : 3))); }

/* the long-K kernel's LDS budget and the residency it is compiled for (q8pwlongk.hip) */
constexpr uint32_t kMaxLdsLongK = 96 * 1024;
constexpr int longk_waves(int kbmax) { return kbmax <= 12 ? 4 : (kbmax <= 20 ? 3 : 2); }

constexpr uint32_t kTableLds = 256;          // the table flavours' copy of the output table, behind everything else in LDS

/* residency as the planners size it: what the registers allow, or what `lds_bytes` per workgroup leaves of a CU */
inline uint32_t resident_per_cu(uint32_t by_registers, uint32_t lds_bytes)
{
  const uint32_t by_lds = lds_bytes > 0 ? (160u * 1024u) / lds_bytes : by_registers;
  return by_lds < by_registers ? (by_lds > 0 ? by_lds : 1u) : by_registers;
}

/* persistent workgroups: the resident set (spread over `nsplit` workgroup columns), or fewer when every wave has a unit */
inline uint32_t persistent_grid(const IgemmParams& p, uint32_t per_cu, uint32_t nsplit = 1)
{
  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t resident = (p.cu_count * per_cu + nsplit - 1) / nsplit;
  const uint32_t needed = (units + kWaves - 1) / kWaves;
  return resident < needed ? resident : needed;
}

/* a run-time K block count in 1 .. 8 as a compile-time constant: f(std::integral_constant<int, KB>) */
template <class F>
int with_kb(uint32_t kb, F&& f)
{
  switch (kb) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

/* the launch a plan describes, of the instantiation its unit's switch picked; max_lds: the kernel's dynamic-LDS budget
 * (0: it has no dynamic LDS) */
template <auto Kernel, class... Args>
int launch_planned(uint32_t max_lds, const PwPlan& plan, hipStream_t stream, const Args&... args)
{
  if (max_lds != 0) allow_dynamic_lds<Kernel>(static_cast<int>(max_lds));
  hipLaunchKernelGGL(Kernel, dim3(plan.grid_x, plan.grid_y), dim3(kThreads), plan.lds_bytes, stream, args...);
  return launch_status();
}

/* measurement builds: QNNP_PW_ABL switches parts of the stream and staged kernels off through izp_fill, which they do not
 * otherwise read */
inline IgemmParams with_ablation_bits(const IgemmParams& p)
{
  IgemmParams pa = p;
#ifdef QNNP_ENABLE_ABLATION
  pa.izp_fill = 0;
  if (const char* env = getenv("QNNP_PW_ABL")) pa.izp_fill = static_cast<uint32_t>(atoi(env));
#endif
  return pa;
}

}  // namespace

}  // namespace qnnp
