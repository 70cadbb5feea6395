/*
 * q8dwlds.hip -- depthwise kernel A: the LDS-tiled kernel, q8_dwconv_lds_kernel<KH, KW, VECL, DW1> (3x3 and 5x5 windows,
 * any stride and dilation, C % 4 == 0, dword-aligned tensors). One family, no device code shared with another unit.
 * Plan and launch: dwlds_plan / dwlds_launch (dwconv_params.h); q8dwconv.hip decides when it runs ("dwconv_kernel" 2
 * forces it).
 *
 *   workgroup = one image x a band of output rows x all output columns x a channel
 *   slab. The input band (with halo, padding materialised as the zero point) is
 *   staged into LDS with 16-byte (or 4-byte) coalesced loads along C, laid out
 *   [row][4-channel group][column] so an output's taps are immediate offsets apart; each thread
 *   owns one 4-channel group (its tap weights live in registers as int16 pairs)
 *   and walks output positions, reading dwords from LDS, pairing taps with
 *   v_perm_b32 and accumulating two taps per v_dot2_i32_i16; one coalesced dword
 *   store of 4 requantized channels per position.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "device_ops.hip.h"
#include "dwconv_params.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "requant.hip.h"

namespace {

using qnnp::DwParams;

typedef short v2s __attribute__((ext_vector_type(2)));

// --------------------------------------------------------------------------
// Kernel A: LDS-tiled
// --------------------------------------------------------------------------
#ifndef QNNP_DW_THREADS
#define QNNP_DW_THREADS 512
#endif
constexpr int kDwThreads = QNNP_DW_THREADS;

/*
 * LDS image of the staged band: [input row][4-channel group][column] dwords, i.e. for one row and one
 * 4-channel group the columns are consecutive dwords. The KW taps of an output are then 4*dw bytes apart
 * (immediate ds_read offsets when dw == 1) and only one address per kernel row is computed.
 * `p.PP` = dwords per (row, group) line, padded so that consecutive groups start on spread-out banks.
 */
template <int KH, int KW, int VECL, bool DW1>
__global__ __launch_bounds__(kDwThreads)
void q8_dwconv_lds_kernel(const DwParams p)
{
  constexpr int TAPS = KH * KW;
  constexpr int PAIRS = (TAPS + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t tile[];   // [IR][CS/4][PP] dwords

  const uint32_t tid = threadIdx.x;
  QNNP_DW_TRACE(p, 0);
  // block -> (image, band, slab); slab fastest so that the blocks sharing input
  // cache lines (same pixels, neighbouring channel slabs) are dispatched together
  // XCD-aware bijective remap (hardware: block b -> XCD b % 8): consecutive logical ids -- the channel slabs
  // of one band, which read the same cache lines -- land on the same XCD / L2
  uint32_t b;
  {
    const uint32_t nwg = gridDim.x;
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t idx = blockIdx.x >> 3;
    const uint32_t q = nwg >> 3, r = nwg & 7u;
    b = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const uint32_t slab = b % p.slabs; b /= p.slabs;
  const uint32_t band = b % p.bands;
  const uint32_t n = b / p.bands;
  const uint32_t c0 = slab * p.CS;
  const uint32_t oy0 = band * p.TOH;
  const uint32_t toh = min(p.TOH, p.OH - oy0);
  const uint32_t ir = (toh - 1) * p.sh + (KH - 1) * p.dh + 1;   // rows actually needed
  const uint32_t q4 = p.CS / 4;                 // 4-channel groups in the slab
  const uint32_t line_bytes = p.PP * 4;         // one (row, group) line
  const uint32_t row_bytes = q4 * line_bytes;

  // ---- stage the input band: coalesced VECL-byte vectors along C, scattered into the group planes ----
  // Batches of kStageBatch vectors per thread: every global load of a batch is issued before the first
  // LDS write, so a thread keeps several loads in flight (a load -> write -> load loop is latency-bound).
  {
    constexpr int kStageBatch = (VECL == 16) ? 4 : 8;
    const uint32_t vpp = p.CS / VECL;                 // vectors per pixel
    const uint32_t nvec = ir * p.IC * vpp;
    const int32_t iy_base = static_cast<int32_t>(oy0 * p.sh) - static_cast<int32_t>(p.pad_top);
    const int32_t ix_base = -static_cast<int32_t>(p.pad_left);
    const uint8_t* img = p.input + static_cast<uint64_t>(n) * p.H * p.W * p.in_stride + c0;
    const uint32_t fill = p.izp * 0x01010101u;
    // incremental (vector-in-pixel, column, row) walk: no divisions in the loop
    uint32_t cv = tid % vpp;
    uint32_t px = tid / vpp;
    uint32_t ixl = px % p.IC;
    uint32_t iyl = px / p.IC;
    const uint32_t d_cv = kDwThreads % vpp;
    const uint32_t d_px = kDwThreads / vpp;
    const uint32_t d_ix = d_px % p.IC;
    const uint32_t d_iy = d_px / p.IC;
    for (uint32_t v0 = tid; v0 < nvec; v0 += kDwThreads * kStageBatch) {
      uint32_t dst[kStageBatch];
      bool live[kStageBatch];
      uint4 val16[VECL == 16 ? kStageBatch : 1];
      uint32_t val4[VECL == 16 ? 1 : kStageBatch];
#pragma unroll
      for (int u = 0; u < kStageBatch; u++) {
        live[u] = v0 + u * kDwThreads < nvec;
        const int32_t iy = iy_base + static_cast<int32_t>(iyl);
        const int32_t ix = ix_base + static_cast<int32_t>(ixl);
        const bool inb = live[u] && iy >= 0 && iy < static_cast<int32_t>(p.H) && ix >= 0 && ix < static_cast<int32_t>(p.W);
        dst[u] = iyl * row_bytes + (cv * (VECL / 4)) * line_bytes + ixl * 4;
        const uint8_t* src =
            img + (static_cast<uint64_t>(static_cast<uint32_t>(iy)) * p.W + static_cast<uint32_t>(ix)) * p.in_stride + cv * VECL;
        if constexpr (VECL == 16) {
          val16[u] = make_uint4(fill, fill, fill, fill);
          if (inb) val16[u] = *reinterpret_cast<const uint4*>(src);
        } else {
          val4[u] = fill;
          if (inb) val4[u] = *reinterpret_cast<const uint32_t*>(src);
        }
        // advance by kDwThreads vectors
        cv += d_cv;
        uint32_t carry = 0;
        if (cv >= vpp) { cv -= vpp; carry = 1; }
        ixl += d_ix + carry;
        iyl += d_iy;
        if (ixl >= p.IC) { ixl -= p.IC; iyl += 1; }
      }
#pragma unroll
      for (int u = 0; u < kStageBatch; u++) {
        if (live[u]) {
          uint8_t* d = tile + dst[u];
          if constexpr (VECL == 16) {
            *reinterpret_cast<uint32_t*>(d) = val16[u].x;
            *reinterpret_cast<uint32_t*>(d + line_bytes) = val16[u].y;
            *reinterpret_cast<uint32_t*>(d + 2 * line_bytes) = val16[u].z;
            *reinterpret_cast<uint32_t*>(d + 3 * line_bytes) = val16[u].w;
          } else {
            *reinterpret_cast<uint32_t*>(d) = val4[u];
          }
        }
      }
    }
  }

  // ---- per-thread channel group: weights as (tap 2i, tap 2i+1) int16 pairs ----
  const uint32_t nslots = kDwThreads / q4;      // positions processed concurrently
  const uint32_t c4 = tid % q4;
  const uint32_t slot = tid / q4;
  const bool active = slot < nslots;
  const uint32_t cg = c0 + c4 * 4;              // first global channel of this thread

  uint32_t wpair[PAIRS][4];
  int32_t bias[4];
  if (active) {
#pragma unroll
    for (int i = 0; i < PAIRS; i++) {
      const uint2 lo = *reinterpret_cast<const uint2*>(p.wadj + (2 * i) * p.c_pad + cg);   // 4 x int16
      uint2 hi = make_uint2(0u, 0u);
      if (2 * i + 1 < TAPS) hi = *reinterpret_cast<const uint2*>(p.wadj + (2 * i + 1) * p.c_pad + cg);
      wpair[i][0] = (lo.x & 0xFFFFu) | (hi.x << 16);
      wpair[i][1] = (lo.x >> 16) | (hi.x & 0xFFFF0000u);
      wpair[i][2] = (lo.y & 0xFFFFu) | (hi.y << 16);
      wpair[i][3] = (lo.y >> 16) | (hi.y & 0xFFFF0000u);
    }
    const int4 bv = *reinterpret_cast<const int4*>(p.bias1 + cg);
    bias[0] = bv.x; bias[1] = bv.y; bias[2] = bv.z; bias[3] = bv.w;
  }

  QNNP_DW_TRACE(p, 1);
  __syncthreads();
  QNNP_DW_TRACE(p, 2);
  if (!active) return;

  const uint32_t npos = toh * p.OW;
  uint8_t* out_ptr = p.output + (static_cast<uint64_t>(n) * p.OH + oy0) * p.OW * p.out_stride + cg +
                     static_cast<uint64_t>(slot) * p.out_stride;
  const uint64_t out_step = static_cast<uint64_t>(nslots) * p.out_stride;
  // incremental (row, column) walk over this thread's positions slot, slot + nslots, ...
  uint32_t ox = slot % p.OW;
  uint32_t oyl = slot / p.OW;
  const uint32_t d_ox = nslots % p.OW;
  const uint32_t d_oy = nslots / p.OW;
  const uint32_t tap_row_bytes = p.dh * row_bytes;
  const uint32_t tap_col_bytes = p.dw * 4;
  // the requantization flavour (shift == 0? clamp == [0,255]?) is chosen once, outside the position loop
  // the LDS address of a position's first tap walks along with (ox, oyl): no multiplies inside the loop
  uint32_t base_off = (oyl * p.sh) * row_bytes + c4 * line_bytes + (ox * p.sw) * 4;
  const uint32_t d_base = (d_oy * p.sh) * row_bytes + (d_ox * p.sw) * 4;
  const uint32_t wrap_base = p.sh * row_bytes - (p.OW * p.sw) * 4;      // one row down, OW columns back
  qnnp::requant_dispatch_ofs(p.rq, [&](auto shift0, auto full) {
    // the offset rounding sequences (requant.hip.h) take accumulator + 2^31: folded into the bias, once per thread
#pragma unroll
    for (int c = 0; c < 4; c++) bias[c] = qnnp::with_rq_offset<decltype(shift0)::value>(bias[c]);
    for (uint32_t pos = slot; pos < npos; pos += nslots) {
      const uint8_t* base = tile + base_off;
      uint32_t in[TAPS];
#pragma unroll
      for (int ky = 0; ky < KH; ky++) {
        const uint8_t* row = base + ky * tap_row_bytes;
#pragma unroll
        for (int kx = 0; kx < KW; kx++) {
          if constexpr (DW1) {
            in[ky * KW + kx] = *reinterpret_cast<const uint32_t*>(row + kx * 4);          // immediate offset
          } else {
            in[ky * KW + kx] = *reinterpret_cast<const uint32_t*>(row + kx * tap_col_bytes);
          }
        }
      }
      int32_t acc0 = bias[0], acc1 = bias[1], acc2 = bias[2], acc3 = bias[3];
#pragma unroll
      for (int i = 0; i < PAIRS; i++) {
        const uint32_t in0 = in[2 * i];
        const uint32_t in1 = (2 * i + 1 < TAPS) ? in[2 * i + 1] : 0u;
        // v_perm_b32: result bytes {in0.c, 0, in1.c, 0} = the two taps of channel c as int16 x2
        const uint32_t p0 = __builtin_amdgcn_perm(in1, in0, 0x0c040c00u);
        const uint32_t p1 = __builtin_amdgcn_perm(in1, in0, 0x0c050c01u);
        const uint32_t p2 = __builtin_amdgcn_perm(in1, in0, 0x0c060c02u);
        const uint32_t p3 = __builtin_amdgcn_perm(in1, in0, 0x0c070c03u);
        acc0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, p0), __builtin_bit_cast(v2s, wpair[i][0]), acc0, false);
        acc1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, p1), __builtin_bit_cast(v2s, wpair[i][1]), acc1, false);
        acc2 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, p2), __builtin_bit_cast(v2s, wpair[i][2]), acc2, false);
        acc3 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, p3), __builtin_bit_cast(v2s, wpair[i][3]), acc3, false);
      }
      const uint32_t packed = qnnp::q31_requantize_pack4<decltype(shift0)::value, decltype(full)::value>(
          acc0, acc1, acc2, acc3, p.rq);
      *reinterpret_cast<uint32_t*>(out_ptr) = packed;
      out_ptr += out_step;
      ox += d_ox;
      base_off += d_base;
      if (ox >= p.OW) { ox -= p.OW; base_off += wrap_base; }
    }
  });
  QNNP_DW_TRACE(p, 3);
  QNNP_DW_TRACE(p, 4);
  QNNP_DW_TRACE(p, 5);
}

constexpr uint32_t kDwLdsBudgetDefault = 48 * 1024;   // bytes per workgroup (3 workgroups per CU)

// measurement knob, read once: LDS budget per workgroup of the LDS-tiled kernel in KiB
uint32_t lds_budget()
{
  static const uint32_t budget = [] {
    if (const char* env = getenv("QNNP_GFX950_DW_LDS_KB")) {
      const int kb = atoi(env);
      if (kb >= 4 && kb <= 64) return static_cast<uint32_t>(kb) * 1024u;
    }
    return kDwLdsBudgetDefault;
  }();
  return budget;
}

template <int KH, int KW>
int launch_lds(const DwParams& p, bool vec16, hipStream_t stream)
{
  const uint32_t blocks = p.batch * p.bands * p.slabs;
  const size_t lds_bytes = static_cast<size_t>(p.IR) * (p.CS / 4) * p.PP * 4;
  const bool dw1 = p.dw == 1;
#define QNNP_DW_LAUNCH(V, D) \
  hipLaunchKernelGGL((q8_dwconv_lds_kernel<KH, KW, V, D>), dim3(blocks), dim3(kDwThreads), lds_bytes, stream, p)
  if (vec16) {
    if (dw1) QNNP_DW_LAUNCH(16, true); else QNNP_DW_LAUNCH(16, false);
  } else {
    if (dw1) QNNP_DW_LAUNCH(4, true); else QNNP_DW_LAUNCH(4, false);
  }
#undef QNNP_DW_LAUNCH
  return qnnp::launch_status();
}

}  // namespace

namespace qnnp {

// Pick slab width / band height for kernel A. Returns false if the shape does not fit.
bool dwlds_plan(DwParams& p)
{
  const uint32_t budget = lds_budget();
  if (p.C % 4 != 0) return false;
  p.IC = (p.OW - 1) * p.sw + (p.KW - 1) * p.dw + 1;
  const uint32_t halo = (p.KH - 1) * p.dh + 1;
  const uint32_t want = p.OH < 4 ? p.OH : 4;
  uint32_t best_cs = 0, best_toh = 0, best_pp = 0;
  // candidate slabs: divisors of C, multiples of 4 (prefer 16), at most 4*kDwThreads channels
  for (uint32_t parts = 1; parts <= p.C / 4; parts++) {
    if (p.C % parts != 0) continue;
    const uint32_t cs = p.C / parts;
    if (cs % 4 != 0 || cs / 4 > kDwThreads) continue;
    if (p.C % 16 == 0 && cs % 16 != 0) continue;      // keep 16-byte staging loads when the tensor allows them
    const uint32_t q4 = cs / 4;
    // line pitch (dwords): >= IC, and == spread (mod 32) so that the q4 group lines of a row start on
    // different banks: spread = 32/q4 for few groups, 1 (odd) for many
    const uint32_t spread = q4 >= 32 ? 1u : (32u + q4 - 1) / q4;
    uint32_t pp = p.IC;
    while (pp % 32 != spread % 32) pp++;
    const uint32_t row_bytes = q4 * pp * 4;
    const uint32_t max_rows = budget / row_bytes;
    if (max_rows < halo) continue;
    uint32_t toh = (max_rows - halo) / p.sh + 1;
    if (toh > p.OH) toh = p.OH;
    if (best_cs == 0) { best_cs = cs; best_toh = toh; best_pp = pp; }   // widest slab that fits at all
    if (toh >= want) { best_cs = cs; best_toh = toh; best_pp = pp; break; }
  }
  if (best_cs == 0) return false;
  p.CS = best_cs;
  p.PP = best_pp;
  p.slabs = p.C / best_cs;
  // keep the machine busy: at least ~4 workgroups per CU when the batch is small
  uint32_t toh = best_toh;
  while (toh > 1 && static_cast<uint64_t>(p.batch) * ((p.OH + toh - 1) / toh) * p.slabs < 1024) {
    toh = (toh + 1) / 2;
  }
  p.TOH = toh;
  p.bands = (p.OH + toh - 1) / toh;
  p.IR = (toh - 1) * p.sh + halo;
  return true;
}

// (the window is 3x3 or 5x5: make_plan asks dwlds_plan for nothing else)
int dwlds_launch(const DwParams& p, bool vec16, hipStream_t stream)
{
  return p.KH == 3 ? launch_lds<3, 3>(p, vec16, stream) : launch_lds<5, 5>(p, vec16, stream);
}

}  // namespace qnnp
