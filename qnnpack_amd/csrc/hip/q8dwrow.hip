/*
 * q8dwrow.hip -- depthwise kernel C: the register sliding window along a row, q8_dwconv_row3x3_kernel<SW, UNAL> (3x3,
 * dilation 1, stride 1 | 2). Its UNAL flavour takes any channel count >= 4 and tensors of any alignment through
 * DwAnyAligned. One family, no device code shared with another unit. Plan and launch: dwrow_plan / dwrow_launch
 * (dwconv_params.h); "dwconv_kernel" 3 forces the aligned flavour, 8 the unaligned one.
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
// Kernel C: register sliding window, 3x3, dilation 1, stride 1 or 2, C % 4 == 0
// --------------------------------------------------------------------------
/*
 * No LDS, no barrier: a thread owns one 4-channel group of one output row segment and slides a 3x3 window
 * of input dwords (4 channels each) along it in registers -- per output only the SW new window columns are
 * loaded (3 or 6 dwords, coalesced along C across the lanes: consecutive lanes = consecutive channel
 * groups, then consecutive output rows, so the three kernel rows of neighbouring lanes hit the same lines
 * in L1). The vertical reuse (an input row feeds up to three output rows) is left to L1/L2.
 * Why: the LDS kernel spends ~70 % of a workgroup's life staging its band behind a barrier (in-kernel cycle
 * stamps); here loads, the VALU tap arithmetic and the requantization of different waves overlap freely at
 * 8+ waves per SIMD.
 * Padding: rows / columns outside the image are clamped to a valid address and replaced by the input zero
 * point after the load (checked path, taken only by waves that touch a border).
 */
constexpr int kRowThreads = 256;

/* UNAL (round 6): any channel count >= 4 and pixels / tensors of any alignment -- ShuffleNet v2's 58 / 122 / 244 / 488-channel depthwise
 * layers (bench/convolution.cc:338-426), which ran on the generic q8_dwconv_direct4 at 0.05-0.13 of their bound. A pixel's channels are
 * cut into (C + 3) / 4 groups of four, the last one starting at C - 4 (it recomputes up to three channels of its neighbour: the same
 * bytes, written twice); every load and store is a dword at whatever address it falls on (the hardware takes unaligned dwords from
 * global memory; the weight and bias tables are read the same way), everything else is the kernel's. */
template <typename T>
struct __attribute__((packed)) DwAnyAligned { T v; };
template <typename T>
__device__ __forceinline__ T dw_load_any(const void* ptr) { return reinterpret_cast<const DwAnyAligned<T>*>(ptr)->v; }
// (HIP's vector types are not POD for the packed attribute: their unaligned loads are spelled out dword by dword)
template <>
__device__ __forceinline__ uint2 dw_load_any<uint2>(const void* ptr)
{
  const uint8_t* b = static_cast<const uint8_t*>(ptr);
  return make_uint2(dw_load_any<uint32_t>(b), dw_load_any<uint32_t>(b + 4));
}
template <>
__device__ __forceinline__ int4 dw_load_any<int4>(const void* ptr)
{
  const uint8_t* b = static_cast<const uint8_t*>(ptr);
  return make_int4(dw_load_any<int32_t>(b), dw_load_any<int32_t>(b + 4), dw_load_any<int32_t>(b + 8), dw_load_any<int32_t>(b + 12));
}
template <typename T>
__device__ __forceinline__ void dw_store_any(void* ptr, T v) { reinterpret_cast<DwAnyAligned<T>*>(ptr)->v = v; }

template <int SW, bool UNAL = false>
__global__ __launch_bounds__(kRowThreads)
void q8_dwconv_row3x3_kernel(const DwParams p)
{
  constexpr int PAIRS = 5;
  QNNP_DW_TRACE(p, 0);
  const uint32_t q4 = UNAL ? (p.C + 3u) / 4u : p.C / 4;
  const uint32_t t = blockIdx.x * kRowThreads + threadIdx.x;       // host checked: fits 32 bits
  const uint32_t c4 = t % q4;
  uint32_t r = t / q4;
  const uint32_t oy = r % p.OH; r /= p.OH;
  const uint32_t seg = r % p.slabs;                                 // `slabs` = column segments per row here
  const uint32_t n = r / p.slabs;
  const bool live = n < p.batch;
  const uint32_t nn = live ? n : 0u;
  const uint32_t cg = UNAL ? min(c4 * 4u, p.C - 4u) : c4 * 4;

  // tap weights as (tap 2i, tap 2i+1) int16 pairs, bias
  uint32_t wpair[PAIRS][4];
  int32_t bias[4];
#pragma unroll
  for (int i = 0; i < PAIRS; i++) {
    const uint2 lo = dw_load_any<uint2>(p.wadj + (2 * i) * p.c_pad + cg);   // 4 x int16
    uint2 hi = make_uint2(0u, 0u);
    if (2 * i + 1 < 9) hi = dw_load_any<uint2>(p.wadj + (2 * i + 1) * p.c_pad + cg);
    wpair[i][0] = (lo.x & 0xFFFFu) | (hi.x << 16);
    wpair[i][1] = (lo.x >> 16) | (hi.x & 0xFFFF0000u);
    wpair[i][2] = (lo.y & 0xFFFFu) | (hi.y << 16);
    wpair[i][3] = (lo.y >> 16) | (hi.y & 0xFFFF0000u);
  }
  {
    const int4 bv = dw_load_any<int4>(p.bias1 + cg);
    bias[0] = bv.x; bias[1] = bv.y; bias[2] = bv.z; bias[3] = bv.w;
  }

  const uint32_t fill = p.izp * 0x01010101u;
  // the three input rows of this output row: 32-bit byte offsets from p.input (host checked < 4 GiB)
  uint32_t voff[3];
  bool row_ok[3];
  bool rows_need_check = false;
#pragma unroll
  for (int ky = 0; ky < 3; ky++) {
    const int32_t iy = static_cast<int32_t>(oy * p.sh) - static_cast<int32_t>(p.pad_top) + ky;
    row_ok[ky] = iy >= 0 && iy < static_cast<int32_t>(p.H);
    rows_need_check |= !row_ok[ky];
    const uint32_t iyc = row_ok[ky] ? static_cast<uint32_t>(iy) : 0u;
    voff[ky] = ((nn * p.H + iyc) * p.W) * p.in_stride + cg;
  }
  const bool wave_rows_check = __builtin_amdgcn_ballot_w64(rows_need_check) != 0;

  const uint32_t ox0 = seg * p.TOH;                                  // `TOH` = outputs per column segment here
  const uint32_t ox1 = live ? min(p.OW, ox0 + p.TOH) : ox0;
  uint8_t* out_ptr = p.output + (static_cast<uint64_t>(nn * p.OH + oy) * p.OW + ox0) * p.out_stride + cg;

  // one window column (three kernel rows) at input column ix
  auto load_col = [&](int32_t ix, uint32_t (&col)[3], bool check) __attribute__((always_inline)) {
    if (check) {
      const bool col_ok = ix >= 0 && ix < static_cast<int32_t>(p.W);
      const uint32_t coff = (col_ok ? static_cast<uint32_t>(ix) : 0u) * p.in_stride;
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        const uint32_t v = dw_load_any<uint32_t>(p.input + (voff[ky] + coff));
        col[ky] = (col_ok && row_ok[ky]) ? v : fill;
      }
    } else {
      const uint32_t coff = static_cast<uint32_t>(ix) * p.in_stride;
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        col[ky] = dw_load_any<uint32_t>(p.input + (voff[ky] + coff));
      }
    }
  };

  qnnp::requant_dispatch_ofs(p.rq, [&](auto shift0, auto full) {
#pragma unroll
    for (int c = 0; c < 4; c++) bias[c] = qnnp::with_rq_offset<decltype(shift0)::value>(bias[c]);
    // window columns kx = 0, 1, 2 of the current output plus the SW columns the NEXT output adds: those are
    // loaded one step ahead, so a load has a whole step of VALU work (and the other waves) to land
    uint32_t w0[3], w1[3], w2[3], n0[3], n1[3];
    int32_t ix = static_cast<int32_t>(ox0 * SW) - static_cast<int32_t>(p.pad_left);   // leftmost window column
    QNNP_DW_TRACE(p, 1);
    load_col(ix, w0, true);
    load_col(ix + 1, w1, true);
    load_col(ix + 2, w2, true);
#ifdef QNNP_ENABLE_ABLATION
    if (p.trace != nullptr) { asm volatile("" :: "v"(w0[0]), "v"(w1[1]), "v"(w2[2])); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
#endif
    QNNP_DW_TRACE(p, 2);
    for (uint32_t ox = ox0; ox < ox1; ox++) {
      // next step's new columns; a wave takes the checked path if any of its lanes touches a border
      const int32_t nx = ix + 3;
      const bool lane_check = nx + (SW - 1) >= static_cast<int32_t>(p.W);
      const bool check = wave_rows_check || lane_check;     // (no ballot here: it would block the unrolling)
      if (ox + 1 < ox1) {
        if (check) {
          load_col(nx, n0, true);
          if (SW == 2) load_col(nx + 1, n1, true);
        } else {
          load_col(nx, n0, false);
          if (SW == 2) load_col(nx + 1, n1, false);
        }
      }
      const uint32_t in[9] = {w0[0], w1[0], w2[0], w0[1], w1[1], w2[1], w0[2], w1[2], w2[2]};
      int32_t acc0 = bias[0], acc1 = bias[1], acc2 = bias[2], acc3 = bias[3];
#pragma unroll
      for (int i = 0; i < PAIRS; i++) {
        const uint32_t in0 = in[2 * i];
        const uint32_t in1 = (2 * i + 1 < 9) ? in[2 * i + 1] : 0u;
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
      dw_store_any<uint32_t>(out_ptr, packed);
      out_ptr += p.out_stride;
      // slide the window by SW columns (register renaming once the loop is unrolled)
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        if (SW == 1) { w0[ky] = w1[ky]; w1[ky] = w2[ky]; w2[ky] = n0[ky]; }
        else { w0[ky] = w2[ky]; w1[ky] = n0[ky]; w2[ky] = n1[ky]; }
      }
      ix += SW;
    }
    QNNP_DW_TRACE(p, 3);
    QNNP_DW_TRACE(p, 4);
    QNNP_DW_TRACE(p, 5);
  });
}

}  // namespace

namespace qnnp {

// geometry of kernel C: `slabs` = column segments per output row, `TOH` = outputs per segment
bool dwrow_plan(DwParams& p, bool unaligned)
{
  if ((unaligned ? p.C < 4 : p.C % 4 != 0) || p.KH != 3 || p.KW != 3 || p.dh != 1 || p.dw != 1) return false;
  if (p.sh != p.sw || (p.sw != 1 && p.sw != 2)) return false;
  if (p.pad_left > 2 || p.pad_top > 2) return false;
  // 32-bit input offsets
  const uint64_t in_bytes = static_cast<uint64_t>(p.batch) * p.H * p.W * p.in_stride;
  if (in_bytes >= (UINT64_C(1) << 32)) return false;
  // Column segments: enough threads for `waves` waves per SIMD over the whole chip (oversubscribing the 7
  // resident ones measured faster than exactly one resident round), but segments of at least 8 outputs
  // (each re-loads two halo columns and pays the start-up latency again).
  uint32_t waves = 8;
#ifdef QNNP_ENABLE_ABLATION
  if (const char* env = getenv("QNNP_DW_ROW_WAVES")) waves = static_cast<uint32_t>(atoi(env));
#endif
  const uint64_t base_threads = static_cast<uint64_t>(p.batch) * p.OH * ((p.C + 3u) / 4u);
  const uint64_t target = static_cast<uint64_t>(p.cu_count) * 4u * waves * 64u;
  uint32_t segs = static_cast<uint32_t>((target + base_threads - 1) / base_threads);
  const uint32_t max_segs = p.OW >= 8 ? p.OW / 8 : 1u;
  if (segs > max_segs) segs = max_segs;
  if (segs < 1) segs = 1;
  p.TOH = (p.OW + segs - 1) / segs;
  p.slabs = (p.OW + p.TOH - 1) / p.TOH;
  return true;
}

int dwrow_launch(const DwParams& p, hipStream_t stream, bool unaligned)
{
  const uint64_t threads = static_cast<uint64_t>(p.batch) * p.slabs * p.OH * ((p.C + 3u) / 4u);
  const uint64_t blocks = (threads + kRowThreads - 1) / kRowThreads;
  if (blocks * kRowThreads > 0xFFFFFFFFull) return QNNP_HIP_EINVAL;
  if (unaligned) {
    if (p.sw == 1) hipLaunchKernelGGL((q8_dwconv_row3x3_kernel<1, true>), dim3(static_cast<uint32_t>(blocks)), dim3(kRowThreads), 0, stream, p);
    else hipLaunchKernelGGL((q8_dwconv_row3x3_kernel<2, true>), dim3(static_cast<uint32_t>(blocks)), dim3(kRowThreads), 0, stream, p);
    return launch_status();
  }
  if (p.sw == 1) {
    hipLaunchKernelGGL(q8_dwconv_row3x3_kernel<1>, dim3(static_cast<uint32_t>(blocks)), dim3(kRowThreads), 0, stream, p);
  } else {
    hipLaunchKernelGGL(q8_dwconv_row3x3_kernel<2>, dim3(static_cast<uint32_t>(blocks)), dim3(kRowThreads), 0, stream, p);
  }
  return launch_status();
}

}  // namespace qnnp
