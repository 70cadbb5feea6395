/*
 * q8pwgw.hip -- pointwise streaming kernels, the global-weights flavours: q8_pw_stream_gw_kernel<RES, TAB> (one wave per
 * 32 x 32 output block) and q8_pw_stream_gwk_kernel<depth, RES, TAB> (one workgroup per block, the reduction split over its
 * waves). Pointwise / fully-connected layers whose weights do not fit LDS, over few rows: late MobileNet layers and
 * classifier heads, any K and N with 16-byte aligned rows. No dynamic LDS, no persistent grid. Launch: pw_gw_launch
 * (igemm_params.h) of a plan made by q8pwconv.hip's pwstream_gw_plan, which picks between the two; q8igemm.hip decides
 * when they run ("gemm_kernel" 6 forces them).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "pwstream_common.hip.h"

namespace qnnp {

namespace {

/*
 * Second flavour for pointwise / fully-connected layers whose weights do NOT fit LDS (K up to ~1000 over few
 * rows: the late MobileNet layers, classifier heads): one WAVE = one 32-row x 32-channel output block, both
 * MFMA operands straight from global memory / L2 (activations: 16 B per lane in B-operand layout; weights: one
 * coalesced 1 KiB fragment), four K blocks of loads in flight ahead of the multiplies, no LDS, no barrier.
 * The tiled kernels launch 49-196 workgroups for these shapes on a 256-CU chip; here every 32x32 block is its
 * own wave (980-7840 waves). Operand traffic is L2-resident by construction (the whole problem is a few MB).
 */
constexpr int kGwUnroll = 4;

/* TAB: the output table flavour. The kernel has no LDS and no barrier and its waves leave early: every wave writes the table
 * for itself (lut_lookup.hip.h stage_table_wave), requested in front of the operands and written where the reduction is
 * done. Without RES only. */
template <bool RES, bool TAB = false>
__global__ __launch_bounds__(kThreads, 4)
void q8_pw_stream_gw_kernel(const IgemmParams p)
{
  static_assert(!(RES && TAB), "a residual add and an output table are never attached together");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t row_in_block = lane & 31u;
  const uint32_t khalf = lane >> 5;
  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;
  const uint32_t units = ((p.rows + 31u) / 32u) * nblocks;
  const uint32_t unit = blockIdx.x * kWaves + wave;        // channel block fastest: neighbours share the rows
  if (unit >= units) return;
  uint8_t (*tab)[256] = nullptr;
  uint32_t tab_dword = 0;
  if constexpr (TAB) {
    __shared__ alignas(16) uint8_t tab_lds[256];
    tab = &tab_lds;
    tab_dword = table_dword(p.table);
  }
  const uint32_t rb = unit / nblocks;
  const uint32_t nb = unit - rb * nblocks;

  uint32_t m = rb * 32u + row_in_block;
  const bool row_ok = m < p.rows;
  if (!row_ok) m = p.rows - 1;
  // (launcher: the input tensor is addressable with 32-bit offsets)
  const __amdgpu_buffer_rsrc_t in_rsrc = buffer_rsrc(p.input, static_cast<int>((p.rows - 1u) * p.input_stride + p.k_total));
  const uint32_t row_off = m * p.input_stride;
  const int8_t* wf = p.packed_w + static_cast<uint64_t>(nb) * kblocks * 1024 + lane * 16;
  const uint32_t kbt = (p.k_total + 31u) / 32u;

  int4 bias4[4];
#pragma unroll
  for (int rg = 0; rg < 4; rg++) {
    bias4[rg] = *reinterpret_cast<const int4*>(p.bias2 + nb * 32 + rg * 8 + khalf * 4);
  }

  v16i acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0;
  uint32_t rs = 0;
  // Two groups of kGwUnroll K blocks are in flight: group g+1 is issued before group g is multiplied (every load is
  // unconditional -- clamped block index, padding source -- so hipcc counts the waits instead of draining). One
  // group per round made the launch a chain of K/128 dependent L2 round trips.
  // Activations come through a buffer descriptor: a piece beyond the row's K gets an out-of-range offset and reads
  // as zeros -- nothing for the row sum, and its weights are zero -- without any branch or pointer select (a
  // uniform "is this block there" branch around a load made hipcc copy the prefetched registers at the loop end,
  // which waits for them).
  auto load_group = [&](uint32_t kb0, v4i (&a)[kGwUnroll], v4i (&w)[kGwUnroll]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kGwUnroll; u++) {
      const uint32_t kb = kb0 + u;
      const uint32_t koff = kb * 32 + khalf * 16;                          // k_total % 16 == 0: whole piece or none
      a[u] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, koff < p.k_total ? row_off + koff : 0xFFFFFFF0u, 0, 0));
      const uint32_t kbc = min(kb, kbt - 1);                               // (clamped fragments meet zeros)
      w[u] = *reinterpret_cast<const v4i*>(wf + static_cast<uint64_t>(kbc) * 1024);
    }
  };
  auto multiply_group = [&](uint32_t kb0, v4i (&a)[kGwUnroll], const v4i (&w)[kGwUnroll]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kGwUnroll; u++) {
      rs = __builtin_amdgcn_sad_u8(a[u].x, 0u, rs);
      rs = __builtin_amdgcn_sad_u8(a[u].y, 0u, rs);
      rs = __builtin_amdgcn_sad_u8(a[u].z, 0u, rs);
      rs = __builtin_amdgcn_sad_u8(a[u].w, 0u, rs);
      // a piece beyond K arrived as zeros and stays zero (a' == 0: the clamped weight fragment beside it is a real one)
      const int flip = static_cast<int>((kb0 + u) * 32 + khalf * 16 < p.k_total ? kFlip : 0u);
      a[u].x ^= flip;
      a[u].y ^= flip;
      a[u].z ^= flip;
      a[u].w ^= flip;
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[u], a[u], acc, 0, 0, 0);
    }
  };
  v4i a0[kGwUnroll], w0[kGwUnroll], a1[kGwUnroll], w1[kGwUnroll];
  load_group(0, a0, w0);
  for (uint32_t kb0 = 0; kb0 < kbt; kb0 += 2 * kGwUnroll) {
    load_group(kb0 + kGwUnroll, a1, w1);
    multiply_group(kb0, a0, w0);
    load_group(kb0 + 2 * kGwUnroll, a0, w0);
    multiply_group(kb0 + kGwUnroll, a1, w1);
  }
  rs += __shfl_xor(rs, 32);                                   // the other K half of the same row
  // (pieces beyond K read as zeros: the raw sum is over the k_total real bytes)
  const int32_t rowterm = p.row_coeff * static_cast<int32_t>(rs - 128u * p.k_total);
  uint8_t* out_row = p.output + static_cast<uint64_t>(rb * 32u + row_in_block) * p.output_stride;
  if constexpr (TAB) stage_table_wave(*tab, tab_dword);
  requant_dispatch_ofs(p.rq, [&](auto shift0, auto full) {
    if constexpr (RES) {
      const uint8_t* res_row = p.residual + static_cast<uint64_t>(row_ok ? rb * 32u + row_in_block : 0u) * p.residual_stride;
      igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 0, true>(
          acc, bias4, with_rq_offset<decltype(shift0)::value>(rowterm), out_row, nb * 32, khalf, row_ok, p, res_row, &p.add);
      return;
    }
    if constexpr (TAB) {
      igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 0, false, true>(
          acc, bias4, with_rq_offset<decltype(shift0)::value>(rowterm), out_row, nb * 32, khalf, row_ok, p, nullptr, nullptr,
          &(*tab)[0]);
      return;
    }
    igemm_store_tile<decltype(shift0)::value, decltype(full)::value>(
        acc, bias4, with_rq_offset<decltype(shift0)::value>(rowterm), out_row, nb * 32, khalf, row_ok, p);
  });
}

/*
 * The same with the reduction SPLIT over the waves of a workgroup (one workgroup = one 32x32 output block): with one
 * wave per block a K = 960 layer is a chain of 8 dependent (load 4 K blocks -> wait -> 4 MFMAs) rounds, ~1.2 us of
 * L2 latency each, and the whole launch lasts exactly as long as that chain (10.6 us for 7x7x960 -> 320 at batch
 * 128, which is 1 us of MFMA work). Here wave w takes K blocks w, w + 4, ... and issues up to eight blocks of loads
 * (16 x 16 bytes per lane) before the first multiply; the partial accumulators and row sums of waves 1-3 meet wave
 * 0's through LDS (12 KiB), and wave 0 requantizes and stores. int32 partial sums are exact, so the split is
 * bit-invisible.
 */
/* TAB: the output table flavour. Wave 0 alone stores: it writes the workgroup's one copy of the table in front of the
 * barrier at which the partial sums meet, and reads it behind it. Without RES only. */
template <int kGwkDepth, bool RES, bool TAB = false>       // K blocks a wave has in flight: 4 or 8
__global__ __launch_bounds__(kThreads, 4)
void q8_pw_stream_gwk_kernel(const IgemmParams p)
{
  static_assert(!(RES && TAB), "a residual add and an output table are never attached together");
  __shared__ __attribute__((aligned(16))) int32_t part[(kWaves - 1) * 17 * 64];   // [wave-1][register | row sum][lane]
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t row_in_block = lane & 31u;
  const uint32_t khalf = lane >> 5;
  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;
  const uint32_t unit = blockIdx.x;                         // channel block fastest: neighbours share the rows
  const uint32_t rb = unit / nblocks;
  const uint32_t nb = unit - rb * nblocks;

  uint32_t m = rb * 32u + row_in_block;
  const bool row_ok = m < p.rows;
  if (!row_ok) m = p.rows - 1;
  // (launcher: the input tensor is addressable with 32-bit offsets; pieces beyond K read as zeros, see the kernel above)
  const __amdgpu_buffer_rsrc_t in_rsrc = buffer_rsrc(p.input, static_cast<int>((p.rows - 1u) * p.input_stride + p.k_total));
  const uint32_t row_off = m * p.input_stride;
  const int8_t* wf = p.packed_w + static_cast<uint64_t>(nb) * kblocks * 1024 + lane * 16;
  const uint32_t kbt = (p.k_total + 31u) / 32u;

  v16i acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0;
  uint32_t rs = 0;
  for (uint32_t kb0 = wave; kb0 < kbt; kb0 += kWaves * kGwkDepth) {
    v4i a[kGwkDepth], w[kGwkDepth];
#pragma unroll
    for (int u = 0; u < kGwkDepth; u++) {
      const uint32_t kb = kb0 + u * kWaves;
      const uint32_t koff = kb * 32 + khalf * 16;                          // k_total % 16 == 0: whole piece or none
      a[u] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, koff < p.k_total ? row_off + koff : 0xFFFFFFF0u, 0, 0));
      const uint32_t kbc = min(kb, kbt - 1);                               // (clamped fragments meet zeros)
      w[u] = *reinterpret_cast<const v4i*>(wf + static_cast<uint64_t>(kbc) * 1024);
    }
#pragma unroll
    for (int u = 0; u < kGwkDepth; u++) {
      rs = __builtin_amdgcn_sad_u8(a[u].x, 0u, rs);
      rs = __builtin_amdgcn_sad_u8(a[u].y, 0u, rs);
      rs = __builtin_amdgcn_sad_u8(a[u].z, 0u, rs);
      rs = __builtin_amdgcn_sad_u8(a[u].w, 0u, rs);
      // a piece beyond K arrived as zeros and stays zero (a' == 0: the clamped weight fragment beside it is a real one)
      const int flip = static_cast<int>((kb0 + u * kWaves) * 32 + khalf * 16 < p.k_total ? kFlip : 0u);
      a[u].x ^= flip;
      a[u].y ^= flip;
      a[u].z ^= flip;
      a[u].w ^= flip;
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[u], a[u], acc, 0, 0, 0);
    }
  }
  // raw sums of the wave's K blocks; sum(a') = sum(a) - 128 * k_total once per row, below
  int32_t rsc = static_cast<int32_t>(rs);
  if (wave != 0) {
    int32_t* mine = part + (wave - 1) * 17 * 64 + lane;
#pragma unroll
    for (int r = 0; r < 16; r++) mine[r * 64] = acc[r];
    mine[16 * 64] = rsc;
  }
  const uint8_t* lut = nullptr;
  if constexpr (TAB) {
    __shared__ alignas(16) uint8_t tab_lds[256];
    if (wave == 0) reinterpret_cast<uint32_t*>(tab_lds)[lane] = reinterpret_cast<const uint32_t*>(p.table)[lane];
    lut = tab_lds;
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < kWaves - 1; w++) {
    const int32_t* other = part + w * 17 * 64 + lane;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] += other[r * 64];
    rsc += other[16 * 64];
  }
  rsc += __shfl_xor(rsc, 32);                                 // the other K half of the same row
  rsc -= static_cast<int32_t>(128u * p.k_total);
  int4 bias4[4];
#pragma unroll
  for (int rg = 0; rg < 4; rg++) {
    bias4[rg] = *reinterpret_cast<const int4*>(p.bias2 + nb * 32 + rg * 8 + khalf * 4);
  }
  uint8_t* out_row = p.output + static_cast<uint64_t>(rb * 32u + row_in_block) * p.output_stride;
  requant_dispatch_ofs(p.rq, [&](auto shift0, auto full) {
    const int32_t rowterm = with_rq_offset<decltype(shift0)::value>(p.row_coeff * rsc);
    if constexpr (RES) {
      const uint8_t* res_row = p.residual + static_cast<uint64_t>(row_ok ? rb * 32u + row_in_block : 0u) * p.residual_stride;
      igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 0, true>(
          acc, bias4, rowterm, out_row, nb * 32, khalf, row_ok, p, res_row, &p.add);
      return;
    }
    if constexpr (TAB) {
      igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 0, false, true>(
          acc, bias4, rowterm, out_row, nb * 32, khalf, row_ok, p, nullptr, nullptr, lut);
      return;
    }
    igemm_store_tile<decltype(shift0)::value, decltype(full)::value>(
        acc, bias4, rowterm, out_row, nb * 32, khalf, row_ok, p);
  });
}

}  // namespace

/* The instantiations: gw, and gwk at depth 4 and 8, each plain, RES and TAB. */
int pw_gw_launch(const IgemmParams& p, const PwPlan& plan, hipStream_t stream)
{
  const auto flavours = [&](auto depth) {
    constexpr int DEPTH = decltype(depth)::value;          // 0: one wave per block
    if constexpr (DEPTH == 0) {
      if (plan.res) return launch_planned<q8_pw_stream_gw_kernel<true>>(0, plan, stream, p);
      if (plan.tab) return launch_planned<q8_pw_stream_gw_kernel<false, true>>(0, plan, stream, p);
      return launch_planned<q8_pw_stream_gw_kernel<false>>(0, plan, stream, p);
    } else {
      if (plan.res) return launch_planned<q8_pw_stream_gwk_kernel<DEPTH, true>>(0, plan, stream, p);
      if (plan.tab) return launch_planned<q8_pw_stream_gwk_kernel<DEPTH, false, true>>(0, plan, stream, p);
      return launch_planned<q8_pw_stream_gwk_kernel<DEPTH, false>>(0, plan, stream, p);
    }
  };
  if (plan.family == PwFamily::Gw) return flavours(std::integral_constant<int, 0>{});
  return plan.depth <= 4 ? flavours(std::integral_constant<int, 4>{}) : flavours(std::integral_constant<int, 8>{});
}

}  // namespace qnnp
