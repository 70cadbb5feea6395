/*
 * q8pwstream.hip -- pointwise streaming kernel, the barrier-free flavour: q8_pw_stream_mfma_kernel<KB, VEC, D2S, RES, TAB>.
 * Pointwise (1x1, stride 1) convolutions and fully-connected layers with a SHORT reduction (K <= 256) over MANY rows whose
 * output rows are one 32-channel block wide or not 16-byte aligned, and depth-to-space deconvolutions (D2S). Same arithmetic
 * as q8igemm.hip (which see); replaces the same reference path: qnnp_ukernel_type_gemm -> q8gemm 4x4c2 / 8x8
 * (src/operator-run.c:770-804, src/q8gemm/4x4c2-sse2.c:14-318). Launch: pw_stream_launch (igemm_params.h) of a plan made by
 * q8pwconv.hip's pwstream_plan, which decides when it runs ("gemm_kernel" 5 forces the short-K kernels).
 *
 * Why a separate kernel: these layers move 10-100x more bytes than they multiply
 * (K = 16..192 against N = 16..576), so they are bound by HBM and by the VALU work
 * of the requantization, not by the matrix cores. The tiled kernels stage
 * activations through LDS behind workgroup barriers, which serialises
 * load -> barrier -> multiply -> barrier -> requantize -> store per tile. Here
 *   - the whole weight matrix (<= 64 KiB of MFMA fragments) and the folded bias are
 *     copied into LDS ONCE per (persistent) workgroup;
 *   - each WAVE then walks 32-row blocks on its own, no barrier in the loop: a
 *     lane loads its 16 bytes of the activation row straight from global memory in
 *     MFMA B-operand layout (lane l = row l%32, K half l/32), the loads of the next
 *     block being in flight while the current one is multiplied and requantized;
 *   - per 32-channel block: K/32 MFMAs against fragments read from LDS, the fused
 *     Q31 epilogue of igemm_epilogue.hip.h, one 16-byte store per lane.
 * Rows are independent, so there is no exchange between waves at all.
 *
 * Zero-point algebra as in pack.h; row sums over the RAW bytes with v_sad_u8 (K
 * padding is loaded as 0x80 = a' of 0 from the fill table, so
 * sum(a') = sum(a) - 128 * 32 * KB).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "pwstream_common.hip.h"

namespace qnnp {

namespace {

/* KB = 32-deep K blocks (k_total <= 32 * KB); VEC = bytes per activation load (16, or 8 when rows are
 * only 8-byte aligned, e.g. 24 channels) */
/* D2S: depth-to-space stores (igemm_params.h) -- a deconvolution whose kernel equals its stride is this pointwise
 * GEMM with stride_h*stride_w times the channels, each phase's block landing on its own output pixel. */
/* RES: the residual add of igemm_params.h rides in the epilogue -- a kernel of its own, so that layers without one
 * run exactly the code they ran before it existed (as a wave-uniform run-time branch it cost them 2-6 %, same box:
 * 28x28x144 -> 32 6.7 -> 7.1 us, 56x56x144 -> 24 15.8 -> 16.4) */
/* TAB: the output table of igemm_params.h rides in the epilogue -- a kernel of its own for the same reason. The
 * workgroup's copy of the table (lut_lookup.hip.h) lies behind the bias in LDS and is written in front of the prologue's
 * barrier, the only one the kernel has. Instantiated without D2S and without RES only. */
template <int KB, int VEC, bool D2S = false, bool RES = false, bool TAB = false>
__global__ __launch_bounds__(kThreads, (KB <= 5) ? 4 : 2)
void q8_pw_stream_mfma_kernel(const IgemmParams p)
{
  static_assert(!TAB || (!D2S && !RES), "the table flavour exists without depth-to-space stores and without a residual");
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  const uint32_t row_in_block = lane & 31u;
  const uint32_t khalf = lane >> 5;

  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;          // fragment blocks per channel block in the packed image

  // ---- once per workgroup: weight fragments (only the KB non-empty K blocks) and bias2 into LDS ----
  // LDS image: [nb][kb < KB] fragments of 1 KiB, then n_pad int32 of bias2
  {
    // LDS-DMA (no VGPR round trip, all of a wave's fragments in flight at once)
    const uint32_t frags = nblocks * KB;
    for (uint32_t f = wave; f < frags; f += kWaves) {
      const uint32_t nb = f / KB;
      const uint32_t kb = f - nb * KB;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (p.packed_w + (static_cast<uint64_t>(nb) * kblocks + kb) * 1024 + lane * 16),
          (__attribute__((address_space(3))) void*) (lds + f * 1024), 16, 0, 0);
    }
    uint8_t* lds_bias = lds + frags * 1024;
    const uint32_t bias_chunks = p.n_pad / 4;             // 16-byte pieces; n_pad is a multiple of 32
    // (where the lane forms of the requantization apply -- requant_dispatch_lane below -- the accumulators start from
    //  bias + 2^31, the second half of the pair table)
    const bool lane_rq = p.bias2u != nullptr && (p.lane.kind == 1 || (p.lane.kind == 2 && p.rq.full_range != 0));
    const int32_t* bias_src = lane_rq ? p.bias2u : p.bias2;
    for (uint32_t c0 = wave * 64; c0 < bias_chunks; c0 += kThreads) {
      const uint32_t c = min(c0 + lane, bias_chunks - 1); // the tail lanes repeat the last piece (same bytes)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (reinterpret_cast<const uint8_t*>(bias_src) + c * 16),
          (__attribute__((address_space(3))) void*) (lds_bias + c0 * 16), 16, 0, 0);
    }
    // (no wait here: the first row block's loads are issued first, so both latencies overlap)
  }
  const uint8_t* lds_w = lds + lane * 16;
  const int4* lds_bias4 = reinterpret_cast<const int4*>(lds + nblocks * KB * 1024);

  // ---- which of this lane's 16-byte K pieces exist (only the last block can be short) ----
  const uint8_t* pad16 = p.fill_table + 0x80 * 16;        // 16 bytes of a' == 0
  const uint32_t k_last = (KB - 1) * 32 + khalf * 16;     // first K position of the lane's last piece
  // VEC 16: the piece is whole or absent. VEC 8: each 8-byte half is whole or absent.
  const bool last_lo_ok = k_last < p.k_total;
  const bool last_hi_ok = k_last + 8 < p.k_total;

  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t unit_stride = gridDim.x * kWaves;

  auto load_rows = [&](uint32_t unit, v4i (&a)[KB]) __attribute__((always_inline)) {
    uint32_t m = unit * 32u + row_in_block;
    if (m >= p.rows) m = p.rows - 1;                      // clamped rows are never stored
    const uint8_t* row = p.input + static_cast<uint64_t>(m) * p.input_stride + khalf * 16;
#pragma unroll
    for (int kb = 0; kb < KB; kb++) {
      const uint8_t* src = row + kb * 32;
      if constexpr (VEC == 16) {
        if (kb == KB - 1) src = last_lo_ok ? src : pad16;
        a[kb] = *reinterpret_cast<const v4i*>(src);
      } else {
        const uint8_t* lo = src;
        const uint8_t* hi = src + 8;
        if (kb == KB - 1) {
          lo = last_lo_ok ? lo : pad16;
          hi = last_hi_ok ? hi : pad16;
        }
        const int2 vlo = *reinterpret_cast<const int2*>(lo);
        const int2 vhi = *reinterpret_cast<const int2*>(hi);
        a[kb] = v4i{vlo.x, vlo.y, vhi.x, vhi.y};
      }
    }
  };

  const uint32_t raw_to_centred = 128u * 32u * KB;

  uint32_t unit = blockIdx.x * kWaves + wave;
  v4i a_next[KB];
  if (unit < units) load_rows(unit, a_next);
  const uint8_t* lut = nullptr;
  if constexpr (TAB) {
    uint8_t* lds_tab = lds + nblocks * KB * 1024 + ((p.n_pad * 4u + 1023u) & ~1023u);      // behind pw_lds_bytes()
    if (tid < 64u) reinterpret_cast<uint32_t*>(lds_tab)[tid] = reinterpret_cast<const uint32_t*>(p.table)[tid];
    lut = lds_tab;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // weights + bias are in LDS (and the first rows landed)
  __syncthreads();

  requant_dispatch_lane(p.rq, p.lane, [&](auto shift0, auto full) {
    constexpr int kSeq = decltype(shift0)::value;
    for (; unit < units; unit += unit_stride) {
      v4i a[KB];
#pragma unroll
      for (int kb = 0; kb < KB; kb++) a[kb] = a_next[kb];
      if (unit + unit_stride < units) load_rows(unit + unit_stride, a_next);

      // row sum over the raw bytes, then recentre at 128
      uint32_t rs = 0;
#pragma unroll
      for (int kb = 0; kb < KB; kb++) {
        rs = __builtin_amdgcn_sad_u8(a[kb].x, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].y, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].z, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].w, 0u, rs);
        a[kb].x ^= static_cast<int>(kFlip);
        a[kb].y ^= static_cast<int>(kFlip);
        a[kb].z ^= static_cast<int>(kFlip);
        a[kb].w ^= static_cast<int>(kFlip);
      }
      rs += __shfl_xor(rs, 32);                           // the other K half of the same row
      // (+ 2^31 for the offset rounding sequences, requant.hip.h: the accumulators start from bias + this)
      const int32_t rowterm = with_rq_offset<decltype(shift0)::value>(p.row_coeff * static_cast<int32_t>(rs - raw_to_centred));
      uint64_t row_addend = 0;                            // lane forms: the row term as the multiply-add's addend
      if constexpr (rq_is_lane<kSeq>()) row_addend = lane_addend(rowterm, p.lane);

      const uint32_t m = unit * 32u + row_in_block;
      uint8_t* out_row = p.output + static_cast<uint64_t>(m) * p.output_stride;
      bool row_ok = m < p.rows;
      if constexpr (D2S) {
        // input pixel (img, iy, ix) -> output pixel (img, iy*sh, ix*sw); the phase offset is added per channel block
        const uint32_t mm = row_ok ? m : 0u;
        const uint32_t rowi = mm / p.d2s_in_w;             // img * in_h + iy
        const uint32_t ix = mm - rowi * p.d2s_in_w;
        const uint64_t out_pixel = (static_cast<uint64_t>(rowi) * p.d2s_sh * p.d2s_in_w + ix) * p.d2s_sw;
        out_row = p.output + out_pixel * p.output_stride;
      }
#ifdef QNNP_ENABLE_ABLATION
      if (p.izp_fill & 1u) row_ok = false;                // measurement: no stores
#endif

      // accumulators start at bias + row term (the MFMA adds into them): two VALU adds per value saved
      int4 bias4[4];
      auto multiply = [&](uint32_t nb, v16i& acc) __attribute__((always_inline)) {
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          acc[rg * 4 + 0] = bias4[rg].x; acc[rg * 4 + 1] = bias4[rg].y;
          acc[rg * 4 + 2] = bias4[rg].z; acc[rg * 4 + 3] = bias4[rg].w;
        }
        const uint8_t* wf = lds_w + nb * (KB * 1024);
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
          const v4i w = *reinterpret_cast<const v4i*>(wf + kb * 1024);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w, a[kb], acc, 0, 0, 0);
        }
      };

#ifdef QNNP_ENABLE_ABLATION
      if (p.izp_fill & 4u) {                              // measurement: CONTIGUOUS stores only (dense rows assumed)
        uint8_t* blk = p.output + static_cast<uint64_t>(unit) * 32u * p.output_stride;
        const uint32_t bytes = 32u * p.output_stride;
        for (uint32_t o = lane * 16; o + 16 <= bytes; o += 1024) {
          if (unit * 32u + 32u <= p.rows) *reinterpret_cast<uint4*>(blk + o) = make_uint4(a[0].x, a[0].y, a[0].z, a[0].w);
        }
        continue;
      }
#endif
      for (uint32_t nb = 0; nb < nblocks; nb++) {
        v16i acc;
        // (read per block, beside the weight fragment: carried over from the previous trip it cost 16 v_mov_b64 per block)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) bias4[rg] = lds_bias4[nb * 8 + rg * 2 + khalf];
#ifdef QNNP_ENABLE_ABLATION
        if (p.izp_fill & 2u) {                            // measurement: stores only (no multiply, no requantization)
          const uint32_t c = nb * 32 + khalf * 16;
          if (row_ok && c < p.n) *reinterpret_cast<uint4*>(out_row + c) = make_uint4(a[0].x, a[0].y, a[0].z, a[0].w);
          continue;
        }
#endif
        multiply(nb, acc);
        if constexpr (D2S) {
          const uint32_t phase = nb / p.d2s_nbpp;
          const uint32_t py = phase / p.d2s_sw;
          const uint32_t px = phase - py * p.d2s_sw;
          uint8_t* phase_row = out_row + (static_cast<uint64_t>(py) * (p.d2s_in_w * p.d2s_sw) + px) * p.output_stride;
          if constexpr (rq_is_lane<kSeq>()) {
            igemm_store_tile_lane<kSeq, decltype(full)::value>(
                acc, row_addend, phase_row, (nb - phase * p.d2s_nbpp) * 32, khalf, row_ok, p);
          } else {
            igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 2>(
                acc, bias4, rowterm, phase_row, (nb - phase * p.d2s_nbpp) * 32, khalf, row_ok, p);
          }
          continue;
        }
        if constexpr (RES) {                              // project layer with its residual add folded in
          const uint8_t* res_row = p.residual + static_cast<uint64_t>(row_ok ? m : 0u) * p.residual_stride;
          if constexpr (rq_is_lane<kSeq>()) {
            igemm_store_tile_lane<kSeq, decltype(full)::value, true>(acc, row_addend, out_row, nb * 32, khalf, row_ok, p, res_row, &p.add);
          } else {
            igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 2, true>(
                acc, bias4, rowterm, out_row, nb * 32, khalf, row_ok, p, res_row, &p.add);
          }
          continue;
        }
        if constexpr (TAB) {                              // an activation table behind the layer folded in
          if constexpr (rq_is_lane<kSeq>()) {
            igemm_store_tile_lane<kSeq, decltype(full)::value, false, true>(
                acc, row_addend, out_row, nb * 32, khalf, row_ok, p, nullptr, nullptr, lut);
          } else {
            igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 2, false, true>(
                acc, bias4, rowterm, out_row, nb * 32, khalf, row_ok, p, nullptr, nullptr, lut);
          }
          continue;
        }
        if constexpr (rq_is_lane<kSeq>()) {
          igemm_store_tile_lane<kSeq, decltype(full)::value>(acc, row_addend, out_row, nb * 32, khalf, row_ok, p);
        } else {
          igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 2>(
              acc, bias4, rowterm, out_row, nb * 32, khalf, row_ok, p);
        }
      }
    }
  });
}

}  // namespace

/* The instantiations: every KB with 16-byte loads plain, D2S, RES and TAB; with 8-byte loads plain, RES and TAB. */
int pw_stream_launch(const IgemmParams& p, const PwPlan& plan, hipStream_t stream)
{
  const IgemmParams pa = with_ablation_bits(p);
  return with_kb(plan.kb, [&](auto kb) {
    constexpr int KB = decltype(kb)::value;
    if (plan.vec == 16) {
      if (plan.d2s) return launch_planned<q8_pw_stream_mfma_kernel<KB, 16, true>>(kMaxLds, plan, stream, pa);
      if (plan.res) return launch_planned<q8_pw_stream_mfma_kernel<KB, 16, false, true>>(kMaxLds, plan, stream, pa);
      if (plan.tab) return launch_planned<q8_pw_stream_mfma_kernel<KB, 16, false, false, true>>(kMaxLds, plan, stream, pa);
      return launch_planned<q8_pw_stream_mfma_kernel<KB, 16>>(kMaxLds, plan, stream, pa);
    }
    if (plan.res) return launch_planned<q8_pw_stream_mfma_kernel<KB, 8, false, true>>(kMaxLds, plan, stream, pa);
    if (plan.tab) return launch_planned<q8_pw_stream_mfma_kernel<KB, 8, false, false, true>>(kMaxLds, plan, stream, pa);
    return launch_planned<q8_pw_stream_mfma_kernel<KB, 8>>(kMaxLds, plan, stream, pa);
  });
}

}  // namespace qnnp
