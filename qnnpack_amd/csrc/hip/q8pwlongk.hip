/*
 * q8pwlongk.hip -- pointwise streaming kernel, the long-K flavour: q8_pw_stream_longk_kernel<KBMAX, SEQ, FULL, RES, PF, TAB>.
 * Pointwise / fully-connected layers with 256 < K <= 1024 and 16-byte aligned rows on both sides: the late MobileNet project
 * layers, ResNet-50's 28x28 512 -> 128. Launch: pw_longk_launch (igemm_params.h) of a plan made by q8pwconv.hip's
 * pwstream_longk_plan; q8igemm.hip decides when it runs ("gemm_kernel" 9 forces it).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "pwstream_common.hip.h"

namespace qnnp {

namespace {

/*
 * Long reductions (256 < K <= 1024) on the same scheme: the late MobileNet project layers (14x14x384 -> 96,
 * 7x7x960 -> 320 ...). A wave has about one unit there, so there is no next unit to prefetch; instead ALL the K
 * blocks of the unit's rows are requested at once (up to 32 x 16 bytes per lane in flight) and the column's weights sit
 * in LDS (up to 96 KiB per workgroup). The one-wave-per-32x32-block kernel of q8pwgw.hip fetches both operands from L2 in
 * groups of four K blocks: a chain of dependent round trips as long as the reduction.
 * KBMAX: register budget in K blocks (12 / 20 / 32); the real count is a run-time value, blocks beyond it are skipped.
 */
/* PF (round 5; KBMAX <= 20): many rows after all -- ResNet-50's 28x28 512 -> 128 is 3136 units, two or more per wave. The rows of
 * a wave's NEXT unit are requested before the current one is multiplied (a second register set, the loop unrolled twice so
 * that the sets swap roles without copies); without it every unit is a full memory round trip in front of its first MFMA. */
/* TAB: the output table flavour, as the staged kernel's. Without RES only. */
template <int KBMAX, int SEQ, bool FULL, bool RES = false, bool PF = false, bool TAB = false>
__global__ __launch_bounds__(kThreads, PF ? 2 : longk_waves(KBMAX))
void q8_pw_stream_longk_kernel(const IgemmParams p, const uint32_t nbp, const uint32_t log_cpr)
{
  static_assert(!PF || KBMAX <= 20, "two row sets of 32 K blocks do not fit the register file");
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  const uint32_t row_in_block = lane & 31u;
  const uint32_t khalf = lane >> 5;

  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;
  const uint32_t kbn = (p.k_total + 31u) / 32u;           // K blocks with data (<= KBMAX)
  const uint32_t nb0 = blockIdx.y * nbp;
  const uint32_t nbn = min(nbp, nblocks - nb0);
  const uint32_t c0 = nb0 * 32u;
  const uint32_t cw = min(p.n - c0, nbn * 32u);
  const bool whole_dense = gridDim.y == 1 && p.output_stride == p.n;
  const uint32_t pitch = whole_dense ? p.n : (16u << log_cpr);
  {
    const uint32_t frags = nbn * kbn;
    for (uint32_t f = wave; f < frags; f += kWaves) {
      const uint32_t nb = f / kbn;
      const uint32_t kb = f - nb * kbn;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (p.packed_w + (static_cast<uint64_t>(nb0 + nb) * kblocks + kb) * 1024 + lane * 16),
          (__attribute__((address_space(3))) void*) (lds + f * 1024), 16, 0, 0);
    }
    uint8_t* lds_bias = lds + nbp * kbn * 1024;
    const uint32_t bias_chunks = nbn * 8u;
    const int32_t* bias_src = rq_is_lane<SEQ>() ? p.bias2u : p.bias2;   // (lane forms: bias + 2^31, the pair table's second half)
    for (uint32_t q0 = wave * 64; q0 < bias_chunks; q0 += kThreads) {
      const uint32_t q = min(q0 + lane, bias_chunks - 1);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (reinterpret_cast<const uint8_t*>(bias_src + c0) + q * 16),
          (__attribute__((address_space(3))) void*) (lds_bias + q0 * 16), 16, 0, 0);
    }
  }
  const uint8_t* lds_w = lds + lane * 16;
  const uint32_t bias_bytes = (nbp * 128u + 1023u) & ~1023u;
  const int4* lds_bias4 = reinterpret_cast<const int4*>(lds + nbp * kbn * 1024);
  uint8_t* stage = lds + nbp * kbn * 1024 + bias_bytes + wave * (32u * pitch);
  const uint8_t* pad16 = p.fill_table + 0x80 * 16;        // 16 bytes of a' == 0
  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t unit_stride = gridDim.x * kWaves;
  const uint32_t raw_to_centred = 128u * 32u * kbn;

  // every K block of the unit's rows at once; a piece beyond K (only in the last block) reads the a' == 0 line
  auto load_rows = [&](uint32_t unit, v4i (&a)[KBMAX]) __attribute__((always_inline)) {
    uint32_t m = unit * 32u + row_in_block;
    if (m >= p.rows) m = p.rows - 1;
    const uint8_t* row = p.input + static_cast<uint64_t>(m) * p.input_stride + khalf * 16;
#pragma unroll
    for (int kb = 0; kb < KBMAX; kb++) {
      if (static_cast<uint32_t>(kb) < kbn) {
        const uint8_t* src = (kb * 32u + khalf * 16u < p.k_total) ? row + kb * 32 : pad16;
        a[kb] = *reinterpret_cast<const v4i*>(src);
      }
    }
  };
  auto recentre = [&](v4i (&a)[KBMAX]) __attribute__((always_inline)) -> uint32_t {
    uint32_t rs = 0;
#pragma unroll
    for (int kb = 0; kb < KBMAX; kb++) {
      if (static_cast<uint32_t>(kb) < kbn) {
        rs = __builtin_amdgcn_sad_u8(a[kb].x, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].y, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].z, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].w, 0u, rs);
        a[kb].x ^= static_cast<int>(kFlip);
        a[kb].y ^= static_cast<int>(kFlip);
        a[kb].z ^= static_cast<int>(kFlip);
        a[kb].w ^= static_cast<int>(kFlip);
      }
    }
    rs += __shfl_xor(rs, 32);
    return rs;
  };

  uint32_t unit = blockIdx.x * kWaves + wave;
  v4i a[KBMAX];
  load_rows(min(unit, units - 1u), a);
  const uint8_t* lut = nullptr;
  if constexpr (TAB) {
    uint8_t* lds_tab = lds + nbp * kbn * 1024 + bias_bytes + kWaves * (32u * pitch);       // behind staged_lds_bytes()
    if (tid < 64u) reinterpret_cast<uint32_t*>(lds_tab)[tid] = reinterpret_cast<const uint32_t*>(p.table)[tid];
    lut = lds_tab;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // weights + bias are in LDS (and the first rows landed)
  __syncthreads();
  if (unit >= units) return;

  const std::integral_constant<int, SEQ> shift0{};
  const std::integral_constant<bool, FULL> full{};
  (void) shift0; (void) full;
  auto process = [&](uint32_t unit_now, v4i (&x)[KBMAX]) __attribute__((always_inline)) {
    const uint32_t rs = recentre(x);
    const int32_t rowterm = with_rq_offset<SEQ>(p.row_coeff * static_cast<int32_t>(rs - raw_to_centred));
    uint64_t row_addend = 0;
    if constexpr (rq_is_lane<SEQ>()) row_addend = lane_addend(rowterm, p.lane);
    uint8_t* img = stage + row_in_block * pitch;
    for (uint32_t nb = 0; nb < nbn; nb++) {
      v16i acc;
      // (read per block, beside the weight fragment: carried over from the previous trip it cost 16 v_mov_b64 per block)
      int4 bias4[4];
#pragma unroll
      for (int rg = 0; rg < 4; rg++) bias4[rg] = lds_bias4[nb * 8 + rg * 2 + khalf];
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        acc[rg * 4 + 0] = bias4[rg].x; acc[rg * 4 + 1] = bias4[rg].y;
        acc[rg * 4 + 2] = bias4[rg].z; acc[rg * 4 + 3] = bias4[rg].w;
      }
      const uint8_t* wf = lds_w + nb * (kbn * 1024);
#pragma unroll
      for (int kb = 0; kb < KBMAX; kb++) {
        if (static_cast<uint32_t>(kb) < kbn) {
          const v4i w = *reinterpret_cast<const v4i*>(wf + kb * 1024);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w, x[kb], acc, 0, 0, 0);
        }
      }
      if constexpr (rq_is_lane<SEQ>()) {
        igemm_stage_tile_lane<SEQ, FULL>(acc, row_addend, img, nb * 32, khalf, p, nb * 32 + khalf * 16 < cw);
      } else {
        igemm_stage_tile<SEQ, FULL, false, 2>(acc, bias4, rowterm, img, nb * 32, khalf, p, nb * 32 + khalf * 16 < cw);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // image complete before it is read back
    stream_copy_out<RES, TAB>(stage, whole_dense, log_cpr, unit_now, c0, cw, p, lane, false, lut);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // read back before the next unit overwrites it
  };
  if constexpr (PF) {
    v4i b[KBMAX];
    for (;;) {
      uint32_t next = unit + unit_stride;
      if (next < units) load_rows(next, b);
      process(unit, a);
      if (next >= units) break;
      unit = next;
      next = unit + unit_stride;
      if (next < units) load_rows(next, a);
      process(unit, b);
      if (next >= units) break;
      unit = next;
    }
  } else {
    for (;;) {
      process(unit, a);
      const uint32_t next = unit + unit_stride;
      if (next >= units) break;
      unit = next;
      load_rows(unit, a);
    }
  }
}

}  // namespace

/* The instantiations: KBMAX 12 / 20 / 32 in every requantization flavour plain, RES and TAB; PF and PF with TAB at
 * KBMAX <= 20 (never with RES). */
int pw_longk_launch(const IgemmParams& p, const PwPlan& plan, hipStream_t stream)
{
  const auto flavours = [&](auto kbmax) {
    int rc = QNNP_HIP_EINVAL;
    requant_dispatch_lane(p.rq, p.lane, [&](auto seq, auto full) {
      constexpr int KBMAX = decltype(kbmax)::value;
      constexpr int SEQ = decltype(seq)::value;
      constexpr bool FULL = decltype(full)::value;
      if constexpr (KBMAX <= 20) {
        if (plan.pf) {
          if (plan.tab) rc = launch_planned<q8_pw_stream_longk_kernel<KBMAX, SEQ, FULL, false, true, true>>(kMaxLdsLongK, plan, stream, p, plan.nbp, plan.log_cpr);
          else rc = launch_planned<q8_pw_stream_longk_kernel<KBMAX, SEQ, FULL, false, true>>(kMaxLdsLongK, plan, stream, p, plan.nbp, plan.log_cpr);
          return;
        }
      }
      if (plan.res) rc = launch_planned<q8_pw_stream_longk_kernel<KBMAX, SEQ, FULL, true>>(kMaxLdsLongK, plan, stream, p, plan.nbp, plan.log_cpr);
      else if (plan.tab) rc = launch_planned<q8_pw_stream_longk_kernel<KBMAX, SEQ, FULL, false, false, true>>(kMaxLdsLongK, plan, stream, p, plan.nbp, plan.log_cpr);
      else rc = launch_planned<q8_pw_stream_longk_kernel<KBMAX, SEQ, FULL>>(kMaxLdsLongK, plan, stream, p, plan.nbp, plan.log_cpr);
    });
    return rc;
  };
  switch (plan.kb) {
    case 12: return flavours(std::integral_constant<int, 12>{});
    case 20: return flavours(std::integral_constant<int, 20>{});
    default: return flavours(std::integral_constant<int, 32>{});
  }
}

}  // namespace qnnp
