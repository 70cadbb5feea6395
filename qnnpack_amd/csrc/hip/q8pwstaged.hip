/*
 * q8pwstaged.hip -- pointwise streaming kernel, the staged flavour: q8_pw_stream_staged_kernel<KB, VEC, SEQ, FULL, RES, TAB>.
 * Short reductions (K <= 256) into 16-byte aligned output rows wider than one channel block -- every MobileNet-style expand /
 * project layer --, dense rows of 8 (mod 16) bytes (24 channels), and strided 1x1 convolutions through a table row per
 * output pixel. Launch: pw_staged_launch (igemm_params.h) of a plan made by q8pwconv.hip's pwstream_plan, which decides
 * when it runs and how the channels are split into workgroup columns ("gemm_kernel" 5 forces the short-K kernels).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "pwstream_common.hip.h"

namespace qnnp {

namespace {

/*
 * Staged flavour: 16-byte aligned rows, n % 16 == 0 -- every MobileNet-style expand / project layer. Differences to
 * the kernel above:
 *   - N split: gridDim.y workgroup columns each own `nbp` of the 32-channel blocks (their weights only in LDS), so a
 *     layer with few row blocks and many channels (14x14x96 -> 576: 784 row blocks) still fills the chip, and any N
 *     fits (the whole-matrix kernel stops at 64 KiB of weights);
 *   - a unit's requantized 32 x (nbp*32) block goes to a per-wave LDS image and leaves in row chunks of >= 64
 *     contiguous bytes (whole contiguous 32-row blocks when rows are dense and N is not split): direct 16-byte
 *     stores put 32-byte partial-line writes on the L2 (2.8 TB/s against 5+ for whole lines, ablation);
 *   - the wave's instruction order is  loads(u+1) -> multiply / requantize(u) -> wait -> re-centre(u+1) ->
 *     stores(u): the only vmcnt wait of the loop sits BEFORE the unit's stores, where everything outstanding
 *     (the next rows, the previous unit's stores) has had a whole multiply phase to complete. hipcc counts loads
 *     and stores in one counter and cannot count a run-time number of stores, so with the stores first it waited
 *     for the stores it had just issued (vmcnt(0) at the loop end) -- a full store round trip per unit per wave.
 *   - the loads are always issued (clamped unit index): a branch around them makes the outstanding count
 *     path-dependent and costs the same vmcnt(0).
 */
/* SEQ / FULL: the requantization flavour (requant.hip.h), chosen on the host -- one kernel per flavour, so that the
 * common ones are not charged the registers of the rare ones */
/* TAB: the output table flavour, as the kernel above; the workgroup's copy of the table lies behind the four waves'
 * images, is written in front of the prologue's barrier and is applied by stream_copy_out. Without RES only. */
template <int KB, int VEC, int SEQ, bool FULL, bool RES = false, bool TAB = false>
__global__ __launch_bounds__(kThreads, staged_waves(KB))
void q8_pw_stream_staged_kernel(const IgemmParams p, const uint32_t nbp, const uint32_t log_cpr_arg)
{
  const uint32_t log_cpr = log_cpr_arg & 31u;
  const bool dense8 = (log_cpr_arg >> 31) != 0u;           // stream_copy_out's third mode
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  const uint32_t row_in_block = lane & 31u;
  const uint32_t khalf = lane >> 5;

  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;
  const uint32_t nb0 = blockIdx.y * nbp;                  // this workgroup column's channel blocks
  const uint32_t nbn = min(nbp, nblocks - nb0);
  const uint32_t c0 = nb0 * 32u;                          // first channel
  const uint32_t cw = min(p.n - c0, nbn * 32u);           // valid bytes per row of the chunk (n % 16 == 0, or dense8)
  const bool whole_dense = !dense8 && gridDim.y == 1 && p.output_stride == p.n;
  const uint32_t pitch = whole_dense ? p.n : (16u << log_cpr);   // row pitch of the image

  // ---- once per workgroup: the column's weight fragments and bias2 into LDS (LDS-DMA) ----
  {
    const uint32_t frags = nbn * KB;
    for (uint32_t f = wave; f < frags; f += kWaves) {
      const uint32_t nb = f / KB;
      const uint32_t kb = f - nb * KB;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (p.packed_w + (static_cast<uint64_t>(nb0 + nb) * kblocks + kb) * 1024 + lane * 16),
          (__attribute__((address_space(3))) void*) (lds + f * 1024), 16, 0, 0);
    }
    uint8_t* lds_bias = lds + nbp * KB * 1024;
    const uint32_t bias_chunks = nbn * 8u;                // 16-byte pieces
    // (lane forms of the requantization: the accumulators start from bias + 2^31, the second half of the pair table)
    const int32_t* bias_src = rq_is_lane<SEQ>() ? p.bias2u : p.bias2;
    for (uint32_t q0 = wave * 64; q0 < bias_chunks; q0 += kThreads) {
      const uint32_t q = min(q0 + lane, bias_chunks - 1); // the tail lanes repeat the last piece (same bytes)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (reinterpret_cast<const uint8_t*>(bias_src + c0) + q * 16),
          (__attribute__((address_space(3))) void*) (lds_bias + q0 * 16), 16, 0, 0);
    }
  }
  const uint8_t* lds_w = lds + lane * 16;
  const uint32_t bias_bytes = (nbp * 128u + 1023u) & ~1023u;
  const int4* lds_bias4 = reinterpret_cast<const int4*>(lds + nbp * KB * 1024);
  uint8_t* stage = lds + nbp * KB * 1024 + bias_bytes + wave * (32u * pitch);

  const uint8_t* pad16 = p.fill_table + 0x80 * 16;        // 16 bytes of a' == 0
  const uint32_t k_last = (KB - 1) * 32 + khalf * 16;
  const bool last_lo_ok = k_last < p.k_total;
  const bool last_hi_ok = k_last + 8 < p.k_total;

  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t unit_stride = gridDim.x * kWaves;

  auto load_rows = [&](uint32_t unit, v4i (&a)[KB]) __attribute__((always_inline)) {
    uint32_t m = unit * 32u + row_in_block;
    if (m >= p.rows) m = p.rows - 1;                      // clamped rows are never stored
    const uint8_t* row = p.input + static_cast<uint64_t>(m) * p.input_stride + khalf * 16;
    if (p.offsets_dense != 0) {                           // strided 1x1 convolution (wave-uniform): the row's table entry
      const uint32_t img = p.rpi_magic != 0 ? __umulhi(m, p.rpi_magic) : m / p.rows_per_image;
      const uint32_t pix = m - img * p.rows_per_image;
      row = p.input + static_cast<uint64_t>(img) * p.image_stride + static_cast<uint32_t>(p.offsets[pix]) + khalf * 16;
    }
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
  // raw bytes -> row sum, then re-centred at 128 in place
  auto recentre = [&](v4i (&a)[KB]) __attribute__((always_inline)) -> uint32_t {
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
    rs += __shfl_xor(rs, 32);                             // the other K half of the same row
    return rs;
  };
  const uint32_t raw_to_centred = 128u * 32u * KB;

  uint32_t unit = blockIdx.x * kWaves + wave;
  v4i a[KB];
  load_rows(min(unit, units - 1u), a);
  const uint8_t* lut = nullptr;
  if constexpr (TAB) {
    uint8_t* lds_tab = lds + nbp * KB * 1024 + bias_bytes + kWaves * (32u * pitch);        // behind staged_lds_bytes()
    if (tid < 64u) reinterpret_cast<uint32_t*>(lds_tab)[tid] = reinterpret_cast<const uint32_t*>(p.table)[tid];
    lut = lds_tab;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // weights + bias are in LDS (and the first rows landed)
  __syncthreads();
  if (unit >= units) return;

  {
    using shift0_t = std::integral_constant<int, SEQ>;
    using full_t = std::integral_constant<bool, FULL>;
    const shift0_t shift0{};
    const full_t full{};
    (void) shift0; (void) full;
    uint32_t rs = recentre(a);
    for (;;) {
      const uint32_t next = unit + unit_stride;
      v4i raw[KB];
      load_rows(min(next, units - 1u), raw);              // always issued (the last one of a wave is wasted)
      // (+ 2^31 for the offset rounding sequences, requant.hip.h: the accumulators start from bias + this)
      const int32_t rowterm = with_rq_offset<decltype(shift0)::value>(p.row_coeff * static_cast<int32_t>(rs - raw_to_centred));
      uint64_t row_addend = 0;                              // lane forms: the row term as the multiply-add's addend
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
        const uint8_t* wf = lds_w + nb * (KB * 1024);
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
          const v4i w = *reinterpret_cast<const v4i*>(wf + kb * 1024);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w, a[kb], acc, 0, 0, 0);
        }
        // (every lane takes part in the half-wave exchange inside; a lane's 16 channels exist or not)
        if constexpr (rq_is_lane<SEQ>()) {
          igemm_stage_tile_lane<SEQ, FULL>(acc, row_addend, img, nb * 32, khalf, p, nb * 32 + khalf * 16 < cw);
        } else {
          igemm_stage_tile<decltype(shift0)::value, decltype(full)::value, false, 2>(
              acc, bias4, rowterm, img, nb * 32, khalf, p, nb * 32 + khalf * 16 < cw);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // image complete before it is read back
      // the next unit's rows: first use here, so the wait for them lands before this unit's stores
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kb = 0; kb < KB; kb++) a[kb] = raw[kb];
      rs = recentre(a);
      __builtin_amdgcn_sched_barrier(0);
#ifdef QNNP_ENABLE_ABLATION
      if (p.izp_fill & 1u) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); if (next >= units) break; unit = next; continue; }
#endif
      stream_copy_out<RES, TAB>(stage, whole_dense, log_cpr, unit, c0, cw, p, lane, dense8, lut);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // read back before the next unit overwrites it
      if (next >= units) break;
      unit = next;
    }
  }
}

}  // namespace

/* The instantiations: every KB and requantization flavour with 16-byte loads plain, RES and TAB; with 8-byte loads plain
 * and TAB (a residual rides in the 16-byte-load flavour only). */
int pw_staged_launch(const IgemmParams& p, const PwPlan& plan, hipStream_t stream)
{
  IgemmParams pa = with_ablation_bits(p);
  pa.tiles_n_magic = reciprocal_floor_plus1(p.n);      // dense8: byte offset / n, exact below 2^32 / n
  return with_kb(plan.kb, [&](auto kb) {
    int rc = QNNP_HIP_EINVAL;
    requant_dispatch_lane(p.rq, p.lane, [&](auto seq, auto full) {
      constexpr int KB = decltype(kb)::value;
      constexpr int SEQ = decltype(seq)::value;
      constexpr bool FULL = decltype(full)::value;
      if (plan.vec == 16) {
        if (plan.res) rc = launch_planned<q8_pw_stream_staged_kernel<KB, 16, SEQ, FULL, true>>(kMaxLds, plan, stream, pa, plan.nbp, plan.log_cpr);
        else if (plan.tab) rc = launch_planned<q8_pw_stream_staged_kernel<KB, 16, SEQ, FULL, false, true>>(kMaxLds, plan, stream, pa, plan.nbp, plan.log_cpr);
        else rc = launch_planned<q8_pw_stream_staged_kernel<KB, 16, SEQ, FULL>>(kMaxLds, plan, stream, pa, plan.nbp, plan.log_cpr);
      } else {
        if (plan.tab) rc = launch_planned<q8_pw_stream_staged_kernel<KB, 8, SEQ, FULL, false, true>>(kMaxLds, plan, stream, pa, plan.nbp, plan.log_cpr);
        else rc = launch_planned<q8_pw_stream_staged_kernel<KB, 8, SEQ, FULL>>(kMaxLds, plan, stream, pa, plan.nbp, plan.log_cpr);
      }
    });
    return rc;
  });
}

}  // namespace qnnp
