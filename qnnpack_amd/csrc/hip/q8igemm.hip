/*
 * q8igemm.hip -- uint8 GEMM and implicit-GEMM convolution on CDNA4 matrix cores.
 *
 * Replaces, as whole-operator launches, the reference's per-tile CPU microkernels
 *   q8gemm_ukernel_4x4c2__sse2  (src/q8gemm/4x4c2-sse2.c:14-318)
 *   q8conv_ukernel_4x4c2__sse2  (src/q8conv/4x4c2-sse2.c:14-273)
 * and their pthreadpool tilers compute_q8gemm / compute_q8conv
 * (src/operator-run.c:39-70, 183-217, 797-802, 837-842).
 *
 * Arithmetic (exact int32, bit-identical to the reference definition
 * test/gemm-microkernel-tester.h:213-226 + qnnp_q31_requantize):
 *   v_mfma_i32_32x32x32_i8 multiplies SIGNED int8, so both operands are
 *   re-centred at 128 (a' = a ^ 0x80, w' = w ^ 0x80 -- the latter at pack time)
 *   and the cross terms are restored from a per-row sum of a' and a folded
 *   per-column bias (pack.h). This is the reference's own "XZP" algebra
 *   (src/operator-run.c:727-743) re-centred for a signed matrix core.
 *
 * Kernel 1 (this file, "generic"): q8_igemm_mfma_kernel
 *   - one workgroup = 4 waves; tile BM x BN x 64, BM = 128, BN in {32, 64, 128}
 *   - activations: global -> VGPR -> (^0x80, row-sum) -> LDS, double buffered,
 *     XOR-swizzled 16-B chunks so the ds_read_b128 fragment reads are conflict free
 *   - weights: pre-packed MFMA fragments (pack.h), one coalesced 1-KiB global read
 *     per fragment per wave straight into VGPRs (weights are L2 resident; no LDS)
 *   - convolution gathers activation rows through the device-side int32 offset
 *     table (indirection.c); im2col is never materialised; padding taps read the
 *     input zero point
 *   - fused epilogue: + bias2 + row_coeff * rowsum -> Q31 requantize -> clamp ->
 *     4 channels packed per dword store
 *   - any M/N/K, any pixel strides, any alignment: the activation load width VEC
 *     (16/8/4/1 bytes) is picked per launch from the actual alignment
 *
 * MFMA operand roles: weights are the "A" operand (32 output channels across
 * lanes 0-31), activations the "B" operand (32 rows across lanes 0-31), so each
 * lane ends up with 4 CONSECUTIVE output channels of one row per accumulator
 * quad: C/D layout col = lane & 31 (row m), reg r -> n = (r & 3) + 8*(r >> 2) +
 * 4*(lane >> 5).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "igemm_epilogue.hip.h"
#include "igemm_params.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "requant.hip.h"

namespace {

using qnnp::IgemmParams;
using qnnp::launch_status;
using qnnp::v4i;
using qnnp::v16i;

constexpr int BK = 64;                       // bytes of K per main-loop step
constexpr uint32_t kPadK = 0x80808080u;      // raw bytes whose a' = a ^ 0x80 is zero
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;


template <int VEC>
__device__ __forceinline__ void load_vec(const uint8_t* p, uint32_t (&w)[4], int j);

template <>
__device__ __forceinline__ void load_vec<16>(const uint8_t* p, uint32_t (&w)[4], int) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
template <>
__device__ __forceinline__ void load_vec<8>(const uint8_t* p, uint32_t (&w)[4], int j) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  w[2 * j] = v.x; w[2 * j + 1] = v.y;
}
template <>
__device__ __forceinline__ void load_vec<4>(const uint8_t* p, uint32_t (&w)[4], int j) {
  w[j] = *reinterpret_cast<const uint32_t*>(p);
}
template <>
__device__ __forceinline__ void load_vec<1>(const uint8_t* p, uint32_t (&w)[4], int j) {
  const uint32_t b = *p;
  const int sh = (j & 3) * 8;
  w[j >> 2] = (w[j >> 2] & ~(0xFFu << sh)) | (b << sh);
}

template <int VEC>
__device__ __forceinline__ void fill_vec(uint32_t fill, uint32_t (&w)[4], int j) {
  if constexpr (VEC == 16) {
    w[0] = fill; w[1] = fill; w[2] = fill; w[3] = fill;
  } else if constexpr (VEC == 8) {
    w[2 * j] = fill; w[2 * j + 1] = fill;
  } else if constexpr (VEC == 4) {
    w[j] = fill;
  } else {
    const int sh = (j & 3) * 8;
    w[j >> 2] = (w[j >> 2] & ~(0xFFu << sh)) | ((fill & 0xFFu) << sh);
  }
}

/*
 * WM x WN waves, each computing TM x TN MFMA tiles of 32x32. PERSISTENT over row tiles: a workgroup
 * keeps one channel tile and walks row tiles m = cta_m, cta_m + ctas_m, ...; the activation loads of the
 * next row tile are issued before the epilogue of the current one, so the (latency-bound) global reads
 * overlap the (VALU-bound) requantization instead of alternating with it.
 */
// PC: per-channel requantization (igemm_tile_pc, igemm_epilogue.hip.h) in place of the per-operator sequences; the main
// loop is the same code. The `false` instantiations are the kernels of every per-tensor operator.
template <int WM, int WN, int TM, int TN, int VEC, bool IS_CONV, bool PAD3 = false, bool PC = false>
__global__ __launch_bounds__(WM * WN * 64, (TM * TN >= 4) ? 2 : 3)
void q8_igemm_mfma_kernel(const IgemmParams p_in)
{
  // phase table (strided deconvolutions): blockIdx.y picks one of several GEMM descriptions sharing this launch
  IgemmParams p = p_in;
  if (p_in.phases != nullptr) {
    const qnnp_hip_igemm_phase ph = p_in.phases[blockIdx.y / p_in.phase_groups];
    p.packed_w = ph.packed_w;
    p.bias2 = ph.bias2;
    p.offsets = ph.offsets;
    p.out_rows = ph.out_rows;
    p.rows = ph.rows;
    p.rows_per_image = ph.rows_per_image;
    p.ks = ph.ks;
    p.k_total = ph.k_total;
    p.k_pad = ph.k_pad;
  }
  constexpr int NT = WM * WN * 64;
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  constexpr int CH = (BM * (BK / 16)) / NT;  // 16-byte activation chunks staged per thread per step
  static_assert((BM * (BK / 16)) % NT == 0, "tile/thread mismatch");
  static_assert(CH >= 1, "tile too small");

  // one LDS object only: [2][BM][BK] activation ring | [BM][BN+16] staged output tile | [BM] int32 row sums
  constexpr int OUT_PITCH = BN + 16;
  constexpr int RING_BYTES = 2 * BM * BK;
  constexpr int OUT_BYTES = BM * OUT_PITCH;
  __shared__ __attribute__((aligned(16))) uint8_t lds[RING_BYTES + OUT_BYTES + BM * 4];
  uint8_t* lds_out = lds + RING_BYTES;
  int32_t* lds_rowsum = reinterpret_cast<int32_t*>(lds + RING_BYTES + OUT_BYTES);

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = tid >> 6;
  const uint32_t wm = wave / WN;
  const uint32_t wn = wave % WN;
  const uint32_t g = p_in.phases != nullptr ? blockIdx.y % p_in.phase_groups : blockIdx.y;

  // XCD-aware bijective remap: consecutive logical ids (which share activation row tiles) land on the
  // same XCD / L2 (hardware: block b -> XCD b % 8).
  const uint32_t tiles_n = (p.n_pad + BN - 1) / BN;
  const uint32_t tiles_m = (p.rows + BM - 1) / BM;
  uint32_t logical;
  {
    const uint32_t nwg = gridDim.x;
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t idx = blockIdx.x >> 3;
    const uint32_t q = nwg >> 3, r = nwg & 7u;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const uint32_t n_tile = logical % tiles_n;
  const uint32_t cta_m = logical / tiles_n;
  const uint32_t ctas_m = gridDim.x / tiles_n;

  const uint32_t ksteps = p.k_pad / BK;
  const uint32_t kblocks = p.k_pad / 32;   // 32-deep fragment blocks per column block
  const uint32_t nblocks = p.n_pad / 32;

  // ---- per-thread activation staging assignment: chunk slots are fixed, rows change per row tile ----
  struct RowCtx {
    const uint8_t* base[CH];   // gemm: row base (+group); conv: image base (+group)
    const int32_t* offs[CH];   // conv: this pixel's row of the offset table
    bool valid[CH];
  };
  uint32_t a_lds[CH];          // swizzled byte offset inside one LDS buffer
  uint32_t a_kchunk[CH];       // 0..3: which 16-byte chunk of the K step
#pragma unroll
  for (int q = 0; q < CH; q++) {
    const uint32_t id = q * NT + tid;
    const uint32_t row = id >> 2;
    const uint32_t c = id & 3u;
    a_kchunk[q] = c;
    a_lds[q] = row * BK + ((c ^ ((row >> 2) & 3u)) << 4);
  }
  auto make_ctx = [&](uint32_t m_tile, RowCtx& ctx) {
#pragma unroll
    for (int q = 0; q < CH; q++) {
      const uint32_t row = (q * NT + tid) >> 2;
      const uint32_t m = m_tile * BM + row;
      ctx.valid[q] = m_tile < tiles_m && m < p.rows;
      const uint32_t mm = ctx.valid[q] ? m : 0u;
      if constexpr (IS_CONV) {
        const uint32_t img = mm / p.rows_per_image;
        const uint32_t pix = mm - img * p.rows_per_image;
        ctx.base[q] = p.input + static_cast<uint64_t>(img) * p.image_stride + static_cast<uint64_t>(g) * p.kc;
        ctx.offs[q] = p.offsets + static_cast<uint64_t>(pix) * p.ks;
      } else {
        ctx.base[q] = p.input + static_cast<uint64_t>(mm) * p.input_stride + static_cast<uint64_t>(g) * p.kc;
        ctx.offs[q] = nullptr;
      }
    }
  };

  // global -> registers for K step `kstep` (raw uint8, already filled for padding)
  auto load_chunks = [&](const RowCtx& ctx, uint32_t kstep, uint32_t (&regs)[CH][4]) {
#pragma unroll
    for (int q = 0; q < CH; q++) {
      const uint32_t kk0 = kstep * BK + a_kchunk[q] * 16;
      regs[q][0] = kPadK; regs[q][1] = kPadK; regs[q][2] = kPadK; regs[q][3] = kPadK;
      uint32_t tap = 0, ch = kk0;
      if constexpr (IS_CONV) {
        tap = kk0 / p.kc;
        ch = kk0 - tap * p.kc;
      }
      if constexpr (VEC == 1 && !PAD3) {
        // Byte gathers (channel counts that are not a multiple of 4), BRANCH-FREE: every load is issued -- an address
        // that must not be read is replaced by the row's / image's base, the value by the zero point or the K padding
        // afterwards. As sixteen `if (inside) load` per chunk this path held an exec mask per byte: 195 spilled SGPRs +
        // 285-339 spilled VGPRs inside the K loop, and a wild address when unrelated code moved its allocation (round 3).
#pragma unroll
        for (int d = 0; d < 4; d++) {
          uint32_t v = 0;
#pragma unroll
          for (int jj = 0; jj < 4; jj++) {
            const uint32_t kk = kk0 + d * 4 + jj;
            const bool in_k = ctx.valid[q] && kk < p.k_total;
            bool real = in_k;
            uint32_t rel = kk;
            if constexpr (IS_CONV) {
              const uint32_t tap_c = tap < p.ks ? tap : p.ks - 1u;     // (beyond k_total: any entry of the pixel's row)
              const int32_t off = ctx.offs[q][tap_c];
              real = in_k && off >= 0;
              rel = static_cast<uint32_t>(off) + ch;
              ch += 1;
              if (ch >= p.kc) { ch = 0; tap += 1; }
            }
            uint32_t b = ctx.base[q][real ? rel : 0u];
            b = real ? b : (in_k ? (p.izp_fill & 0xFFu) : 0x80u);
            v |= b << (8 * jj);
          }
          regs[q][d] = v;
        }
        continue;
      }
#pragma unroll
      for (int j = 0; j < 16 / VEC; j++) {
        const uint32_t kk = kk0 + j * VEC;
        if (ctx.valid[q] && kk < p.k_total) {
          if constexpr (IS_CONV) {
            const int32_t off = ctx.offs[q][tap];
            if (off >= 0) {
              if constexpr (PAD3) {
                // 3-channel pixel: one unaligned dword (the 4th byte belongs to the next pixel and is
                // replaced by K padding); the very last pixel of the tensor is fetched bytewise
                const uint8_t* src = ctx.base[q] + off;
                uint32_t v;
                if (src + 4 <= p.input_end) {
                  v = *reinterpret_cast<const u32_unaligned*>(src);
                } else {
                  v = static_cast<uint32_t>(src[0]) | (static_cast<uint32_t>(src[1]) << 8) |
                      (static_cast<uint32_t>(src[2]) << 16);
                }
                regs[q][j] = (v & 0x00FFFFFFu) | 0x80000000u;
              } else {
                load_vec<VEC>(ctx.base[q] + off + ch, regs[q], j);
              }
            } else {
              fill_vec<VEC>(p.izp_fill, regs[q], j);   // padding tap: a == input zero point
            }
          } else {
            load_vec<VEC>(ctx.base[q] + kk, regs[q], j);
          }
        }
        if constexpr (IS_CONV) {
          ch += VEC;
          if (ch >= p.kc) { ch = 0; tap += 1; }   // VEC divides kc, so taps never straddle a vector
        }
      }
    }
  };

  int32_t rowsum_part[CH];
  // registers -> LDS: recentre at 128, accumulate the row sum of a'
  auto store_chunks = [&](uint32_t buf, const uint32_t (&regs)[CH][4]) {
#pragma unroll
    for (int q = 0; q < CH; q++) {
      v4i x;
      x.x = static_cast<int>(regs[q][0] ^ kPadK);
      x.y = static_cast<int>(regs[q][1] ^ kPadK);
      x.z = static_cast<int>(regs[q][2] ^ kPadK);
      x.w = static_cast<int>(regs[q][3] ^ kPadK);
      int32_t s = rowsum_part[q];
      s = __builtin_amdgcn_sdot4(x.x, 0x01010101, s, false);
      s = __builtin_amdgcn_sdot4(x.y, 0x01010101, s, false);
      s = __builtin_amdgcn_sdot4(x.z, 0x01010101, s, false);
      s = __builtin_amdgcn_sdot4(x.w, 0x01010101, s, false);
      rowsum_part[q] = s;
      *reinterpret_cast<v4i*>(lds + buf * (BM * BK) + a_lds[q]) = x;
    }
  };

  // weight fragments: lane l reads its 16 bytes of the (column block, K block) panel
  const uint32_t nb0 = n_tile * (BN / 32) + wn * TN;   // first 32-column block of this wave
  const int8_t* w_lane = p.packed_w + (static_cast<uint64_t>(g) * nblocks * kblocks) * 1024 + lane * 16;
  auto load_wfrags = [&](uint32_t kstep, v4i (&wf)[TN][2]) {
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      const uint32_t nb = nb0 + tn;
#pragma unroll
      for (int ksub = 0; ksub < 2; ksub++) {
        if (nb < nblocks) {
          const uint32_t kb = kstep * 2 + ksub;
          wf[tn][ksub] = *reinterpret_cast<const v4i*>(
              w_lane + (static_cast<uint64_t>(nb) * kblocks + kb) * 1024);
        } else {
          wf[tn][ksub] = v4i{0, 0, 0, 0};
        }
      }
    }
  };

  const uint32_t frag_row0 = wm * (TM * 32) + (lane & 31u);
  const uint32_t frag_khalf = lane >> 5;

  RowCtx ctx, ctx_next;
  uint32_t a_regs[CH][4];
  v4i w_cur[TN][2];
  v4i w_nxt[TN][2];

  make_ctx(cta_m, ctx);
  load_chunks(ctx, 0, a_regs);
  load_wfrags(0, w_cur);
  uint32_t step = 0;                           // global K-step counter: LDS ring slot = step & 1

  for (uint32_t m_tile = cta_m; m_tile < tiles_m; m_tile += ctas_m) {
    v16i acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; tm++)
#pragma unroll
      for (int tn = 0; tn < TN; tn++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[tm][tn][r] = 0;
#pragma unroll
    for (int q = 0; q < CH; q++) rowsum_part[q] = 0;

    for (uint32_t kstep = 0; kstep < ksteps; kstep++, step++) {
      const uint32_t buf = step & 1u;
      store_chunks(buf, a_regs);
      __syncthreads();
      if (kstep + 1 < ksteps) {
        load_chunks(ctx, kstep + 1, a_regs);
        load_wfrags(kstep + 1, w_nxt);
      } else {
        // last K step of this row tile: fetch the first step of the NEXT row tile now, so its latency
        // hides under this tile's MFMAs and epilogue
        make_ctx(m_tile + ctas_m, ctx_next);
        load_chunks(ctx_next, 0, a_regs);
        if (ksteps > 1) load_wfrags(0, w_nxt);
      }
      const uint8_t* a_tile = lds + buf * (BM * BK);
#pragma unroll
      for (int ksub = 0; ksub < 2; ksub++) {
        v4i af[TM];
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
          const uint32_t row = frag_row0 + tm * 32;
          const uint32_t chunk = (ksub * 2 + frag_khalf) ^ ((row >> 2) & 3u);
          af[tm] = *reinterpret_cast<const v4i*>(a_tile + row * BK + (chunk << 4));
        }
#pragma unroll
        for (int tm = 0; tm < TM; tm++)
#pragma unroll
          for (int tn = 0; tn < TN; tn++)
            acc[tm][tn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(w_cur[tn][ksub], af[tm], acc[tm][tn], 0, 0, 0);
      }
      if (ksteps > 1) {
#pragma unroll
        for (int tn = 0; tn < TN; tn++) {
          w_cur[tn][0] = w_nxt[tn][0];
          w_cur[tn][1] = w_nxt[tn][1];
        }
      }
      // no second barrier: the next step writes the other ring slot, whose last readers all passed
      // this step's barrier
    }
    ctx = ctx_next;

    // bias of this lane's 4-channel groups (issued before the barrier so the latency hides; L1/L2 resident)
    int4 bias4[TN][4];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
      uint32_t nb = nb0 + tn;
      if (nb >= nblocks) nb = nblocks - 1;       // clamped blocks are never stored
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const uint32_t ncol = nb * 32 + rg * 8 + frag_khalf * 4;
        bias4[tn][rg] = *reinterpret_cast<const int4*>(p.bias2 + static_cast<uint64_t>(g) * p.n_pad + ncol);
      }
    }

    // ---- row sums: the 4 threads that staged one row are adjacent lanes ----
#pragma unroll
    for (int q = 0; q < CH; q++) {
      int32_t s = rowsum_part[q];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      if (a_kchunk[q] == 0) lds_rowsum[(q * NT + tid) >> 2] = s;
    }
    __syncthreads();

    // ---- fused epilogue (igemm_epilogue.hip.h); the requantization flavour is chosen once per tile ----
    if constexpr (PC) {
      const qnnp_requant_pc_entry* table = p.rq_pc + static_cast<uint64_t>(g) * p.n_pad;
      const bool staged = p.store_mode == 2 && p.out_rows == nullptr;
#pragma unroll
      for (int tm = 0; tm < TM; tm++) {
        const uint32_t row = frag_row0 + tm * 32;
        const uint32_t m = m_tile * BM + row;
        const int32_t rowterm = p.row_coeff * lds_rowsum[row];
        uint64_t out_pixel = m;
        if (p.out_rows != nullptr && m < p.rows) {
          const uint32_t img_m = m / p.rows_per_image;
          out_pixel = static_cast<uint64_t>(img_m) * p.out_image_rows +
                      static_cast<uint32_t>(p.out_rows[m - img_m * p.rows_per_image]);
        }
        uint8_t* out_row = p.output + out_pixel * p.output_stride + static_cast<uint64_t>(g) * p.n;
#pragma unroll
        for (int tn = 0; tn < TN; tn++) {
          const uint32_t nb = nb0 + tn;
          if (nb >= nblocks) continue;       // wave-uniform
          if (staged) {
            qnnp::igemm_tile_pc<true>(acc[tm][tn], bias4[tn], rowterm, table + nb * 32, lds_out + row * OUT_PITCH,
                                      (wn * TN + tn) * 32, frag_khalf, true, p);
          } else {
            qnnp::igemm_tile_pc<false>(acc[tm][tn], bias4[tn], rowterm, table + nb * 32, out_row, nb * 32, frag_khalf, m < p.rows, p);
          }
        }
      }
      if (staged) {
        __syncthreads();
        const uint32_t m0 = m_tile * BM;
        const uint32_t n0 = n_tile * BN;
        const uint32_t rows_valid = min(static_cast<uint32_t>(BM), p.rows - m0);
        const uint32_t n_valid = min(static_cast<uint32_t>(BN), p.n - n0);
        qnnp::igemm_copy_out<NT>(
            lds_out, OUT_PITCH, rows_valid, n_valid,
            p.output + static_cast<uint64_t>(m0) * p.output_stride + static_cast<uint64_t>(g) * p.n + n0,
            p.output_stride, tid);
      }
    } else if (p.store_mode == 2 && p.out_rows == nullptr) {
      // staged: requantized tile -> LDS (row-major image of the output) -> line-sized coalesced stores
      qnnp::requant_dispatch_ofs(p.rq, [&](auto shift0, auto full) {
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
          const uint32_t row = frag_row0 + tm * 32;
          const int32_t rowterm = qnnp::with_rq_offset<decltype(shift0)::value>(p.row_coeff * lds_rowsum[row]);
#pragma unroll
          for (int tn = 0; tn < TN; tn++) {
            if (nb0 + tn >= nblocks) continue;       // wave-uniform
            qnnp::igemm_stage_tile<decltype(shift0)::value, decltype(full)::value>(
                acc[tm][tn], bias4[tn], rowterm, lds_out + row * OUT_PITCH, (wn * TN + tn) * 32, frag_khalf, p);
          }
        }
      });
      __syncthreads();
      const uint32_t m0 = m_tile * BM;
      const uint32_t n0 = n_tile * BN;
      const uint32_t rows_valid = min(static_cast<uint32_t>(BM), p.rows - m0);
      const uint32_t n_valid = min(static_cast<uint32_t>(BN), p.n - n0);
      qnnp::igemm_copy_out<NT>(
          lds_out, OUT_PITCH, rows_valid, n_valid,
          p.output + static_cast<uint64_t>(m0) * p.output_stride + static_cast<uint64_t>(g) * p.n + n0,
          p.output_stride, tid);
    } else {
      qnnp::requant_dispatch_ofs(p.rq, [&](auto shift0, auto full) {
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
          const uint32_t row = frag_row0 + tm * 32;
          const uint32_t m = m_tile * BM + row;
          const int32_t rowterm = qnnp::with_rq_offset<decltype(shift0)::value>(p.row_coeff * lds_rowsum[row]);
          uint64_t out_pixel = m;
          if (p.out_rows != nullptr && m < p.rows) {          // scattered rows (deconvolution phases)
            const uint32_t img_m = m / p.rows_per_image;
            out_pixel = static_cast<uint64_t>(img_m) * p.out_image_rows +
                        static_cast<uint32_t>(p.out_rows[m - img_m * p.rows_per_image]);
          }
          uint8_t* out_row = p.output + out_pixel * p.output_stride + static_cast<uint64_t>(g) * p.n;
#pragma unroll
          for (int tn = 0; tn < TN; tn++) {
            const uint32_t nb = nb0 + tn;
            if (nb >= nblocks) continue;       // wave-uniform
            qnnp::igemm_store_tile<decltype(shift0)::value, decltype(full)::value>(
                acc[tm][tn], bias4[tn], rowterm, out_row, nb * 32, frag_khalf, m < p.rows, p);
          }
        }
      });
    }
  }
}

template <int WM, int WN, int TM, int TN, int VEC, bool IS_CONV, bool PAD3 = false, bool PC = false>
int launch_generic(const IgemmParams& p, uint32_t groups, hipStream_t stream)
{
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  const uint32_t tiles_m = (p.rows + BM - 1) / BM;
  const uint32_t tiles_n = (p.n_pad + BN - 1) / BN;
  // persistent over row tiles: exactly as many workgroups as are co-resident on the chip, each walking
  // tiles_m / ctas_m row tiles
  static int blocks_per_cu = 0;       // per instantiation; benign race (same value)
  if (blocks_per_cu == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &nb, q8_igemm_mfma_kernel<WM, WN, TM, TN, VEC, IS_CONV, PAD3, PC>, WM * WN * 64, 0) != hipSuccess || nb < 1) {
      (void) hipGetLastError();
      nb = 2;
    }
    blocks_per_cu = nb;
  }
  const uint32_t target = p.cu_count * static_cast<uint32_t>(blocks_per_cu);
  uint32_t ctas_m = target / (tiles_n * groups);
  if (ctas_m < 1) ctas_m = 1;
  if (ctas_m > tiles_m) ctas_m = tiles_m;
  const dim3 grid(ctas_m * tiles_n, groups, 1);     // (with a phase table `groups` is the number of phases)
  const dim3 block(WM * WN * 64, 1, 1);
  hipLaunchKernelGGL((q8_igemm_mfma_kernel<WM, WN, TM, TN, VEC, IS_CONV, PAD3, PC>), grid, block, 0, stream, p);
  return launch_status();
}

template <int VEC, bool IS_CONV, bool PAD3 = false, bool PC = false>
int dispatch_tile(const IgemmParams& p, uint32_t groups, hipStream_t stream, const char** name)
{
  if (p.n_pad <= 32) {
    *name = PC ? (PAD3 ? "q8_igemm_pc_mfma_128x32_c3" : "q8_igemm_pc_mfma_128x32")
               : (PAD3 ? "q8_igemm_mfma_128x32_c3" : "q8_igemm_mfma_128x32");
    return launch_generic<4, 1, 1, 1, VEC, IS_CONV, PAD3, PC>(p, groups, stream);
  }
  if (p.n_pad <= 64) {
    *name = PC ? (PAD3 ? "q8_igemm_pc_mfma_128x64_c3" : "q8_igemm_pc_mfma_128x64")
               : (PAD3 ? "q8_igemm_mfma_128x64_c3" : "q8_igemm_mfma_128x64");
    return launch_generic<4, 1, 1, 2, VEC, IS_CONV, PAD3, PC>(p, groups, stream);
  }
  *name = PC ? (PAD3 ? "q8_igemm_pc_mfma_128x128_c3" : "q8_igemm_pc_mfma_128x128")
             : (PAD3 ? "q8_igemm_mfma_128x128_c3" : "q8_igemm_mfma_128x128");
  return launch_generic<2, 2, 2, 2, VEC, IS_CONV, PAD3, PC>(p, groups, stream);
}

template <bool IS_CONV, bool PC = false>
int dispatch_vec(const IgemmParams& p, uint32_t groups, uint32_t vec, hipStream_t stream, const char** name)
{
  switch (vec) {
    case 16: return dispatch_tile<16, IS_CONV, false, PC>(p, groups, stream, name);
    case 8: return dispatch_tile<8, IS_CONV, false, PC>(p, groups, stream, name);
    case 4: return dispatch_tile<4, IS_CONV, false, PC>(p, groups, stream, name);
    default: return dispatch_tile<1, IS_CONV, false, PC>(p, groups, stream, name);
  }
}

// What qnnp_hip_igemm_run derives from its arguments before it picks a kernel
struct IgemmSetup {
  IgemmParams p;           // the standard weight image
  IgemmParams pc;          // the zero-point-centred image, where `centred`
  bool centred;
  bool pad3;               // 3-channel slot mode
  uint32_t vec;            // activation load width
  qnnp::ConvGeom geom;
  // the streaming kernels' launch plans (igemm_params.h), made where supported() asks whether the kernel takes the operator --
  // once per run -- and handed to launch(); family None: not asked, or refused
  mutable qnnp::PwPlan pw, longk, gw, c3;
};

// Kernel zero points 127 / 128: the zero-point-centred image (convolution.c / fully-connected.c), with its own bias pair and no
// row term. False: the operator has none.
bool centred_params(const IgemmParams& p, const struct qnnp_hip_igemm_args* a, IgemmParams* pc)
{
  if (a->centre_flip == 0 || a->packed_w_centred == nullptr || a->bias2_centred == nullptr || a->bias2_pair == 0) return false;
  *pc = p;
  pc->packed_w = a->packed_w_centred;
  pc->bias2 = a->bias2_centred;
  pc->bias2u = a->bias2_centred + static_cast<size_t>(a->groups) * a->n_pad;
  pc->a_flip = (a->centre_flip & 0xFFu) * 0x01010101u;
  pc->row_coeff = 0;
  return true;
}

// Argument checks and the parameters every kernel starts from
int derive(const struct qnnp_hip_igemm_args* a, IgemmSetup& s)
{
  if (a == nullptr || a->rows == 0 || a->groups == 0 || a->groups > 65535u) return QNNP_HIP_EINVAL;
  if (a->n_pad % 32 != 0 || a->k_pad % BK != 0 || a->k_pad < a->k_total) return QNNP_HIP_EINVAL;

  IgemmParams& p = s.p;
  p.input = a->input;
  p.output = a->output;
  p.packed_w = a->packed_w;
  p.bias2 = a->bias2;
  p.offsets = a->offsets;
  p.d2s_sh = a->d2s_stride_h;
  p.d2s_sw = a->d2s_stride_w;
  p.d2s_in_h = a->d2s_input_h;
  p.d2s_in_w = a->d2s_input_w;
  p.d2s_nbpp = 0;
  if (a->d2s_stride_h != 0) {
    const uint32_t phases = a->d2s_stride_h * a->d2s_stride_w;
    if (a->offsets != nullptr || a->groups != 1 || phases == 0 || a->n_pad % (32u * phases) != 0 ||
        a->d2s_input_h == 0 || a->d2s_input_w == 0) return QNNP_HIP_EINVAL;
    p.d2s_nbpp = a->n_pad / 32u / phases;
  }
  p.out_rows = a->out_rows;
  p.out_image_rows = a->out_image_rows;
  p.phases = a->phases;
  p.phase_groups = a->groups;
  if (a->phases != nullptr && (a->nphases == 0 || a->nphases * a->groups > 65535u || a->variant != 1 ||
                               a->offsets == nullptr)) return QNNP_HIP_EINVAL;
  if (a->out_rows != nullptr && a->phases == nullptr && (a->offsets == nullptr || a->variant != 1 || a->rows_per_image == 0)) return QNNP_HIP_EINVAL;
  p.rows = a->rows;
  p.rows_per_image = a->rows_per_image;
  p.image_stride = a->image_stride;
  p.n = a->n;
  p.n_pad = a->n_pad;
  p.kc = a->kc_slot;
  p.input_end = a->input + a->input_bytes;
  p.ks = a->ks;
  p.k_total = a->k_total;
  p.k_pad = a->k_pad;
  p.input_stride = a->input_stride;
  p.output_stride = a->output_stride;
  p.row_coeff = a->row_coeff;
  const bool pad3 = a->offsets != nullptr && a->kc == 3 && a->kc_slot == 4 && a->groups == 1;
  if (a->kc_slot != a->kc && !pad3) return QNNP_HIP_EINVAL;
  // padding taps read the input zero point; in 3-channel slot mode the slot's 4th byte is K padding (a' = 0)
  p.izp_fill = pad3 ? ((a->input_zero_point & 0xFFu) * 0x00010101u) | 0x80000000u
                    : (a->input_zero_point & 0xFFu) * 0x01010101u;
  p.rq = qnnp::make_requant_dev(a->rq);
  p.lane = qnnp::make_requant_lane(a->rq);
  p.bias2u = a->bias2_pair != 0 ? a->bias2 + static_cast<size_t>(a->groups) * a->n_pad : nullptr;
  if (p.bias2u == nullptr) p.lane.kind = 0;      // no table to start from: the offset forms
  p.stream_out = a->streaming_mode == 0 ? (qnnp_hip_streaming_stores() != 0 ? 1u : 0u) : (a->streaming_mode == 2 ? 1u : 0u);
  p.a_flip = 0;
  // per-channel requantization: the table, and the operator's clamp and zero point as the definition takes them
  p.rq_pc = a->rq_pc;
  p.pc_lo = a->rq.output_min_less_zero_point;
  p.pc_hi = a->rq.output_max_less_zero_point;
  p.pc_zp = a->rq.output_zero_point;
  // a table row per output pixel with its one tap inside the image: a strided 1x1 convolution without padding taps
  p.offsets_dense = (a->offsets != nullptr && a->ks == 1 && a->kernel_height == 1 && a->kernel_width == 1 && a->groups == 1 &&
                     a->pad_top == 0 && a->pad_left == 0 && a->rows_per_image > 0 && a->output_height > 0 && a->output_width > 0 &&
                     static_cast<uint64_t>(a->output_height - 1) * a->stride_height < a->input_height &&
                     static_cast<uint64_t>(a->output_width - 1) * a->stride_width < a->input_width &&
                     a->rows_per_image == a->output_height * a->output_width) ? 1u : 0u;
  // (rows_per_image == 1 -- one output pixel per image, e.g. a 2x2 input at stride 2 -- has no 32-bit magic: 2^32 / 1 + 1
  //  wraps to 1 and hi32(m * 1) is 0 for every row. It takes the divide, which is m / 1.)
  p.rpi_magic = (p.offsets_dense != 0 && a->rows_per_image > 1 &&
                 static_cast<uint64_t>(a->rows) * a->rows_per_image < (UINT64_C(1) << 32))
                    ? qnnp::reciprocal_floor_plus1(a->rows_per_image) : 0u;
  p.fill_table = qnnp_hip_fill_table();
  p.trace = nullptr;
#ifdef QNNP_ENABLE_ABLATION
  p.trace = static_cast<unsigned long long*>(qnnp_hip_trace_buffer());
#endif
  p.cu_count = qnnp::active_cu_count();

  // widest activation vector the actual alignment allows (a vector never straddles a tap)
  const uintptr_t in_addr = reinterpret_cast<uintptr_t>(a->input);
  uint32_t vec = 1;
  const uint32_t candidates[3] = {16u, 8u, 4u};
  for (uint32_t v : candidates) {
    if (a->kc % v == 0 && a->input_stride % v == 0 && in_addr % v == 0) {
      vec = v;
      break;
    }
  }
  if (pad3) vec = 4;   // one (unaligned) dword per tap
  const uintptr_t out_addr = reinterpret_cast<uintptr_t>(a->output);
  p.store_mode = 0;
  if (a->n % 16 == 0 && a->output_stride % 16 == 0 && out_addr % 16 == 0) {
    p.store_mode = 2;
  } else if (a->n % 4 == 0 && a->output_stride % 4 == 0 && out_addr % 4 == 0) {
    p.store_mode = 1;
  }
  s.pad3 = pad3; s.vec = vec;

  // Fused residual add: carried by the pointwise streaming kernels' epilogues (what a MobileNet-style project layer runs
  // on) when the residual rows are laid out like the output rows; everything else reports "not folded" and the caller
  // adds in place with the stand-alone kernel.
  p.residual = nullptr;
  p.residual_stride = 0;
  // (the output table is no part of the parameters the plan is made from: launch() hands it to a kernel that carries it)
  p.table = nullptr;
  if (a->table_folded != nullptr) *a->table_folded = 0;
  if (a->table != nullptr && (a->table_folded == nullptr || a->residual != nullptr || reinterpret_cast<uintptr_t>(a->table) % 4 != 0)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->residual_folded != nullptr) *a->residual_folded = 0;
  if (a->residual != nullptr) {
    if (a->residual_add == nullptr || a->residual_folded == nullptr) return QNNP_HIP_EINVAL;
    const uintptr_t res_addr = reinterpret_cast<uintptr_t>(a->residual);
    const uint32_t align = p.store_mode == 2 ? 16u : 4u;
    if (p.store_mode != 0 && a->groups == 1 && a->d2s_stride_h == 0 && a->offsets == nullptr &&
        a->residual_stride == a->output_stride && res_addr % align == 0) {
      p.residual = a->residual;
      p.residual_stride = a->residual_stride;
      p.add = *a->residual_add;
    }
  }
  qnnp::ConvGeom& geom = s.geom;
  geom.H = a->input_height; geom.W = a->input_width; geom.OH = a->output_height; geom.OW = a->output_width;
  geom.KH = a->kernel_height; geom.KW = a->kernel_width; geom.sh = a->stride_height; geom.sw = a->stride_width;
  geom.dh = a->dilation_height; geom.dw = a->dilation_width; geom.pad_top = a->pad_top; geom.pad_left = a->pad_left;
  s.centred = centred_params(p, a, &s.pc);
  s.pw = s.longk = s.gw = s.c3 = qnnp::PwPlan{};
  return QNNP_HIP_OK;
}

// A plan: the launcher (Generic: this file's tile kernel), the weight image it runs on (Rowsum: the standard image and its row
// term with a_flip = 0x80808080, q8gemm256x.hip's ROWSUM flavour) and the launcher's flavour argument: wave / row-slot flavour,
// 128-row tile width, gemm256c opt, or gemm256_launch's `lean` (0 never, 1 where supported, 2 forced) with the kBig* flags.
enum class Kernel : uint8_t { Generic, Wave, Ws16s, Patch, Lds, Rows16, Rows32, C3, Mid, U, Pw, LongK, Gw, Big, BigC, BigX };
enum class Image : uint8_t { Standard, Centred, Rows, Rowsum };
constexpr uint32_t kBigWaves4 = 4u, kBigRows128 = 8u, kBigPingpong = 16u;
struct IgemmPlan { Kernel kernel; Image image; uint32_t option; };

// "gemm_kernel" codes (include/qnnpack_gfx950_test.h). 0 is the automatic choice; codes not named here (1, and 13 / 31 when
// they reach this function) take the generic tile kernel.
enum : int {
  kCodeBig = 2, kCodeLds = 3, kCodeBigWaves4 = 4, kCodePw = 5, kCodeGw = 6, kCodeC3 = 7, kCodeWave = 8, kCodeLongK = 9,
  kCodeBigRows128 = 10, kCodeBigPingpong = 11, kCodeWaveReg = 12, kCodeRows = 14, kCodeBigLean = 15, kCodeBigWaves4Lean = 16,
  kCodeBigC = 20, kCodeBigCAB = 21, kCodePatch = 22, kCodeBigX = 23, kCodeMid = 24, kCodeMid64 = 25, kCodeMid128 = 26,
  kCodeWaveWs32 = 27, kCodeBigXRowsum = 28, kCodeU = 29, kCodeRowsLds = 30, kCodeWs16s = 32,
};

// What each code forces. 4 / 10 / 11 / 16 are refused by gemm256_launch outside measurement builds.
IgemmPlan forced_plan(int code, Image wave_image)
{
  switch (code) {
    case kCodeBig: return {Kernel::Big, Image::Standard, 0u};   // the general flavour, for A/B
    case kCodeBigWaves4: return {Kernel::Big, Image::Standard, kBigWaves4};
    case kCodeBigRows128: return {Kernel::Big, Image::Standard, kBigRows128};
    case kCodeBigPingpong: return {Kernel::Big, Image::Standard, kBigPingpong};
    case kCodeBigLean: return {Kernel::Big, Image::Standard, 2u};
    case kCodeBigWaves4Lean: return {Kernel::Big, Image::Standard, kBigWaves4 | 2u};
    case kCodeBigC: return {Kernel::BigC, Image::Centred, 0u};
    case kCodeBigCAB: return {Kernel::BigC, Image::Centred, 2u};
    case kCodeBigX: return {Kernel::BigX, Image::Centred, 0u};
    case kCodeBigXRowsum: return {Kernel::BigX, Image::Rowsum, 0u};
    case kCodeMid: return {Kernel::Mid, Image::Centred, 0u};
    case kCodeMid64: return {Kernel::Mid, Image::Centred, 64u};
    case kCodeMid128: return {Kernel::Mid, Image::Centred, 128u};
    case kCodeU: return {Kernel::U, Image::Standard, 0u};
    case kCodePw: return {Kernel::Pw, Image::Standard, 0u};
    case kCodeLongK: return {Kernel::LongK, Image::Standard, 0u};
    case kCodeGw: return {Kernel::Gw, Image::Standard, 0u};
    case kCodeC3: return {Kernel::C3, Image::Standard, 0u};
    case kCodeLds: return {Kernel::Lds, Image::Standard, 0u};
    case kCodePatch: return {Kernel::Patch, Image::Standard, 0u};
    case kCodeWs16s: return {Kernel::Ws16s, Image::Centred, 0u};
    case kCodeWave: return {Kernel::Wave, wave_image, 0u};
    case kCodeWaveReg: return {Kernel::Wave, wave_image, 1u};    // the round-2 register-path kernel
    case kCodeWaveWs32: return {Kernel::Wave, wave_image, 2u};   // the 32x32x32 weight-stationary kernel (A/B)
    case kCodeRows: return {Kernel::Rows16, Image::Rows, 1u};     // the register-path kernel
    case kCodeRowsLds: return {Kernel::Rows16, Image::Rows, 2u};  // the LDS-staged kernel or nothing
    default: return {Kernel::Generic, Image::Standard, 0u};
  }
}

// The parameters of a plan's image; `built` holds the ones made here
const IgemmParams& image_params(const IgemmSetup& s, const struct qnnp_hip_igemm_args* a, Image image, IgemmParams& built)
{
  if (image == Image::Standard) return s.p;
  if (image == Image::Centred) return s.pc;
  built = s.p;
  if (image == Image::Rowsum) built.a_flip = 0x80808080u;
  if (image == Image::Rows && a->bias2_rows != nullptr) {   // the row-slot image centred on kernel zero point 127: no row term
    built.bias2 = a->bias2_rows;
    built.bias2u = a->bias2_rows + a->n_pad;
    built.row_coeff = 0;
    built.a_flip = 0x7F7F7F7Fu;
  }
  return built;
}

// The 256x256 kernels on a recentred image (q8gemm256c.hip / q8gemm256x.hip), beyond what the 256x256 kernel itself needs
bool big_image_ok(const IgemmSetup& s, const struct qnnp_hip_igemm_args* a, Image image)
{
  IgemmParams built;
  const bool has_image = image == Image::Centred ? s.centred : s.p.bias2u != nullptr;
  return has_image && qnnp::gemm256c_supported(image_params(s, a, image, built), s.vec);
}

// The streaming plan of a kernel that has one (supported() made it), else nullptr
const qnnp::PwPlan* stream_plan(const IgemmSetup& s, Kernel k)
{
  switch (k) {
    case Kernel::Pw: return &s.pw;
    case Kernel::LongK: return &s.longk;
    case Kernel::Gw: return &s.gw;
    case Kernel::C3: return &s.c3;
    default: return nullptr;
  }
}

// Whether a kernel takes the operator: its *_supported predicate and what the dispatch adds to it. For the streaming kernels
// the predicate is "the plan succeeds", and the plan stays in `s` for launch(): an attached output table is no part of the
// parameters, so the plan is asked beside them whether the launch would carry it.
bool supported(const IgemmSetup& s, const struct qnnp_hip_igemm_args* a, Kernel k, Image image = Image::Standard)
{
  const IgemmParams& p = s.p;
  const bool direct = a->offsets != nullptr && !s.pad3 && a->rows_per_image > 0;   // the direct convolutions
  const uint32_t batch = direct ? a->rows / a->rows_per_image : 0u;
  switch (k) {
    case Kernel::Wave: return direct && p.store_mode == 2 && qnnp::convwave_supported(p, s.geom, a->groups, s.vec, batch);
    case Kernel::Ws16s: return s.centred && a->groups == 1 && direct && qnnp::convws16s_supported(s.pc, s.geom, a->groups, s.vec, batch);
    case Kernel::Patch: return direct && qnnp::convpatch_supported(p, s.geom, a->groups, s.vec, batch);
    case Kernel::Lds: return direct && a->output_stride % 16 == 0 && qnnp::convlds_supported(p, s.geom, a->groups, s.vec);
    // (store_mode 1 with channels % 8 == 0: ShuffleNet's 3 -> 24 layer -- the kernel checks the 8-byte alignment it needs itself)
    case Kernel::Rows16:
      return s.pad3 && (p.store_mode == 2 || (p.store_mode == 1 && a->n % 8u == 0)) &&
             qnnp::conv_c3rows_supported(p, s.geom, a->groups, a->packed_w_rows16, a->kc);
    case Kernel::Rows32: return s.pad3 && p.store_mode == 2 && qnnp::conv_c3rows32_supported(p, s.geom, a->groups, a->packed_w_rows16, a->kc);
    case Kernel::C3: return s.pad3 && qnnp::convstream_c3_plan(p, a->groups, &s.c3);
    case Kernel::Mid: return !s.pad3 && s.centred && a->groups == 1 && qnnp::gemm128x_supported(s.pc, s.vec);
    case Kernel::U: return !s.pad3 && qnnp::gemm128u_supported(p);
    case Kernel::Pw: return !s.pad3 && qnnp::pwstream_plan(p, a->groups, s.vec, a->table != nullptr, &s.pw);
    case Kernel::LongK: return !s.pad3 && qnnp::pwstream_longk_plan(p, a->groups, s.vec, a->table != nullptr, &s.longk);
    case Kernel::Gw: return !s.pad3 && qnnp::pwstream_gw_plan(p, a->groups, s.vec, a->table != nullptr, &s.gw);
    case Kernel::Big: return !s.pad3 && qnnp::gemm256_supported(p, s.vec);
    case Kernel::BigC: case Kernel::BigX: return supported(s, a, Kernel::Big) && big_image_ok(s, a, image);
    case Kernel::Generic: break;
  }
  return true;
}

// The kernel choice. It makes no HIP call. QNNP_HIP_EINVAL: a forced kernel that does not take the operator.
int make_plan(const IgemmSetup& s, const struct qnnp_hip_igemm_args* a, IgemmPlan* plan)
{
  const Image wave_image = s.centred && a->groups == 1 ? Image::Centred : Image::Standard;
  // Per-channel operators: the per-channel flavour of the generic kernel, before any other rule. It is the only kernel that
  // reads the table, so a forced code other than the generic kernel's is refused, never run per tensor.
  if (a->rq_pc != nullptr) {
    if ((a->variant != 0 && a->variant != 1) || s.p.d2s_sh != 0 || a->residual != nullptr) return QNNP_HIP_EINVAL;
    *plan = IgemmPlan{Kernel::Generic, Image::Standard, 0u};
    return QNNP_HIP_OK;
  }
  if (s.p.d2s_sh != 0 && a->variant != kCodePw) return QNNP_HIP_EINVAL;   // depth-to-space exists in the streaming kernel only
  if (a->variant != 0) {
    *plan = forced_plan(a->variant, wave_image);
    // 14 / 30: the 32-byte-slot flavour for 5- and 7-row windows (ResNet's 7x7 entry layer) where the 16-byte one refuses
    if (plan->kernel == Kernel::Rows16 && !supported(s, a, Kernel::Rows16)) plan->kernel = Kernel::Rows32;
    // 28: kernel zero point 128 has no row term -- gemm256x_launch would run (and report) the centred flavour, which is 23's
    if (plan->image == Image::Rowsum && s.p.row_coeff == 0) return QNNP_HIP_EINVAL;
    return supported(s, a, plan->kernel, plan->image) ? QNNP_HIP_OK : QNNP_HIP_EINVAL;
  }
  auto pick = [plan](Kernel k, Image image = Image::Standard, uint32_t option = 0u) { *plan = IgemmPlan{k, image, option}; return QNNP_HIP_OK; };
  auto pick_mid = [&]() { return pick(Kernel::Mid, Image::Centred); };
  // 3x3 / stride 1 / dilation 1 windows with 32 or 64 channels in and out (BASELINE configs[2]): one wave per 8x8 block of
  // positions, patches streamed by LDS-DMA, no barriers (q8convwave.hip) -- 31 us against 37.7 us for the LDS-tiled
  // kernel on configs[2], same box. Other windows the wave kernel accepts run on it only when forced.
  const qnnp::ConvGeom& g = s.geom;
  const bool wave_k33 = g.KH == 3 && g.KW == 3 && g.sh == 1 && g.sw == 1 && g.dh == 1 && g.dw == 1;
  if (wave_k33 && a->rows >= 16384u && supported(s, a, Kernel::Wave)) return pick(Kernel::Wave, wave_image);
  // (round 6) dense 3x3 / stride 1 with 16 / 32 / 48 / 64 input channels and a centred image (SqueezeNet's fire modules): the
  // weight-stationary kernel with the channel count as a template argument (q8convws16s.hip)
  // (auto: everything but 64 -> 32 / 64, which the rule above has taken; 64 -> 256 leaves the patch kernel: 27 x 27 24.7 -> 19.5 us,
  //  13 x 13 9.4 -> 9.0: profiles/r06/conv3x3_small_channels_r06y.txt)
  if (a->rows >= 16384u && supported(s, a, Kernel::Ws16s)) return pick(Kernel::Ws16s, Image::Centred);
  // Dense 3x3 with many channels (ResNet's 128 / 256 / 512-channel layers): patch in LDS, weights streamed (q8convpatch.hip)
  if (a->rows >= 4096u && supported(s, a, Kernel::Patch)) return pick(Kernel::Patch);
  // Dense convolutions with power-of-two channel counts: LDS-tiled direct convolution (input read once).
  if (a->kernel_height * a->kernel_width > 1 && supported(s, a, Kernel::Lds)) return pick(Kernel::Lds);
  // 3-channel images (first layers) with dense pixels: one 16-byte fetch per kernel row (q8convc3.hip), then its 32-byte-slot
  // flavour for 5- and 7-row windows; each the LDS-staged kernel where its plan takes the shape
  if (a->rows >= 2048u && supported(s, a, Kernel::Rows16)) return pick(Kernel::Rows16, Image::Rows);
  if (a->rows >= 2048u && supported(s, a, Kernel::Rows32)) return pick(Kernel::Rows32, Image::Rows);
  // 3-channel images (first layers): barrier-free streaming kernel with an in-register tap gather.
  if (a->rows >= 2048u && supported(s, a, Kernel::C3)) return pick(Kernel::C3);
  // Mid-size GEMMs on the zero-point-centred image: 128-row tiles of four waves, two or three workgroups per CU (q8gemm128x.hip,
  // round 6). Where auto takes it (measured at batch 128, profiles/r06/mid_gemm_by_forced_kernel_r06d.txt) is decided below,
  // next to the kernel it replaces.
  const bool mid_ok = supported(s, a, Kernel::Mid);
  // (strided 1x1 convolutions over few rows -- ResNet-18's 28x28 128 -> 256 and 14x14 256 -> 512 shortcuts, 25 k / 6 k output pixels:
  //  7.9 -> 6.1 us and 8.2 -> 5.4 against the streaming kernel's table rows; with 100 k rows the streaming kernel keeps them)
  if (mid_ok && a->offsets != nullptr && a->rows <= 32768u && a->k_total >= 128u && a->k_total <= 256u && a->rows >= 2048u) return pick_mid();
  // (round 6: pointwise layers whose channel count forces BYTE stores on the streaming kernel -- ShuffleNet v2's 24 -> 58 / 122 at 56 x 56:
  //  56.3 / 122.1 us -- run on the register-staged 128-row GEMM instead: 36.3 / 78.6 us, profiles/r06/ugemm_by_forced_kernel_r06p.txt)
  // (... and, with the transposed 16-byte stores of that kernel, the streaming kernel's DWORD-store shapes -- channel counts of 4 mod 8 --
  //  from 56 channels up: 56 x 56 24 -> 60 / 68 20.9 / 24.5 -> 17.1 / 22.4 us (profiles/r06/ugemm_transposed_stores_r06v.txt); 24 -> 36
  //  stays, 12.0 against 13.8, and so do multiples of 8 -- 24 -> 88 12.9 against 23.8, 88 -> 88 8.2 against 10.0: run r06w's lists)
  // (SqueezeNet's 13 x 13 512 -> 1000 with a centred image: the 128-row centred GEMM with dword-aligned stores, 25.7 against 27.8 us)
  if (mid_ok && s.p.store_mode == 1 && a->n >= 256u && a->k_total >= 256u && a->rows >= 2048u && a->offsets == nullptr) return pick_mid();
  // (... and wide ones: a channel run of 360 -- ShuffleNet v1 g8's 12 -> 45 as a dense 96 -> 360 -- 31.3 us on the streaming kernel, 21.0 here;
  //  SqueezeNet's 13 x 13 512 -> 1000 35.1 us on the 256-wide GEMM's padding path, 25.5 here: run r06z's lists against r06w's)
  if ((s.p.store_mode == 0 || (s.p.store_mode == 1 && ((a->n % 8u != 0u && a->n >= 56u) || a->n >= 256u))) && a->rows >= 2048u &&
      a->residual == nullptr && supported(s, a, Kernel::U)) return pick(Kernel::U);
  // Short-K pointwise / fully-connected layers over many rows: barrier-free streaming kernel.
  const bool pw_ok = supported(s, a, Kernel::Pw);
  // (round 6: few rows x many channels -- ShuffleNet's last 1x1, 7x7 192 -> 1024 at 6 k rows: the streaming kernel runs one chain per
  //  wave, 8.3 us; the 128-row GEMMs 6.0 (centred image) / 6.8 us (standard image): profiles/r06/ugemm_transposed_stores_r06v.txt)
  const bool few_rows_wide = !s.pad3 && a->rows >= 2048u && a->rows <= 8192u && a->n >= 512u && a->k_total >= 192u &&
      a->residual == nullptr && a->offsets == nullptr;
  if (few_rows_wide && pw_ok && mid_ok) return pick_mid();
  if (few_rows_wide && pw_ok && supported(s, a, Kernel::U)) return pick(Kernel::U);
  if (pw_ok && a->rows >= 2048u) return pick(Kernel::Pw);
  // Long reductions over few rows with 16-byte aligned rows on both sides: weights of a channel column in LDS, every
  // K block of a unit's rows in flight at once.
  const bool lk_ok = supported(s, a, Kernel::LongK);
  // (auto where it measured ahead, batch 128 MobileNetV2: the 14x14 project layers -- 784 row blocks, K = 384 / 576:
  //  8.6 against 10.1 us, 10.8 against 13.0 -- and 7x7x320 -> 1280 with its 40 channel blocks, 11.1 against 12.5 on
  //  the tiled kernel; with ~200 row blocks and few channel blocks the one-wave-per-block kernel below keeps the lead:
  //  7x7x960 -> 160 11.1 against 6.6 us)
  const uint32_t lk_units = (a->rows + 31u) / 32u;
  // (round 5: problems the 256-wide LDS-DMA GEMM takes -- N >= 256, K >= 512, rows >= 2048 -- go THERE, not to the long-K / one-wave
  //  kernels: ResNet-50's 14x14 1024 -> 256 25.4 -> 14.6 us, 7x7 512 -> 2048 28.8 -> 12.0, 7x7 2048 -> 512 41.4 -> 22.4, same box,
  //  profiles/r05/pointwise_rows_by_forced_kernel_r05var.txt)
  //  -- when the channels fill whole 256-wide tiles: MobileNetV2's 7x7 960 -> 320 (a quarter of its second tile is padding) stays
  //  on the one-wave kernel, 11.2 against 13.0 us)
  const bool big_first = a->n >= 256 && a->n % 256u == 0 && a->k_total >= 512 && a->rows >= 2048 && supported(s, a, Kernel::Big);
  // (round 5: many rows with FEW channels -- ResNet-50's 28x28 512 -> 128: the weights of the whole row fit LDS and the flavour with
  //  the next unit's rows in flight streams them; 35 us on the generic tile kernel before)
  const bool lk_many_rows = a->rows > 65536u && a->n_pad <= 128u && a->k_total <= 640u;
  const bool lk_auto = !big_first && (a->rows <= 65536u || lk_many_rows) && (lk_units >= 512u || a->n_pad >= 512u);
  // (round 6: what the long-K kernel took automatically goes to the 128-row centred GEMM where that exists -- MobileNetV2's 14x14 project
  //  layers 7.2 -> 5.6, 8.1 -> 6.2, 9.7 -> 7.3 us, 7x7x320 -> 1280 12.4 -> 7.9, ResNet-50's 28x28 512 -> 128 32.6 -> 21.2)
  if (lk_ok && lk_auto && mid_ok && a->rows >= 2048u) return pick_mid();
  // (... and without a centred image -- K = 464: ShuffleNet v2 x1.0's 7x7 464 -> 1024 -- to the register-staged one: 13.5 -> 10.7 us)
  if (few_rows_wide && lk_ok && lk_auto && supported(s, a, Kernel::U)) return pick(Kernel::U);
  if (lk_ok && lk_auto) return pick(Kernel::LongK);
  // Small problems with a long reduction (late MobileNet layers, classifier heads): one wave per 32x32 block,
  // operands from L2 -- the tiled kernels would launch fewer workgroups than there are CUs.
  const bool gw_ok = supported(s, a, Kernel::Gw);
  // (selected when the 128-row x 128-channel tiling of the generic kernel would not even give ~1.5 workgroups
  //  per CU; MobileNetV2 layer 30 -- 490 tiles -- measured faster on the tiled kernel, layers 19-29 on this one)
  const uint64_t generic_tiles = static_cast<uint64_t>((a->rows + 127u) / 128u) * ((a->n_pad + 127u) / 128u);
  // (round 6: with >= 256 channels the 128-row centred GEMM is ahead -- 7x7x960 -> 320 10.5 -> 8.0 us; 160 channels stay here, 5.9 / 7.0
  //  against 6.0 / 7.8)
  if (gw_ok && generic_tiles <= 400u && !big_first && mid_ok && a->n >= 256u && a->rows >= 2048u) return pick_mid();
  if (gw_ok && generic_tiles <= 400u && !big_first) return pick(Kernel::Gw);
  // Large MFMA-bound problems take the 256x256 LDS-DMA kernel; everything else the generic one.
  const bool big_ok = supported(s, a, Kernel::Big);
  // (strided 1x1 convolutions -- a table row per output pixel, one tap -- from K = 256: ResNet-50's 56x56 stride-2 256 -> 512
  //  70.8 -> 51.3 us on the offset-table flavour of the 256-wide kernel)
  const bool strided_pw = a->offsets != nullptr && a->ks == 1 && a->n % 256u == 0 && a->k_total >= 256;
  const bool big_auto = a->n >= 256 && (a->k_total >= 512 || strided_pw) && a->rows >= 2048;
  // (round 6: launches of at most ~100 tiles of 256 x 256 leave most CUs idle for the length of a long K loop -- ResNet-50's 7x7 2048 -> 512,
  //  50 tiles: 22.1 -> 15.0 us on 128-row tiles, 14x14 1024 -> 256, 98 tiles: 17.1 -> 16.0; from ~200 tiles on the wide kernel leads)
  if (big_auto && mid_ok && static_cast<uint64_t>((a->rows + 255u) / 256u) * ((a->n_pad + 255u) / 256u) <= 100u) return pick_mid();
  // Operators with a zero-point-centred weight image (kernel zero point 127 or 128, q8gemm256c.hip): no row term at all.
  // Round 6: auto takes the v_mfma_i32_16x16x64_i8 flavour (q8gemm256x.hip: 59.1 -> 52.6 us on 4096^3, same box, interleaved;
  // 20 keeps the 32x32x32 one).
  if (big_auto && a->centre_flip != 0 && big_ok && big_image_ok(s, a, Image::Centred)) return pick(Kernel::BigX, Image::Centred);
  // Round 6: every OTHER kernel zero point on the 16x16x64 kernel as well -- the standard image and its row term (15 keeps the lean
  // 32x32x32 kernel it replaces).
  if (big_auto && big_ok && big_image_ok(s, a, Image::Rowsum)) return pick(Kernel::BigX, Image::Rowsum);
  // Round 6: what is left of the 1x1 / fully connected class -- grouped, odd channel counts, unaligned rows -- on the 128 x 128 kernel
  // that stages its activation tile through registers (q8gemm128u.hip; 1 keeps the generic tile kernel).
  if (!(big_ok && big_auto) && supported(s, a, Kernel::U)) return pick(Kernel::U);
  if (big_ok && big_auto) return pick(Kernel::Big, Image::Standard, 1u);
  return pick(Kernel::Generic);
}

int launch(const IgemmSetup& s, const struct qnnp_hip_igemm_args* a, const IgemmPlan& plan, const char** kernel_name)
{
  const IgemmParams& p = s.p;
  IgemmParams built;
  const IgemmParams& q = image_params(s, a, plan.image, built);
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const uint32_t batch = a->rows_per_image > 0 ? a->rows / a->rows_per_image : 0u;
  const char* name = nullptr;
  int rc = QNNP_HIP_EINVAL;
  switch (plan.kernel) {
    case Kernel::Wave: rc = qnnp::convwave_launch(p, s.geom, batch, stream, &name, plan.option, plan.image == Image::Centred ? &s.pc : nullptr); break;
    case Kernel::Ws16s: rc = qnnp::convws16s_launch(q, s.geom, batch, stream, &name); break;
    case Kernel::Patch: rc = qnnp::convpatch_launch(q, s.geom, batch, stream, &name); break;
    case Kernel::Lds: rc = qnnp::convlds_launch(q, s.geom, batch, stream, &name); break;
    case Kernel::Rows16: rc = qnnp::conv_c3rows_launch(q, s.geom, a->packed_w_rows16, stream, &name, plan.option); break;
    case Kernel::Rows32: rc = qnnp::conv_c3rows32_launch(q, s.geom, a->packed_w_rows16, stream, &name, plan.option); break;
    case Kernel::C3: rc = qnnp::convstream_c3_launch(q, s.c3, stream, &name); break;
    case Kernel::Mid: rc = qnnp::gemm128x_launch(q, a->groups, stream, &name, plan.option); break;
    case Kernel::U: rc = qnnp::gemm128u_launch(q, a->groups, stream, &name, plan.option); break;
    // the pointwise streaming kernels carry an attached output table in their epilogues where their LDS has the room for
    // it: the same kernel and grid either way, so the table is handed over here, behind the plan
    case Kernel::Pw:
    case Kernel::LongK:
    case Kernel::Gw: {
      const qnnp::PwPlan& sp = *stream_plan(s, plan.kernel);
      IgemmParams t = q;
      if (sp.tab) t.table = a->table;
      rc = qnnp::pwstream_launch(t, sp, stream, &name);
      if (rc == QNNP_HIP_OK && sp.tab) *a->table_folded = 1;
      break;
    }
    case Kernel::Big:
      rc = qnnp::gemm256_launch(q, a->groups, stream, &name, (plan.option & kBigWaves4) != 0, (plan.option & kBigRows128) != 0,
                                (plan.option & kBigPingpong) != 0, plan.option & 3u);
      break;
    case Kernel::BigC: rc = qnnp::gemm256c_launch(q, a->groups, stream, &name, plan.option); break;
    case Kernel::BigX: rc = qnnp::gemm256x_launch(q, a->groups, stream, &name); break;
    case Kernel::Generic:
      if (a->rq_pc != nullptr) {
        if (s.pad3) rc = dispatch_tile<4, true, true, true>(p, a->groups, stream, &name);
        else if (a->offsets != nullptr) rc = dispatch_vec<true, true>(p, a->phases != nullptr ? a->nphases * a->groups : a->groups, s.vec, stream, &name);
        else rc = dispatch_vec<false, true>(p, a->groups, s.vec, stream, &name);
        break;
      }
      if (s.pad3) rc = dispatch_tile<4, true, true>(p, a->groups, stream, &name);
      else if (a->offsets != nullptr) rc = dispatch_vec<true>(p, a->phases != nullptr ? a->nphases * a->groups : a->groups, s.vec, stream, &name);
      else rc = dispatch_vec<false>(p, a->groups, s.vec, stream, &name);
      break;
  }
  if (kernel_name != nullptr) *kernel_name = name;
  // the pointwise streaming kernels carry the fused residual add in their epilogues
  if (rc == QNNP_HIP_OK && p.residual != nullptr && (plan.kernel == Kernel::Pw || plan.kernel == Kernel::LongK || plan.kernel == Kernel::Gw))
    *a->residual_folded = 1;
  return rc;
}

}  // namespace

extern "C" int qnnp_hip_igemm_run(const struct qnnp_hip_igemm_args* a, const char** kernel_name)
{
  IgemmSetup s;
  IgemmPlan plan;
  int rc = derive(a, s);
  if (rc == QNNP_HIP_OK) rc = make_plan(s, a, &plan);
  return rc == QNNP_HIP_OK ? launch(s, a, plan, kernel_name) : rc;
}

extern "C" int qnnp_hip_igemm_plan(const struct qnnp_hip_igemm_args* a, struct qnnp_hip_igemm_plan* out, const char** kernel_name)
{
  static const uint8_t no_table[1] = {0};
  IgemmSetup s;
  IgemmPlan plan;
  if (out == nullptr) return QNNP_HIP_EINVAL;
  const struct qnnp_hip_igemm_plan nothing{};
  *out = nothing;
  if (kernel_name != nullptr) *kernel_name = nullptr;
  int rc = derive(a, s);
  if (rc != QNNP_HIP_OK) return rc;
  // Without a device there is no fill table, and the streaming kernels' predicates refuse on that. No plan reads the table,
  // so this entry plans as if it were there.
  if (s.p.fill_table == nullptr) s.p.fill_table = s.pc.fill_table = no_table;
  rc = make_plan(s, a, &plan);
  if (rc != QNNP_HIP_OK) return rc;
  out->kernel = static_cast<uint32_t>(plan.kernel);
  out->image = static_cast<uint32_t>(plan.image);
  out->option = plan.option;
  out->vec = s.vec;
  out->store_mode = s.p.store_mode;
  if (const qnnp::PwPlan* sp = stream_plan(s, plan.kernel)) {
    const bool pointwise = plan.kernel != Kernel::C3;
    if (kernel_name != nullptr) *kernel_name = qnnp::pwstream_kernel_name(*sp);
    out->family = static_cast<uint32_t>(sp->family);
    out->kb = sp->kb; out->kvec = sp->vec; out->depth = sp->depth;
    out->d2s = sp->d2s; out->res = sp->res; out->tab = sp->tab; out->pf = sp->pf; out->c3_staged = sp->c3_staged;
    out->seq = sp->seq; out->full = sp->full;
    out->grid_x = sp->grid_x; out->grid_y = sp->grid_y; out->lds_bytes = sp->lds_bytes;
    out->nbp = sp->nbp; out->log_cpr = sp->log_cpr; out->per_cu = sp->per_cu;
    // (as launch() reports them)
    out->residual_folded = pointwise && s.p.residual != nullptr;
    out->table_folded = pointwise && sp->tab;
  }
  return rc;
}
