/*
 * qd8f32gemm4m.hip -- the second launch of the dynamically quantized fully connected operator with MXFP4 weights: OCP
 * Microscaling E2M1 codes, two per byte, and one E8M0 power-of-two scale per output channel and block of THIRTY-TWO K positions
 * (qnnp_gfx950_create_fully_connected_nc_f32_qd8_mxfp4w; include/qnnpack_gfx950_dynamic.h has the definition). No reference
 * counterpart.
 *
 * Twice an E2M1 value is a small integer, w2 in {0, +-1, +-2, +-3, +-4, +-6, +-8, +-12}, so the block runs on the INTEGER
 * matrix cores like qd8f32gemm4s.hip's: ONE v_mfma_i32_16x16x32_i8 is ONE block of a 16 x 16 tile, C = 0, and its result
 * becomes a term of the ordered float chain at once. The scale is 2^(e - 127) and the halving of w2 goes into it: the term is
 * (float) acc_b * 2^(e - 128), a 17-bit integer times a power of two, exact. No float matrix instruction, no tolerance.
 *
 * The weight image (hip/qnnp_hip.h) is qd8f32gemm4s.hip's block-32 pair-fragment image holding the RAW codes: 16 bytes per
 * lane, bytes 0 .. 7 of lane l = 16 g + channel the positions 8 g .. 8 g + 7 of each tile of the pair (low nibble: the even
 * tile, high nibble: the odd one), bytes 8 .. 15 the positions 32 + 8 g .. + 7. The four blocks of a pair, in K order, are
 * (dwords 0 1, low), (dwords 2 3, low), (dwords 0 1, high), (dwords 2 3, high).
 *
 * The decode, in registers, per dword of four codes (mx_decode, qd8_mxfp4.hip.h): the 16-entry table code -> w2 as two 8-entry byte tables held
 * in two register pairs -- the magnitudes {0 1 2 3 | 4 6 8 12} and their negations {0 -1 -2 -3 | -4 -6 -8 -12} --, both
 * looked up by v_perm_b32 with the selector code & 7 (masked: selector values 8 .. 15 mean other things), and a third
 * v_perm_b32 that takes byte i of the one or the other by the code's bit 3 (selector i + 4 * sign). A lookup has no carry,
 * so no byte can borrow from its neighbour, and code 8 (-0) is the byte 0. Operations per dword as compiled: and, perm, perm, shift,
 * and, or, perm = 7 for the low nibbles (the and and the or stay two: v_and_or_b32 takes one literal, and both constants are
 * literals), and one more shift for the high ones: 15 per eight weights of an image dword, where qd8f32gemm4z.hip's unpack
 * has 8.
 *
 * ONE table (hip/qnnp_hip.h), indexed like the weight image per channel and K-tile PAIR, [n_pad / 16][kpairs][16]: four
 * int32 of 256 * wsum2 + e, wsum2 = sum w2 over the block (|wsum2| <= 384) -- one 16-byte load per lane and pair where
 * qd8f32gemm4s.hip has a 16-byte and an 8-byte one, 4 bytes per block against 6, and no scale float is loaded: the exponent and
 * wsum2 are three integer operations per (channel, block), and the exponent enters the term through v_ldexp_f32 (GEMV) or
 * as a float built from it (tile kernel).
 *
 * Per output (r, c):
 *   t_b = ldexp((float) (L_b + zero_offset_r * wsum2), e - 128)      L_b: the block's MFMA result, sum (q - 128) * w2
 *   ysum = ((0 + t_0) + t_1) + ... + t_{nb-1};  y = clamp(ysum * scale_r + bias[c])
 * |L_b| <= 128 * 12 * 32, |acc_b| <= 255 * 12 * 32 = 97920 < 2^17. Blocks between K and the end of the last 64-wide tile hold
 * code 0 and the entry 128 (wsum2 0, exponent 0): their terms are +0.0f, and ysum, which starts at +0.0f, is never -0.0f, so
 * adding them changes no bit. The odd tile of a last pair past k_pad is neither multiplied nor walked.
 *
 *   qd8_f32_mxfp4w_gemv_mfma_16        rows <= 16. The pass, regions, owners, barriers and walk of
 *       qd8_f32_qb4w_b32_gemv_mfma_16 (512 threads per 16-channel block, eight waves with an 8-KiB LDS region each, a pass of
 *       32 K tiles, wave w taking tiles 4 w .. 4 w + 3 = eight blocks = eight MFMAs): per pass and lane two weight loads and
 *       TWO table loads where that kernel has four.
 *   qd8_f32_mxfp4w_gemm_mfma_128x128   rows > 16. The staging, stages, barrier per step, snake order and flush-under-MFMA
 *       schedule of qd8_f32_qb4w_b32_gemm_mfma_128x128; the table entries of step kp + 1 (16 registers where that kernel
 *       holds 24) are requested at the top of step kp. A block's four exponents and four wsum2 are unpacked once per block
 *       and channel column, the exponent as the float 2^(e - 128); the flush is integer multiply-add, convert and ONE fused
 *       multiply-add, exact here because the scale is a power of two (mx_add_term): three vector operations per term where
 *       that kernel has four, 192 per block against 256, in the place that bounds it.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "per_device.h"
#include "qd8_epilogue.hip.h"
#include "qd8_mxfp4.hip.h"
#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

struct Mxfp4wParams {
  Qd8Params q;                                  // w: the block-32 pair fragments of raw E2M1 codes; chan_tab: the bias only
  const v4i* table;                             // [n_pad / 16][kpairs][16]: the pair's four blocks, 256 * wsum2 + e
};

/* ---- 128 x kBN tiles -------------------------------------------------------------------------------------------------- */
constexpr int kTN = 4;                          // accumulator tiles per wave along N: a wave is 64 x 64
constexpr int kBM = 128;
constexpr int kBN = 2 * 16 * kTN;
constexpr int kBK = 64;                         // one K tile; a step is two
constexpr int kAHalf = kBM * kBK;               // 8 KiB: the rows' bytes of one K tile
constexpr int kATile = 2 * kAHalf;
constexpr int kWTile = kBN * kBK;               // 2 kTN pair fragments, packed
constexpr int kWFrags = kWTile / 1024 / 4;      // pair fragments each wave brings in
constexpr int kStage = kATile + kWTile;
constexpr int kGemmThreads = 256;
static_assert(kBN == 128 && kWFrags == 2, "the kernel is named by its tile");

__global__ __launch_bounds__(kGemmThreads, 2)
void qd8_f32_mxfp4w_gemm_mfma_128x128_kernel(const Mxfp4wParams mp)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStage];

  const Qd8Params& p = mp.q;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t wm = wave >> 1, wn = wave & 1u;
  const uint32_t m_tile = blockIdx.x / p.tiles_n;
  const uint32_t n_tile = blockIdx.x - m_tile * p.tiles_n;
  const uint32_t ktiles = p.k_pad / kBK;
  const uint32_t kpairs = (ktiles + 1u) / 2u;
  const uint32_t nblocks = p.n_pad / 16;
  const uint32_t m0 = m_tile * kBM;
  const uint32_t last_row = p.rows - 1u - m0;            // of this tile, relative (m0 < rows)

  // activations and weights are staged as in qd8_f32_qb4w_b32_gemm_mfma_128x128: waves 0 and 1 bring in the even K tile's
  // half, waves 2 and 3 the odd one's; piece pc = (wave & 1) * 256 + i * 64 + lane of a half = (row pc >> 2, slot pc & 3)
  const uint32_t a_half = wave >> 1;
  const uint8_t* a_tile = scalar_ptr(p.a + static_cast<uint64_t>(m0) * p.k_pad + a_half * kBK);
  uint32_t a_src[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t pc = (wave & 1u) * 256u + i * 64u + lane;
    const uint32_t row = pc >> 2, slot = pc & 3u;
    a_src[i] = min(row, last_row) * p.k_pad + ((slot ^ a_swizzle(row)) << 4);
  }
  // weights: pair fragment f = wave * kWFrags + i of the tile = channel block n_tile * (kBN / 16) + f (past the image: the last)
  const uint8_t* w_frag[kWFrags];
#pragma unroll
  for (int i = 0; i < kWFrags; i++) {
    const uint32_t nb = min(n_tile * (kBN / 16) + wave * kWFrags + i, nblocks - 1u);
    w_frag[i] = scalar_ptr(p.w + static_cast<uint64_t>(nb) * kpairs * 1024u);
  }
  // the odd half of a last pair past k_pad is not fetched: it would lie behind the row (behind the tensor, for the last row)
  auto stage = [&](uint32_t kp, uint32_t slot) __attribute__((always_inline)) {
    uint8_t* st = lds + slot * kStage;
    if (2u * kp + a_half < ktiles) {
#pragma unroll
      for (int i = 0; i < 4; i++) dma16_saddr(scalar_ptr(a_tile + kp * (2 * kBK)), a_src[i], st + (wave * 4u + i) * 1024u);
    }
#pragma unroll
    for (int i = 0; i < kWFrags; i++) {
      dma16_saddr(scalar_ptr(w_frag[i] + kp * 1024u), lane * 16u, st + kATile + (wave * kWFrags + i) * 1024u);
    }
  };

  const uint32_t frow = lane & 15u, fg = lane >> 4;
  // the 8-byte operand of block half h of a tile: 16-byte slot 2 h + fg / 2 of the row, its half fg % 2
  uint32_t a_off[2];                                                                        // + tile half * 8192 + tm * 1024
#pragma unroll
  for (uint32_t h = 0; h < 2; h++) {
    a_off[h] = (wm * 64u + frow) * kBK + (((2u * h + (fg >> 1)) ^ a_swizzle(frow)) << 4) + 8u * (fg & 1u);
  }
  const uint32_t w_off = kATile + wn * (kTN * 1024u) + lane * 16u;                        // + tn * 1024
  // the lane's channels c_base + 16 tn: their table entries, per pair (the channel block is wave-uniform; past the image:
  // the last block)
  const uint32_t c_base = n_tile * kBN + wn * (16u * kTN) + frow;
  uint32_t t_chan[kTN];
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) {
    t_chan[tn] = min(n_tile * (kBN / 16) + wn * kTN + tn, nblocks - 1u) * kpairs * 16u + frow;     // < 2^20 * 2^8 * 2^4
  }
  // the lane's sixteen rows: 128 - zp_r
  int32_t zo[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
    const RowQuad rows = qd8_load_rows(m0 + wm * 64u + tm * 16u, p);
#pragma unroll
    for (int r = 0; r < 4; r++) zo[tm][r] = rows.e[r].zero_offset;
  }

  float ysum[4][kTN][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) {
#pragma unroll
      for (int r = 0; r < 4; r++) ysum[tm][tn][r] = 0.0f;
    }
  }

  v4i tab_next[kTN], tab_now[kTN];
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) tab_next[tn] = mp.table[t_chan[tn]];
  stage(0u, 0u);
  for (uint32_t kp = 0; kp < kpairs; kp++) {
    const uint32_t slot = kp & 1u;
    // pair kp and its table entries were requested a step ago; behind the barrier every wave's part has landed and every
    // wave is done reading the other stage
    wait_vmcnt<0>();
    __syncthreads();
    QNNP_PIN();
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) tab_now[tn] = tab_next[tn];
    if (kp + 1u < kpairs) {
      stage(kp + 1u, slot ^ 1u);
#pragma unroll
      for (int tn = 0; tn < kTN; tn++) tab_next[tn] = mp.table[t_chan[tn] + (kp + 1u) * 16u];
    }
    QNNP_PIN();
    const uint8_t* st = lds + slot * kStage;
    v4i fw[kTN];
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) fw[tn] = *reinterpret_cast<const v4i*>(st + w_off + tn * 1024);
    const int blocks = 2u * kp + 1u < ktiles ? 4 : 2;     // 2: the last pair of an odd tile count
    // the pending row: MFMA results whose flush is written behind the next four MFMAs
    v4i t[2][kTN];
    int32_t ws_prev[kTN] = {0, 0, 0, 0};
    float sc_prev[kTN] = {0.0f, 0.0f, 0.0f, 0.0f};
    auto flush = [&](int tm, const v4i (&acc)[kTN], const int32_t (&ws)[kTN], const float (&sc)[kTN]) __attribute__((always_inline)) {
#pragma unroll
      for (int tn = 0; tn < kTN; tn++) {
#pragma unroll
        for (int r = 0; r < 4; r++) ysum[tm][tn][r] = mx_add_term(ysum[tm][tn][r], acc[tn][r], zo[tm][r], ws[tn], sc[tn]);
      }
    };
#pragma unroll
    for (int b = 0; b < 4; b++) {
      if (b < blocks) {
        int32_t ws[kTN];
        float sc[kTN];
        long op[kTN], fa[4];
#pragma unroll
        for (int tn = 0; tn < kTN; tn++) {
          ws[tn] = tab_now[tn][b] >> 8;
          sc[tn] = mx_scale(tab_now[tn][b]);
          op[tn] = mx_operand(fw[tn], b);
        }
#pragma unroll
        for (int tm = 0; tm < 4; tm++) {
          fa[tm] = *reinterpret_cast<const long*>(st + (b >> 1) * kAHalf + a_off[b & 1] + tm * 1024);
        }
#pragma unroll
        for (int tm = 0; tm < 4; tm++) {
#pragma unroll
          for (int j = 0; j < kTN; j++) {
            const int tn = (tm & 1) != 0 ? kTN - 1 - j : j;                // snake: one operand changes per MFMA
            t[tm & 1][tn] = __builtin_amdgcn_mfma_i32_16x16x32_i8(fa[tm], op[tn], v4i{0, 0, 0, 0}, 0, 0, 0);
          }
          // behind this row's MFMAs: the row before it (the last row of the block before, for tm = 0)
          if (tm > 0) flush(tm - 1, t[(tm - 1) & 1], ws, sc);
          else if (b > 0) flush(3, t[1], ws_prev, sc_prev);
        }
#pragma unroll
        for (int tn = 0; tn < kTN; tn++) {
          ws_prev[tn] = ws[tn];
          sc_prev[tn] = sc[tn];
        }
      }
    }
    flush(3, t[1], ws_prev, sc_prev);
    QNNP_PIN();
  }

  float bias[kTN];
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) bias[tn] = p.chan_tab[min(c_base + tn * 16u, p.n_pad - 1u)].bias;
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
    const uint32_t row0 = m0 + wm * 64u + tm * 16u;
    const RowQuad rows = qd8_load_rows(row0, p);
    const uint32_t first = row0 + 4u * fg;
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) {
      const uint32_t c = c_base + tn * 16u;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) {
        const float y = qb4w_finish(ysum[tm][tn][r], rows.e[r], bias[tn], p.out_min, p.out_max);
        if (first + r < p.rows && c < p.n) p.out[static_cast<uint64_t>(first + r) * p.out_stride + c] = y;
      }
    }
  }
}

/* ---- rows <= 16 ------------------------------------------------------------------------------------------------------ */
constexpr int kGemvWaves = 8;
constexpr int kGemvThreads = kGemvWaves * 64;
constexpr int kGemvTiles = 4;                 // K tiles per wave and pass
constexpr int kGemvPairs = kGemvTiles / 2;    // = weight loads and table entries per lane and pass
constexpr int kGemvBlocks = 2 * kGemvTiles;   // blocks, MFMAs and 1-KiB term planes per wave and pass
constexpr int kGemvRegion = kGemvBlocks * 1024;      // a wave's LDS: the staged tiles under the first half of its terms
constexpr int kGemvPass = kGemvWaves * kGemvTiles;   // 32 tiles = 2048 K positions = 64 KiB of LDS
constexpr int kGemvOwners = 4;                // waves 0 .. 3 own the 256 outputs, one per lane
static_assert(kGemvWaves * kGemvRegion == 64 * 1024, "two workgroups per CU");

__global__ __launch_bounds__(kGemvThreads)
void qd8_f32_mxfp4w_gemv_mfma_16_kernel(const Mxfp4wParams mp)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kGemvWaves * kGemvRegion];

  const Qd8Params& p = mp.q;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nb = blockIdx.x;
  const uint32_t ktiles = p.k_pad / 64u;
  const uint32_t kpairs = (ktiles + 1u) / 2u;
  const uint32_t frow = lane & 15u, fg = lane >> 4;

  const v4i* w_block = reinterpret_cast<const v4i*>(p.w + static_cast<uint64_t>(nb) * kpairs * 1024u);
  const v4i* t_chan = mp.table + static_cast<uint64_t>(nb) * kpairs * 16u + frow;
  const uint64_t a_base = scalar_ptr(reinterpret_cast<uint64_t>(p.a));
  const uint32_t a_lane = min(frow, p.rows - 1u) * p.k_pad + fg * 16u;      // rows past the batch re-read the last: never stored
  uint8_t* mine = lds + wave * kGemvRegion;                                   // this wave's tiles of a pass, fragment order
  const uint32_t mine_off = __builtin_amdgcn_readfirstlane(lds_offset(mine));
  // the lane's operand of block half h of a staged tile: staged lane 16 (2 h + fg / 2) + frow, its half fg % 2
  const uint32_t a_piece = ((fg >> 1) * 16u + frow) * 16u + 8u * (fg & 1u);       // + tile * 1024 + h * 512
  // the rows of this lane's accumulator registers, for the terms it produces
  int32_t zo[4];
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) zo[r] = p.rows_tab[min(4u * fg + r, p.rows - 1u)].zero_offset;

  float ysum = 0.0f;                            // owners: output (row 4 fg + wave, channel frow)
  for (uint32_t pass0 = 0; pass0 < ktiles; pass0 += kGemvPass) {
    const uint32_t kt0 = pass0 + wave * kGemvTiles;                          // even: pair kt0 / 2 starts at it
    if (kt0 < ktiles) {
      // pairs and tiles past K re-read the last one (fixed counts; they are left out below). Every counted load of the pass
      // goes out before the first LDS-DMA request.
      v4i fw[kGemvPairs], tab[kGemvPairs];
#pragma unroll
      for (int t = 0; t < kGemvPairs; t++) {
        const uint64_t pair = min(kt0 / 2u + t, kpairs - 1u);
        fw[t] = w_block[pair * 64u + lane];
        tab[t] = t_chan[pair * 16u];
      }
      QNNP_PIN();
#pragma unroll
      for (int t = 0; t < kGemvTiles; t++) {
        const uint32_t kt = min(kt0 + t, ktiles - 1u);
        dma16_saddr_ordered(scalar_ptr(a_base + kt * 64u), a_lane, __builtin_amdgcn_readfirstlane(mine_off + t * 1024u));
      }
      wait_vmcnt<0>();       // the wave reads only what it brought in itself: no barrier
      QNNP_PIN();
      // block j of the wave = pair j / 4, block j % 4 of it = tile j / 2, half j % 2: one MFMA, one term per register
      float term[kGemvBlocks][4];
#pragma unroll
      for (int j = 0; j < kGemvBlocks; j++) {
        const int32_t v = tab[j / 4][j % 4];
        const long fa = *reinterpret_cast<const long*>(mine + (j / 2) * 1024 + (j % 2) * 512 + a_piece);
        const v4i acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(fa, mx_operand(fw[j / 4], j % 4), v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) term[j][r] = mx_term(acc[r], zo[r], v >> 8, (v & 255) - 128);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the LDS reads are done before the terms overwrite the tiles
      // this wave's blocks become their terms: block j at mine + j * 1024, plane r (256 bytes) = accumulator register r
#pragma unroll
      for (int j = 0; j < kGemvBlocks; j++) {
        if (kt0 + j / 2 < ktiles) {
#pragma unroll
          for (int r = 0; r < 4; r++) *reinterpret_cast<float*>(mine + j * 1024 + r * 256 + lane * 4u) = term[j][r];
        }
      }
    }
    __syncthreads();
    // the pass's terms lie in ascending K order: region w, then block j. The owners walk them upward.
    if (wave < kGemvOwners) {
      const uint8_t* plane = lds + wave * 256u + lane * 4u;
#pragma unroll
      for (int w = 0; w < kGemvWaves; w++) {
#pragma unroll
        for (int j = 0; j < kGemvBlocks; j++) {
          if (pass0 + w * kGemvTiles + j / 2 < ktiles) {
            ysum = ysum + *reinterpret_cast<const float*>(plane + w * kGemvRegion + j * 1024);
          }
        }
      }
    }
    __syncthreads();         // every owner has read its terms before the next pass's tiles land on them
  }
  if (wave >= kGemvOwners) return;
  const uint32_t row = 4u * fg + wave;
  const uint32_t c = nb * 16u + frow;            // < n_pad
  const float y = qb4w_finish(ysum, p.rows_tab[min(row, p.rows - 1u)], p.chan_tab[c].bias, p.out_min, p.out_max);
  if (row < p.rows && c < p.n) p.out[static_cast<uint64_t>(row) * p.out_stride + c] = y;
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_qd8_mxfp4w_gemm_run(const struct qnnp_hip_qd8_mxfp4w_gemm_args* b, const char** kernel_name)
{
  using namespace qnnp;
  if (b == nullptr) return QNNP_HIP_EINVAL;
  const struct qnnp_hip_qd8_gemm_args* a = &b->gemm;
  if (a->quantized == nullptr || a->row_table == nullptr || a->packed_w == nullptr || a->channel_table == nullptr ||
      b->block_table == nullptr || a->output == nullptr ||
      (reinterpret_cast<uintptr_t>(a->output) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a->quantized) & 15u) != 0 ||
      (reinterpret_cast<uintptr_t>(a->packed_w) & 15u) != 0 || (reinterpret_cast<uintptr_t>(b->block_table) & 15u) != 0 ||
      a->n == 0 || a->n >= (1u << 24) || a->n_pad != ((a->n + 15u) & ~15u) || a->k_pad == 0 || a->k_pad > 32768u ||
      a->k_pad % 64u != 0 || a->rows > 0x7FFFFFFFu || a->output_stride < a->n) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  Mxfp4wParams mp;
  Qd8Params& p = mp.q;
  p.a = reinterpret_cast<const uint8_t*>(a->quantized);
  p.rows_tab = a->row_table;
  p.w = reinterpret_cast<const uint8_t*>(a->packed_w);      // block-32 pair fragments [n_pad / 16][ceil(k_pad / 128)][1024]
  p.chan_tab = a->channel_table;
  p.out = a->output;
  p.out_stride = a->output_stride;
  p.rows = a->rows;
  p.n = a->n;
  p.n_pad = a->n_pad;
  p.k_pad = a->k_pad;
  p.tiles_n = (a->n + kBN - 1u) / kBN;
  p.out_min = a->output_min;
  p.out_max = a->output_max;
  mp.table = reinterpret_cast<const v4i*>(b->block_table);
  if (a->rows <= 16u) {
    const dim3 grid(a->n_pad / 16u), block(kGemvThreads);
    hipLaunchKernelGGL(qd8_f32_mxfp4w_gemv_mfma_16_kernel, grid, block, 0, stream, mp);
    if (kernel_name != nullptr) *kernel_name = "qd8_f32_mxfp4w_gemv_mfma_16";
    return launch_status();
  }
  const uint64_t tiles = static_cast<uint64_t>((a->rows + kBM - 1u) / kBM) * p.tiles_n;
  if (tiles > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;          // a grid that would wrap is refused, not launched
  const dim3 grid(static_cast<uint32_t>(tiles)), block(kGemmThreads);
  hipLaunchKernelGGL(qd8_f32_mxfp4w_gemm_mfma_128x128_kernel, grid, block, 0, stream, mp);
  if (kernel_name != nullptr) *kernel_name = "qd8_f32_mxfp4w_gemm_mfma_128x128";
  return launch_status();
}
