/*
 * qd8f32gemm4z.hip -- the second launch of the dynamically quantized fully connected operator with UNSIGNED 4-bit weights,
 * block-wise scales and one integer ZERO POINT per output channel and block
 * (qnnp_gfx950_create_fully_connected_nc_f32_qd8_qb4w_zp; include/qnnpack_gfx950_dynamic.h has the definition):
 * w = (u - z) * scale with u, z in [0, 15], the form of AWQ and asymmetric GPTQ weights. No reference counterpart.
 *
 * The weight image is qd8f32gemm4.hip's (1-KiB pair fragments) holding the raw nibbles u; the rows, the row table and the
 * channel table's bias are the int8 operator's; the ordered chain, its one owner per output and the two kernels' shapes are
 * qd8f32gemm4b.hip's. New is WHERE THE ZERO POINT ENTERS: at the unpack, so that the MFMA operand byte is u - z itself, an
 * int8 in [-15, 15], and nothing about the zero point is left for the flush. Per dword of eight nibbles, with
 * zz = z * 0x01010101:
 *   even K tile   (((d & 0x0F0F0F0F) | 0x80808080) - zz) ^ 0x80808080
 *   odd K tile    ((((d >> 4) & 0x0F0F0F0F) | 0x80808080) - zz) ^ 0x80808080
 * Every byte of the minuend is 0x80 + u >= 0x80 and every byte of zz at most 0x0F, so no borrow leaves a byte: byte i of the
 * difference is 0x80 + u_i - z in [0x71, 0x8F], and the exclusive-or turns it into the two's-complement byte u_i - z. Four
 * vector operations per dword where qc4w_even / qc4w_odd need two (one for the odd half).
 *
 * The zero point must be in a register before the block's MFMAs. It comes from the PAIR TABLE (hip/qnnp_hip.h): one
 * uint16 per channel and K-tile pair, [n_pad / 16][ceil(k_pad / 128)][16], low byte = the zero point of the block that holds
 * K tile 2 kp, high byte = that of tile 2 kp + 1 (equal for B >= 128). It is indexed like the weight image, whatever the
 * block size, and is fetched with the weights it belongs to. The block table holds, per 16-channel block nb and K block b,
 * sixteen {scale, wsum = sum (u - z)} at ((nb * nblk + b) * 16 + channel % 16).
 *
 * Per output (r, c):
 *   t_b = (float) (L_b + zero_offset_r * wsum) * scale      L_b: the MFMA sum of the block, sum (q - 128) * (u - z)
 *   ysum = ((0 + t_0) + t_1) + ... + t_{nb-1};  y = clamp(ysum * scale_r + bias[c])
 * The integer is acc_b itself (|L_b| <= 128 * 15 * 256, |acc_b| <= 255 * 15 * 256 < 2^20: the conversion is exact), the
 * scale is the caller's, so t_b has the definition's one rounding with no argument about factors of 16.
 *
 *   qd8_f32_qb4w_zp_gemv_mfma_16        rows <= 16. qd8_f32_qb4w_gemv_mfma_16 with the unpack above: one 512-thread
 *       workgroup per 16-channel block, eight waves, a pass of 64 K tiles of which wave w takes tiles 8 w .. 8 w + 7: its four
 *       weight loads, its four zero-point pairs and its 8 / 4 / 2 block-table entries first, then eight LDS-DMA activation
 *       tiles into its 8-KiB staging region, vmcnt(0), unpack, one accumulator per block. The wave turns its own blocks into
 *       their t_b and, its LDS reads drained, writes them as float32 over the head of its staging region: block j of the
 *       wave at j * 1024, as four 256-byte planes, plane r = rows 4 (l / 16) + r of lane l. Behind one barrier the pass's
 *       terms lie in LDS in ascending K order (region w, then j). The OWNERS are waves 0 .. 3, lane l of wave v owning
 *       output (row 4 (l / 16) + v, channel l % 16): each walks the pass's blocks upward with one conflict-free 4-byte LDS
 *       read and one v_add_f32 per block, ysum in a register across passes. A second barrier frees the staging. No atomics,
 *       64 KiB of LDS. Tiles past k_pad / 64 are neither multiplied nor walked.
 *   qd8_f32_qb4w_zp_gemm_mfma_128x128   rows > 16. qd8_f32_qb4w_gemm_mfma_128x128's data movement and flushes (a K step
 *       is a tile pair, one barrier per step, snake order, a float ysum beside every accumulator register, a flush at every
 *       block boundary while K runs upward). The lane's four zero-point pairs of step kp + 1 are requested at the top of
 *       step kp, ONE STEP AHEAD, and are moved into the registers the unpack reads behind the next step's vmcnt(0): a
 *       step never waits for its zero points under its own MFMAs. Each half unpacks its four weight operands once, ahead
 *       of its sixteen MFMAs.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "per_device.h"
#include "qd8_epilogue.hip.h"
#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

struct Qb4wZpParams {
  Qd8Params q;                                  // w: pair fragments of raw nibbles; chan_tab: the bias only
  const qnnp_hip_qd8_zp_block_entry* btab;      // [n_pad / 16][nblk][16]
  const uint16_t* zpairs;                       // [n_pad / 16][kpairs][16]
  uint32_t nblk;                                // k_pad / block size
};

/* the two MFMA operands of a pair fragment: bytes u - z, the zero point taken from its half of the pair entry */
__device__ __forceinline__ v4i qb4w_zp_operand(const v4i& nibbles, uint32_t z)
{
  const int m = 0x0F0F0F0F, h = static_cast<int>(0x80808080u), zz = static_cast<int>(z * 0x01010101u);
  return (((nibbles & v4i{m, m, m, m}) | v4i{h, h, h, h}) - v4i{zz, zz, zz, zz}) ^ v4i{h, h, h, h};
}
__device__ __forceinline__ v4i qb4w_zp_even(const v4i& d, uint32_t pair) { return qb4w_zp_operand(d, pair & 0xFFu); }
__device__ __forceinline__ v4i qb4w_zp_odd(const v4i& d, uint32_t pair) { return qb4w_zp_operand(d >> 4, pair >> 8); }

/* one term of the ordered sum: sum = the MFMA sum of the block, |sum + zero_offset * wsum| = |acc_b| < 2^20 */
__device__ __forceinline__ float qb4w_zp_term(int32_t sum, int32_t zero_offset, const qnnp_hip_qd8_zp_block_entry& be)
{
  return static_cast<float>(sum + zero_offset * be.wsum) * be.scale;
}

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

template <int kTpb>                             // K tiles per block: 1, 2 or 4
__global__ __launch_bounds__(kGemmThreads, 2)
void qd8_f32_qb4w_zp_gemm_mfma_128x128_kernel(const Qb4wZpParams bp)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStage];

  const Qd8Params& p = bp.q;
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

  // activations and weights are staged as in qd8_f32_qc4w_gemm_mfma_128x128: waves 0 and 1 bring in the even K tile's half,
  // waves 2 and 3 the odd one's; piece pc = (wave & 1) * 256 + i * 64 + lane of a half = (row pc >> 2, slot pc & 3)
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
  const uint32_t a_off = (wm * 64u + frow) * kBK + ((fg ^ a_swizzle(frow)) << 4);       // + half * 8192 + tm * 1024
  const uint32_t w_off = kATile + wn * (kTN * 1024u) + lane * 16u;                        // + tn * 1024
  // the lane's channels c_base + 16 tn: their rows of both tables (the channel block is wave-uniform; past the image: the
  // last block)
  const uint32_t c_base = n_tile * kBN + wn * (16u * kTN) + frow;
  const qnnp_hip_qd8_zp_block_entry* b_chan[kTN];
  const uint16_t* z_chan[kTN];
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) {
    const uint32_t nb = min(n_tile * (kBN / 16) + wn * kTN + tn, nblocks - 1u);
    b_chan[tn] = bp.btab + static_cast<uint64_t>(nb) * bp.nblk * 16u + frow;
    z_chan[tn] = bp.zpairs + static_cast<uint64_t>(nb) * kpairs * 16u + frow;
  }
  // the lane's sixteen rows: 128 - zp_r
  int32_t zo[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
    const RowQuad rows = qd8_load_rows(m0 + wm * 64u + tm * 16u, p);
#pragma unroll
    for (int r = 0; r < 4; r++) zo[tm][r] = rows.e[r].zero_offset;
  }

  v4i acc[4][kTN];
  float ysum[4][kTN][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) {
      acc[tm][tn] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 4; r++) ysum[tm][tn][r] = 0.0f;
    }
  }
  // a block boundary: every accumulator register becomes one term of its output's chain, and starts again
  auto flush = [&](const qnnp_hip_qd8_zp_block_entry (&be)[kTN]) __attribute__((always_inline)) {
#pragma unroll
    for (int tm = 0; tm < 4; tm++) {
#pragma unroll
      for (int tn = 0; tn < kTN; tn++) {
#pragma unroll
        for (int r = 0; r < 4; r++) ysum[tm][tn][r] = ysum[tm][tn][r] + qb4w_zp_term(acc[tm][tn][r], zo[tm][r], be[tn]);
        acc[tm][tn] = v4i{0, 0, 0, 0};
      }
    }
  };
  // sixteen MFMAs of one K tile: the half's activation fragments against its four unpacked weight operands, snake order
  auto multiply = [&](const uint8_t* a_frags, const v4i (&op)[kTN]) __attribute__((always_inline)) {
    v4i fa[4];
#pragma unroll
    for (int tm = 0; tm < 4; tm++) fa[tm] = *reinterpret_cast<const v4i*>(a_frags + tm * 1024);
#pragma unroll
    for (int tm = 0; tm < 4; tm++) {
#pragma unroll
      for (int j = 0; j < kTN; j++) {
        const int tn = (tm & 1) != 0 ? kTN - 1 - j : j;                  // snake: one operand changes per MFMA
        acc[tm][tn] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[tm], op[tn], acc[tm][tn], 0, 0, 0);
      }
    }
  };

  uint32_t z_next[kTN], z_now[kTN];
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) z_next[tn] = z_chan[tn][0];
  stage(0u, 0u);
  for (uint32_t kp = 0; kp < kpairs; kp++) {
    const uint32_t slot = kp & 1u;
    // pair kp and its zero points were requested a step ago; behind the barrier every wave's part has landed and every wave
    // is done reading the other stage
    wait_vmcnt<0>();
    __syncthreads();
    QNNP_PIN();
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) z_now[tn] = z_next[tn];
    if (kp + 1u < kpairs) {
      stage(kp + 1u, slot ^ 1u);
#pragma unroll
      for (int tn = 0; tn < kTN; tn++) z_next[tn] = z_chan[tn][static_cast<uint64_t>(kp + 1u) * 16u];
    }
    // the table entries of the block(s) that end in this step, requested ahead of the MFMAs they land under
    qnnp_hip_qd8_zp_block_entry be0[kTN], be1[kTN];
    const uint32_t b0 = kTpb == 1 ? 2u * kp : (kTpb == 2 ? kp : kp / 2u);
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) {
      if (kTpb != 4 || (kp & 1u) != 0) be0[tn] = b_chan[tn][static_cast<uint64_t>(b0) * 16u];
      if constexpr (kTpb == 1) be1[tn] = b_chan[tn][static_cast<uint64_t>(min(b0 + 1u, bp.nblk - 1u)) * 16u];
    }
    QNNP_PIN();
    const uint8_t* st = lds + slot * kStage;
    v4i fw[kTN], op[kTN];
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) fw[tn] = *reinterpret_cast<const v4i*>(st + w_off + tn * 1024);
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) op[tn] = qb4w_zp_even(fw[tn], z_now[tn]);
    multiply(st + a_off, op);
    if constexpr (kTpb == 1) flush(be0);
    if (2u * kp + 1u < ktiles) {                 // always, unless B = 64 and K / 64 is odd
#pragma unroll
      for (int tn = 0; tn < kTN; tn++) op[tn] = qb4w_zp_odd(fw[tn], z_now[tn]);
      multiply(st + kAHalf + a_off, op);
      if constexpr (kTpb == 1) flush(be1);
    }
    if (kTpb == 2 || (kTpb == 4 && (kp & 1u) != 0)) flush(be0);
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
constexpr int kGemvTiles = 8;                 // K tiles per wave and pass
constexpr int kGemvPairs = kGemvTiles / 2;    // = weight loads, and zero-point pairs, per lane and pass
constexpr int kGemvPass = kGemvWaves * kGemvTiles;   // 64 tiles = 4096 K positions = 64 KiB of LDS
constexpr int kGemvOwners = 4;                // waves 0 .. 3 own the 256 outputs, one per lane

template <int kTpb>                             // K tiles per block: 1, 2 or 4
__global__ __launch_bounds__(kGemvThreads)
void qd8_f32_qb4w_zp_gemv_mfma_16_kernel(const Qb4wZpParams bp)
{
  constexpr int kBpw = kGemvTiles / kTpb;       // blocks per wave and pass: 8, 4 or 2
  __shared__ __attribute__((aligned(16))) uint8_t lds[kGemvPass * 1024];

  const Qd8Params& p = bp.q;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nb = blockIdx.x;
  const uint32_t ktiles = p.k_pad / 64u;        // a multiple of kTpb: a block is there whole or not at all
  const uint32_t kpairs = (ktiles + 1u) / 2u;
  const uint32_t frow = lane & 15u, fg = lane >> 4;

  const v4i* w_block = reinterpret_cast<const v4i*>(p.w + static_cast<uint64_t>(nb) * kpairs * 1024u);
  const qnnp_hip_qd8_zp_block_entry* b_chan = bp.btab + static_cast<uint64_t>(nb) * bp.nblk * 16u + frow;
  const uint16_t* z_chan = bp.zpairs + static_cast<uint64_t>(nb) * kpairs * 16u + frow;
  const uint64_t a_base = scalar_ptr(reinterpret_cast<uint64_t>(p.a));
  const uint32_t a_lane = min(frow, p.rows - 1u) * p.k_pad + fg * 16u;      // rows past the batch re-read the last: never stored
  uint8_t* mine = lds + wave * (kGemvTiles * 1024);                           // this wave's tiles of a pass, fragment order
  const uint32_t mine_off = __builtin_amdgcn_readfirstlane(lds_offset(mine));
  // the rows of this lane's accumulator registers, for the terms it produces
  int32_t zo[4];
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) zo[r] = p.rows_tab[min(4u * fg + r, p.rows - 1u)].zero_offset;

  float ysum = 0.0f;                            // owners: output (row 4 fg + wave, channel frow)
  for (uint32_t pass0 = 0; pass0 < ktiles; pass0 += kGemvPass) {
    const uint32_t kt0 = pass0 + wave * kGemvTiles;                          // even: pair kt0 / 2 starts at it
    if (kt0 < ktiles) {
      // pairs, tiles and blocks past K re-read the last one (fixed counts; they are left out below). Every counted load of
      // the pass goes out before the first LDS-DMA request.
      v4i fw[kGemvPairs];
      uint32_t zp[kGemvPairs];
      qnnp_hip_qd8_zp_block_entry be[kBpw];
#pragma unroll
      for (int t = 0; t < kGemvPairs; t++) {
        const uint64_t pair = min(kt0 / 2u + t, kpairs - 1u);
        fw[t] = w_block[pair * 64u + lane];
        zp[t] = z_chan[pair * 16u];
      }
#pragma unroll
      for (int j = 0; j < kBpw; j++) be[j] = b_chan[static_cast<uint64_t>(min(kt0 / kTpb + j, bp.nblk - 1u)) * 16u];
      QNNP_PIN();
#pragma unroll
      for (int t = 0; t < kGemvTiles; t++) {
        const uint32_t kt = min(kt0 + t, ktiles - 1u);
        dma16_saddr_ordered(scalar_ptr(a_base + kt * 64u), a_lane, __builtin_amdgcn_readfirstlane(mine_off + t * 1024u));
      }
      wait_vmcnt<0>();       // the wave reads only what it brought in itself: no barrier
      QNNP_PIN();
      v4i acc[kBpw];
#pragma unroll
      for (int j = 0; j < kBpw; j++) acc[j] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < kGemvPairs; t++) {
        const v4i fa0 = *reinterpret_cast<const v4i*>(mine + (2 * t) * 1024 + lane * 16u);
        const v4i fa1 = *reinterpret_cast<const v4i*>(mine + (2 * t + 1) * 1024 + lane * 16u);
        if (kt0 + 2 * t < ktiles) {
          acc[2 * t / kTpb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa0, qb4w_zp_even(fw[t], zp[t]), acc[2 * t / kTpb], 0, 0, 0);
        }
        if (kt0 + 2 * t + 1 < ktiles) {
          acc[(2 * t + 1) / kTpb] =
              __builtin_amdgcn_mfma_i32_16x16x64_i8(fa1, qb4w_zp_odd(fw[t], zp[t]), acc[(2 * t + 1) / kTpb], 0, 0, 0);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the LDS reads are done before the terms overwrite the tiles
      // this wave's blocks become their terms: block j at mine + j * 1024, plane r (256 bytes) = accumulator register r
#pragma unroll
      for (int j = 0; j < kBpw; j++) {
        if (kt0 + j * kTpb < ktiles) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            *reinterpret_cast<float*>(mine + j * 1024 + r * 256 + lane * 4u) = qb4w_zp_term(acc[j][r], zo[r], be[j]);
          }
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
        for (int j = 0; j < kBpw; j++) {
          if (pass0 + w * kGemvTiles + j * kTpb < ktiles) {
            ysum = ysum + *reinterpret_cast<const float*>(plane + w * (kGemvTiles * 1024) + j * 1024);
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

extern "C" int qnnp_hip_qd8_qb4w_zp_gemm_run(const struct qnnp_hip_qd8_qb4w_zp_gemm_args* b, const char** kernel_name)
{
  using namespace qnnp;
  if (b == nullptr) return QNNP_HIP_EINVAL;
  const struct qnnp_hip_qd8_gemm_args* a = &b->gemm;
  if (a->quantized == nullptr || a->row_table == nullptr || a->packed_w == nullptr || a->channel_table == nullptr ||
      b->block_table == nullptr || b->zero_point_pairs == nullptr || a->output == nullptr ||
      (reinterpret_cast<uintptr_t>(a->output) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a->quantized) & 15u) != 0 ||
      (reinterpret_cast<uintptr_t>(a->packed_w) & 15u) != 0 || (reinterpret_cast<uintptr_t>(b->block_table) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(b->zero_point_pairs) & 1u) != 0 ||
      a->n == 0 || a->n >= (1u << 24) || a->n_pad != ((a->n + 15u) & ~15u) || a->k_pad == 0 || a->k_pad > 32768u ||
      (b->block_size != 64u && b->block_size != 128u && b->block_size != 256u) || a->k_pad % b->block_size != 0 ||
      a->rows > 0x7FFFFFFFu || a->output_stride < a->n) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  Qb4wZpParams bp;
  Qd8Params& p = bp.q;
  p.a = reinterpret_cast<const uint8_t*>(a->quantized);
  p.rows_tab = a->row_table;
  p.w = reinterpret_cast<const uint8_t*>(a->packed_w);      // pair fragments [n_pad / 16][ceil(k_pad / 128)][1024]
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
  bp.btab = b->block_table;
  bp.zpairs = b->zero_point_pairs;
  bp.nblk = a->k_pad / b->block_size;
  if (a->rows <= 16u) {
    const dim3 grid(a->n_pad / 16u), block(kGemvThreads);
    if (b->block_size == 64u) hipLaunchKernelGGL(qd8_f32_qb4w_zp_gemv_mfma_16_kernel<1>, grid, block, 0, stream, bp);
    else if (b->block_size == 128u) hipLaunchKernelGGL(qd8_f32_qb4w_zp_gemv_mfma_16_kernel<2>, grid, block, 0, stream, bp);
    else hipLaunchKernelGGL(qd8_f32_qb4w_zp_gemv_mfma_16_kernel<4>, grid, block, 0, stream, bp);
    if (kernel_name != nullptr) *kernel_name = "qd8_f32_qb4w_zp_gemv_mfma_16";
    return launch_status();
  }
  const uint64_t tiles = static_cast<uint64_t>((a->rows + kBM - 1u) / kBM) * p.tiles_n;
  if (tiles > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;          // a grid that would wrap is refused, not launched
  const dim3 grid(static_cast<uint32_t>(tiles)), block(kGemmThreads);
  if (b->block_size == 64u) hipLaunchKernelGGL(qd8_f32_qb4w_zp_gemm_mfma_128x128_kernel<1>, grid, block, 0, stream, bp);
  else if (b->block_size == 128u) hipLaunchKernelGGL(qd8_f32_qb4w_zp_gemm_mfma_128x128_kernel<2>, grid, block, 0, stream, bp);
  else hipLaunchKernelGGL(qd8_f32_qb4w_zp_gemm_mfma_128x128_kernel<4>, grid, block, 0, stream, bp);
  if (kernel_name != nullptr) *kernel_name = "qd8_f32_qb4w_zp_gemm_mfma_128x128";
  return launch_status();
}
