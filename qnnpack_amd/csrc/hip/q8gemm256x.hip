/*
 * q8gemm256x.hip -- the zero-point-centred 256 x 256 uint8 GEMM on v_mfma_i32_16x16x64_i8 (round 6; BASELINE.json configs[1]).
 *
 * Same role, same algebra, same weight image, same tile -> XCD map as q8gemm256c.hip; its own LDS-DMA ring (it replaces
 * q8gemm_ukernel_4x4c2__sse2, reference src/q8gemm/4x4c2-sse2.c:14-318, and its tiler compute_q8gemm,
 * src/operator-run.c:39-70, 797-802, for MFMA-bound problems whose kernel zero point is 127 or 128). What changes is the
 * matrix instruction, and with it the fragment geometry and the epilogue.
 *
 * WHY. This GEMM is bound by the chip's power budget, not by issue slots (the matrix pipe is busy ~80 % of
 * the launch at ~1.4 GHz of 2.4; removing stalls returns as a lower clock). tools/ubench_mfma2.hip (profiles/r06/) measures
 * what the two int8 shapes sustain on RANDOM operands with nothing else in the loop: 32x32x32 3.41-3.47 PetaOP/s at 1.74 GHz,
 * 16x16x64 4.06-4.09 at 2.05 GHz -- the 16 x 16 shape reads and writes 4 accumulator registers per 16 K MACs (K = 64 per
 * instruction) where the 32 x 32 one moves 16 per 32 K MACs: half the accumulator traffic per MAC, +18 % rate under the same
 * power cap. LDS fragment traffic per MAC is the same for a 64 x 128 wave tile (12 ds_read_b128 per 64-byte K tile).
 *
 * Geometry. 8 waves = 4 (rows) x 2 (channels); a wave owns 64 rows x 128 channels = 4 x 8 tiles of 16 x 16, 128 accumulator
 * registers. Weights are operand A, activations operand B:
 *   operand lane l: row / channel (l & 15) of the tile, K bytes [16 g, 16 g + 16) of the 64-byte K tile, g = l >> 4
 *   result  lane l, register r: activation row (l & 15), channel 4 (l >> 4) + r  -- four consecutive channels = one output dword
 * Activations travel in PAIRS of K tiles (gemm256x_map.h holds every index map and the schedule below as constexpr functions;
 * this file calls them, tests/test_gemm256x_map.py proves them on the host). The pair image in LDS is row-major [256 rows][8
 * slots of 16 B] as LDS-DMA lays it (lane L of a piece -> row L >> 3, slot L & 7: EIGHT consecutive lanes fetch one row's 128
 * contiguous bytes -- a whole cache line where the row is 128-byte aligned, one L2 request where the 64-byte tiles of the first
 * version made two: 6.32 M -> 4.37 M requests per 4096^3 launch, profiles/kpairs/); slot s of row r holds K chunk
 * s ^ f(r), f(r) = ((r >> 1) & 3) | ((((r >> 2) ^ (r >> 3)) & 1) << 2). Two rows share a 256-byte bank row at this pitch; f makes
 * the 16x16x64 fragment read of K tile h of the pair (lane -> row l & 15, chunk 4 h + (l >> 4)) conflict-free for
 * ds_read_b128's 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (MI355X_MICROARCH.md, LDS): every group touches
 * the sixteen 16-byte bank quads once. An odd tile count ends in an unpaired tile: the lanes of its upper 64 bytes fetch the
 * lower 64 once more, into slots nothing reads -- no lane ever reads past its row's K bytes.
 * The weight image is the one pack.h makes for the 32x32x32 kernels -- 1 KiB fragments
 * [32 channels][32 K bytes], position ((c & 31) + 32 ((k & 31) >> 4)) * 16 -- read with other lane addresses: lane l of
 * 16-channel tile t takes fragment (t >> 1, g >> 1), position (16 (t & 1) + (l & 15) + 32 (g & 1)) * 16; conflict-free as well.
 *
 * Pipeline per K tile (one instruction covers the whole 64 bytes of K, so every accumulator is touched once per tile):
 * LDS: three activation pair slots of 32 KiB, a ring of three 16 KiB weight tiles, 4 KiB of bias lines = 148 KiB.
 *   prologue: pair 0, weight tile 0, bias line | pair 1, weight tiles 1, 2; vmcnt(8) + barrier: tile 0 resident
 *   phase 1: 16 MFMAs  a[0..3] x wl[0..3]   | read wh[0..3] (this tile), lgkmcnt(4) twice for a[2], a[3], lgkmcnt(0) at the end
 *                                           | LDS-DMA activation pieces 2 (kt & 1), 2 (kt & 1) + 1 of pair (kt >> 1) + 2, behind
 *                                           | MFMAs 0 and 8, into the slot pair (kt >> 1) - 1 left (last read: phase 2 of tile kt - 2 or - 3)
 *   -- vmcnt(6) + barrier: weight tile kt + 1 and the pair of tile kt + 1 resident, every read of tile kt done --
 *      (behind weight tile kt + 1 were issued: phase 1 and 2 of tile kt - 1 and phase 1 of tile kt; vmcnt(4) in tile 0)
 *   phase 2: 16 MFMAs  a[0..3] x wh[0..3]   | read wl[0..3], a[0..3] of tile kt + 1, a[tm] right behind its last use,
 *                                           | lgkmcnt(1) twice | re-centre them
 *                                           | LDS-DMA pieces 0, 1 of weight tile kt + 3, behind MFMAs 0 and 8, into tile kt's slot
 *   drain: the last five tiles stop issuing -- activation pieces up to tile T - 5 (T - 4 for an odd count T), weight pieces up to
 *   T - 4 -- and wait with vmcnt 6, 4, 2, 0 (odd: 6, 6, 4, 0); behind the vmcnt(0) barrier of tile T - 2 nothing synchronizes.
 * So an activation piece is issued four or five barriers, a weight piece two K tiles ahead of the barrier that needs it, and
 * no slot is refilled before the barrier behind its last fragment read. The ring's period is 6 tiles (three pairs).
 * 48 fragment registers, no double buffer: in both phases the activation operand stays for four MFMAs and the weight operand
 * walks 0123 3210 ... (one operand changes per MFMA: the order the microbenchmark prices highest).
 *
 * Epilogue without LDS: requantize four accumulators -> one dword; two 4 x 4 dword transposes over the four 16-lane rows
 * (v_permlane32_swap + v_permlane16_swap, 8 instructions per 16-row block) give every lane 16 consecutive channels of its
 * row; one DPP row rotate by 8 under a bank mask pairs them so that a store instruction writes eight whole 128-byte lines.
 *
 * Requirements: as q8gemm256c.hip (gemm256c_supported).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "device_ops.hip.h"
#include "gemm256x_map.h"
#include "igemm_params.h"
#include "per_device.h"
#include "requant.hip.h"

namespace qnnp {

namespace {

namespace map = g256x;

constexpr int kBM = 256;
constexpr int kBN = 256;
constexpr int kBK = 64;                        // bytes of K per tile = one 16x16x64 step
constexpr int kThreads = 512;                  // 8 waves: 4 (rows) x 2 (channels), 64 x 128 outputs per wave
constexpr int kTM = 4;                         // 16-row MFMA tiles per wave
constexpr int kTN = 8;                         // 16-channel MFMA tiles per wave
constexpr int kHalf = kTN / 2;                 // weight fragments per phase
constexpr int kMma = kTM * kHalf;              // MFMAs per phase
static_assert(kBM == map::kRows && kBK == map::kTileK && kThreads == map::kWgThreads, "gemm256x_map.h describes this tile");

// what one K tile does beside its MFMAs (gemm256x_map.h, schedule): P1 = phase 1's activation pieces (0 none, 1 whole, 2 of the
// unpaired last tile), P2 = phase 2 issues weight pieces, SYNC = vmcnt of the wait + barrier (-1: none), MORE = a next tile exists
template <int P1, bool P2, int SYNC, bool MORE>
struct Tile {
  static constexpr int p1 = P1;
  static constexpr bool p2 = P2;
  static constexpr int sync = SYNC;
  static constexpr bool more = MORE;
};
constexpr int kSlotsEven = 0, kSlotsOdd = 1, kSlotsLiteral = 2;
using FirstTile = Tile<1, true, map::kFirstVmcnt, true>;
using SteadyTile = Tile<1, true, map::kSteadyVmcnt, true>;
template <bool ODD, uint32_t LEFT>
using DrainTile = Tile<map::p1_mode(ODD, LEFT), map::p2_issues(LEFT), map::sync_vmcnt(ODD, LEFT), LEFT != 1>;

/*
 * SEQ / CLAMP: rounding sequence and clamp class of the requantization (requant.hip.h), chosen by the launcher.
 * SLOTS: kSlotsLiteral -- the K tile count is 4 above a multiple of the ring period of 6 (map::literal_slots; K = 1024 and 4096
 * are): every ring slot is a literal, the drain included. Every other count takes run-time slots, kSlotsEven or kSlotsOdd by its
 * parity: the two drains differ (an odd count ends in an unpaired tile), and as two branches of one kernel their join made the
 * register allocator spill the accumulators.
 * ABL: measurement-only ablation mask (builds with -DQNNP_ENABLE_ABLATION, env QNNP_GFX950_ABLATE); 0 in the product.
 * 1 = no epilogue, 2 = no recentring, 4 = no MFMA, 8 = no LDS-DMA after the prologue, 16 = no fragment reads after the
 * prologue, 32 = no per-tile wait + barrier, 64 = no global stores.
 */
/* ROWSUM (round 6): any OTHER kernel zero point, on the standard image (w - 128, activations ^ 0x80): the kernel-zero-point row term
 * (128 - kzp) * sum_k (a(m,k) - 128) of q8gemm256.hip is added to the accumulators in front of the requantization. The sums are
 * taken over the RAW fragment bytes with v_sad_u8 (one per dword, beside the re-centring XOR); a lane holds chunk g of its row, the
 * four lanes of a row are summed once in the epilogue -- and the result lane of a row is its operand lane, nothing moves. */
/* Inside a phase the weight operand walks its four fragments in SNAKE order (0123 3210 0123 3210): only ONE operand changes per MFMA.
 * tools/ubench_mfma2.hip: 4.27 POP/s against 4.18 for "activation held for four, weights 0123 0123" (and 4.20 for holding it for eight);
 * this kernel, interleaved on one box: 49.96 -> 49.36 us (profiles/r06/gemm_ab_c16_snake_r06k.txt).
 * OPT (measurement builds, env QNNP_C16_OPT; 0 in the product): 1 = the plain order, for that A/B; 4 = static priority 1 for
 * the younger four waves (s_setprio in front of the loop): 49.72 us against 49.75, inside the 0.5 us round-to-round spread
 * (profiles/kpairs/gemm_ablation_c16.txt) -- not in the product. */
template <int SEQ, int CLAMP, int SLOTS, int ABL = 0, bool ROWSUM = false, int OPT = 0>
__global__ __launch_bounds__(kThreads, 2)
void q8_gemm_mfma_256x256_c16_kernel(const IgemmParams p)
{
  static_assert(SEQ == kRqShift0Ofs || SEQ == kRqBoundedOfs || SEQ == kRqGeneral, "offset forms, or the general one");
  __shared__ __attribute__((aligned(16))) uint8_t lds[map::kLdsBytes];    // the ONE LDS object

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t wm = wave >> 1;       // 64-row slice
  const uint32_t wn = wave & 1u;       // 128-channel half
  const uint32_t g = blockIdx.y;
  QNNP_TRACE_WAVE04(p, lane, wave, 0);
  QNNP_TRACE_WAVE04_WALL(p, lane, wave, 0);

  // Workgroup -> tile (q8gemm256.hip): contiguous logical ids per XCD, bands of four row tiles -- an XCD's 32 workgroups of a
  // 16 x 16-tile launch cover 4 row tiles x 8 channel tiles, the most compact block 32 tiles allow (4 + 8 operand panels).
  const uint32_t tiles_m = (p.rows + kBM - 1) / kBM;
  const uint32_t tiles_n = p.n_pad / kBN;
  uint32_t m_tile, n_tile;
  {
    const uint32_t nwg = gridDim.x;
    const uint32_t xcd = blockIdx.x & 7u;
    const uint32_t idx = blockIdx.x >> 3;
    const uint32_t q = nwg >> 3, r = nwg & 7u;
    const uint32_t logical = xcd * q + min(xcd, r) + idx;
    constexpr uint32_t kBand = 4;
    const uint32_t band = p.tiles_n_magic != 0 ? __umulhi(logical >> 2, p.tiles_n_magic) : logical >> 2;   // logical / (4 * tiles_n)
    const uint32_t within = logical - band * kBand * tiles_n;
    const uint32_t rows_in_band = min(kBand, tiles_m - band * kBand);
    if (rows_in_band == kBand) {
      m_tile = band * kBand + (within & 3u);
      n_tile = within >> 2;
    } else {
      m_tile = band * kBand + within % rows_in_band;
      n_tile = within / rows_in_band;
    }
  }

  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;
  const uint32_t ktiles = p.k_pad / kBK;
  const uint32_t nb0 = n_tile * (kBN / 32);

  // ---- LDS-DMA sources: wave-uniform bases + loop-invariant 32-bit lane offsets ----
  // (strided 1x1 convolutions -- igemm_params.h `offsets_dense`: a row's address comes from the operator's table, the lane
  //  offsets are then absolute; the launcher checks that the tensor ends below 2^32)
  const bool table_rows = p.offsets_dense != 0;
  const uint8_t* a_base = scalar_ptr(table_rows ? p.input + static_cast<uint64_t>(g) * p.kc
      : p.input + static_cast<uint64_t>(m_tile * kBM) * p.input_stride + static_cast<uint64_t>(g) * p.kc);
  // (activations travel in pairs of K tiles, gemm256x_map.h: piece i of a pair = rows 64 i .. 64 i + 63, eight consecutive
  //  lanes fetch one row's 128 contiguous bytes)
  uint32_t a_voff[map::kAPieces];
#pragma unroll
  for (uint32_t i = 0; i < map::kAPieces; i++) {
    const uint32_t m = map::a_clamp_row(m_tile * kBM + map::a_dma_row(i, tid), p.rows);   // results of clamped rows are never stored
    a_voff[i] = (m - m_tile * kBM) * p.input_stride + map::a_dma_src(tid, false);
    if (table_rows) {
      const uint32_t img = p.rpi_magic != 0 ? __umulhi(m, p.rpi_magic) : m / p.rows_per_image;
      const uint32_t pix = m - img * p.rows_per_image;
      a_voff[i] = img * static_cast<uint32_t>(p.image_stride) + static_cast<uint32_t>(p.offsets[pix]) + map::a_dma_src(tid, false);
    }
  }
  // an odd tile count ends in an unpaired tile: its lanes of the upper 64 bytes fetch the lower 64 once more
  const uint32_t a_half_back = map::a_dma_src(tid, false) - map::a_dma_src(tid, true);
  // weight fragment F = i * 8 + wave: channel block nb0 + i * 4 + (wave >> 1), K block (wave & 1) of the tile's two
  const uint8_t* w_base = scalar_ptr(reinterpret_cast<const uint8_t*>(p.packed_w) + static_cast<uint64_t>(g) * nblocks * kblocks * 1024 +
      (static_cast<uint64_t>(nb0 + (wave >> 1)) * kblocks + (wave & 1u)) * 1024);
  uint32_t w_voff[2];
#pragma unroll
  for (int i = 0; i < 2; i++) w_voff[i] = lane * 16 + static_cast<uint32_t>(i) * 4u * kblocks * 1024u;

  // activation piece `piece` of a pair -> pair slot `slot`; weight piece `piece` of a tile (fragments 8 piece + wave) -> weight slot
  auto a_dst = [&](uint32_t piece, uint32_t slot) __attribute__((always_inline)) -> uint8_t* {
    return lds + map::kABase + slot * map::kPairBytes + map::a_dma_wave_dst(piece, wave);
  };
  auto w_dst = [&](uint32_t piece, uint32_t slot) __attribute__((always_inline)) -> uint8_t* {
    return lds + map::kWBase + slot * map::kWTileBytes + (piece * 8 + wave) * 1024;
  };
  auto a_src = [&](uint32_t pair) __attribute__((always_inline)) -> const uint8_t* {
    return a_base + static_cast<uint64_t>(pair) * map::kPairK;
  };
  auto w_src = [&](uint32_t kt) __attribute__((always_inline)) -> const uint8_t* {
    return w_base + static_cast<uint64_t>(kt) * 2048;
  };
  auto stage_pair = [&](uint32_t pair) __attribute__((always_inline)) {
#pragma unroll
    for (uint32_t piece = 0; piece < map::kAPieces; piece++) dma16_saddr(a_src(pair), a_voff[piece], a_dst(piece, map::a_slot(pair)));
  };
  auto stage_w = [&](uint32_t kt) __attribute__((always_inline)) {
#pragma unroll
    for (uint32_t piece = 0; piece < map::kWPieces; piece++) dma16_saddr(w_src(kt), w_voff[piece], w_dst(piece, map::w_slot(kt)));
  };

  // ---- prologue, part 1: the first tile's DMA, the folded bias, the rest of the ring ----
  stage_pair(0);
  stage_w(0);

  // the wave's 128 folded biases (+ 2^31 for the offset forms): ONE LDS-DMA instruction, lanes 0..31, 512 bytes
  const int32_t* bias_tab = SEQ == kRqGeneral ? p.bias2 : p.bias2u;
  uint8_t* bias_line = lds + map::kBiasBase + wave * 512;
  if (lane < 32) {
    dma16_saddr(scalar_ptr(reinterpret_cast<const uint8_t*>(bias_tab + static_cast<uint64_t>(g) * p.n_pad + (nb0 + wn * 4) * 32)),
                   lane * 16, bias_line);
  }

  stage_pair(1);
  stage_w(1);
  stage_w(2);

  // ---- fragment addresses ----
  const uint32_t frow = lane & 15u;              // row / channel of a 16 x 16 tile
  const uint32_t fg = lane >> 4;                 // K chunk of the operand; channel quad of the result
  // a ds_read immediate reaches 64 KiB: two pair slots, or the whole weight ring
  uint32_t a_off[2][2];                          // [K tile of the pair][pair slots 0, 1 / 2]  + tm * 2048 + (slot & 1) * kPairBytes
  uint32_t w_off;                                // + (tn >> 1) * 2048 + (tn & 1) * 256 + slot * kWTileBytes
#pragma unroll
  for (uint32_t h = 0; h < 2; h++) {
#pragma unroll
    for (uint32_t s2 = 0; s2 < 2; s2++) {
      a_off[h][s2] = map::kABase + map::a_lds_byte(map::a_frag_row(wm, 0, lane), map::a_frag_chunk(h, lane)) + s2 * 2 * map::kPairBytes;
      asm volatile("" : "+v"(a_off[h][s2]));
    }
  }
  w_off = map::kWBase + (wn * 8 + (fg >> 1)) * 1024 + (frow + 32 * (fg & 1u)) * 16;
  asm volatile("" : "+v"(w_off));
  v4i fa[kTM];                                   // activation fragments of the current K tile (operand B)
  v4i wl[kHalf], wh[kHalf];                      // weight fragments: channel tiles 0..3 / 4..7 of the wave (operand A)

  // slot known at compile time: address register + immediates; run-time slot: one add. h: K tile of the pair, a literal always.
  auto read_a = [&](auto known_c, uint32_t h, uint32_t slot, int tm) __attribute__((always_inline)) {
    const uint32_t imm = tm * 16 * map::kPairK;  // == a_lds_byte(a_frag_row(wm, tm, lane), .) - a_lds_byte(a_frag_row(wm, 0, lane), .)
    if constexpr (decltype(known_c)::value) {
      fa[tm] = *reinterpret_cast<const v4i*>(lds + a_off[h][slot >> 1] + (slot & 1u) * map::kPairBytes + imm);
    } else {
      fa[tm] = *reinterpret_cast<const v4i*>(lds + slot * map::kPairBytes + a_off[h][0] + imm);
    }
  };
  auto read_w = [&](auto known_c, uint32_t slot, int tn, v4i& dst) __attribute__((always_inline)) {
    const uint32_t imm = (tn >> 1) * 2048 + (tn & 1) * 256;
    dst = *reinterpret_cast<const v4i*>(lds + slot * map::kWTileBytes + w_off + imm);
  };

  const uint32_t flip = p.a_flip;                // 0x80808080 (kzp 128) or 0x7F7F7F7F (kzp 127), scalar
  uint32_t rs[kTM] = {0u, 0u, 0u, 0u};           // ROWSUM: sum of the raw bytes of this lane's chunks of rows 16 tm + (lane & 15)
  // half (0 / 1) of the recentring of one activation fragment: 2 of its 4 dwords
  auto flip_half = [&](int tm, int half) __attribute__((always_inline)) {
    if constexpr (ROWSUM) {
      if (half) {
        rs[tm] = __builtin_amdgcn_sad_u8(static_cast<uint32_t>(fa[tm].z), 0u, rs[tm]);
        rs[tm] = __builtin_amdgcn_sad_u8(static_cast<uint32_t>(fa[tm].w), 0u, rs[tm]);
      } else {
        rs[tm] = __builtin_amdgcn_sad_u8(static_cast<uint32_t>(fa[tm].x), 0u, rs[tm]);
        rs[tm] = __builtin_amdgcn_sad_u8(static_cast<uint32_t>(fa[tm].y), 0u, rs[tm]);
      }
      // (pinned HERE: left alone, hipcc sinks the sums of the unrolled drain tiles to the epilogue, where their result is first
      //  needed, and keeps -- spills -- the raw fragments until then)
      asm volatile("" : "+v"(rs[tm]));
    }
    if constexpr ((ABL & 2) != 0) {
      asm volatile("" : "+v"(fa[tm]));
    } else if (half) {
      fa[tm].z ^= static_cast<int>(flip);
      fa[tm].w ^= static_cast<int>(flip);
      asm volatile("" : "+v"(fa[tm].z), "+v"(fa[tm].w));
    } else {
      fa[tm].x ^= static_cast<int>(flip);
      fa[tm].y ^= static_cast<int>(flip);
      asm volatile("" : "+v"(fa[tm].x), "+v"(fa[tm].y));
    }
  };

  v4i acc[kTM][kTN];
  auto mma = [&](const v4i& w, int tm, int tn) __attribute__((always_inline)) {
    if constexpr ((ABL & 4) != 0) return;
    acc[tm][tn] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w, fa[tm], acc[tm][tn], 0, 0, 0);
  };

  // ---- prologue, part 2: tile 0 and the bias line have landed (loads complete in issue order) ----
  wait_vmcnt<map::kPrologueVmcnt>();
  __builtin_amdgcn_s_barrier();
  QNNP_TRACE_WAVE04(p, lane, wave, 1);
  using T = std::true_type;
  using F = std::false_type;
#pragma unroll
  for (int tm = 0; tm < kTM; tm++) read_a(T{}, 0u, 0u, tm);
#pragma unroll
  for (int tn = 0; tn < kHalf; tn++) read_w(T{}, 0u, tn, wl[tn]);
  // accumulators: lane l holds, in register r of tile tn, channel (nb0 + wn * 4) * 32 + tn * 16 + 4 * (l >> 4) + r
  // (its own wave's DMA: visible behind the vmcnt wait above; four addresses per read, broadcasts)
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) {
    const v4i b = *reinterpret_cast<const v4i*>(bias_line + tn * 64 + fg * 16);
#pragma unroll
    for (int tm = 0; tm < kTM; tm++) acc[tm][tn] = b;
  }
  // fa[0], fa[1] re-centred here, fa[2], fa[3] left raw: the state every tile's phase 1 starts in (it re-centres the last two)
#pragma unroll
  for (int tm = 0; tm < 2; tm++) { flip_half(tm, 0); flip_half(tm, 1); }
  asm volatile("" : "+v"(wl[0]), "+v"(wl[1]), "+v"(wl[2]), "+v"(wl[3]));
  if constexpr ((ABL & 16) != 0) { wh[0] = wl[0]; wh[1] = wl[1]; wh[2] = wl[2]; wh[3] = wl[3]; }

  if constexpr ((OPT & 4) != 0) {
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  }

  /*
   * One K tile (see the file comment). tile_c: a Tile<> -- what the tile issues and waits for. KNOWN: the slots are literals.
   * h_c: kt & 1, the K tile of its pair, always a literal. ws = map::w_slot(kt), as = map::a_slot(kt >> 1).
   */
  auto iteration = [&](auto tile_c, auto known_c, auto h_c, uint32_t kt, uint32_t ws, uint32_t as) __attribute__((always_inline)) {
    using TileT = decltype(tile_c);
    constexpr int P1 = (ABL & 8) != 0 ? 0 : TileT::p1;
    constexpr bool MORE = TileT::more;
    constexpr bool P2F = TileT::p2 && (ABL & 8) == 0;
    constexpr int SYNC = (ABL & 32) != 0 ? -1 : TileT::sync;
    constexpr bool KNOWN = decltype(known_c)::value;
    constexpr bool READS = (ABL & 16) == 0;
    constexpr uint32_t H = decltype(h_c)::value;
    const uint32_t ws_next = ws + 1 == map::kWSlots ? 0 : ws + 1;                   // weight tile kt + 1
    const uint32_t as_fill = as == 0 ? map::kASlots - 1 : as - 1;                    // pair (kt >> 1) + 2, where pair (kt >> 1) - 1 was
    const uint32_t as_next = H == 0 ? as : (as + 1 == map::kASlots ? 0 : as + 1);   // the pair of tile kt + 1
    // phase 1's activation piece j: lane offset (the unpaired last tile: upper-half lanes step back into the lower half)
    auto a_piece_off = [&](uint32_t piece) __attribute__((always_inline)) -> uint32_t {
      return P1 == 2 ? a_voff[piece] - a_half_back : a_voff[piece];
    };

    // ---- phase 1: fa x wl; the tile's second four weight fragments arrive, one behind each of the first MFMAs ----
    QNNP_PIN();
#pragma unroll
    for (int i = 0; i < kMma; i++) {
      const int tm = i / kHalf, tn = ((OPT & 1) == 0 && (tm & 1) != 0) ? kHalf - 1 - i % kHalf : i % kHalf;
      if constexpr (P1 != 0 && KNOWN) {
        if (i % 8 == 0) { dma16_set_m0(a_dst(map::a_issue_piece(H, i / 8), as_fill)); QNNP_PIN(); }
      }
      mma(wl[tn], tm, tn);
      QNNP_PIN();
      if constexpr (READS) {
        if (i < kHalf) { read_w(known_c, ws, kHalf + i, wh[i]); QNNP_PIN(); }
      }
      if constexpr (P1 != 0 && KNOWN) {
        if (i % 8 == 0) { dma16_saddr_m0_set(a_src(map::a_issue_pair(kt)), a_piece_off(map::a_issue_piece(H, i / 8))); QNNP_PIN(); }
      } else if constexpr (P1 != 0) {
        if (i % 8 == 0) {
          dma16_saddr(a_src(map::a_issue_pair(kt)), a_piece_off(map::a_issue_piece(H, i / 8)), a_dst(map::a_issue_piece(H, i / 8), as_fill));
          QNNP_PIN();
        }
      }
      // the last two activation fragments of this tile were read at the end of the previous phase 2: re-centre them ahead of
      // their first use (MFMA 8 and 12)
      // (LDS reads return in order: behind fa[2] came fa[3] and wh[0..2] by now, behind fa[3] the four wh reads)
      if (i == 2) { __builtin_amdgcn_s_waitcnt(0xC47F); QNNP_PIN(); }     // lgkmcnt(4): fa[2] has landed
      if (i == 2 || i == 3) { flip_half(2, i - 2); QNNP_PIN(); }
      if (i == 6) { __builtin_amdgcn_s_waitcnt(0xC47F); QNNP_PIN(); }     // lgkmcnt(4): fa[3] has landed
      if (i == 6 || i == 7) { flip_half(3, i - 6); QNNP_PIN(); }
      if (i == kMma - 2) { __builtin_amdgcn_s_waitcnt(0xC07F); QNNP_PIN(); }   // wh complete
    }
    asm volatile("" : "+v"(wh[0]), "+v"(wh[1]), "+v"(wh[2]), "+v"(wh[3]));
    QNNP_PIN();

    if constexpr (SYNC >= 0) {
      wait_vmcnt<SYNC>();
      __builtin_amdgcn_s_barrier();         // (behind the one with vmcnt(0) nothing synchronizes the waves)
    }
    QNNP_PIN();

    // ---- phase 2: fa x wh; the next tile's first four weight fragments and its activation fragments arrive, fa[tm] right
    //      behind the last MFMA that reads the old one ----
#pragma unroll
    for (int i = 0; i < kMma; i++) {
      const int tm = i / kHalf, tn = ((OPT & 1) == 0 && (tm & 1) != 0) ? kHalf - 1 - i % kHalf : i % kHalf;
      if constexpr (P2F && KNOWN) {
        if (i % 8 == 0) { dma16_set_m0(w_dst(i / 8, ws)); QNNP_PIN(); }
      }
      mma(wh[tn], tm, kHalf + tn);
      QNNP_PIN();
      if constexpr (MORE && READS) {
        if (tm == 0) { read_w(known_c, ws_next, tn, wl[tn]); QNNP_PIN(); }
        if (i % kHalf == kHalf - 1) { read_a(known_c, 1u - H, as_next, tm); QNNP_PIN(); }
      }
      if constexpr (P2F && KNOWN) {
        if (i % 8 == 0) { dma16_saddr_m0_set(w_src(map::w_issue_tile(kt)), w_voff[i / 8]); QNNP_PIN(); }
      } else if constexpr (P2F) {
        if (i % 8 == 0) { dma16_saddr(w_src(map::w_issue_tile(kt)), w_voff[i / 8], w_dst(i / 8, ws)); QNNP_PIN(); }
      }
      if constexpr (MORE) {
        // fa[0] (read behind MFMA 3) re-centred behind MFMAs 9, 10; fa[1] (behind MFMA 7) behind MFMAs 13, 14
        if (i == 9) { __builtin_amdgcn_s_waitcnt(0xC17F); QNNP_PIN(); }      // lgkmcnt(1): all but fa[1]
        if (i == 9 || i == 10) { flip_half(0, i - 9); QNNP_PIN(); }
        if (i == 13) { __builtin_amdgcn_s_waitcnt(0xC17F); QNNP_PIN(); }     // lgkmcnt(1): all but fa[2]
        if (i == 13 || i == 14) { flip_half(1, i - 13); QNNP_PIN(); }
      }
    }
    if constexpr (MORE) asm volatile("" : "+v"(wl[0]), "+v"(wl[1]), "+v"(wl[2]), "+v"(wl[3]));
    QNNP_PIN();
  };

  // tile kt with kt % 6 == X: both slots and the K tile of the pair are literals
  auto lit = [&](auto tile_c, auto x_c, uint32_t kt) __attribute__((always_inline)) {
    constexpr uint32_t X = decltype(x_c)::value;
    static_assert(X < map::kPeriod, "one ring period");
    iteration(tile_c, T{}, std::integral_constant<uint32_t, (X & 1u)>{}, kt, map::w_slot(X), map::a_slot(X >> 1));
  };
  using X0 = std::integral_constant<uint32_t, 0>;
  using X1 = std::integral_constant<uint32_t, 1>;
  using X2 = std::integral_constant<uint32_t, 2>;
  using X3 = std::integral_constant<uint32_t, 3>;
  using X4 = std::integral_constant<uint32_t, 4>;
  using X5 = std::integral_constant<uint32_t, 5>;

  // (the launcher guarantees ktiles >= 8: tile 0, two steady tiles at least, the five of the drain)
  lit(FirstTile{}, X0{}, 0u);
  QNNP_TRACE_WAVE04(p, lane, wave, 2);
  uint32_t kt = 1;
  if constexpr (SLOTS == kSlotsLiteral) {
    // ktiles % 6 == 4 (map::literal_slots): whole ring periods, four more steady tiles, the drain -- kt % 6 == 1 at every stop
    for (; kt + map::kPeriod + 4 + map::kDrain <= ktiles; kt += map::kPeriod) {
      lit(SteadyTile{}, X1{}, kt);
      lit(SteadyTile{}, X2{}, kt + 1);
      lit(SteadyTile{}, X3{}, kt + 2);
      lit(SteadyTile{}, X4{}, kt + 3);
      lit(SteadyTile{}, X5{}, kt + 4);
      lit(SteadyTile{}, X0{}, kt + 5);
    }
    lit(SteadyTile{}, X1{}, kt);
    lit(SteadyTile{}, X2{}, kt + 1);
    lit(SteadyTile{}, X3{}, kt + 2);
    lit(SteadyTile{}, X4{}, kt + 3);
    QNNP_TRACE_WAVE04(p, lane, wave, 3);
    lit(DrainTile<false, 5>{}, X5{}, kt + 4);       // the last activation pieces
    lit(DrainTile<false, 4>{}, X0{}, kt + 5);       // the last weight pieces
    lit(DrainTile<false, 3>{}, X1{}, kt + 6);
    QNNP_TRACE_WAVE04(p, lane, wave, 4);
    lit(DrainTile<false, 2>{}, X2{}, kt + 7);       // the final wait + barrier: everything resident
    lit(DrainTile<false, 1>{}, X3{}, kt + 8);       // last tile
  } else {
    uint32_t ws = 1, as = 0;                        // == map::w_slot(kt), map::a_slot(kt >> 1)
    using H0 = std::integral_constant<uint32_t, 0>;
    using H1 = std::integral_constant<uint32_t, 1>;
    auto odd_tile = [&](auto tile_c) __attribute__((always_inline)) {     // kt odd: the next tile opens the next pair
      iteration(tile_c, F{}, H1{}, kt, ws, as);
      kt++;
      ws = ws + 1 == map::kWSlots ? 0 : ws + 1;
      as = as + 1 == map::kASlots ? 0 : as + 1;
    };
    auto even_tile = [&](auto tile_c) __attribute__((always_inline)) {
      iteration(tile_c, F{}, H0{}, kt, ws, as);
      kt++;
      ws = ws + 1 == map::kWSlots ? 0 : ws + 1;
    };
    while (kt + 1 + map::kDrain < ktiles) {         // steady state, run-time slots: tiles 1 .. ktiles - 6, two at a time
      odd_tile(SteadyTile{});
      even_tile(SteadyTile{});
    }
    QNNP_TRACE_WAVE04(p, lane, wave, 3);
    if constexpr (SLOTS == kSlotsOdd) {
      odd_tile(SteadyTile{});                       // ktiles - 6, the last steady one
      even_tile(DrainTile<true, 5>{});              // pieces 0, 1 of the unpaired last tile
      odd_tile(DrainTile<true, 4>{});               // its pieces 2, 3; the last weight pieces
      even_tile(DrainTile<true, 3>{});
      odd_tile(DrainTile<true, 2>{});               // the final wait + barrier: everything resident
      even_tile(DrainTile<true, 1>{});              // last tile
    } else {
      odd_tile(DrainTile<false, 5>{});              // the last activation pieces
      even_tile(DrainTile<false, 4>{});             // the last weight pieces
      odd_tile(DrainTile<false, 3>{});
      even_tile(DrainTile<false, 2>{});             // the final wait + barrier: everything resident
      odd_tile(DrainTile<false, 1>{});              // last tile
    }
    QNNP_TRACE_WAVE04(p, lane, wave, 4);
  }
  QNNP_TRACE_WAVE04(p, lane, wave, 5);

  // ---- fused epilogue: Q31 requantize in registers -> lane transposes -> whole 128-byte lines, no LDS ----
  if constexpr ((ABL & 1) != 0) {
#pragma unroll
    for (int tm = 0; tm < kTM; tm++) {
#pragma unroll
      for (int tn = 0; tn < kTN; tn++) asm volatile("" : : "v"(acc[tm][tn]));
    }
    return;
  }
  const uint32_t m0 = m_tile * kBM + wm * 64;
  const uint32_t n0 = (nb0 + wn * 4) * 32;
  uint8_t* out0 = p.output + static_cast<uint64_t>(m0) * p.output_stride + static_cast<uint64_t>(g) * p.n + n0;
  // a store instruction of block tm writes rows (frow & 7) [+ 8], bytes (frow >> 3) * 64 + fg * 16 .. + 16 of the wave's 128
  const uint32_t st_row = frow & 7u;
  const uint32_t st_col = (frow >> 3) * 64 + fg * 16;
  const bool col_ok = n0 + st_col < p.n;
  // 4 x 4 dword transpose over the four 16-lane rows: in  q[j] at lane row g = element (g, j);  out q[j] at lane row g = (j, g)
  auto transpose4 = [&](uint32_t (&q)[4]) __attribute__((always_inline)) {
    const auto s02 = __builtin_amdgcn_permlane32_swap(q[0], q[2], false, false);   // {q0.r0 q0.r1 q2.r0 q2.r1}, {q0.r2 q0.r3 q2.r2 q2.r3}
    const auto s13 = __builtin_amdgcn_permlane32_swap(q[1], q[3], false, false);
    const auto lo = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);  // {q0.r0 q1.r0 q2.r0 q3.r0}, {q0.r1 q1.r1 q2.r1 q3.r1}
    const auto hi = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);  // {.. r2 ..}, {.. r3 ..}
    q[0] = lo[0]; q[1] = lo[1]; q[2] = hi[0]; q[3] = hi[1];
  };
#pragma unroll
  for (int tm = 0; tm < kTM; tm++) {
    if constexpr (ROWSUM) {
      // the row's four chunk sums (lanes l, l ^ 16, l ^ 32, l ^ 48), then (128 - kzp) * (sum of a - 128 K) onto every accumulator of
      // the row (wrapping: the accumulators may carry the 2^31 offset of the offset forms)
      uint32_t t = rs[tm];
      t += static_cast<uint32_t>(__shfl_xor(static_cast<int>(t), 16));
      t += static_cast<uint32_t>(__shfl_xor(static_cast<int>(t), 32));
      const uint32_t term = static_cast<uint32_t>(p.row_coeff) * (t - 128u * p.k_pad);
#pragma unroll
      for (int tn = 0; tn < kTN; tn++) {
#pragma unroll
        for (int r = 0; r < 4; r++) acc[tm][tn][r] = static_cast<int>(static_cast<uint32_t>(acc[tm][tn][r]) + term);
      }
    }
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      lo[j] = q31_requantize_pack4_clamp<SEQ, CLAMP>(acc[tm][j][0], acc[tm][j][1], acc[tm][j][2], acc[tm][j][3], p.rq);
      hi[j] = q31_requantize_pack4_clamp<SEQ, CLAMP>(acc[tm][4 + j][0], acc[tm][4 + j][1], acc[tm][4 + j][2], acc[tm][4 + j][3], p.rq);
    }
    transpose4(lo);        // lane (row, g): channels 16 g .. 16 g + 15 of its row (bytes 0..63 of the wave's 128)
    transpose4(hi);        // ... and channels 64 + 16 g ..
    // whole lines: rows 0..7 of the block keep their low halves and take the high halves of the SAME rows from lanes row + 8
    typedef int nt_v4i __attribute__((ext_vector_type(4)));
    nt_v4i x, y;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      // row_ror:8 = the other half of the 16-lane row; bank mask 0xC = lanes 8..15 of a row take the source, 0x3 = lanes 0..7
      x[j] = __builtin_amdgcn_update_dpp(static_cast<int>(lo[j]), static_cast<int>(hi[j]), 0x128, 0xF, 0xC, false);
      y[j] = __builtin_amdgcn_update_dpp(static_cast<int>(hi[j]), static_cast<int>(lo[j]), 0x128, 0xF, 0x3, false);
    }
    const uint32_t rx = tm * 16 + st_row, ry = rx + 8;
    nt_v4i* dx = reinterpret_cast<nt_v4i*>(out0 + static_cast<uint64_t>(rx) * p.output_stride + st_col);
    nt_v4i* dy = reinterpret_cast<nt_v4i*>(out0 + static_cast<uint64_t>(ry) * p.output_stride + st_col);
    const bool stores = (ABL & 64) == 0 || p.rows == 0xFFFFFFFFu;
    if (m0 + rx < p.rows && col_ok && stores) {
      if (p.stream_out) asm volatile("global_store_dwordx4 %0, %1, off nt" : : "v"(dx), "v"(x) : "memory");
      else *dx = x;
    }
    if (m0 + ry < p.rows && col_ok && stores) {
      if (p.stream_out) asm volatile("global_store_dwordx4 %0, %1, off nt" : : "v"(dy), "v"(y) : "memory");
      else *dy = y;
    }
    if (tm == 1) QNNP_TRACE_WAVE04(p, lane, wave, 6);
  }
  QNNP_TRACE_WAVE04(p, lane, wave, 7);
#ifdef QNNP_ENABLE_ABLATION
  if (p.trace != nullptr) {                      // when the stores have left the wave
    wait_vmcnt<0>();
    QNNP_TRACE_WAVE04_WALL(p, lane, wave, 1);
  }
#endif
}
#undef QNNP_PIN

template <int SLOTS, bool ROWSUM>
int launch_x(const IgemmParams& p, const dim3& grid, hipStream_t stream)
{
  int rc = QNNP_HIP_EINVAL;
#ifdef QNNP_ENABLE_ABLATION
  if constexpr (SLOTS == kSlotsLiteral && !ROWSUM) {
    const char* env = getenv("QNNP_GFX950_ABLATE");
    const int abl = env != nullptr ? atoi(env) : 0;
#define QNNP_ABL_CASE(V) case V: hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kRqShift0Ofs, 1, kSlotsLiteral, V>), grid, dim3(kThreads), 0, stream, p); \
        return launch_status();
    switch (abl) {
      QNNP_ABL_CASE(1) QNNP_ABL_CASE(2) QNNP_ABL_CASE(4) QNNP_ABL_CASE(8) QNNP_ABL_CASE(16) QNNP_ABL_CASE(24)
      QNNP_ABL_CASE(27) QNNP_ABL_CASE(32) QNNP_ABL_CASE(59) QNNP_ABL_CASE(64)
      default: break;
    }
#undef QNNP_ABL_CASE
    const char* oenv = getenv("QNNP_C16_OPT");
    if (oenv != nullptr && atoi(oenv) == 1) {
      hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kRqShift0Ofs, 1, kSlotsLiteral, 0, false, 1>), grid, dim3(kThreads), 0, stream, p);
      return launch_status();
    }
    if (oenv != nullptr && atoi(oenv) == 4) {
      hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kRqShift0Ofs, 1, kSlotsLiteral, 0, false, 4>), grid, dim3(kThreads), 0, stream, p);
      return launch_status();
    }
  }
#endif
  if (p.rq.f.shift != 0 && p.rq.f.bounded && p.rq.f.ofs_kind == 2 && !p.rq.full_range) {
    // bounded accumulators, shift >= 1, a clamp other than [0, 255]: the bounded sequence with the clamp class picked here
    if (p.rq.zp_late == 0) hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kRqBoundedOfs, 1, SLOTS, 0, ROWSUM>), grid, dim3(kThreads), 0, stream, p);
    else hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kRqBoundedOfs, 2, SLOTS, 0, ROWSUM>), grid, dim3(kThreads), 0, stream, p);
    return launch_status();
  }
  requant_dispatch_ofs(p.rq, [&](auto seq, auto full) {
    constexpr int kSeq = decltype(seq)::value;
    if constexpr (decltype(full)::value) {
      hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kSeq, 0, SLOTS, 0, ROWSUM>), grid, dim3(kThreads), 0, stream, p);
    } else if (p.rq.zp_late == 0) {             // zero point folded (or zero): no add behind the clamp
      hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kSeq, 1, SLOTS, 0, ROWSUM>), grid, dim3(kThreads), 0, stream, p);
    } else {
      hipLaunchKernelGGL((q8_gemm_mfma_256x256_c16_kernel<kSeq, 2, SLOTS, 0, ROWSUM>), grid, dim3(kThreads), 0, stream, p);
    }
    rc = launch_status();
  });
  return rc;
}

}  // namespace

/* `p` must carry the CENTRED weight image, its bias pair table and a_flip (q8igemm.hip); gemm256c_supported(p) holds.
 * p.row_coeff != 0: the STANDARD image (centred on 128, a_flip 0x80808080) of an operator with another kernel zero point -- the
 * flavour that adds the kernel-zero-point row term (ROWSUM). */
int gemm256x_launch(const IgemmParams& p, uint32_t groups, hipStream_t stream, const char** name)
{
  const uint32_t tiles_m = (p.rows + kBM - 1) / kBM;
  const uint32_t tiles_n = p.n_pad / kBN;
  const dim3 grid(tiles_m * tiles_n, groups, 1);
  IgemmParams pm = p;
  // x / tiles_n == hi32(x * magic) for x < 2^32 / tiles_n (the tile ids); 0 stands for tiles_n == 1
  pm.tiles_n_magic = tiles_n == 1 ? 0u : reciprocal_floor_plus1(tiles_n);
  const uint32_t ktiles = p.k_pad / kBK;
  const int slots = map::literal_slots(ktiles) ? kSlotsLiteral : (ktiles & 1u) != 0 ? kSlotsOdd : kSlotsEven;
  if (p.row_coeff != 0) {
    *name = "q8_gemm_mfma_256x256_r16";
    return slots == kSlotsLiteral ? launch_x<kSlotsLiteral, true>(pm, grid, stream)
         : slots == kSlotsOdd   ? launch_x<kSlotsOdd, true>(pm, grid, stream) : launch_x<kSlotsEven, true>(pm, grid, stream);
  }
  *name = "q8_gemm_mfma_256x256_c16";
  return slots == kSlotsLiteral ? launch_x<kSlotsLiteral, false>(pm, grid, stream)
       : slots == kSlotsOdd   ? launch_x<kSlotsOdd, false>(pm, grid, stream) : launch_x<kSlotsEven, false>(pm, grid, stream);
}

}  // namespace qnnp
