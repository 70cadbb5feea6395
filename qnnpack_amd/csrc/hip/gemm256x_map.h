/*
 * gemm256x_map.h -- index maps and the LDS-DMA schedule of q8gemm256x.hip (the 256 x 256 GEMM on v_mfma_i32_16x16x64_i8).
 *
 * Plain constexpr functions, no HIP types: the kernel calls them on the device, tests/test_gemm256x_map.py compiles them
 * into a host program and proves what the kernel relies on (the DMA map is a bijection, the fragment reads return the MFMA
 * operand layout, every ds_read_b128 lane group is conflict-free, no lane reads outside its row, every counted wait covers
 * what the barrier behind it needs, no slot is refilled while it may still be read). Neither side restates them.
 *
 * Activations travel in PAIRS of 64-byte K tiles: 128 contiguous bytes of a row = one whole cache line where the row base is
 * 128-byte aligned. The pair image in LDS is row-major [256 rows][8 slots of 16 B] = 32 KiB; slot s of row r holds K chunk
 * s ^ a_swizzle(r) of the pair. Weights keep their 64-byte tiles (pack.h's image: 16 fragments of 1 KiB per tile).
 *
 * LDS: three activation pair slots (96 KiB), a three-slot ring of weight tiles (48 KiB), the waves' bias lines (4 KiB).
 */
#pragma once

#include <stdint.h>

namespace qnnp {
namespace g256x {

constexpr uint32_t kRows = 256;                  // activation rows of a workgroup tile
constexpr uint32_t kTileK = 64;                  // bytes of K per MFMA step = one K tile
constexpr uint32_t kPairK = 2 * kTileK;          // bytes of K per activation pair
constexpr uint32_t kChunk = 16;                  // bytes per lane of an LDS-DMA instruction / a ds_read_b128
constexpr uint32_t kPairChunks = kPairK / kChunk;
constexpr uint32_t kWgThreads = 512;
constexpr uint32_t kAPieces = 4;                 // LDS-DMA instructions per thread and activation pair: 64 rows each
constexpr uint32_t kWPieces = 2;                 // ... and weight tile: 8 fragments of 1 KiB each
constexpr uint32_t kPieceRows = kWgThreads / kPairChunks;
constexpr uint32_t kASlots = 3;
constexpr uint32_t kWSlots = 3;
constexpr uint32_t kPairBytes = kRows * kPairK;  // 32 KiB
constexpr uint32_t kWTileBytes = 256 * kTileK;   // 16 KiB
constexpr uint32_t kABase = 0;
constexpr uint32_t kWBase = kABase + kASlots * kPairBytes;
constexpr uint32_t kBiasBase = kWBase + kWSlots * kWTileBytes;
constexpr uint32_t kLdsBytes = kBiasBase + 8 * 512;
static_assert(kLdsBytes <= 160 * 1024, "one workgroup per CU, within the CU's LDS");

/* Slot of K chunk c of row r: c ^ a_swizzle(r). At the 128-byte row pitch two rows share a 256-byte bank row, so a
 * ds_read_b128 lane group (8 rows reading chunk c, 8 reading c + 1) must spread over 2 row parities x 8 slots: bits 0-1 of
 * the swizzle separate the row pairs of a quartet of pairs, bit 2 moves rows 4..11 into the other slot quad. */
constexpr uint32_t a_swizzle(uint32_t r) { return ((r >> 1) & 3u) | ((((r >> 2) ^ (r >> 3)) & 1u) << 2); }

/* ---- LDS-DMA: thread `tid` (0..511) of piece `piece` (0..3) of a pair ---- */
constexpr uint32_t a_dma_row(uint32_t piece, uint32_t tid) { return piece * kPieceRows + (tid >> 3); }
/* K chunk of the pair the lane fetches. `half`: the pair is the unpaired last tile of an odd tile count -- only chunks 0..3
 * exist; the lanes of the upper four fetch the lower four once more (into slots nothing reads), never past the row. */
constexpr uint32_t a_dma_chunk(uint32_t tid, bool half)
{
  const uint32_t c = (tid & 7u) ^ a_swizzle(tid >> 3);   // a_swizzle(row) == a_swizzle(tid >> 3): piece * 64 leaves bits 1-3
  return half ? (c & 3u) : c;
}
/* byte of the pair slot the lane's 16 bytes land at: M0 (a_dma_wave_dst) + lane * 16 */
constexpr uint32_t a_dma_dst(uint32_t piece, uint32_t tid) { return (piece * kWgThreads + tid) * kChunk; }
constexpr uint32_t a_dma_wave_dst(uint32_t piece, uint32_t wave) { return (piece * kWgThreads + wave * 64u) * kChunk; }
/* the tensor row a tile row stands for: rows at and past `rows` re-read the last one (their results are never stored) */
constexpr uint32_t a_clamp_row(uint32_t m, uint32_t rows) { return m < rows ? m : rows - 1u; }
/* lane offset of the fetch from the row's first byte of the pair */
constexpr uint32_t a_dma_src(uint32_t tid, bool half) { return a_dma_chunk(tid, half) * kChunk; }

/* ---- fragment reads: lane l of row tile tm of wave row wm, K tile h (0 / 1) of the pair ---- */
constexpr uint32_t a_frag_row(uint32_t wm, uint32_t tm, uint32_t lane) { return 64u * wm + 16u * tm + (lane & 15u); }
constexpr uint32_t a_frag_chunk(uint32_t h, uint32_t lane) { return 4u * h + (lane >> 4); }
constexpr uint32_t a_lds_byte(uint32_t row, uint32_t chunk) { return row * kPairK + ((chunk ^ a_swizzle(row)) << 4); }

/* ---- ring slots ---- */
constexpr uint32_t a_slot(uint32_t pair) { return pair % kASlots; }
constexpr uint32_t w_slot(uint32_t kt) { return kt % kWSlots; }
constexpr uint32_t num_pairs(uint32_t ktiles) { return (ktiles + 1u) / 2u; }
constexpr bool pair_is_half(uint32_t pair, uint32_t ktiles) { return (ktiles & 1u) != 0 && pair + 1u == num_pairs(ktiles); }

/*
 * ---- schedule ----
 * Prologue: pair 0, weight tile 0, bias line | pair 1, weight tiles 1, 2; wait vmcnt(kPrologueVmcnt) + barrier: tile 0 resident.
 * Tile kt: phase 1 issues activation pieces 2 (kt & 1), 2 (kt & 1) + 1 of pair (kt >> 1) + 2   (into the slot of pair (kt >> 1) - 1);
 *          counted wait + barrier(kt): weight tile kt + 1 and the pair of tile kt + 1 are resident, every read of tile kt is done;
 *          phase 2 issues the two pieces of weight tile kt + 3                                   (into the slot of tile kt).
 * So an activation piece is issued four or five barriers, a weight piece two K tiles, ahead of the barrier that needs it.
 */
constexpr uint32_t a_issue_pair(uint32_t kt) { return (kt >> 1) + 2u; }
constexpr uint32_t a_issue_piece(uint32_t kt, uint32_t j) { return 2u * (kt & 1u) + j; }
constexpr uint32_t w_issue_tile(uint32_t kt) { return kt + 3u; }
constexpr int kPrologueVmcnt = 8;                // behind pair 0, weight tile 0, the bias line: pair 1 (4), weight tiles 1, 2 (2 + 2)
constexpr int kFirstVmcnt = 4;                   // barrier(0), behind weight tile 1: weight tile 2 (2), phase 1 of tile 0 (2)
constexpr int kSteadyVmcnt = 6;                  // barrier(kt), behind weight tile kt + 1: phase 1 (kt - 1), phase 2 (kt - 1), phase 1 (kt)
constexpr uint32_t kDrain = 5;                   // the last tiles differ: `left` = ktiles - kt, 5 .. 1
/* what phase 1 of the tile issues: 0 nothing, 1 two whole pieces, 2 two pieces of the unpaired last tile */
constexpr int p1_mode(bool odd, uint32_t left) { return odd ? (left >= 6 ? 1 : left >= 4 ? 2 : 0) : (left >= 5 ? 1 : 0); }
constexpr bool p2_issues(uint32_t left) { return left >= 4; }
/* vmcnt of the tile's wait + barrier; -1: none (the last tile has nothing behind it to wait for). The 0 at left == 2 is the
 * last one that has anything to wait for: behind it every tile is resident. */
constexpr int sync_vmcnt(bool odd, uint32_t left)
{
  if (left >= 6) return kSteadyVmcnt;
  if (odd) return left == 5 ? 6 : left == 4 ? 6 : left == 3 ? 4 : left == 2 ? 0 : -1;
  return left == 5 ? 6 : left == 4 ? 4 : left == 3 ? 2 : left == 2 ? 0 : -1;
}
/* ring slots as literals: the tile count the ALIGNED kernel is written for (period 6: three pairs = six weight tiles) */
constexpr uint32_t kPeriod = 6;
constexpr bool literal_slots(uint32_t ktiles) { return ktiles >= 10u && ktiles % kPeriod == 4u; }

}  // namespace g256x
}  // namespace qnnp
