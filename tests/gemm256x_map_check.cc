/*
 * gemm256x_map_check.cc -- host model of the index maps and the LDS-DMA schedule of the 256 x 256 16x16x64 GEMM
 * (qnnpack_amd/csrc/hip/gemm256x_map.h, the functions the kernel itself calls). Stand-alone: tests/test_gemm256x_map.py
 * compiles it with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and runs it; exit status 0 = all hold.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "gemm256x_map.h"

namespace m = qnnp::g256x;

static int failures = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      if (failures < 20) { printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
      failures++;                                               \
    }                                                           \
  } while (0)

/* 1. the DMA of a pair covers rows x chunks once, onto the 16-byte slot the fragment reads expect; a wave instruction
 *    writes 1 KiB of contiguous LDS; eight consecutive lanes fetch one row's 128 contiguous bytes */
static void check_dma_map()
{
  std::vector<int> hits(m::kPairBytes / m::kChunk, 0);
  std::set<uint32_t> cells;
  for (uint32_t piece = 0; piece < m::kAPieces; piece++) {
    for (uint32_t tid = 0; tid < m::kWgThreads; tid++) {
      const uint32_t row = m::a_dma_row(piece, tid), chunk = m::a_dma_chunk(tid, false), dst = m::a_dma_dst(piece, tid);
      CHECK(row < m::kRows && chunk < m::kPairChunks && dst + m::kChunk <= m::kPairBytes, "piece %u tid %u", piece, tid);
      if (dst + m::kChunk > m::kPairBytes) continue;
      hits[dst / m::kChunk]++;
      cells.insert(row * m::kPairChunks + chunk);
      CHECK(dst == m::a_lds_byte(row, chunk), "piece %u tid %u lands at %u, readers expect %u", piece, tid, dst, m::a_lds_byte(row, chunk));
      CHECK(dst == m::a_dma_wave_dst(piece, tid >> 6) + (tid & 63u) * m::kChunk, "M0 + lane * 16: piece %u tid %u", piece, tid);
      CHECK(m::a_dma_src(tid, false) == chunk * m::kChunk, "tid %u", tid);
      // the unpaired last tile: the same 64 bytes for both halves of the lanes, never the upper 64
      CHECK(m::a_dma_chunk(tid, true) == (chunk & 3u) && m::a_dma_src(tid, true) + m::kChunk <= m::kTileK, "tid %u", tid);
      if ((tid & 7u) == 0) {
        uint32_t mask = 0;
        for (uint32_t j = 0; j < 8; j++) {
          CHECK(m::a_dma_row(piece, tid + j) == row, "piece %u tid %u", piece, tid + j);
          mask |= 1u << m::a_dma_chunk(tid + j, false);
        }
        CHECK(mask == 0xFFu, "lanes %u..%u fetch chunks %#x of row %u", tid, tid + 7, mask, row);
      }
    }
    for (uint32_t wave = 0; wave < 8; wave++) CHECK(m::a_dma_wave_dst(piece, wave) % 1024u == 0, "piece %u wave %u", piece, wave);
  }
  for (size_t i = 0; i < hits.size(); i++) CHECK(hits[i] == 1, "LDS slot %zu written %d times", i, hits[i]);
  CHECK(cells.size() == m::kRows * m::kPairChunks, "%zu (row, chunk) cells fetched", cells.size());
}

/* 2. + 3. fragment reads return the operand layout of v_mfma_i32_16x16x64_i8 (lane l: row l & 15 of the tile, K bytes
 *    16 (l >> 4) .. + 16 of the 64-byte tile), and every ds_read_b128 lane group touches 16 different bank quads */
static void check_fragment_reads()
{
  // the LDS image as the DMA model lays it: (row, chunk) per 16-byte slot
  std::vector<uint32_t> image(m::kPairBytes / m::kChunk, ~0u);
  for (uint32_t piece = 0; piece < m::kAPieces; piece++) {
    for (uint32_t tid = 0; tid < m::kWgThreads; tid++) {
      image[m::a_dma_dst(piece, tid) / m::kChunk] = m::a_dma_row(piece, tid) * m::kPairChunks + m::a_dma_chunk(tid, false);
    }
  }
  static const uint32_t groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                         {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                         {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                         {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  for (uint32_t wm = 0; wm < 4; wm++) {
    for (uint32_t tm = 0; tm < 4; tm++) {
      for (uint32_t h = 0; h < 2; h++) {
        uint32_t addr[64];
        for (uint32_t lane = 0; lane < 64; lane++) {
          const uint32_t row = m::a_frag_row(wm, tm, lane), chunk = m::a_frag_chunk(h, lane);
          CHECK(row == 64 * wm + 16 * tm + (lane & 15u) && chunk == 4 * h + (lane >> 4), "wm %u tm %u h %u lane %u", wm, tm, h, lane);
          addr[lane] = m::a_lds_byte(row, chunk);
          CHECK(addr[lane] % m::kChunk == 0 && addr[lane] < m::kPairBytes, "lane %u", lane);
          CHECK(image[addr[lane] / m::kChunk] == row * m::kPairChunks + chunk, "wm %u tm %u h %u lane %u reads cell %u", wm, tm, h, lane,
                image[addr[lane] / m::kChunk]);
          // the kernel keeps the address of tm == 0 and reaches the other row tiles by an immediate
          CHECK(addr[lane] == m::a_lds_byte(m::a_frag_row(wm, 0, lane), chunk) + tm * 16 * m::kPairK, "wm %u tm %u lane %u", wm, tm, lane);
        }
        for (int grp = 0; grp < 4; grp++) {
          uint32_t quads = 0;
          for (int i = 0; i < 16; i++) quads |= 1u << ((addr[groups[grp][i]] / 16u) % 16u);     // 64 banks x 4 B = 16 quads of 16 B
          CHECK(quads == 0xFFFFu, "wm %u tm %u h %u lane group %d: bank quads %#x", wm, tm, h, grp, quads);
        }
      }
    }
  }
  // slots: a read immediate reaches 64 KiB
  CHECK(m::kPairBytes + 3 * 16 * m::kPairK + m::kPairBytes - 1 < 65536u + m::kPairBytes, "two pair slots per address register");
  CHECK((m::kWSlots - 1) * m::kWTileBytes + 3 * 2048 + 256 + m::kWTileBytes <= 65536u + m::kWTileBytes, "the weight ring per address register");
}

/*
 * 4. the schedule, walked as the kernel walks it, for one tile count and one row layout:
 *    - no lane reads a byte outside [row base, row base + K) of a row below `rows` (row_base[] gives each tensor row's first
 *      byte: the plain form m * stride, or the operator's table);
 *    - every piece is issued once, at least two K tiles ahead of the barrier that needs it resident;
 *    - the counted wait of every barrier covers what the reads behind it need;
 *    - no slot is refilled before the barrier that follows its last fragment read.
 */
struct Dma { int kind; uint32_t index, piece; };   // kind 0: activation pair, 1: weight tile, 2: bias line

static void check_schedule(uint32_t ktiles, uint32_t rows, const std::vector<uint64_t>& row_base, uint64_t tensor_bytes, const char* what)
{
  const uint32_t K = ktiles * m::kTileK, npairs = m::num_pairs(ktiles);
  const uint32_t tiles_m = (rows + m::kRows - 1) / m::kRows;
  const bool odd = (ktiles & 1u) != 0;
  std::vector<Dma> issued;
  size_t complete = 0;                             // issued[0 .. complete) have landed and a barrier has passed
  std::vector<int> a_count(npairs * m::kAPieces, 0), w_count(ktiles * m::kWPieces, 0);
  std::vector<int> barrier_at(ktiles, 0);
  auto resident = [&](int kind, uint32_t index, uint32_t pieces) {
    uint32_t seen = 0;
    for (size_t i = 0; i < complete; i++) seen += issued[i].kind == kind && issued[i].index == index;
    return seen == pieces;
  };
  auto issue_a = [&](uint32_t pair, uint32_t piece, bool half, uint32_t kt_now, bool prologue) {
    CHECK(pair < npairs && piece < m::kAPieces, "%s T %u: pair %u piece %u", what, ktiles, pair, piece);
    if (pair >= npairs) return;
    CHECK(half == m::pair_is_half(pair, ktiles), "%s T %u: pair %u half %d", what, ktiles, pair, half);
    a_count[pair * m::kAPieces + piece]++;
    issued.push_back({0, pair, piece});
    if (!prologue) {
      CHECK(2 * pair - 1 >= kt_now + 2, "%s T %u: pair %u issued in tile %u, needed at barrier %u", what, ktiles, pair, kt_now, 2 * pair - 1);
      // the slot held pair - 3, last read in phase 2 of tile 2 (pair - 3): the barrier of tile 2 (pair - 3) + 1 must lie behind us
      // (pair 2 is the first into its slot)
      CHECK(pair < m::kASlots || (m::a_slot(pair) == m::a_slot(pair - m::kASlots) && kt_now >= 2 * (pair - m::kASlots) + 2 &&
                                  barrier_at[2 * (pair - m::kASlots) + 1]),
            "%s T %u: pair %u refills its slot in tile %u", what, ktiles, pair, kt_now);
    }
    for (uint32_t m_tile = 0; m_tile < tiles_m; m_tile++) {
      for (uint32_t tid = 0; tid < m::kWgThreads; tid++) {
        const uint32_t mrow = m::a_clamp_row(m_tile * m::kRows + m::a_dma_row(piece, tid), rows);
        CHECK(mrow < rows, "%s T %u rows %u: row %u", what, ktiles, rows, mrow);
        const uint64_t in_row = static_cast<uint64_t>(pair) * m::kPairK + m::a_dma_src(tid, half);
        CHECK(in_row + m::kChunk <= K, "%s T %u: pair %u piece %u tid %u reads bytes %llu.. of a %u-byte row", what, ktiles, pair, piece, tid,
              static_cast<unsigned long long>(in_row), K);
        CHECK(row_base[mrow] + in_row + m::kChunk <= tensor_bytes, "%s T %u rows %u: read past the tensor", what, ktiles, rows);
      }
    }
  };
  auto issue_w = [&](uint32_t tile, uint32_t piece, uint32_t kt_now, bool prologue) {
    CHECK(tile < ktiles, "%s T %u: weight tile %u", what, ktiles, tile);
    if (tile >= ktiles) return;
    w_count[tile * m::kWPieces + piece]++;
    issued.push_back({1, tile, piece});
    if (!prologue) {
      // needed at barrier(tile - 1); issued behind barrier(kt_now); the slot held tile - 3 == kt_now, last read in its phase 1
      CHECK(tile - 1 >= kt_now + 2 && m::w_slot(tile) == m::w_slot(kt_now) && barrier_at[kt_now], "%s T %u: weight tile %u issued in tile %u", what,
            ktiles, tile, kt_now);
    }
  };
  auto barrier = [&](int vmcnt) {
    CHECK(static_cast<size_t>(vmcnt) <= issued.size(), "%s T %u", what, ktiles);
    if (issued.size() - vmcnt > complete) complete = issued.size() - vmcnt;
  };

  // prologue
  for (uint32_t piece = 0; piece < m::kAPieces; piece++) issue_a(0, piece, false, 0, true);
  for (uint32_t piece = 0; piece < m::kWPieces; piece++) issue_w(0, piece, 0, true);
  issued.push_back({2, 0, 0});
  for (uint32_t piece = 0; piece < m::kAPieces; piece++) issue_a(1, piece, false, 0, true);
  for (uint32_t tile = 1; tile < 3; tile++) {
    for (uint32_t piece = 0; piece < m::kWPieces; piece++) issue_w(tile, piece, 0, true);
  }
  barrier(m::kPrologueVmcnt);
  CHECK(resident(0, 0, m::kAPieces) && resident(1, 0, m::kWPieces) && resident(2, 0, 1), "%s T %u: tile 0 behind the prologue", what, ktiles);

  for (uint32_t kt = 0; kt < ktiles; kt++) {
    const uint32_t left = ktiles - kt;
    const int p1 = kt == 0 ? 1 : m::p1_mode(odd, left);
    const bool p2 = kt == 0 ? true : m::p2_issues(left);
    const int sync = kt == 0 ? m::kFirstVmcnt : m::sync_vmcnt(odd, left);
    // phase 1 reads the tile's upper weight fragments
    CHECK(resident(1, kt, m::kWPieces), "%s T %u: weight tile %u in its phase 1", what, ktiles, kt);
    if (p1 != 0) {
      for (uint32_t j = 0; j < 2; j++) issue_a(m::a_issue_pair(kt), m::a_issue_piece(kt, j), p1 == 2, kt, false);
    }
    if (sync >= 0) { barrier(sync); barrier_at[kt] = 1; }
    if (kt + 1 < ktiles) {   // phase 2 reads the next tile's lower weight fragments and its activation fragments
      CHECK(resident(1, kt + 1, m::kWPieces), "%s T %u: weight tile %u behind barrier %u", what, ktiles, kt + 1, kt);
      CHECK(resident(0, (kt + 1) >> 1, m::kAPieces), "%s T %u: pair %u behind barrier %u", what, ktiles, (kt + 1) >> 1, kt);
    }
    if (p2) {
      for (uint32_t piece = 0; piece < m::kWPieces; piece++) issue_w(m::w_issue_tile(kt), piece, kt, false);
    }
  }
  for (size_t i = 0; i < a_count.size(); i++) CHECK(a_count[i] == 1, "%s T %u: pair %zu piece %zu issued %d times", what, ktiles, i / 4, i % 4, a_count[i]);
  for (size_t i = 0; i < w_count.size(); i++) CHECK(w_count[i] == 1, "%s T %u: weight tile %zu piece %zu issued %d times", what, ktiles, i / 2, i % 2, w_count[i]);
  CHECK(m::literal_slots(ktiles) ? (!odd && ktiles % m::kPeriod == 4 && ktiles >= m::kPeriod + 4) : true, "T %u", ktiles);
}

int main()
{
  check_dma_map();
  check_fragment_reads();
  static const uint32_t kRowCounts[] = {1, 255, 256, 257};
  for (uint32_t ktiles = 8; ktiles <= 40; ktiles++) {
    const uint32_t K = ktiles * m::kTileK;
    for (uint32_t rows : kRowCounts) {
      for (uint32_t stride : {K, K + 16}) {
        // plain rows; the last row ends where the tensor ends
        std::vector<uint64_t> base(rows);
        for (uint32_t r = 0; r < rows; r++) base[r] = static_cast<uint64_t>(r) * stride;
        check_schedule(ktiles, rows, base, static_cast<uint64_t>(rows - 1) * stride + K, stride == K ? "dense rows" : "strided rows");
      }
      // table rows (a strided 1 x 1 convolution): output row r reads input pixel 2 r of a tensor that ends behind the last one read
      std::vector<uint64_t> base(rows);
      for (uint32_t r = 0; r < rows; r++) base[r] = static_cast<uint64_t>(2 * r) * K;
      check_schedule(ktiles, rows, base, static_cast<uint64_t>(2 * (rows - 1)) * K + K, "table rows");
    }
  }
  if (failures != 0) { printf("%d checks failed\n", failures); return 1; }
  printf("gemm256x map: all checks hold\n");
  return 0;
}
