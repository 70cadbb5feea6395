/*
 * qd8f32gemm4g.hip -- the launches behind the row kernel of the GROUPED dynamically quantized fully connected operator with
 * MXFP4 weights (qnnp_gfx950_create_grouped_fully_connected_nc_f32_qd8_mxfp4w; include/qnnpack_gfx950_dynamic.h has the
 * definition): `groups` weight sets -- the experts of a mixture-of-experts layer -- and per output row j an id, group_ids[j],
 * that the DEVICE reads when the launches run. Output row j is input row j / A times the weights of that group; an id outside
 * [0, groups) leaves the row unwritten. No reference counterpart.
 *
 * The arithmetic per output row is qd8f32gemm4m.hip's, bit for bit: the decode and the terms are qd8_mxfp4.hip.h's, the image,
 * the table, the split of K, the LDS regions, the owners of the ordered chain and the flush schedule are that unit's, kernel
 * for kernel. What is here is the scheduling around it, which nothing fixes before the ids are read:
 *
 *   qd8_grouped_plan (one workgroup of 1024 threads, one thread per possible group). A histogram of the valid ids in LDS
 *       (LDS atomics), two inclusive scans over the groups in one sweep -- rows per group and TILES per group, a tile being
 *       up to H rows of ONE group --, then a second pass over the ids that deals each row j a position in its group's run of
 *       `perm` (an LDS cursor per group), and one 16-byte entry per tile, {group, first position in perm, rows 1 .. H, 0},
 *       found per tile by a binary search of the tile scan so that one crowded group does not serialise the writing. Last,
 *       the tile count. The order of the rows inside a group is whatever the atomics gave: every output row is computed for
 *       itself, so no bit depends on it.
 *
 *   The product kernels run on a grid that the HOST fixed before any id existed: T x column tiles workgroups with
 *       T = floor(R / H) + min(groups, R) >= sum_g ceil(count_g / H), R the number of output rows: a group with count_g rows
 *       has floor(count_g / H) full tiles, in all at most floor(R / H), and at most one partial tile, and at most min(groups, R)
 *       groups have a row at all. A workgroup whose tile index is at or past the device's tile count leaves at once. Inside a
 *       tile the group picks the image, the table and the bias base -- wave-uniform, so scalar -- and the rows are GATHERED:
 *       row i of the tile is input row perm[first + i] / A, whose quantized bytes the LDS-DMA fetches at the byte offset
 *       (perm[first + i] / A) * k_pad from ONE scalar base (a 32-bit lane offset: input rows * k_pad <= 2^31 is the host's check),
 *       whose row entry gives the zero offset and the scale, and whose result is SCATTERED to output row perm[first + i]. Rows
 *       past the tile's count re-read its last row and are never stored. j / A is one v_mul_hi_u32 with ceil(2^32 / A), exact
 *       for j < 2^20 and A <= 8 (the error term j * (A - 1) / (A * 2^32) is below 1 / A).
 *
 *   qd8_f32_mxfp4w_grouped_mfma_16        H = 16: qd8_f32_mxfp4w_gemv_mfma_16 per (tile, 16-channel block)
 *   qd8_f32_mxfp4w_grouped_mfma_128x128   H = 128: qd8_f32_mxfp4w_gemm_mfma_128x128 per (tile, 128-channel tile)
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

struct GroupedParams {
  const uint8_t* a;                             // [input rows][k_pad] int8
  const qnnp_hip_qd8_row_entry* rows_tab;       // [input rows]
  const uint8_t* w;                             // [groups] block-32 pair-fragment images of raw E2M1 codes
  const v4i* table;                             // [groups][n_pad / 16][kpairs][16]: 256 * wsum2 + e
  const float* bias;                            // [groups][n_pad]
  const uint32_t* perm;                         // what the plan kernel wrote
  const qnnp_hip_qd8_grouped_tile* tiles;
  const uint32_t* tile_count;
  float* out;
  uint64_t out_stride;                          // elements
  uint32_t rows;                                // output rows R
  uint32_t n, n_pad, k_pad;
  uint32_t tiles_n;                             // column tiles per row tile
  uint32_t inv_a;                               // ceil(2^32 / A); 0 stands for A = 1
  float out_min, out_max;
};

/* the input row of output row j */
__device__ __forceinline__ uint32_t source_row(uint32_t j, uint32_t inv_a) { return inv_a == 0u ? j : __umulhi(j, inv_a); }

/* this workgroup's tile, in scalar registers */
struct Tile {
  uint32_t group, first, rows;
};
__device__ __forceinline__ Tile load_tile(const GroupedParams& p, uint32_t index)
{
  const qnnp_hip_qd8_grouped_tile t = p.tiles[index];
  Tile tile;
  tile.group = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(t.group));
  tile.first = __builtin_amdgcn_readfirstlane(t.first);
  tile.rows = __builtin_amdgcn_readfirstlane(t.rows);
  return tile;
}
/* output row of row i of the tile (rows past its count: the last); the min keeps a gather inside the tensors whatever perm holds */
__device__ __forceinline__ uint32_t tile_row(const GroupedParams& p, const Tile& t, uint32_t i)
{
  return min(p.perm[t.first + min(i, t.rows - 1u)], p.rows - 1u);
}

/* ---- the plan --------------------------------------------------------------------------------------------------------- */
constexpr int kPlanThreads = 1024;              // = the largest group count

__global__ __launch_bounds__(kPlanThreads)
void qd8_grouped_plan_kernel(const int32_t* ids, uint32_t rows, uint32_t groups, uint32_t tile_shift, uint32_t max_tiles,
                             uint32_t* perm, qnnp_hip_qd8_grouped_tile* tiles, uint32_t* tile_count)
{
  __shared__ uint32_t count[kPlanThreads];      // rows of group g
  __shared__ uint32_t start[kPlanThreads];      // inclusive scan of count, then the first position of group g in perm
  __shared__ uint32_t tend[kPlanThreads];       // inclusive scan of the groups' tile counts
  __shared__ uint32_t cursor[kPlanThreads];     // next free position of group g

  const uint32_t tid = threadIdx.x;
  const uint32_t tile_rows = 1u << tile_shift;
  count[tid] = 0u;
  __syncthreads();
  for (uint32_t j = tid; j < rows; j += kPlanThreads) {
    const uint32_t g = static_cast<uint32_t>(ids[j]);       // a negative id is a large one
    if (g < groups) atomicAdd(&count[g], 1u);
  }
  __syncthreads();
  const uint32_t c = count[tid];                // 0 for tid >= groups
  start[tid] = c;
  tend[tid] = (c + tile_rows - 1u) >> tile_shift;
  __syncthreads();
  for (uint32_t off = 1; off < kPlanThreads; off <<= 1) {
    const uint32_t s = tid >= off ? start[tid - off] : 0u;
    const uint32_t e = tid >= off ? tend[tid - off] : 0u;
    __syncthreads();
    start[tid] += s;
    tend[tid] += e;
    __syncthreads();
  }
  const uint32_t first = start[tid] - c;
  __syncthreads();
  start[tid] = first;
  cursor[tid] = first;
  __syncthreads();
  // the ids are read a second time: were they to change under the launch, a position could leave its group's run, but not perm
  for (uint32_t j = tid; j < rows; j += kPlanThreads) {
    const uint32_t g = static_cast<uint32_t>(ids[j]);
    if (g < groups) {
      const uint32_t at = atomicAdd(&cursor[g], 1u);
      if (at < rows) perm[at] = j;
    }
  }
  const uint32_t total = min(tend[kPlanThreads - 1], max_tiles);      // the bound holds: min is for a reader of this line
  for (uint32_t t = tid; t < total; t += kPlanThreads) {
    uint32_t lo = 0u, hi = groups - 1u;         // the first group whose scan is above t
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (tend[mid] > t) hi = mid; else lo = mid + 1u;
    }
    const uint32_t in_group = t - (tend[lo] - ((count[lo] + tile_rows - 1u) >> tile_shift));
    const uint32_t done = in_group << tile_shift;
    qnnp_hip_qd8_grouped_tile entry;
    entry.group = static_cast<int32_t>(lo);
    entry.first = start[lo] + done;
    entry.rows = min(tile_rows, count[lo] - done);
    entry.zero = 0u;
    tiles[t] = entry;
  }
  if (tid == 0u) *tile_count = total;
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

/* the zero offsets, or at the end the whole entries and output rows, of the lane's four rows of accumulator tile row i0 */
struct GatheredQuad {
  qnnp_hip_qd8_row_entry e[4];
  uint32_t out_row[4];
};
__device__ __forceinline__ GatheredQuad load_gathered(const GroupedParams& p, const Tile& t, uint32_t i0)
{
  const uint32_t first = i0 + 4u * ((threadIdx.x & 63u) >> 4);
  GatheredQuad q;
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) {
    q.out_row[r] = tile_row(p, t, first + r);
    q.e[r] = p.rows_tab[source_row(q.out_row[r], p.inv_a)];
  }
  return q;
}

__global__ __launch_bounds__(kGemmThreads, 2)
void qd8_f32_mxfp4w_grouped_mfma_128x128_kernel(const GroupedParams p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStage];

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t wm = wave >> 1, wn = wave & 1u;
  const uint32_t m_tile = blockIdx.x / p.tiles_n;
  if (m_tile >= *p.tile_count) return;                   // the grid is the bound T, the routing needed fewer tiles
  const uint32_t n_tile = blockIdx.x - m_tile * p.tiles_n;
  const Tile tl = load_tile(p, m_tile);
  const uint32_t ktiles = p.k_pad / kBK;
  const uint32_t kpairs = (ktiles + 1u) / 2u;
  const uint32_t nblocks = p.n_pad / 16;
  const uint64_t group_block = static_cast<uint64_t>(tl.group) * nblocks;      // the group's first channel block

  // activations and weights are staged as in qd8_f32_mxfp4w_gemm_mfma_128x128: waves 0 and 1 bring in the even K tile's
  // half, waves 2 and 3 the odd one's; piece pc = (wave & 1) * 256 + i * 64 + lane of a half = (row pc >> 2, slot pc & 3),
  // the row being a gathered one
  const uint32_t a_half = wave >> 1;
  const uint8_t* a_tile = scalar_ptr(p.a + a_half * kBK);
  uint32_t a_src[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t pc = (wave & 1u) * 256u + i * 64u + lane;
    const uint32_t row = pc >> 2, slot = pc & 3u;
    a_src[i] = source_row(tile_row(p, tl, row), p.inv_a) * p.k_pad + ((slot ^ a_swizzle(row)) << 4);   // < 2^31: the host's check
  }
  // weights: pair fragment f = wave * kWFrags + i of the tile = channel block n_tile * (kBN / 16) + f of the group's image
  // (past it: its last)
  const uint8_t* w_frag[kWFrags];
#pragma unroll
  for (int i = 0; i < kWFrags; i++) {
    const uint32_t nb = min(n_tile * (kBN / 16) + wave * kWFrags + i, nblocks - 1u);
    w_frag[i] = scalar_ptr(p.w + (group_block + nb) * kpairs * 1024u);
  }
  // the odd half of a last pair past k_pad is not fetched: it would lie behind the row (behind the scratch, for the last row)
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
  // the lane's channels c_base + 16 tn: their entries of the group's table, per pair (the channel block is wave-uniform;
  // past the image: the last block)
  const v4i* table = reinterpret_cast<const v4i*>(scalar_ptr(reinterpret_cast<const uint8_t*>(p.table + group_block * kpairs * 16u)));
  const uint32_t c_base = n_tile * kBN + wn * (16u * kTN) + frow;
  uint32_t t_chan[kTN];
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) {
    t_chan[tn] = min(n_tile * (kBN / 16) + wn * kTN + tn, nblocks - 1u) * kpairs * 16u + frow;     // < 2^20 * 2^8 * 2^4
  }
  // the lane's sixteen rows: 128 - zp_r of the rows they were gathered from
  int32_t zo[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
    const GatheredQuad rows = load_gathered(p, tl, wm * 64u + tm * 16u);
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
  for (int tn = 0; tn < kTN; tn++) tab_next[tn] = table[t_chan[tn]];
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
      for (int tn = 0; tn < kTN; tn++) tab_next[tn] = table[t_chan[tn] + (kp + 1u) * 16u];
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

  const float* group_bias = p.bias + static_cast<uint64_t>(tl.group) * p.n_pad;
  float bias[kTN];
#pragma unroll
  for (int tn = 0; tn < kTN; tn++) bias[tn] = group_bias[min(c_base + tn * 16u, p.n_pad - 1u)];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
    const uint32_t i0 = wm * 64u + tm * 16u;
    const GatheredQuad rows = load_gathered(p, tl, i0);
    const uint32_t first = i0 + 4u * fg;
#pragma unroll
    for (int tn = 0; tn < kTN; tn++) {
      const uint32_t c = c_base + tn * 16u;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) {
        const float y = qb4w_finish(ysum[tm][tn][r], rows.e[r], bias[tn], p.out_min, p.out_max);
        if (first + r < tl.rows && c < p.n) p.out[static_cast<uint64_t>(rows.out_row[r]) * p.out_stride + c] = y;
      }
    }
  }
}

/* ---- tiles of 16 rows ------------------------------------------------------------------------------------------------- */
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
void qd8_f32_mxfp4w_grouped_mfma_16_kernel(const GroupedParams p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kGemvWaves * kGemvRegion];

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t m_tile = blockIdx.x / p.tiles_n;             // tiles_n = n_pad / 16 here
  if (m_tile >= *p.tile_count) return;
  const uint32_t nb = blockIdx.x - m_tile * p.tiles_n;
  const Tile tl = load_tile(p, m_tile);
  const uint32_t ktiles = p.k_pad / 64u;
  const uint32_t kpairs = (ktiles + 1u) / 2u;
  const uint32_t frow = lane & 15u, fg = lane >> 4;
  const uint64_t block = static_cast<uint64_t>(tl.group) * p.tiles_n + nb;       // channel block nb of the group's image

  const v4i* w_block = reinterpret_cast<const v4i*>(p.w + block * kpairs * 1024u);
  const v4i* t_chan = p.table + block * kpairs * 16u + frow;
  const uint64_t a_base = scalar_ptr(reinterpret_cast<uint64_t>(p.a));
  // rows past the tile's count re-read its last: never stored. < 2^31: the host's check
  const uint32_t a_lane = source_row(tile_row(p, tl, frow), p.inv_a) * p.k_pad + fg * 16u;
  uint8_t* mine = lds + wave * kGemvRegion;                                   // this wave's tiles of a pass, fragment order
  const uint32_t mine_off = __builtin_amdgcn_readfirstlane(lds_offset(mine));
  // the lane's operand of block half h of a staged tile: staged lane 16 (2 h + fg / 2) + frow, its half fg % 2
  const uint32_t a_piece = ((fg >> 1) * 16u + frow) * 16u + 8u * (fg & 1u);       // + tile * 1024 + h * 512
  // the rows of this lane's accumulator registers, for the terms it produces
  int32_t zo[4];
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) zo[r] = p.rows_tab[source_row(tile_row(p, tl, 4u * fg + r), p.inv_a)].zero_offset;

  float ysum = 0.0f;                            // owners: output (row 4 fg + wave of the tile, channel frow)
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
  const uint32_t out_row = tile_row(p, tl, row);
  const float y = qb4w_finish(ysum, p.rows_tab[source_row(out_row, p.inv_a)],
                              p.bias[static_cast<uint64_t>(tl.group) * p.n_pad + c], p.out_min, p.out_max);
  if (row < tl.rows && c < p.n) p.out[static_cast<uint64_t>(out_row) * p.out_stride + c] = y;
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_qd8_mxfp4w_grouped_run(const struct qnnp_hip_qd8_mxfp4w_grouped_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr) return QNNP_HIP_EINVAL;
  if (a->quantized == nullptr || a->row_table == nullptr || a->packed_w == nullptr || a->block_table == nullptr ||
      a->bias == nullptr || a->group_ids == nullptr || a->perm == nullptr || a->tiles == nullptr || a->tile_count == nullptr ||
      a->output == nullptr || (reinterpret_cast<uintptr_t>(a->output) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(a->group_ids) & 3u) != 0 || (reinterpret_cast<uintptr_t>(a->quantized) & 15u) != 0 ||
      (reinterpret_cast<uintptr_t>(a->packed_w) & 15u) != 0 || (reinterpret_cast<uintptr_t>(a->block_table) & 15u) != 0 ||
      (reinterpret_cast<uintptr_t>(a->tiles) & 15u) != 0 || a->n == 0 || a->n >= (1u << 24) ||
      a->n_pad != ((a->n + 15u) & ~15u) || a->k_pad == 0 || a->k_pad > 32768u || a->k_pad % 64u != 0 ||
      a->rows >= (1u << 20) || a->assignments == 0 || a->assignments > 8u || a->rows % a->assignments != 0 ||
      static_cast<uint64_t>(a->rows / a->assignments) * a->k_pad > (1ull << 31) || a->groups == 0 || a->groups > 1024u ||
      (a->tile_rows != 16u && a->tile_rows != 128u) ||
      a->max_tiles != a->rows / a->tile_rows + (a->groups < a->rows ? a->groups : a->rows) || a->output_stride < a->n) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  const bool wide = a->tile_rows == 128u;
  const uint32_t tiles_n = wide ? (a->n + kBN - 1u) / kBN : a->n_pad / 16u;
  const uint64_t grid_size = static_cast<uint64_t>(a->max_tiles) * tiles_n;
  if (grid_size > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;      // a grid that would wrap is refused, not launched
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  hipLaunchKernelGGL(qd8_grouped_plan_kernel, dim3(1), dim3(kPlanThreads), 0, stream, a->group_ids, a->rows, a->groups,
                     wide ? 7u : 4u, a->max_tiles, a->perm, a->tiles, a->tile_count);
  const int planned = launch_status();
  if (planned != QNNP_HIP_OK) return planned;
  GroupedParams p;
  p.a = reinterpret_cast<const uint8_t*>(a->quantized);
  p.rows_tab = a->row_table;
  p.w = reinterpret_cast<const uint8_t*>(a->packed_w);
  p.table = reinterpret_cast<const v4i*>(a->block_table);
  p.bias = a->bias;
  p.perm = a->perm;
  p.tiles = a->tiles;
  p.tile_count = a->tile_count;
  p.out = a->output;
  p.out_stride = a->output_stride;
  p.rows = a->rows;
  p.n = a->n;
  p.n_pad = a->n_pad;
  p.k_pad = a->k_pad;
  p.tiles_n = tiles_n;
  p.inv_a = a->assignments == 1u ? 0u : static_cast<uint32_t>(((1ull << 32) + a->assignments - 1u) / a->assignments);
  p.out_min = a->output_min;
  p.out_max = a->output_max;
  const dim3 grid(static_cast<uint32_t>(grid_size));
  if (wide) {
    hipLaunchKernelGGL(qd8_f32_mxfp4w_grouped_mfma_128x128_kernel, grid, dim3(kGemmThreads), 0, stream, p);
    if (kernel_name != nullptr) *kernel_name = "qd8_f32_mxfp4w_grouped_mfma_128x128";
  } else {
    hipLaunchKernelGGL(qd8_f32_mxfp4w_grouped_mfma_16_kernel, grid, dim3(kGemvThreads), 0, stream, p);
    if (kernel_name != nullptr) *kernel_name = "qd8_f32_mxfp4w_grouped_mfma_16";
  }
  return launch_status();
}
