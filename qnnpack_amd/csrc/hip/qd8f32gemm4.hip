/*
 * qd8f32gemm4.hip -- the second launch of the dynamically quantized fully connected operator with 4-BIT weights
 * (qnnp_gfx950_create_fully_connected_nc_f32_qd8_qc4w; include/qnnpack_gfx950_dynamic.h has the definition): int8 rows
 * (what f32qd8rows.hip wrote) times signed nibbles on v_mfma_i32_16x16x64_i8, behind the float epilogue of
 * qd8_epilogue.hip.h. The first kernels of this library that read an operand narrower than a byte. No reference counterpart.
 *
 * The weight image (dynamic-fully-connected.c packs it) is made of 1-KiB PAIR fragments, one per channel block nb and
 * K-tile pair kp, at (nb * kpairs + kp) * 1024 with kpairs = ceil(k_pad / 128). Byte j of lane l's sixteen bytes holds
 * two weights of channel 16 nb + l % 16: K position 128 kp + 16 (l / 16) + j in its low nibble and K position
 * 128 kp + 64 + 16 (l / 16) + j in its high nibble. One 16-byte load per lane is therefore the MFMA's second operand for
 * TWO consecutive 64-deep K tiles, and a dword d of it unpacks with three vector operations:
 *   (d & 0x0F0F0F0F) << 4     the even K tile
 *    d & 0xF0F0F0F0           the odd K tile
 * Either way a byte is the nibble in its top four bits, which read as int8 is 16 * w in [-128, 112]: no sign extension,
 * no subtraction. The loop accumulates 16 * sum (q - 128) * w, at most 128 * 128 * 32768 = 2^29 in magnitude; the epilogue
 * shifts right by four arithmetically -- exact, every term is a multiple of 16 -- and hands the sum to qd8_store_tile.
 * K tiles past k_pad / 64 (the odd half of the last pair when that count is odd) are neither fetched as activations
 * beyond a row's k_pad bytes nor multiplied.
 *
 *   qd8_f32_qc4w_gemm_mfma_128x128   rows > 16. 128 x 128 tiles, four waves of 64 x 64. A K step is one tile PAIR, 128
 *       K positions: the activation tile is 128 x 128 bytes kept as two 8-KiB halves, each [row][4 chunks] with the chunk
 *       swizzle of qd8f32gemm.hip; the weight tile stays PACKED in LDS, eight pair fragments = 8 KiB. 24 KiB per stage,
 *       48 KiB double-buffered, all by 16-byte LDS-DMA. A lane reads its sixteen packed bytes back at lane * 16, unpacks
 *       them in registers and feeds two MFMAs per accumulator tile: 32 MFMAs per wave behind one barrier.
 *   qd8_f32_qc4w_gemv_mfma_16        rows <= 16. One 512-thread workgroup per 16-channel block, eight waves splitting K,
 *       eight K tiles per wave and pass as in qd8_f32_gemv_mfma_16 -- which is FOUR 16-byte weight loads per lane. All
 *       four are issued before the pass's eight LDS-DMA requests, so nothing has to wait between them.
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

/* the two MFMA operands in one packed register quadruple */
__device__ __forceinline__ v4i qc4w_even(const v4i& d)
{
  const int m = 0x0F0F0F0F;
  return (d & v4i{m, m, m, m}) << 4;
}
__device__ __forceinline__ v4i qc4w_odd(const v4i& d)
{
  const int m = static_cast<int>(0xF0F0F0F0u);
  return d & v4i{m, m, m, m};
}
/* 16 * sum -> sum: every term was a multiple of 16 */
__device__ __forceinline__ v4i qc4w_scale_down(const v4i& acc) { return acc >> 4; }

/* ---- 128 x 128 tiles ------------------------------------------------------------------------------------------------ */
constexpr int kBM = 128;
constexpr int kBN = 128;
constexpr int kBK = 64;                        // one K tile; a step is two
constexpr int kAHalf = kBM * kBK;             // 8 KiB: the rows' bytes of one K tile
constexpr int kATile = 2 * kAHalf;
constexpr int kWTile = kBN * kBK;             // 8 KiB: eight pair fragments, packed
constexpr int kStage = kATile + kWTile;       // 24 KiB
constexpr int kGemmThreads = 256;

__global__ __launch_bounds__(kGemmThreads, 2)
void qd8_f32_qc4w_gemm_mfma_128x128_kernel(const Qd8Params p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStage];

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

  // activations: waves 0 and 1 bring in the even K tile's half, waves 2 and 3 the odd one's. Piece pc = (wave & 1) * 256 +
  // i * 64 + lane of a half's 512 = (row pc >> 2, slot pc & 3), which holds the row's chunk slot ^ swizzle(row). Lane
  // offsets are relative to the tile's first row: below 128 * 32768.
  const uint32_t a_half = wave >> 1;
  const uint8_t* a_tile = scalar_ptr(p.a + static_cast<uint64_t>(m0) * p.k_pad + a_half * kBK);
  uint32_t a_src[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t pc = (wave & 1u) * 256u + i * 64u + lane;
    const uint32_t row = pc >> 2, slot = pc & 3u;
    a_src[i] = min(row, last_row) * p.k_pad + ((slot ^ a_swizzle(row)) << 4);
  }
  // weights: pair fragment f = wave * 2 + i of the tile's eight = channel block n_tile * 8 + f (past the image: the last block)
  const uint8_t* w_frag[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const uint32_t nb = min(n_tile * 8u + wave * 2u + i, nblocks - 1u);
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
    for (int i = 0; i < 2; i++) dma16_saddr(scalar_ptr(w_frag[i] + kp * 1024u), lane * 16u, st + kATile + (wave * 2u + i) * 1024u);
  };

  const uint32_t frow = lane & 15u, fg = lane >> 4;
  const uint32_t a_off = (wm * 64u + frow) * kBK + ((fg ^ a_swizzle(frow)) << 4);       // + half * 8192 + tm * 1024
  const uint32_t w_off = kATile + wn * 4096u + lane * 16u;                                // + tn * 1024
  v4i acc[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
#pragma unroll
    for (int tn = 0; tn < 4; tn++) acc[tm][tn] = v4i{0, 0, 0, 0};
  }

  stage(0u, 0u);
  for (uint32_t kp = 0; kp < kpairs; kp++) {
    const uint32_t slot = kp & 1u;
    // pair kp was requested a step ago and is all this wave has in flight; behind the barrier every wave's part has landed and
    // every wave is done reading the other stage
    wait_vmcnt<0>();
    __syncthreads();
    QNNP_PIN();
    if (kp + 1u < kpairs) stage(kp + 1u, slot ^ 1u);
    QNNP_PIN();
    const uint8_t* st = lds + slot * kStage;
    v4i fa[4], fw[4];
#pragma unroll
    for (int tn = 0; tn < 4; tn++) fw[tn] = *reinterpret_cast<const v4i*>(st + w_off + tn * 1024);
#pragma unroll
    for (int tm = 0; tm < 4; tm++) fa[tm] = *reinterpret_cast<const v4i*>(st + a_off + tm * 1024);
#pragma unroll
    for (int tm = 0; tm < 4; tm++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int tn = (tm & 1) != 0 ? 3 - j : j;                // snake: one operand changes per MFMA
        acc[tm][tn] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[tm], qc4w_even(fw[tn]), acc[tm][tn], 0, 0, 0);
      }
    }
    if (2u * kp + 1u < ktiles) {
#pragma unroll
      for (int tm = 0; tm < 4; tm++) fa[tm] = *reinterpret_cast<const v4i*>(st + kAHalf + a_off + tm * 1024);
#pragma unroll
      for (int tm = 0; tm < 4; tm++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int tn = (tm & 1) != 0 ? 3 - j : j;
          acc[tm][tn] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[tm], qc4w_odd(fw[tn]), acc[tm][tn], 0, 0, 0);
        }
      }
    }
    QNNP_PIN();
  }

  const uint32_t c_base = n_tile * kBN + wn * 64u + frow;
  qnnp_hip_qd8_channel_entry ch[4];
#pragma unroll
  for (int tn = 0; tn < 4; tn++) ch[tn] = p.chan_tab[min(c_base + tn * 16u, p.n_pad - 1u)];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
    const uint32_t row0 = m0 + wm * 64u + tm * 16u;
    const RowQuad rows = qd8_load_rows(row0, p);
#pragma unroll
    for (int tn = 0; tn < 4; tn++) qd8_store_tile(qc4w_scale_down(acc[tm][tn]), row0, rows, c_base + tn * 16u, ch[tn], p);
  }
}

/* ---- rows <= 16 ------------------------------------------------------------------------------------------------------ */
constexpr int kGemvWaves = 8;
constexpr int kGemvThreads = kGemvWaves * 64;
constexpr int kGemvTiles = 8;                 // K tiles per wave and pass
constexpr int kGemvPairs = kGemvTiles / 2;    // = weight loads per lane and pass
constexpr int kGemvPass = kGemvWaves * kGemvTiles;   // 64 tiles = 4096 K positions = 64 KiB of LDS

__global__ __launch_bounds__(kGemvThreads)
void qd8_f32_qc4w_gemv_mfma_16_kernel(const Qd8Params p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kGemvPass * 1024];

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nb = blockIdx.x;
  const uint32_t ktiles = p.k_pad / 64u;
  const uint32_t kpairs = (ktiles + 1u) / 2u;
  const uint32_t frow = lane & 15u, fg = lane >> 4;

  const v4i* w_block = reinterpret_cast<const v4i*>(p.w + static_cast<uint64_t>(nb) * kpairs * 1024u);
  const uint64_t a_base = scalar_ptr(reinterpret_cast<uint64_t>(p.a));
  const uint32_t a_lane = min(frow, p.rows - 1u) * p.k_pad + fg * 16u;      // rows past the batch re-read the last: never stored
  uint8_t* mine = lds + wave * (kGemvTiles * 1024);                           // this wave's tiles of a pass, fragment order
  const uint32_t mine_off = __builtin_amdgcn_readfirstlane(lds_offset(mine));

  v4i acc = v4i{0, 0, 0, 0};
  for (uint32_t kt0 = wave * kGemvTiles; kt0 < ktiles; kt0 += kGemvPass) {       // kt0 is even: pair kt0 / 2 starts at it
    // pairs and tiles past K re-read the last one (fixed counts; their products are left out below). Every weight load
    // of the pass goes out before the first LDS-DMA request, which the compiler does not count: it has nothing to wait
    // for between them.
    v4i fw[kGemvPairs];
#pragma unroll
    for (int t = 0; t < kGemvPairs; t++) fw[t] = w_block[static_cast<uint64_t>(min(kt0 / 2u + t, kpairs - 1u)) * 64u + lane];
    QNNP_PIN();
#pragma unroll
    for (int t = 0; t < kGemvTiles; t++) {
      const uint32_t kt = min(kt0 + t, ktiles - 1u);
      dma16_saddr_ordered(scalar_ptr(a_base + kt * 64u), a_lane, __builtin_amdgcn_readfirstlane(mine_off + t * 1024u));
    }
    wait_vmcnt<0>();       // the wave reads only what it brought in itself: no barrier
    QNNP_PIN();
#pragma unroll
    for (int t = 0; t < kGemvPairs; t++) {
      const v4i fa0 = *reinterpret_cast<const v4i*>(mine + (2 * t) * 1024 + lane * 16u);
      const v4i fa1 = *reinterpret_cast<const v4i*>(mine + (2 * t + 1) * 1024 + lane * 16u);
      if (kt0 + 2 * t < ktiles) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa0, qc4w_even(fw[t]), acc, 0, 0, 0);
      if (kt0 + 2 * t + 1 < ktiles) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa1, qc4w_odd(fw[t]), acc, 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the LDS reads are done before the next pass overwrites the tiles
  }

  // the eight partial tiles meet in LDS (over the staged tiles, which every wave is done with behind the barrier)
  __syncthreads();
  v4i* partial = reinterpret_cast<v4i*>(lds);
  partial[wave * 64u + lane] = acc;
  __syncthreads();
  if (wave != 0) return;
  v4i sum = partial[lane];
#pragma unroll
  for (int w = 1; w < kGemvWaves; w++) {
    const v4i part = partial[w * 64 + lane];
    sum[0] += part[0];
    sum[1] += part[1];
    sum[2] += part[2];
    sum[3] += part[3];
  }
  const uint32_t c = nb * 16u + frow;            // < n_pad
  qd8_store_tile(qc4w_scale_down(sum), 0u, qd8_load_rows(0u, p), c, p.chan_tab[c], p);
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_qd8_qc4w_gemm_run(const struct qnnp_hip_qd8_gemm_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->quantized == nullptr || a->row_table == nullptr || a->packed_w == nullptr ||
      a->channel_table == nullptr || a->output == nullptr || (reinterpret_cast<uintptr_t>(a->output) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(a->quantized) & 15u) != 0 || (reinterpret_cast<uintptr_t>(a->packed_w) & 15u) != 0 ||
      a->n == 0 || a->n >= (1u << 24) || a->n_pad != ((a->n + 15u) & ~15u) || a->k_pad == 0 || a->k_pad % 64u != 0 ||
      a->k_pad > 32768u || a->rows > 0x7FFFFFFFu || a->output_stride < a->n) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  Qd8Params p;
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
  if (a->rows <= 16u) {
    hipLaunchKernelGGL(qd8_f32_qc4w_gemv_mfma_16_kernel, dim3(a->n_pad / 16u), dim3(kGemvThreads), 0, stream, p);
    if (kernel_name != nullptr) *kernel_name = "qd8_f32_qc4w_gemv_mfma_16";
    return launch_status();
  }
  const uint64_t tiles = static_cast<uint64_t>((a->rows + kBM - 1u) / kBM) * p.tiles_n;
  if (tiles > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;          // a grid that would wrap is refused, not launched
  hipLaunchKernelGGL(qd8_f32_qc4w_gemm_mfma_128x128_kernel, dim3(static_cast<uint32_t>(tiles)), dim3(kGemmThreads), 0, stream, p);
  if (kernel_name != nullptr) *kernel_name = "qd8_f32_qc4w_gemm_mfma_128x128";
  return launch_status();
}
