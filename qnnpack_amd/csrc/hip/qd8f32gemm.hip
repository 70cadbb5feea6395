/*
 * qd8f32gemm.hip -- the second launch of the dynamically quantized fully connected operator (dynamic-fully-connected.c;
 * include/qnnpack_gfx950_dynamic.h has the definition): int8 rows (what f32qd8rows.hip wrote) times int8 weights on
 * v_mfma_i32_16x16x64_i8, and the first epilogue in this library that writes FLOATS from an int32 accumulator. No
 * reference counterpart.
 *
 * Both operands are plain signed int8 -- the rows are q - 128, the weights symmetric -- so the loop has no re-centring
 * and no row sums. The activation fragment is the MFMA's FIRST operand: lane l then holds, in register r, row
 * 4 (l / 16) + r of channel l % 16. So the sixteen lanes that share l / 16 write sixteen consecutive floats of one row --
 * whole 64-byte runs without any lane exchange -- a lane needs ONE channel entry per 16-column tile, and the four row
 * entries of a tile row are 32 consecutive bytes.
 *
 * The epilogue (qd8_finish in qd8_epilogue.hip.h, shared by both kernels and by qd8f32gemm4.hip), per output, in this
 * order, every float operation rounded once:
 *   acc += (128 - zp_r) * wsum[c]            the rows are centred on 128, the definition on zp_r
 *   s = scale_r * kernel_scale[c];  y = (float) acc * s;  y = y + bias[c];  y = min(max(y, output_min), output_max)
 * The file is compiled with contraction off (the pragma below): y * s + bias must not become one fused operation.
 *
 *   qd8_f32_gemm_mfma_128x128   rows > 16. 128 x 128 tiles, four waves of 64 x 64 = sixteen accumulator tiles each. Both
 *       operands reach LDS by 16-byte LDS-DMA, double-buffered over 64-byte K steps (2 x 16 KiB): the activation tile as
 *       [row][4 chunks] with q8gemm128x.hip's chunk swizzle (rows 8 .. 15 of sixteen keep chunk c in slot c ^ 3), the
 *       weight tile as the packed image's own 1-KiB fragments, which a lane reads back at lane * 16 -- no conflicts by
 *       construction. One barrier per K step. Rows past the batch and channel blocks past the image re-read valid ones
 *       and are never stored.
 *   qd8_f32_gemv_mfma_16        rows <= 16, the usual batch of a dynamic linear: the tile kernel would spend 7/8 of its
 *       rows on padding. One 512-thread workgroup per 16-channel block; its eight waves split K, eight 64-byte tiles per
 *       wave and pass. A wave streams its weight fragments straight from HBM into registers (the image is in fragment
 *       order: 1 KiB per load instruction, every byte read once across the grid) and brings the matching activation
 *       tiles into LDS in fragment order by LDS-DMA, once per workgroup. The eight partial accumulators meet in LDS,
 *       wave 0 adds them up in a fixed order (integers: exact) and runs the epilogue. No atomics, no second launch.
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

/* ---- 128 x 128 tiles ------------------------------------------------------------------------------------------------ */
constexpr int kBM = 128;
constexpr int kBN = 128;
constexpr int kBK = 64;
constexpr int kATile = kBM * kBK;             // 8 KiB
constexpr int kWTile = kBN * kBK;             // 8 KiB: eight fragments
constexpr int kStage = kATile + kWTile;
constexpr int kGemmThreads = 256;

__global__ __launch_bounds__(kGemmThreads, 2)
void qd8_f32_gemm_mfma_128x128_kernel(const Qd8Params p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kStage];

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t wm = wave >> 1, wn = wave & 1u;
  const uint32_t m_tile = blockIdx.x / p.tiles_n;
  const uint32_t n_tile = blockIdx.x - m_tile * p.tiles_n;
  const uint32_t ktiles = p.k_pad / kBK;
  const uint32_t nblocks = p.n_pad / 16;
  const uint32_t m0 = m_tile * kBM;
  const uint32_t last_row = p.rows - 1u - m0;            // of this tile, relative (m0 < rows)

  // activations: piece pc = wave * 128 + i * 64 + lane of the tile's 512 = (row pc >> 2, slot pc & 3), which holds the row's chunk
  // slot ^ swizzle(row). Lane offsets are relative to the tile's first row: below 128 * 32768.
  const uint8_t* a_tile = scalar_ptr(p.a + static_cast<uint64_t>(m0) * p.k_pad);
  uint32_t a_src[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const uint32_t pc = wave * 128u + i * 64u + lane;
    const uint32_t row = pc >> 2, slot = pc & 3u;
    a_src[i] = min(row, last_row) * p.k_pad + ((slot ^ a_swizzle(row)) << 4);
  }
  // weights: fragment f = wave * 2 + i of the tile's eight = channel block n_tile * 8 + f (past the image: the last block)
  const uint8_t* w_frag[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const uint32_t nb = min(n_tile * 8u + wave * 2u + i, nblocks - 1u);
    w_frag[i] = scalar_ptr(p.w + static_cast<uint64_t>(nb) * ktiles * 1024u);
  }
  auto stage = [&](uint32_t kt, uint32_t slot) __attribute__((always_inline)) {
    uint8_t* st = lds + slot * kStage;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      dma16_saddr(scalar_ptr(a_tile + kt * kBK), a_src[i], st + (wave * 2u + i) * 1024u);
      dma16_saddr(scalar_ptr(w_frag[i] + kt * 1024u), lane * 16u, st + kATile + (wave * 2u + i) * 1024u);
    }
  };

  const uint32_t frow = lane & 15u, fg = lane >> 4;
  const uint32_t a_off = (wm * 64u + frow) * kBK + ((fg ^ a_swizzle(frow)) << 4);       // + tm * 1024
  const uint32_t w_off = kATile + wn * 4096u + lane * 16u;                                // + tn * 1024
  v4i acc[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; tm++) {
#pragma unroll
    for (int tn = 0; tn < 4; tn++) acc[tm][tn] = v4i{0, 0, 0, 0};
  }

  stage(0u, 0u);
  for (uint32_t kt = 0; kt < ktiles; kt++) {
    const uint32_t slot = kt & 1u;
    // tile kt was requested a step ago and is all this wave has in flight; behind the barrier every wave's part has landed and
    // every wave is done reading the other stage
    wait_vmcnt<0>();
    __syncthreads();
    QNNP_PIN();
    if (kt + 1u < ktiles) stage(kt + 1u, slot ^ 1u);
    QNNP_PIN();
    const uint8_t* st = lds + slot * kStage;
    v4i fa[4], fw[4];
#pragma unroll
    for (int tm = 0; tm < 4; tm++) fa[tm] = *reinterpret_cast<const v4i*>(st + a_off + tm * 1024);
#pragma unroll
    for (int tn = 0; tn < 4; tn++) fw[tn] = *reinterpret_cast<const v4i*>(st + w_off + tn * 1024);
#pragma unroll
    for (int tm = 0; tm < 4; tm++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int tn = (tm & 1) != 0 ? 3 - j : j;                // snake: one operand changes per MFMA
        acc[tm][tn] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[tm], fw[tn], acc[tm][tn], 0, 0, 0);
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
    for (int tn = 0; tn < 4; tn++) qd8_store_tile(acc[tm][tn], row0, rows, c_base + tn * 16u, ch[tn], p);
  }
}

/* ---- rows <= 16 ------------------------------------------------------------------------------------------------------ */
constexpr int kGemvWaves = 8;
constexpr int kGemvThreads = kGemvWaves * 64;
constexpr int kGemvTiles = 8;                 // K tiles per wave and pass
constexpr int kGemvPass = kGemvWaves * kGemvTiles;   // 64 tiles = 4096 K positions = 64 KiB of LDS

__global__ __launch_bounds__(kGemvThreads)
void qd8_f32_gemv_mfma_16_kernel(const Qd8Params p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kGemvPass * 1024];

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nb = blockIdx.x;
  const uint32_t ktiles = p.k_pad / 64u;
  const uint32_t frow = lane & 15u, fg = lane >> 4;

  const v4i* w_block = reinterpret_cast<const v4i*>(p.w + static_cast<uint64_t>(nb) * ktiles * 1024u);
  const uint64_t a_base = scalar_ptr(reinterpret_cast<uint64_t>(p.a));
  const uint32_t a_lane = min(frow, p.rows - 1u) * p.k_pad + fg * 16u;      // rows past the batch re-read the last: never stored
  uint8_t* mine = lds + wave * (kGemvTiles * 1024);                           // this wave's tiles of a pass, fragment order
  const uint32_t mine_off = __builtin_amdgcn_readfirstlane(lds_offset(mine));

  v4i acc = v4i{0, 0, 0, 0};
  for (uint32_t kt0 = wave * kGemvTiles; kt0 < ktiles; kt0 += kGemvPass) {
    // tiles past K re-read the last one (fixed counts; their products are left out below)
    v4i fw[kGemvTiles];
#pragma unroll
    for (int t = 0; t < kGemvTiles; t++) {
      const uint32_t kt = min(kt0 + t, ktiles - 1u);
      fw[t] = w_block[static_cast<uint64_t>(kt) * 64u + lane];
      dma16_saddr_ordered(scalar_ptr(a_base + kt * 64u), a_lane, __builtin_amdgcn_readfirstlane(mine_off + t * 1024u));
    }
    wait_vmcnt<0>();       // the wave reads only what it brought in itself: no barrier
#pragma unroll
    for (int t = 0; t < kGemvTiles; t++) {
      const v4i fa = *reinterpret_cast<const v4i*>(mine + t * 1024 + lane * 16u);
      if (kt0 + t < ktiles) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fw[t], acc, 0, 0, 0);
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
  qd8_store_tile(sum, 0u, qd8_load_rows(0u, p), c, p.chan_tab[c], p);
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_qd8_gemm_run(const struct qnnp_hip_qd8_gemm_args* a, const char** kernel_name)
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
  p.w = reinterpret_cast<const uint8_t*>(a->packed_w);
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
    hipLaunchKernelGGL(qd8_f32_gemv_mfma_16_kernel, dim3(a->n_pad / 16u), dim3(kGemvThreads), 0, stream, p);
    if (kernel_name != nullptr) *kernel_name = "qd8_f32_gemv_mfma_16";
    return launch_status();
  }
  const uint64_t tiles = static_cast<uint64_t>((a->rows + kBM - 1u) / kBM) * p.tiles_n;
  if (tiles > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;          // a grid that would wrap is refused, not launched
  hipLaunchKernelGGL(qd8_f32_gemm_mfma_128x128_kernel, dim3(static_cast<uint32_t>(tiles)), dim3(kGemmThreads), 0, stream, p);
  if (kernel_name != nullptr) *kernel_name = "qd8_f32_gemm_mfma_128x128";
  return launch_status();
}
