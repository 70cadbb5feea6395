/*
 * f32qd8rmsnormrows.hip -- the first launch of the dynamically quantized fully connected operator after an RMSNORM setup
 * (dynamic-fully-connected.c; include/qnnpack_gfx950_dynamic.h has the definition): the row that is quantized is
 * h[k] = x[k] * r * gamma[k] with x = input + residual (or the input itself) and r = 1 / sqrt(mean(x^2) + epsilon). The sum
 * x, where there is a residual, goes out as the next layer's residual stream; h exists in registers only: it is never written
 * as floats. No reference counterpart. Float32, every operation rounded once: contraction is off for the file, and the
 * divisions and the square root are the IEEE ones (correctly rounded).
 *
 *   x = residual ? flush(flush(input) + flush(residual)) : input            flush(v): a signed zero for |v| < 2^-126
 *   sq = x * x, a zero if <= 2^-126;  the in-piece tree (+8, +4, +2, +1) gives one sum per piece of sixteen
 *   across pieces j = i * 256 + wave * 64 + lane the tree of the header, steps 512 .. 1:
 *       512, 256   a lane's own four pieces: (s0 + s2) + (s1 + s3)
 *       128, 64    the four waves' lane values through LDS: (w0 + w2) + (w1 + w3)
 *       32 .. 1    an xor butterfly inside the wave: v_permlane32_swap, then ds_swizzle 16, 8, 4, 2, 1
 *   Every sq is +0 or a positive normal number and v + (+0) is v in every bit, so pieces that do not exist add nothing and
 *   the tree over 1024 pieces is the tree over the pieces a kernel has. A butterfly leaves s[j] + s[j ^ h] in BOTH lanes:
 *   float addition is commutative in every bit but a NaN's payload, which no output shows.
 *   m = S / (float) K;  v = m + epsilon;  r = 1.0f / sqrtf(v)               every lane computes them from the same S
 *   t = x * r, h = t * gamma, each a signed zero if <= 2^-126 in magnitude
 * and from h on everything is f32qd8rows.hip's, through the helpers of f32qd8rows.hip.h: range, scale, zero point, the int8
 * row q - 128 in whole 16-byte stores with the pad up to k_pad zeroed, {scale, 128 - zp} into the row table.
 *
 * Two kernels; K <= 16384 (the setup refuses more: the row has to stay in registers between the sum and the scaling, which
 * is also what makes the in-place residual update safe -- a lane has read every element it is going to write):
 *   f32_qd8_rmsnorm_rows_wave    K <= 1024: one wave per row, four rows per workgroup, one piece per lane. All twelve (eight
 *                                without a residual) 16-byte loads of a lane are issued before the first add; between them
 *                                and the stores there are lane exchanges only, no LDS memory and no barrier.
 *   f32_qd8_rmsnorm_rows_block   K <= 16384: one workgroup per row, up to four pieces per lane kept as x. The 256 lane sums
 *                                meet in LDS once; after ONE barrier every wave reads all four waves' values for its lanes
 *                                and runs the same combine and butterfly, so all 256 lanes hold S in the same bits with no
 *                                broadcast and no second barrier. gamma's loads are issued in front of that exchange and are
 *                                first needed behind it: their latency lies under the barrier. The range reduction behind
 *                                it is block_range's, on LDS words of its own (a fast wave may already write its range while
 *                                a slow one still reads the sums). A lane skips every piece that begins at or past K:
 *                                at K = 2880, 180 of 256 lanes have one piece and nobody has a second.
 * The _x4 flavours (a base of input, residual, residual_out or gamma, or with more than one row a stride of those, no
 * multiple of 16 bytes) move dwords; so does the one piece of a row that K cuts, in both flavours. Nothing at or past K is
 * read or written in any float tensor. All stores are ordinary vector stores.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "f32qd8rows.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

struct NormRowsParams {
  const float* x;
  const float* residual;     // or nullptr (the RES = false kernels never look at it)
  float* residual_out;       // or nullptr; may be `residual` itself
  const float* gamma;
  int8_t* q;
  qnnp_hip_qd8_row_entry* table;
  uint64_t x_stride;         // elements
  uint64_t residual_stride;  // elements, of both residual tensors
  uint32_t rows, k, k_pad;
  float epsilon;
};

/* a signed zero for what is a denormal, or may be one in one denormal mode and not in the other */
__device__ __forceinline__ float flush_below(float v)      // exact values: sums of two floats, loaded elements
{
  return fabsf(v) < 0x1.0p-126f ? copysignf(0.0f, v) : v;
}
__device__ __forceinline__ float flush_through(float v)    // products: one that ROUNDS to 2^-126 is a zero in either mode
{
  return fabsf(v) <= 0x1.0p-126f ? copysignf(0.0f, v) : v;
}

/* the sixteen floats of a piece to elements e0 .. e0 + 15 of the row; nothing at or past K is written */
template <bool VEC>
__device__ __forceinline__ void store_floats(const Piece& p, float* row, uint32_t e0, uint32_t k)
{
  if (VEC && e0 + kPiece <= k) {
    f32x4* dst = reinterpret_cast<f32x4*>(row + e0);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      f32x4 t;
#pragma unroll
      for (int i = 0; i < 4; i++) t[i] = p.v[4 * j + i];
      dst[j] = t;
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPiece; i++) {
      if (e0 + i < k) row[e0 + i] = p.v[i];
    }
  }
}

/* x = input + residual, in place in `x`; elements from K on stay 0 + 0 = 0 */
__device__ __forceinline__ void add_residual(Piece& x, const Piece& residual)
{
#pragma unroll
  for (uint32_t i = 0; i < kPiece; i++) x.v[i] = flush_below(flush_below(x.v[i]) + flush_below(residual.v[i]));
}

/* the piece's sum of squares: the in-piece tree of the header */
__device__ __forceinline__ float piece_square_sum(const Piece& x)
{
  float u[kPiece];
#pragma unroll
  for (uint32_t i = 0; i < kPiece; i++) u[i] = flush_through(x.v[i] * x.v[i]);
#pragma unroll
  for (uint32_t step = kPiece / 2; step != 0; step /= 2) {
#pragma unroll
    for (uint32_t i = 0; i < step; i++) u[i] = u[i] + u[i + step];
  }
  return u[0];
}

/* steps 32, 16, 8, 4, 2, 1 of the tree over a wave's 64 pieces: every lane ends up with the sum, in the same bits */
__device__ __forceinline__ float wave_sum(float s)
{
  float low, high;
  both_halves(s, low, high);            // s of lane l % 32 and of lane l % 32 + 32, in every lane
  s = low + high;
  s = s + swizzle_xor<16>(s);
  s = s + swizzle_xor<8>(s);
  s = s + swizzle_xor<4>(s);
  s = s + swizzle_xor<2>(s);
  s = s + swizzle_xor<1>(s);
  return s;
}

/* r of the row from its sum of squares: two IEEE divisions and the correctly rounded square root */
__device__ __forceinline__ float row_rsqrt(float s, const NormRowsParams& p)
{
  const float m = s / static_cast<float>(p.k);     // K <= 16384: the conversion is exact
  const float v = m + p.epsilon;
  return 1.0f / sqrtf(v);
}

/* x becomes h, in place */
__device__ __forceinline__ void scale_piece(Piece& x, const Piece& gamma, float r)
{
#pragma unroll
  for (uint32_t i = 0; i < kPiece; i++) {
    const float t = flush_through(x.v[i] * r);
    x.v[i] = flush_through(t * gamma.v[i]);
  }
}

template <bool VEC, bool RES>
__global__ __launch_bounds__(kRowsThreads)
void f32_qd8_rmsnorm_rows_wave_kernel(const NormRowsParams p)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = static_cast<uint64_t>(blockIdx.x) * (kRowsThreads / 64) + (threadIdx.x >> 6);
  if (row >= p.rows) return;                                  // (wave-uniform; no barrier in this kernel)
  const uint32_t e0 = lane * kPiece;
  Piece x = load_piece<VEC>(p.x + row * p.x_stride, e0, p.k);          // lanes past K hold zeros and touch no memory
  Piece residual;
  if (RES) residual = load_piece<VEC>(p.residual + row * p.residual_stride, e0, p.k);
  const Piece gamma = load_piece<VEC>(p.gamma, e0, p.k);
  if (RES) {
    add_residual(x, residual);
    if (p.residual_out != nullptr && e0 < p.k) store_floats<VEC>(x, p.residual_out + row * p.residual_stride, e0, p.k);
  }
  const float r = row_rsqrt(wave_sum(piece_square_sum(x)), p);
  scale_piece(x, gamma, r);
  float lo = 0.0f, hi = 0.0f;
  piece_range(x, lo, hi);
  wave_range(lo, hi);
  const RowQuant rq = row_quant(lo, hi);
  if (e0 < p.k_pad) store_piece(x, p.q + row * p.k_pad, e0, p.k, rq);
  if (lane == 0) store_entry(p.table + row, rq);
}

template <bool VEC, bool RES>
__global__ __launch_bounds__(kRowsThreads)
void f32_qd8_rmsnorm_rows_block_kernel(const NormRowsParams p)
{
  __shared__ float sums[kRowsThreads];
  __shared__ float range[4][2];
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = blockIdx.x;
  const float* x_row = p.x + row * p.x_stride;
  Piece x[kBlockPieces], residual[kBlockPieces];
  float s[kBlockPieces];
  /* every load of input and residual first: a store to residual_out, which may be the residual itself, orders the loads
   * behind it, and a lane's four pieces must not become four round trips */
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    if (e0 < p.k) {
      x[i] = load_piece<VEC>(x_row, e0, p.k);
      if (RES) residual[i] = load_piece<VEC>(p.residual + row * p.residual_stride, e0, p.k);
    } else {
#pragma unroll
      for (uint32_t e = 0; e < kPiece; e++) x[i].v[e] = 0.0f;
    }
  }
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    s[i] = 0.0f;
    if (e0 < p.k) {
      if (RES) {
        add_residual(x[i], residual[i]);
        if (p.residual_out != nullptr) store_floats<VEC>(x[i], p.residual_out + row * p.residual_stride, e0, p.k);
      }
      s[i] = piece_square_sum(x[i]);
    }
  }
  /* issued here, first needed behind the barrier */
  Piece gamma[kBlockPieces];
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    if (e0 < p.k) gamma[i] = load_piece<VEC>(p.gamma, e0, p.k);
  }
  sums[threadIdx.x] = (s[0] + s[2]) + (s[1] + s[3]);                  // steps 512 and 256
  __syncthreads();
  const float total = wave_sum((sums[lane] + sums[128 + lane]) + (sums[64 + lane] + sums[192 + lane]));   // 128 and 64, then 32 .. 1
  const float r = row_rsqrt(total, p);
  float lo = 0.0f, hi = 0.0f;
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    if (e0 < p.k) {
      scale_piece(x[i], gamma[i], r);
      piece_range(x[i], lo, hi);
    }
  }
  wave_range(lo, hi);
  block_range(lo, hi, range);
  const RowQuant rq = row_quant(lo, hi);
  int8_t* q_row = p.q + row * p.k_pad;
#pragma unroll
  for (int i = 0; i < kBlockPieces; i++) {
    const uint32_t e0 = (i * kRowsThreads + threadIdx.x) * kPiece;
    if (e0 < p.k_pad) store_piece(x[i], q_row, e0, p.k, rq);
  }
  if (threadIdx.x == 0) store_entry(p.table + row, rq);
}

template <bool VEC, bool RES>
void launch_rmsnorm_rows(const NormRowsParams& p, hipStream_t stream)
{
  if (p.k <= kWaveMaxK) {
    hipLaunchKernelGGL((f32_qd8_rmsnorm_rows_wave_kernel<VEC, RES>), dim3((p.rows + 3u) / 4u), dim3(kRowsThreads), 0, stream, p);
  } else {
    hipLaunchKernelGGL((f32_qd8_rmsnorm_rows_block_kernel<VEC, RES>), dim3(p.rows), dim3(kRowsThreads), 0, stream, p);
  }
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_qd8_rmsnorm_rows_run(const struct qnnp_hip_qd8_rmsnorm_rows_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->quantized == nullptr || a->row_table == nullptr || a->gamma == nullptr ||
      (a->residual == nullptr && a->residual_out != nullptr) ||
      ((reinterpret_cast<uintptr_t>(a->input) | reinterpret_cast<uintptr_t>(a->gamma) | reinterpret_cast<uintptr_t>(a->residual) |
        reinterpret_cast<uintptr_t>(a->residual_out)) & 3u) != 0 ||
      (reinterpret_cast<uintptr_t>(a->quantized) & 15u) != 0 ||
      a->k == 0 || a->k > kBlockMaxK || a->k_pad != ((a->k + 63u) & ~63u) || a->rows > 0x7FFFFFFFu || a->input_stride < a->k ||
      (a->residual != nullptr && a->residual_stride < a->k)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  NormRowsParams p;
  p.x = a->input;
  p.residual = a->residual;
  p.residual_out = a->residual_out;
  p.gamma = a->gamma;
  p.q = a->quantized;
  p.table = a->row_table;
  p.x_stride = a->input_stride;
  p.residual_stride = a->residual_stride;
  p.rows = a->rows;
  p.k = a->k;
  p.k_pad = a->k_pad;
  p.epsilon = a->epsilon;
  const bool res = a->residual != nullptr;
  const uintptr_t bases = reinterpret_cast<uintptr_t>(a->input) | reinterpret_cast<uintptr_t>(a->gamma) |
      reinterpret_cast<uintptr_t>(a->residual) | reinterpret_cast<uintptr_t>(a->residual_out);
  const bool vec = (bases & 15u) == 0 && (a->rows == 1 || (a->input_stride % 4 == 0 && (!res || a->residual_stride % 4 == 0)));
  if (vec && res) launch_rmsnorm_rows<true, true>(p, stream);
  else if (vec) launch_rmsnorm_rows<true, false>(p, stream);
  else if (res) launch_rmsnorm_rows<false, true>(p, stream);
  else launch_rmsnorm_rows<false, false>(p, stream);
  if (kernel_name != nullptr) {
    *kernel_name = a->k <= kWaveMaxK ? (vec ? "f32_qd8_rmsnorm_rows_wave" : "f32_qd8_rmsnorm_rows_wave_x4")
                                     : (vec ? "f32_qd8_rmsnorm_rows_block" : "f32_qd8_rmsnorm_rows_block_x4");
  }
  return launch_status();
}
