/*
 * f32qd8rows.hip.h -- what the row kernels of the dynamically quantized fully connected operator share: f32qd8rows.hip (the
 * input row is x itself) and f32qd8gatedrows.hip (the input row holds gate and up values, x = act(gate) * up is computed in
 * registers) and f32qd8rmsnormrows.hip (x = rmsnorm(input + residual) * gamma, likewise). A lane's piece is SIXTEEN
 * consecutive elements of x; the load of a piece of floats, the range reduction, the row's scale and zero point, the
 * quantization of one element and the two stores are the same code in both units, so the quantized row and the row table
 * entry of a given x are the same bytes whichever unit produced them. include/qnnpack_gfx950_dynamic.h has the definition.
 * Float32, every operation rounded once: no multiply is followed by an add anywhere in here, so nothing can fuse.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

constexpr uint32_t kRowsThreads = 256;
constexpr uint32_t kPiece = 16;                                  // elements of a lane's piece
constexpr uint32_t kWaveMaxK = 64 * kPiece;                      // 1024
constexpr int kBlockPieces = 4;                                  // pieces a lane of the block kernel keeps in registers
constexpr uint32_t kBlockMaxK = kRowsThreads * kPiece * kBlockPieces;   // 16384

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Piece {
  float v[kPiece];
};

/* the piece at elements e0 .. e0 + 15 of the row; elements from K on read as 0, which neither end of the range sees */
template <bool VEC>
__device__ __forceinline__ Piece load_piece(const float* row, uint32_t e0, uint32_t k)
{
  Piece p;
  if (VEC && e0 + kPiece <= k) {
    const f32x4* src = reinterpret_cast<const f32x4*>(row + e0);
    const f32x4 a = src[0], b = src[1], c = src[2], d = src[3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      p.v[i] = a[i];
      p.v[4 + i] = b[i];
      p.v[8 + i] = c[i];
      p.v[12 + i] = d[i];
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kPiece; i++) p.v[i] = e0 + i < k ? row[e0 + i] : 0.0f;
  }
  return p;
}

__device__ __forceinline__ void piece_range(const Piece& p, float& lo, float& hi)
{
#pragma unroll
  for (uint32_t i = 0; i < kPiece; i++) {
    lo = fminf(lo, p.v[i]);
    hi = fmaxf(hi, p.v[i]);
  }
}

/* the xor butterfly over the 32 lanes of a half (ds_swizzle, bit mode: and 0x1F, or 0, xor X), then the other half */
template <int X>
__device__ __forceinline__ float swizzle_xor(float v)
{
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (X << 10) | 0x1F));
}
/* v of lanes 0 .. 31 in `low` and of lanes 32 .. 63 in `high`, in every lane (v is uniform within each half by now) */
__device__ __forceinline__ void both_halves(float v, float& low, float& high)
{
  const uint32_t bits = static_cast<uint32_t>(__float_as_int(v));
  const auto s = __builtin_amdgcn_permlane32_swap(bits, bits, false, false);
  low = __int_as_float(static_cast<int>(s[0]));
  high = __int_as_float(static_cast<int>(s[1]));
}
__device__ __forceinline__ void wave_range(float& lo, float& hi)
{
  float a, b;
  lo = fminf(lo, swizzle_xor<1>(lo));   hi = fmaxf(hi, swizzle_xor<1>(hi));
  lo = fminf(lo, swizzle_xor<2>(lo));   hi = fmaxf(hi, swizzle_xor<2>(hi));
  lo = fminf(lo, swizzle_xor<4>(lo));   hi = fmaxf(hi, swizzle_xor<4>(hi));
  lo = fminf(lo, swizzle_xor<8>(lo));   hi = fmaxf(hi, swizzle_xor<8>(hi));
  lo = fminf(lo, swizzle_xor<16>(lo));  hi = fmaxf(hi, swizzle_xor<16>(hi));
  both_halves(lo, a, b);
  lo = fminf(a, b);                     // (min and max are exact: the order of the operands changes no bit but the sign of a zero,
  both_halves(hi, a, b);                //  and here every lane uses the same order)
  hi = fmaxf(a, b);
}

/* the workgroup's range from the four waves' (all lanes of a wave hold the same pair), in the same order in every lane */
__device__ __forceinline__ void block_range(float& lo, float& hi, float (*lds)[2])
{
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    lds[wave][0] = lo;
    lds[wave][1] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(lds[0][0], lds[1][0]), fminf(lds[2][0], lds[3][0]));
  hi = fmaxf(fmaxf(lds[0][1], lds[1][1]), fmaxf(lds[2][1], lds[3][1]));
}

struct RowQuant {
  float scale, inv, t_lo, t_hi;
  int32_t zp;
};

__device__ __forceinline__ RowQuant row_quant(float lo, float hi)
{
  RowQuant r;
  float scale = (hi - lo) / 255.0f;
  if (!(scale >= 0x1.0p-60f && scale <= 0x1.0p+60f)) scale = 1.0f;
  r.scale = scale;
  r.inv = 1.0f / scale;
  r.zp = static_cast<int32_t>(rintf(fminf(-lo * r.inv, 255.0f)));   // -lo >= 0: in [0, 255]
  r.t_lo = static_cast<float>(-r.zp);
  r.t_hi = static_cast<float>(255 - r.zp);
  return r;
}

__device__ __forceinline__ uint32_t quantize_one(float x, const RowQuant& r)
{
  float t = x * r.inv;
  t = t != t ? 0.0f : t;
  t = fminf(fmaxf(t, r.t_lo), r.t_hi);
  return static_cast<uint32_t>(static_cast<int32_t>(rintf(t)) + r.zp) ^ 0x80u;   // q in [0, 255] -> q - 128 as a byte
}

/* the piece as sixteen int8 at q_row + e0 (e0 < k_pad); elements from K on are the pad: zero */
__device__ __forceinline__ void store_piece(const Piece& p, int8_t* q_row, uint32_t e0, uint32_t k, const RowQuant& r)
{
  u32x4 out;
#pragma unroll
  for (uint32_t d = 0; d < 4; d++) {
    uint32_t word = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
      const uint32_t e = e0 + 4 * d + b;
      const uint32_t byte = e < k ? quantize_one(p.v[4 * d + b], r) : 0u;
      word |= byte << (8 * b);
    }
    out[d] = word;
  }
  *reinterpret_cast<u32x4*>(q_row + e0) = out;
}

__device__ __forceinline__ void store_entry(qnnp_hip_qd8_row_entry* entry, const RowQuant& r)
{
  entry->scale = r.scale;
  entry->zero_offset = 128 - r.zp;
}

}  // namespace

}  // namespace qnnp
