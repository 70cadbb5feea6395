/*
 * f32q8.hip -- float32 -> uint8 (quantize) and uint8 -> float32 (dequantize), the two ends of a quantized network
 * (quantize.c, dequantize.c; include/qnnpack_gfx950_float.h). No reference counterpart. Float32, every operation rounded
 * once -- there is no multiply followed by an add anywhere, so nothing can fuse:
 *   quantize:    t = x * inv_scale;  t = isnan(t) ? 0 : t;  t = min(max(t, lo), hi);  y = (int) rintf(t) + zero_point
 *   dequantize:  y = (float) ((int) x - zero_point) * scale
 * HBM-bound by construction, 5 bytes per element: the kernels are about coalescing, and the float side is indexed with 64
 * bits (its byte offsets pass 4 GiB long before an element count passes 2^31).
 *
 * ROWS (f32q8_{quantize,dequantize}_x16 / _x4 / _x1), built like q8mul.hip: 256-thread workgroups, a lane's piece is 16, 4
 * or 1 elements OF ONE ROW, short rows share a workgroup (lane -> (row, piece) by one magic divide), rows longer than a
 * workgroup span gridDim.y workgroups, grid-stride loops capped by the compute-unit count. The 16-element piece is four
 * 16-byte float accesses and one 16-byte byte access. THE DISPATCH RULE: rows that are dense on both sides (both strides
 * == channels), or a single row, are ONE row of rows * channels elements; then the widest piece W of 16, 4, 1 is taken for
 * which the byte-side base -- and, with more than one row, the byte-side stride -- is a multiple of W, and for W = 16 also
 * the float base is a multiple of 16 bytes and, with more than one row, the float stride a multiple of 4 elements. The
 * channel count does not enter: the last piece of a row may be partial and then goes element by element. So a dense NHWC
 * float image of 3 or 21 channels takes the 16-element kernel.
 *
 * PLANAR (f32q8_{quantize,dequantize}_planar): float NCHW <-> byte NHWC, transposed through LDS so that both sides see
 * contiguous runs. A tile is up to 64 channels x 256 / 512 / 1024 pixels of one image (at most 16 KiB of bytes): on the
 * float side every channel of the tile is a contiguous run along p, one dword per lane; on the byte side the tile is whole
 * pixels. Where the byte tensor is dense and the tile holds every channel, the tile's bytes are ONE contiguous run: it is
 * kept in LDS at the run's own offset within 16 bytes, so it moves as aligned 16-byte pieces with a bytewise head and
 * tail, whatever the base alignment. Otherwise (a pixel stride above the channel count, or more than 64 channels) the
 * bytes of each pixel's run go one per lane, adjacent lanes adjacent bytes.
 *
 * The streaming hint goes on the stores; the output is never in place.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "row_map.hip.h"

namespace qnnp {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

/* quantize: mul = 1 / scale, lo / hi = the clamp less the zero point; dequantize: mul = scale */
struct F32Q8Math {
  float mul, lo, hi;
  int32_t zero_point;
};

__device__ __forceinline__ uint32_t quantize_one(float x, const F32Q8Math& m)
{
  float t = x * m.mul;
  t = t != t ? 0.0f : t;
  t = fminf(fmaxf(t, m.lo), m.hi);
  return static_cast<uint32_t>(static_cast<int32_t>(rintf(t)) + m.zero_point);   // |t| <= 255: in [0, 255]
}

__device__ __forceinline__ float dequantize_one(uint32_t x, const F32Q8Math& m)
{
  return static_cast<float>(static_cast<int32_t>(x) - m.zero_point) * m.mul;
}

__device__ __forceinline__ uint32_t quantize_x4(f32x4 v, const F32Q8Math& m)
{
  return quantize_one(v.x, m) | (quantize_one(v.y, m) << 8) | (quantize_one(v.z, m) << 16) | (quantize_one(v.w, m) << 24);
}

__device__ __forceinline__ f32x4 dequantize_x4(uint32_t x, const F32Q8Math& m)
{
  f32x4 v;
  v.x = dequantize_one(x & 0xFFu, m);
  v.y = dequantize_one((x >> 8) & 0xFFu, m);
  v.z = dequantize_one((x >> 16) & 0xFFu, m);
  v.w = dequantize_one(x >> 24, m);
  return v;
}

template <bool STREAM, typename T>
__device__ __forceinline__ void store(T value, T* to)
{
  if constexpr (STREAM) {
    __builtin_nontemporal_store(value, to);
  } else {
    *to = value;
  }
}

/* ---- rows ---------------------------------------------------------------------------------------------------------- */
struct RowsParams {
  float* f;                 // the float tensor (read by quantize, written by dequantize)
  uint8_t* q;               // the byte tensor (written by quantize, read by dequantize)
  uint64_t f_stride;        // elements between rows
  uint64_t q_stride;        // bytes between rows
  uint64_t row_len;         // elements of a row (rows * channels when the rows were joined)
  uint64_t pieces;          // ceil(row_len / VEC)
  uint32_t rows;            // < 2^31
  uint32_t pieces_inv;      // reciprocal_ceil(pieces) when pieces <= kThreads
  uint32_t rows_per_block;  // rows of one row group: kThreads / pieces, or 1 for rows longer than a workgroup
  uint32_t groups;          // ceil(rows / rows_per_block)
  F32Q8Math m;
};

/* one piece: `valid` (1 .. VEC) elements from pf / pq on; only the last piece of a row has valid < VEC */
template <bool QUANT, int VEC, bool STREAM>
__device__ __forceinline__ void rows_piece(float* pf, uint8_t* pq, uint32_t valid, const F32Q8Math& m)
{
  if (VEC > 1 && valid == static_cast<uint32_t>(VEC)) {
    if constexpr (VEC == 16 && QUANT) {
      const f32x4* v = reinterpret_cast<const f32x4*>(pf);
      const f32x4 a = v[0], b = v[1], c = v[2], d = v[3];
      u32x4 z;
      z.x = quantize_x4(a, m);
      z.y = quantize_x4(b, m);
      z.z = quantize_x4(c, m);
      z.w = quantize_x4(d, m);
      store<STREAM>(z, reinterpret_cast<u32x4*>(pq));
    } else if constexpr (VEC == 16) {
      const u32x4 x = *reinterpret_cast<const u32x4*>(pq);
      f32x4* v = reinterpret_cast<f32x4*>(pf);
      store<STREAM>(dequantize_x4(x.x, m), v);
      store<STREAM>(dequantize_x4(x.y, m), v + 1);
      store<STREAM>(dequantize_x4(x.z, m), v + 2);
      store<STREAM>(dequantize_x4(x.w, m), v + 3);
    } else if constexpr (VEC == 4 && QUANT) {
      f32x4 a;
      a.x = pf[0];
      a.y = pf[1];
      a.z = pf[2];
      a.w = pf[3];
      *reinterpret_cast<uint32_t*>(pq) = quantize_x4(a, m);
    } else if constexpr (VEC == 4) {
      const f32x4 a = dequantize_x4(*reinterpret_cast<const uint32_t*>(pq), m);
      pf[0] = a.x;
      pf[1] = a.y;
      pf[2] = a.z;
      pf[3] = a.w;
    }
    return;
  }
  for (uint32_t i = 0; i < valid; i++) {
    if constexpr (QUANT) {
      pq[i] = static_cast<uint8_t>(quantize_one(pf[i], m));
    } else {
      pf[i] = dequantize_one(pq[i], m);
    }
  }
}

/* grid x: row groups (grid-stride); grid y: the kThreads-piece chunks of a row longer than a workgroup (grid-stride) */
template <bool QUANT, int VEC, bool STREAM>
__global__ __launch_bounds__(kThreads)
void f32q8_rows_kernel(const RowsParams p)
{
  uint32_t rl = 0;
  uint64_t k0 = static_cast<uint64_t>(blockIdx.y) * kThreads + threadIdx.x;
  if (p.pieces <= static_cast<uint64_t>(kThreads)) {
    const uint32_t pieces = static_cast<uint32_t>(p.pieces);
    rl = div_magic(threadIdx.x, p.pieces_inv);
    k0 = threadIdx.x - rl * pieces;
    if (rl >= p.rows_per_block) return;
  }
  const uint64_t k_step = static_cast<uint64_t>(gridDim.y) * kThreads;
  for (uint32_t grp = blockIdx.x; grp < p.groups; grp += gridDim.x) {
    const uint32_t r = grp * p.rows_per_block + rl;         // < rows + kThreads: no wrap
    if (r >= p.rows) continue;                              // (the last group)
    float* pf = p.f + static_cast<uint64_t>(r) * p.f_stride;
    uint8_t* pq = p.q + static_cast<uint64_t>(r) * p.q_stride;
    for (uint64_t k = k0; k < p.pieces; k += k_step) {
      const uint64_t e = k * VEC;                           // < row_len
      const uint64_t left = p.row_len - e;
      rows_piece<QUANT, VEC, STREAM>(pf + e, pq + e, left < static_cast<uint64_t>(VEC) ? static_cast<uint32_t>(left) : VEC, p.m);
    }
  }
}

/* ---- planar -------------------------------------------------------------------------------------------------------- */
constexpr uint32_t kTileBytes = 16384;    // bytes of one tile: tile_p * tile_c at most
constexpr uint32_t kTileChannels = 64;
constexpr int kPixelsPerLane = 4;         // tile_p <= kPixelsPerLane * kThreads

struct PlanarParams {
  float* f;                 // dense NCHW
  uint8_t* q;               // NHWC, q_stride bytes between pixels
  uint64_t q_stride;
  uint64_t tiles;           // batch * ptiles * ctiles
  uint32_t pixels, channels;
  uint32_t tile_p;          // pixels of a tile: 256, 512 or 1024
  uint32_t tile_c;          // channels of a tile: min(channels, kTileChannels)
  uint32_t ptiles, ctiles;
  uint32_t tile_c_inv;      // reciprocal_ceil(tile_c)
  uint32_t last_c_inv;      // reciprocal_ceil(channels of the last channel tile)
  uint32_t linear;          // 1: one channel tile and q_stride == channels -- a tile's bytes are one contiguous run
  F32Q8Math m;
};

struct Tile {
  uint32_t n, c0, ct, p0, np;
};

/* tile t -> image, channel range, pixel range; all wave-uniform */
__device__ __forceinline__ Tile tile_of(uint64_t t, const PlanarParams& p)
{
  uint32_t ci, pi, n;
  if ((t >> 32) == 0) {
    const uint32_t t32 = static_cast<uint32_t>(t), t2 = t32 / p.ctiles;
    ci = t32 - t2 * p.ctiles;
    n = t2 / p.ptiles;
    pi = t2 - n * p.ptiles;
  } else {
    const uint64_t t2 = t / p.ctiles;
    ci = static_cast<uint32_t>(t - t2 * p.ctiles);
    n = static_cast<uint32_t>(t2 / p.ptiles);
    pi = static_cast<uint32_t>(t2 - static_cast<uint64_t>(n) * p.ptiles);
  }
  Tile tile;
  tile.n = n;
  tile.c0 = ci * p.tile_c;
  tile.ct = p.channels - tile.c0 < p.tile_c ? p.channels - tile.c0 : p.tile_c;
  tile.p0 = pi * p.tile_p;
  tile.np = p.pixels - tile.p0 < p.tile_p ? p.pixels - tile.p0 : p.tile_p;
  return tile;
}

/* The tile's bytes between LDS (`lds` + shift .. + shift + bytes, pixel-major: byte px * ct + c) and the byte tensor
 * (`g`: the tile's first byte). TO_GLOBAL: LDS -> global, else global -> LDS. Linear tiles: shift is g's offset within 16
 * bytes, so LDS offset lo and global address (g - shift) + lo are 16-byte aligned together. */
template <bool TO_GLOBAL, bool STREAM>
__device__ __forceinline__ void move_tile_bytes(uint8_t* lds, uint8_t* g, uint32_t shift, const Tile& t, const PlanarParams& p)
{
  const uint32_t bytes = t.np * t.ct;
  if (p.linear) {
    const uint32_t end = shift + bytes;
    uint8_t* base = g - shift;
    for (uint32_t lo = threadIdx.x * 16u; lo < end; lo += kThreads * 16u) {
      if (lo >= shift && lo + 16u <= end) {
        if constexpr (TO_GLOBAL) {
          store<STREAM>(*reinterpret_cast<const u32x4*>(lds + lo), reinterpret_cast<u32x4*>(base + lo));
        } else {
          *reinterpret_cast<u32x4*>(lds + lo) = *reinterpret_cast<const u32x4*>(base + lo);
        }
      } else {
        const uint32_t from = lo < shift ? shift : lo, to = lo + 16u < end ? lo + 16u : end;
        for (uint32_t i = from; i < to; i++) {
          if constexpr (TO_GLOBAL) {
            store<STREAM>(lds[i], base + i);
          } else {
            lds[i] = base[i];
          }
        }
      }
    }
  } else {
    const uint32_t ct_inv = t.ct == p.tile_c ? p.tile_c_inv : p.last_c_inv;
    for (uint32_t i = threadIdx.x; i < bytes; i += kThreads) {
      const uint32_t px = div_magic(i, ct_inv);             // i < 2^14, ct <= 64
      uint8_t* at = g + static_cast<uint64_t>(px) * p.q_stride + (i - px * t.ct);
      if constexpr (TO_GLOBAL) {
        store<STREAM>(lds[i], at);
      } else {
        lds[i] = *at;
      }
    }
  }
}

template <bool STREAM>
__global__ __launch_bounds__(kThreads)
void f32q8_quantize_planar_kernel(const PlanarParams p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kTileBytes + 16];
  for (uint64_t ti = blockIdx.x; ti < p.tiles; ti += gridDim.x) {
    const Tile t = tile_of(ti, p);
    uint8_t* out = p.q + (static_cast<uint64_t>(t.n) * p.pixels + t.p0) * p.q_stride + t.c0;
    const uint32_t shift = p.linear ? static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) & 15u) : 0u;
    const float* in = p.f + (static_cast<uint64_t>(t.n) * p.channels + t.c0) * p.pixels + t.p0;
    for (uint32_t c = 0; c < t.ct; c++) {
      const float* row = in + static_cast<uint64_t>(c) * p.pixels;
      float v[kPixelsPerLane];
#pragma unroll
      for (int j = 0; j < kPixelsPerLane; j++) {
        const uint32_t px = threadIdx.x + j * kThreads;
        v[j] = px < t.np ? row[px] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < kPixelsPerLane; j++) {
        const uint32_t px = threadIdx.x + j * kThreads;
        if (px < t.np) lds[shift + px * t.ct + c] = static_cast<uint8_t>(quantize_one(v[j], p.m));
      }
    }
    __syncthreads();
    move_tile_bytes<true, STREAM>(lds, out, shift, t, p);
    __syncthreads();   // the next tile overwrites the LDS image
  }
}

template <bool STREAM>
__global__ __launch_bounds__(kThreads)
void f32q8_dequantize_planar_kernel(const PlanarParams p)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kTileBytes + 16];
  for (uint64_t ti = blockIdx.x; ti < p.tiles; ti += gridDim.x) {
    const Tile t = tile_of(ti, p);
    uint8_t* in = p.q + (static_cast<uint64_t>(t.n) * p.pixels + t.p0) * p.q_stride + t.c0;
    const uint32_t shift = p.linear ? static_cast<uint32_t>(reinterpret_cast<uintptr_t>(in) & 15u) : 0u;
    float* out = p.f + (static_cast<uint64_t>(t.n) * p.channels + t.c0) * p.pixels + t.p0;
    move_tile_bytes<false, false>(lds, in, shift, t, p);
    __syncthreads();
    for (uint32_t c = 0; c < t.ct; c++) {
      float* row = out + static_cast<uint64_t>(c) * p.pixels;
#pragma unroll
      for (int j = 0; j < kPixelsPerLane; j++) {
        const uint32_t px = threadIdx.x + j * kThreads;
        if (px < t.np) store<STREAM>(dequantize_one(lds[shift + px * t.ct + c], p.m), row + px);
      }
    }
    __syncthreads();   // the next tile overwrites the LDS image
  }
}

/* ---- launch -------------------------------------------------------------------------------------------------------- */
bool streaming_hint(uint32_t streaming_mode)
{
  return streaming_mode == 0 ? qnnp_hip_streaming_stores() != 0 : streaming_mode == 2;
}

/* 16, 4 or 1: the dispatch rule of the header comment; joins dense rows (rows and row_len are updated) */
uint32_t rows_piece_width(const void* f, const void* q, uint32_t& rows, uint64_t& row_len, uint64_t f_stride, uint64_t q_stride)
{
  if (rows == 1 || (f_stride == row_len && q_stride == row_len)) {
    row_len *= rows;
    rows = 1;
  }
  const bool many = rows > 1;
  if (aligned(address(q), 16) && aligned(address(f), 16) && (!many || (aligned(q_stride, 16) && aligned(f_stride, 4)))) return 16;
  if (aligned(address(q), 4) && (!many || aligned(q_stride, 4))) return 4;
  return 1;
}

template <bool QUANT>
int rows_run(float* f, uint8_t* q, uint32_t rows, uint32_t channels, uint64_t f_stride, uint64_t q_stride,
             const F32Q8Math& m, uint32_t streaming_mode, const char** kernel_name)
{
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  RowsParams p;
  p.f = f;
  p.q = q;
  p.f_stride = f_stride;
  p.q_stride = q_stride;
  p.row_len = channels;
  p.rows = rows;
  const uint32_t vec = rows_piece_width(f, q, p.rows, p.row_len, f_stride, q_stride);
  p.pieces = (p.row_len + vec - 1) / vec;
  const bool shared = p.pieces <= static_cast<uint64_t>(kThreads);
  p.pieces_inv = shared ? reciprocal_ceil(static_cast<uint32_t>(p.pieces)) : 0u;
  p.rows_per_block = shared ? kThreads / static_cast<uint32_t>(p.pieces) : 1u;
  p.groups = static_cast<uint32_t>((static_cast<uint64_t>(p.rows) + p.rows_per_block - 1) / p.rows_per_block);
  p.m = m;

  // beyond the cap the grid-stride loops take further passes
  const uint64_t cap = active_cu_count() * 16u;
  const uint64_t chunks = shared ? 1u : (p.pieces + kThreads - 1) / kThreads;
  uint64_t gy = chunks < cap ? chunks : cap;
  if (gy > kMaxGridY) gy = kMaxGridY;
  const uint64_t cap_x = cap / gy > 0 ? cap / gy : 1u;
  const dim3 grid(static_cast<uint32_t>(p.groups < cap_x ? p.groups : cap_x), static_cast<uint32_t>(gy));

  const char* name = nullptr;
  if (vec == 16) {
    if (streaming_hint(streaming_mode)) {
      hipLaunchKernelGGL((f32q8_rows_kernel<QUANT, 16, true>), grid, dim3(kThreads), 0, stream, p);
    } else {
      hipLaunchKernelGGL((f32q8_rows_kernel<QUANT, 16, false>), grid, dim3(kThreads), 0, stream, p);
    }
    name = QUANT ? "f32q8_quantize_x16" : "f32q8_dequantize_x16";
  } else if (vec == 4) {
    hipLaunchKernelGGL((f32q8_rows_kernel<QUANT, 4, false>), grid, dim3(kThreads), 0, stream, p);
    name = QUANT ? "f32q8_quantize_x4" : "f32q8_dequantize_x4";
  } else {
    hipLaunchKernelGGL((f32q8_rows_kernel<QUANT, 1, false>), grid, dim3(kThreads), 0, stream, p);
    name = QUANT ? "f32q8_quantize_x1" : "f32q8_dequantize_x1";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}

template <bool QUANT>
int planar_run(float* f, uint8_t* q, uint32_t batch, uint32_t pixels, uint32_t channels, uint64_t q_stride,
               const F32Q8Math& m, uint32_t streaming_mode, const char** kernel_name)
{
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  PlanarParams p;
  p.f = f;
  p.q = q;
  p.q_stride = q_stride;
  p.pixels = pixels;
  p.channels = channels;
  p.tile_c = channels < kTileChannels ? channels : kTileChannels;
  p.tile_p = p.tile_c <= 16u ? 1024u : (p.tile_c <= 32u ? 512u : 256u);   // tile_p * tile_c <= kTileBytes
  p.ptiles = (pixels + p.tile_p - 1) / p.tile_p;
  p.ctiles = (channels + p.tile_c - 1) / p.tile_c;
  p.tiles = static_cast<uint64_t>(batch) * p.ptiles * p.ctiles;   // < 2^31 * 2^25
  p.tile_c_inv = reciprocal_ceil(p.tile_c);
  p.last_c_inv = reciprocal_ceil(channels - (p.ctiles - 1) * p.tile_c);
  p.linear = p.ctiles == 1 && q_stride == channels ? 1u : 0u;
  p.m = m;

  const uint64_t cap = active_cu_count() * 16u;
  const dim3 grid(static_cast<uint32_t>(p.tiles < cap ? p.tiles : cap));
  const bool hint = streaming_hint(streaming_mode);
  if (QUANT) {
    if (hint) {
      hipLaunchKernelGGL((f32q8_quantize_planar_kernel<true>), grid, dim3(kThreads), 0, stream, p);
    } else {
      hipLaunchKernelGGL((f32q8_quantize_planar_kernel<false>), grid, dim3(kThreads), 0, stream, p);
    }
  } else {
    if (hint) {
      hipLaunchKernelGGL((f32q8_dequantize_planar_kernel<true>), grid, dim3(kThreads), 0, stream, p);
    } else {
      hipLaunchKernelGGL((f32q8_dequantize_planar_kernel<false>), grid, dim3(kThreads), 0, stream, p);
    }
  }
  if (kernel_name != nullptr) *kernel_name = QUANT ? "f32q8_quantize_planar" : "f32q8_dequantize_planar";
  return launch_status();
}

/* what the kernels' index arithmetic relies on (the setups check the same) */
bool shape_ok(const void* f, const void* q, uint32_t planar, uint32_t rows, uint32_t pixels, uint32_t channels,
              uint64_t f_stride, uint64_t q_stride)
{
  if (f == nullptr || q == nullptr || !aligned(address(f), 4) || channels == 0 || channels > 0x7FFFFFFFu ||
      rows > 0x7FFFFFFFu || q_stride < channels) {
    return false;
  }
  if (planar != 0) {
    return pixels != 0 && static_cast<uint64_t>(rows) * pixels <= 0x7FFFFFFFu &&
        static_cast<uint64_t>(channels) * pixels <= 0x7FFFFFFFu;
  }
  return f_stride >= channels;
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_quantize_run(const struct qnnp_hip_quantize_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || !shape_ok(a->input, a->output, a->planar, a->rows, a->pixels, a->channels, a->input_stride, a->output_stride)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  const F32Q8Math m = {a->inv_scale, a->clamp_lo, a->clamp_hi, a->zero_point};
  float* f = const_cast<float*>(a->input);
  if (a->planar != 0) {
    return planar_run<true>(f, a->output, a->rows, a->pixels, a->channels, a->output_stride, m, a->streaming_mode, kernel_name);
  }
  return rows_run<true>(f, a->output, a->rows, a->channels, a->input_stride, a->output_stride, m, a->streaming_mode, kernel_name);
}

extern "C" int qnnp_hip_dequantize_run(const struct qnnp_hip_dequantize_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || !shape_ok(a->output, a->input, a->planar, a->rows, a->pixels, a->channels, a->output_stride, a->input_stride)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  const F32Q8Math m = {a->scale, 0.0f, 0.0f, a->zero_point};
  uint8_t* q = const_cast<uint8_t*>(a->input);
  if (a->planar != 0) {
    return planar_run<false>(a->output, q, a->rows, a->pixels, a->channels, a->input_stride, m, a->streaming_mode, kernel_name);
  }
  return rows_run<false>(a->output, q, a->rows, a->channels, a->output_stride, a->input_stride, m, a->streaming_mode, kernel_name);
}
