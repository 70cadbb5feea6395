/*
 * x8shuffle.hip -- channel shuffle (x8) and clamp (u8), NC layout with pixel strides.
 *
 * channel shuffle  replaces x8zip_x{2,3,4,m}__sse2 (reference src/x8zip/) and the channel-shuffle case of
 *                  qnnp_run_operator (src/operator-run.c:1109-1147): y[c * G + g] = x[g * gc + c] for every pixel.
 * clamp            replaces u8clamp_ukernel__sse2 (reference src/u8clamp/sse2.c) and the clamp case
 *                  (src/operator-run.c:1054-1089): y = min(max(x, output_min), output_max) for every byte.
 *
 * Both move bytes and are bound by HBM bandwidth. Several lanes serve one pixel row when it is short, several
 * workgroups when it is long (RowMap, row_map.hip.h): a lane's row and item come from one magic-reciprocal divide of
 * its thread index, no per-element division.
 *
 * Channel shuffle, three kernels:
 *   register  G = 2 or 4, gc % 4 == 0, base pointers and strides multiples of 4 bytes (16 for the x16 flavour, which
 *             also needs gc % 16 == 0). A lane loads the same dword (dwordx4) of each of the G groups and transposes
 *             the G x 4 bytes with v_perm_b32 (2 per dword for G = 2, a 4x4 transpose of 8 for G = 4); it stores G
 *             contiguous dwords (dwordx4). No LDS.
 *   lds       any G, gc and alignment, G * gc <= 32768. A workgroup stages whole input rows in LDS with aligned 16-byte
 *             loads (the chunk holding a row's first byte starts up to 15 bytes before it: an aligned 16-byte chunk
 *             never crosses a page, so the extra bytes are readable and are not used), then builds each output dword
 *             from four LDS bytes. Whole dwords inside the output row are stored as dwords, the partial ones at the
 *             row's ends byte by byte, so the bytes between strided pixels are never written.
 *   gather    G * gc > 32768 (a row no longer fits the LDS tile): one output byte per lane, read from global memory.
 * Clamp: the bytewise clamp of u8_bytewise.hip.h on dwords. Contiguous tensors (strides == channels) are one flat
 * range; otherwise each row is walked on its own. Pieces are 16, 4 or 1 bytes, the largest size that divides both the
 * distance between input and output and the difference of their strides, so input and output pieces are aligned
 * alike; partial pieces at the ends of a range are stored byte by byte. In place (input == output, equal strides) a lane
 * reads and writes only its own piece.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "row_map.hip.h"
#include "u8_bytewise.hip.h"

namespace qnnp {

namespace {

constexpr uint32_t kLdsTile = 4096;             // bytes of staged input rows per workgroup (more rows when they fit)
constexpr uint32_t kLdsMaxChannels = 32768;     // longest row the lds kernel stages (pitch <= 32784 bytes)
constexpr int kLoadsInFlight = 4;               // lds kernel: staging loads per lane before it waits (four fetches)
constexpr uint32_t kTilesPerCu = 8;             // lds kernel: smaller tiles until there are this many per CU

/* ---- channel shuffle ----------------------------------------------------------------------------------------- */

/* the G dwords of output channels [4c * G, 4c * G + 4G) from dword c of each group: v[g] = x[g * gc + 4c .. + 3] */
template <int G>
__device__ __forceinline__ void zip(const uint32_t (&v)[G], uint32_t (&o)[G])
{
  if constexpr (G == 2) {
    o[0] = __builtin_amdgcn_perm(v[1], v[0], 0x05010400u);   // a0 b0 a1 b1
    o[1] = __builtin_amdgcn_perm(v[1], v[0], 0x07030602u);   // a2 b2 a3 b3
  } else {
    const uint32_t t0 = __builtin_amdgcn_perm(v[1], v[0], 0x05010400u);   // a0 b0 a1 b1
    const uint32_t t1 = __builtin_amdgcn_perm(v[1], v[0], 0x07030602u);   // a2 b2 a3 b3
    const uint32_t u0 = __builtin_amdgcn_perm(v[3], v[2], 0x05010400u);   // c0 d0 c1 d1
    const uint32_t u1 = __builtin_amdgcn_perm(v[3], v[2], 0x07030602u);   // c2 d2 c3 d3
    o[0] = __builtin_amdgcn_perm(u0, t0, 0x05040100u);                    // a0 b0 c0 d0
    o[1] = __builtin_amdgcn_perm(u0, t0, 0x07060302u);                    // a1 b1 c1 d1
    o[2] = __builtin_amdgcn_perm(u1, t1, 0x05040100u);                    // a2 b2 c2 d2
    o[3] = __builtin_amdgcn_perm(u1, t1, 0x07060302u);                    // a3 b3 c3 d3
  }
}

/* register path: item k of a row = bytes [k * VEC, k * VEC + VEC) of every group */
template <int G, int VEC>
__global__ __launch_bounds__(kThreads)
void x8_shuffle_reg_kernel(const qnnp_hip_x8_args p, const RowMap m)
{
  uint32_t rl, k;
  if (!row_item(m, rl, k)) return;
  const uint32_t c = k * VEC;
  for (uint32_t grp = blockIdx.y; grp < m.groups; grp += gridDim.y) {
    const uint32_t r = grp * m.rows_per_block + rl;
    if (r >= m.rows) break;
    const uint8_t* x = p.input + static_cast<uint64_t>(r) * p.input_stride + c;
    uint8_t* y = p.output + static_cast<uint64_t>(r) * p.output_stride + static_cast<uint64_t>(c) * G;
    if constexpr (VEC == 4) {
      uint32_t v[G], o[G];
#pragma unroll
      for (int g = 0; g < G; g++) v[g] = *reinterpret_cast<const uint32_t*>(x + static_cast<uint64_t>(g) * p.group_channels);
      zip<G>(v, o);
#pragma unroll
      for (int g = 0; g < G; g++) reinterpret_cast<uint32_t*>(y)[g] = o[g];
    } else {
      uint4 q[G];
#pragma unroll
      for (int g = 0; g < G; g++) q[g] = *reinterpret_cast<const uint4*>(x + static_cast<uint64_t>(g) * p.group_channels);
      uint32_t o[4][G];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        uint32_t v[G];
#pragma unroll
        for (int g = 0; g < G; g++) v[g] = i == 0 ? q[g].x : i == 1 ? q[g].y : i == 2 ? q[g].z : q[g].w;
        zip<G>(v, o[i]);
      }
      uint4* y4 = reinterpret_cast<uint4*>(y);
      if constexpr (G == 2) {
        y4[0] = make_uint4(o[0][0], o[0][1], o[1][0], o[1][1]);
        y4[1] = make_uint4(o[2][0], o[2][1], o[3][0], o[3][1]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) y4[i] = make_uint4(o[i][0], o[i][1], o[i][2], o[i][3]);
      }
    }
  }
}

struct LdsPlan {
  uint32_t rows_per_tile;
  uint32_t pitch;           // bytes of LDS per staged row (16 * in_chunks)
  uint32_t in_chunks, in_inv;
  uint32_t out_dwords, out_inv;
  uint32_t groups_inv;
  uint32_t tiles;
};

__global__ __launch_bounds__(kThreads)
void x8_shuffle_lds_kernel(const qnnp_hip_x8_args p, const LdsPlan q)
{
  extern __shared__ uint4 lds[];
  const uint8_t* lds8 = reinterpret_cast<const uint8_t*>(lds);
  const uint32_t C = p.channels;
  for (uint32_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const uint32_t p0 = tile * q.rows_per_tile;
    const uint32_t rows = min(q.rows_per_tile, p.pixels - p0);
    // stage: the aligned 16-byte chunks holding each input row, kLoadsInFlight loads issued before the first LDS write
    const uint32_t chunks = rows * q.in_chunks;
    // a chunk every lane may read: the tile's first one (lanes without a chunk of their own load it and drop it)
    const uintptr_t first = reinterpret_cast<uintptr_t>(p.input + static_cast<uint64_t>(p0) * p.input_stride) &
        ~static_cast<uintptr_t>(15);
    const auto fetch = [&](uint32_t i, uint4& v, uint32_t& slot) {
      const uint32_t rl = div_magic(i, q.in_inv);
      const uint32_t k = i - rl * q.in_chunks;
      const uintptr_t row = reinterpret_cast<uintptr_t>(p.input + static_cast<uint64_t>(p0 + rl) * p.input_stride);
      const uintptr_t a = (row & ~static_cast<uintptr_t>(15)) + 16u * k;
      const bool mine = i < chunks && a < row + C;
      slot = mine ? rl * (q.pitch / 16u) + k : ~0u;
      v = *reinterpret_cast<const uint4*>(mine ? a : first);
    };
    for (uint32_t i0 = threadIdx.x; i0 < chunks; i0 += kLoadsInFlight * kThreads) {
      uint4 v0, v1, v2, v3;
      uint32_t s0, s1, s2, s3;
      fetch(i0, v0, s0);
      fetch(i0 + kThreads, v1, s1);
      fetch(i0 + 2 * kThreads, v2, s2);
      fetch(i0 + 3 * kThreads, v3, s3);
      if (s0 != ~0u) lds[s0] = v0;
      if (s1 != ~0u) lds[s1] = v1;
      if (s2 != ~0u) lds[s2] = v2;
      if (s3 != ~0u) lds[s3] = v3;
    }
    __syncthreads();
    // output dwords: byte o of a row is input channel (o % G) * gc + o / G
    for (uint32_t i = threadIdx.x; i < rows * q.out_dwords; i += kThreads) {
      const uint32_t rl = div_magic(i, q.out_inv);
      const uint32_t k = i - rl * q.out_dwords;
      const uintptr_t irow = reinterpret_cast<uintptr_t>(p.input + static_cast<uint64_t>(p0 + rl) * p.input_stride);
      const uint8_t* src = lds8 + rl * q.pitch + (irow & 15u);
      const uintptr_t orow = reinterpret_cast<uintptr_t>(p.output + static_cast<uint64_t>(p0 + rl) * p.output_stride);
      const uintptr_t a = (orow & ~static_cast<uintptr_t>(3)) + 4u * k;
      const int32_t o0 = static_cast<int32_t>(static_cast<intptr_t>(a - orow));   // -3 .. C + 3
      if (o0 >= static_cast<int32_t>(C)) continue;
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int32_t o = o0 + b;
        if (o >= 0 && o < static_cast<int32_t>(C)) {
          const uint32_t cc = div_magic(static_cast<uint32_t>(o), q.groups_inv);
          const uint32_t g = static_cast<uint32_t>(o) - cc * p.groups;
          w |= static_cast<uint32_t>(src[g * p.group_channels + cc]) << (8 * b);
        }
      }
      if (o0 >= 0 && o0 + 4 <= static_cast<int32_t>(C)) {
        *reinterpret_cast<uint32_t*>(a) = w;
      } else {
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const int32_t o = o0 + b;
          if (o >= 0 && o < static_cast<int32_t>(C)) reinterpret_cast<uint8_t*>(a)[b] = static_cast<uint8_t>(w >> (8 * b));
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads)
void x8_shuffle_gather_kernel(const qnnp_hip_x8_args p, const RowMap m)
{
  uint32_t rl, o;
  if (!row_item(m, rl, o)) return;
  const uint32_t cc = o / p.groups;
  const uint32_t g = o - cc * p.groups;
  const uint64_t src = static_cast<uint64_t>(g) * p.group_channels + cc;
  for (uint32_t grp = blockIdx.y; grp < m.groups; grp += gridDim.y) {
    const uint32_t r = grp * m.rows_per_block + rl;
    if (r >= m.rows) break;
    p.output[static_cast<uint64_t>(r) * p.output_stride + o] = p.input[static_cast<uint64_t>(r) * p.input_stride + src];
  }
}

/* ---- clamp --------------------------------------------------------------------------------------------------- */

/* the VEC-byte piece of output at address a (VEC-aligned) from the input piece at in_a; only bytes in [lo, hi) are
 * stored */
template <int VEC>
__device__ __forceinline__ void clamp_piece(uintptr_t a, uintptr_t in_a, uintptr_t lo, uintptr_t hi, uint32_t qmin,
                                            uint32_t qmax, uint32_t clamp_hi, uint32_t clamp_lo)
{
  if constexpr (VEC == 1) {
    const uint32_t x = *reinterpret_cast<const uint8_t*>(in_a);
    *reinterpret_cast<uint8_t*>(a) = static_cast<uint8_t>(min(max(x, qmin), qmax));
  } else {
    constexpr int D = VEC / 4;
    uint32_t v[D];
    if constexpr (VEC == 16) {
      const uint4 x = *reinterpret_cast<const uint4*>(in_a);
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
      v[0] = *reinterpret_cast<const uint32_t*>(in_a);
    }
#pragma unroll
    for (int i = 0; i < D; i++) v[i] = clamp_u8x4(v[i], clamp_hi, clamp_lo);
    if (a >= lo && a + VEC <= hi) {
      if constexpr (VEC == 16) {
        *reinterpret_cast<uint4*>(a) = make_uint4(v[0], v[1], v[2], v[3]);
      } else {
        *reinterpret_cast<uint32_t*>(a) = v[0];
      }
    } else {
#pragma unroll
      for (int b = 0; b < VEC; b++) {
        if (a + b >= lo && a + b < hi) reinterpret_cast<uint8_t*>(a)[b] = static_cast<uint8_t>(v[b / 4] >> (8 * (b % 4)));
      }
    }
  }
}

/* contiguous tensors: the bytes [output, output + bytes) in VEC-aligned pieces, grid-stride */
template <int VEC>
__global__ __launch_bounds__(kThreads)
void u8_clamp_flat_kernel(const qnnp_hip_x8_args p, const uint64_t bytes, const uint64_t pieces)
{
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p.output);
  const uintptr_t delta = reinterpret_cast<uintptr_t>(p.input) - lo;      // a multiple of VEC (mod 2^64)
  const uintptr_t base = lo & ~static_cast<uintptr_t>(VEC - 1);
  const uint32_t clamp_hi = clamp_hi_bound(p.output_max), clamp_lo = clamp_lo_bound(p.output_min);
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < pieces; i += step) {
    const uintptr_t a = base + i * VEC;
    clamp_piece<VEC>(a, a + delta, lo, lo + bytes, p.output_min, p.output_max, clamp_hi, clamp_lo);
  }
}

/* strided tensors: item k of a row = the k-th VEC-aligned piece touching the output row */
template <int VEC>
__global__ __launch_bounds__(kThreads)
void u8_clamp_rows_kernel(const qnnp_hip_x8_args p, const RowMap m)
{
  uint32_t rl, k;
  if (!row_item(m, rl, k)) return;
  const uint32_t clamp_hi = clamp_hi_bound(p.output_max), clamp_lo = clamp_lo_bound(p.output_min);
  for (uint32_t grp = blockIdx.y; grp < m.groups; grp += gridDim.y) {
    const uint32_t r = grp * m.rows_per_block + rl;
    if (r >= m.rows) break;
    const uintptr_t orow = reinterpret_cast<uintptr_t>(p.output + static_cast<uint64_t>(r) * p.output_stride);
    const uintptr_t irow = reinterpret_cast<uintptr_t>(p.input + static_cast<uint64_t>(r) * p.input_stride);
    const uintptr_t a = (orow & ~static_cast<uintptr_t>(VEC - 1)) + static_cast<uintptr_t>(k) * VEC;
    if (a >= orow + p.channels) continue;
    clamp_piece<VEC>(a, a + (irow - orow), orow, orow + p.channels, p.output_min, p.output_max, clamp_hi, clamp_lo);
  }
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_channel_shuffle_run(const struct qnnp_hip_x8_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->output == nullptr || a->groups < 2 || a->group_channels == 0 ||
      static_cast<uint64_t>(a->groups) * a->group_channels != a->channels || a->input_stride < a->channels ||
      a->output_stride < a->channels || a->pixels > 0x7FFFFFFFu) {
    return QNNP_HIP_EINVAL;
  }
  if (a->pixels == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const uint64_t in = address(a->input), out = address(a->output);
  const auto fits = [&](uint64_t v) {
    return aligned(a->group_channels, v) && aligned(in, v) && aligned(out, v) && aligned(a->input_stride, v) &&
        aligned(a->output_stride, v);
  };
  const char* name = nullptr;
  if ((a->groups == 2 || a->groups == 4) && fits(4)) {
    const int vec = fits(16) ? 16 : 4;
    dim3 grid;
    const RowMap m = row_map(a->pixels, a->group_channels / vec, grid);
    if (a->groups == 2 && vec == 16) {
      hipLaunchKernelGGL((x8_shuffle_reg_kernel<2, 16>), grid, dim3(kThreads), 0, stream, *a, m);
      name = "x8_shuffle_g2_x16";
    } else if (a->groups == 2) {
      hipLaunchKernelGGL((x8_shuffle_reg_kernel<2, 4>), grid, dim3(kThreads), 0, stream, *a, m);
      name = "x8_shuffle_g2_x4";
    } else if (vec == 16) {
      hipLaunchKernelGGL((x8_shuffle_reg_kernel<4, 16>), grid, dim3(kThreads), 0, stream, *a, m);
      name = "x8_shuffle_g4_x16";
    } else {
      hipLaunchKernelGGL((x8_shuffle_reg_kernel<4, 4>), grid, dim3(kThreads), 0, stream, *a, m);
      name = "x8_shuffle_g4_x4";
    }
  } else if (a->channels <= kLdsMaxChannels) {
    LdsPlan q;
    q.in_chunks = (a->channels + 30u) / 16u;                 // 16-byte chunks touching a row, wherever it starts
    q.pitch = 16u * q.in_chunks;
    q.rows_per_tile = q.pitch < kLdsTile ? kLdsTile / q.pitch : 1u;
    const uint64_t want_tiles = static_cast<uint64_t>(kTilesPerCu) * active_cu_count();
    const uint32_t spread = static_cast<uint32_t>((a->pixels + want_tiles - 1) / want_tiles);   // >= 1
    if (q.rows_per_tile > spread) q.rows_per_tile = spread;
    q.in_inv = reciprocal_ceil(q.in_chunks);
    q.out_dwords = (a->channels + 6u) / 4u;                  // dwords touching a row, wherever it starts
    q.out_inv = reciprocal_ceil(q.out_dwords);
    q.groups_inv = reciprocal_ceil(a->groups);
    q.tiles = (a->pixels + q.rows_per_tile - 1) / q.rows_per_tile;
    const uint32_t blocks = q.tiles < (1u << 20) ? q.tiles : (1u << 20);
    hipLaunchKernelGGL(x8_shuffle_lds_kernel, dim3(blocks), dim3(kThreads), q.rows_per_tile * q.pitch, stream, *a, q);
    name = "x8_shuffle_lds";
  } else {
    dim3 grid;
    const RowMap m = row_map(a->pixels, a->channels, grid);
    hipLaunchKernelGGL(x8_shuffle_gather_kernel, grid, dim3(kThreads), 0, stream, *a, m);
    name = "x8_shuffle_gather";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}

extern "C" int qnnp_hip_clamp_run(const struct qnnp_hip_x8_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->output == nullptr || a->channels == 0 ||
      a->input_stride < a->channels || a->output_stride < a->channels || a->output_min > a->output_max ||
      a->output_max > 255u || a->pixels > 0x7FFFFFFFu) {
    return QNNP_HIP_EINVAL;
  }
  if (a->pixels == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const uint64_t delta = address(a->input) - address(a->output);
  const bool flat = a->pixels == 1 || (a->input_stride == a->channels && a->output_stride == a->channels);
  const uint64_t stride_delta = flat ? 0 : a->input_stride - a->output_stride;
  const int vec = aligned(delta, 16) && aligned(stride_delta, 16) ? 16 : (aligned(delta, 4) && aligned(stride_delta, 4) ? 4 : 1);
  const char* name = nullptr;
  if (flat) {
    const uint64_t bytes = static_cast<uint64_t>(a->pixels) * a->channels;
    const uint64_t pieces = (address(a->output) % vec + bytes + vec - 1) / vec;
    const uint64_t want = (pieces + kThreads - 1) / kThreads;
    const uint32_t cap = active_cu_count() * 16u;
    const dim3 grid(static_cast<uint32_t>(want < cap ? want : cap));
    if (vec == 16) {
      hipLaunchKernelGGL(u8_clamp_flat_kernel<16>, grid, dim3(kThreads), 0, stream, *a, bytes, pieces);
      name = "u8_clamp_flat_x16";
    } else if (vec == 4) {
      hipLaunchKernelGGL(u8_clamp_flat_kernel<4>, grid, dim3(kThreads), 0, stream, *a, bytes, pieces);
      name = "u8_clamp_flat_x4";
    } else {
      hipLaunchKernelGGL(u8_clamp_flat_kernel<1>, grid, dim3(kThreads), 0, stream, *a, bytes, pieces);
      name = "u8_clamp_flat_x1";
    }
  } else {
    const uint32_t items = vec == 1 ? a->channels : (a->channels + 2u * vec - 2u) / vec;
    dim3 grid;
    const RowMap m = row_map(a->pixels, items, grid);
    if (vec == 16) {
      hipLaunchKernelGGL(u8_clamp_rows_kernel<16>, grid, dim3(kThreads), 0, stream, *a, m);
      name = "u8_clamp_rows_x16";
    } else if (vec == 4) {
      hipLaunchKernelGGL(u8_clamp_rows_kernel<4>, grid, dim3(kThreads), 0, stream, *a, m);
      name = "u8_clamp_rows_x4";
    } else {
      hipLaunchKernelGGL(u8_clamp_rows_kernel<1>, grid, dim3(kThreads), 0, stream, *a, m);
      name = "u8_clamp_rows_x1";
    }
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
