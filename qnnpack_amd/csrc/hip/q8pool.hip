/*
 * q8pool.hip -- windowed max pooling (uint8) and average pooling (q8), NHWC.
 *
 * max pooling  replaces u8maxpool_ukernel_16x9p8q__sse2 / u8maxpool_ukernel_sub16__sse2 (reference src/u8maxpool/) and
 *              the max-pooling case of qnnp_run_operator (src/operator-run.c:899-940) with its indirection buffer
 *              (src/indirection.c:192-230): every window tap reads the pixel at its coordinates CLAMPED into the image.
 * avg pooling  replaces q8avgpool_ukernel_{up8x9,mp8x9p8q,up8xm}__sse2 (reference src/q8avgpool/) and the average-pooling
 *              case (src/operator-run.c:845-898): taps in padding read the zero buffer, which holds the input zero point
 *              (src/average-pooling.c:139-150), so they add nothing to sum (x - izp); the divisor is the whole window
 *              (the scale of qnnp_avgpool_quantize is input_scale / (output_scale * pooling_size)).
 *
 * Both are byte-streaming kernels: no LDS, no indirection table. A workgroup takes output rows (n, oy) one at a time
 * and a run of (ox, channel vector) items of each, channel vector fastest; a lane walks the taps of its window and keeps
 * VEC channels of the result in registers. VEC = 16 (dwordx4 loads) when channels, both pixel strides and both base pointers are
 * multiples of 16 bytes, else 4 (dword loads), else 1 (bytes).
 *
 * A lane visits only the taps whose coordinates differ: for max pooling the in-image taps of each axis plus ONE tap
 * clamped onto the first / last row or column when the window reaches past that edge (the max is idempotent, so the
 * other clamped taps repeat it); for average pooling only the in-image taps. A window lying wholly in padding thus
 * costs one or two taps per axis, whatever its size.
 *
 * Bytewise u8 max on packed dwords, 3 VALU per dword per tap: v_pk_max_u16 on the raw dwords yields the max of the odd
 * bytes in the high halves of the 16-bit lanes (the high byte decides a 16-bit comparison), and v_pk_max_u16 on the
 * dwords shifted left by 8 in each lane (v_pk_lshlrev_b16) yields the even bytes the same way; one v_perm_b32 joins them.
 * The average sums bytes as packed 16-bit halves (v_perm_b32 splits a dword into even and odd bytes, two v_pk_add_u16
 * add them: 4 VALU per dword per tap) while the window has at most 257 in-image taps (257 * 255 < 2^16), and in int32
 * otherwise.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "avgpool_math.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "u8_bytewise.hip.h"

namespace qnnp {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPackedTaps = 257;   // 257 * 255 = 65535: the largest tap count a 16-bit lane can sum

/* In-image taps [a, b) of the k taps p0 + t*d (t in [0, k)) along an axis of n pixels; b >= a. The setup keeps the
 * padded extent below 2^31, so no term here overflows int32. */
__device__ __forceinline__ void in_image_taps(int32_t p0, uint32_t k, uint32_t d, uint32_t n, int32_t& a, int32_t& b)
{
  const int32_t kk = static_cast<int32_t>(k);
  const int32_t last = static_cast<int32_t>(n) - 1 - p0;          // offset of the last pixel from the window start
  if (d == 1) {
    a = p0 < 0 ? min(-p0, kk) : 0;
    b = last < 0 ? 0 : min(last + 1, kk);
  } else {
    const uint32_t before = p0 < 0 ? static_cast<uint32_t>(-p0) : 0u;
    const uint32_t q = before / d;
    a = min(static_cast<int32_t>(q + (q * d != before ? 1u : 0u)), kk);
    b = last < 0 ? 0 : min(static_cast<int32_t>(static_cast<uint32_t>(last) / d) + 1, kk);
  }
  b = max(a, b);
}

/* taps to visit for max pooling: the in-image ones plus one clamped tap on each side the window reaches past */
__device__ __forceinline__ void max_taps(int32_t p0, uint32_t k, uint32_t d, uint32_t n, int32_t& begin, int32_t& end)
{
  int32_t a, b;
  in_image_taps(p0, k, d, n, a, b);
  begin = a > 0 ? a - 1 : 0;
  end = b < static_cast<int32_t>(k) ? b + 1 : static_cast<int32_t>(k);
}

__device__ __forceinline__ uint32_t clamp_coord(int32_t v, uint32_t n)
{
  return static_cast<uint32_t>(min(max(v, 0), static_cast<int32_t>(n) - 1));
}

/* the VEC / 4 dwords of one tap */
template <int VEC>
__device__ __forceinline__ void load_taps(const uint8_t* px, uint32_t (&v)[VEC / 4])
{
  if constexpr (VEC == 16) {
    const uint4 q = *reinterpret_cast<const uint4*>(px);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *reinterpret_cast<const uint32_t*>(px);
  }
}

template <int VEC>
__global__ __launch_bounds__(kThreads)
void q8_maxpool_kernel(const qnnp_hip_pool_args p, const uint32_t cvecs, const uint32_t rows)
{
  const uint32_t item = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t ox = item / cvecs;
  if (ox >= p.output_width) return;
  const uint32_t c = (item - ox * cvecs) * VEC;
  const int32_t x0 = static_cast<int32_t>(ox * p.stride_width) - static_cast<int32_t>(p.pad_left);
  int32_t tx_begin, tx_end;
  max_taps(x0, p.kernel_width, p.dilation_width, p.input_width, tx_begin, tx_end);
  const uint32_t clamp_hi = clamp_hi_bound(p.output_max);
  const uint32_t clamp_lo = clamp_lo_bound(p.output_min);

  for (uint32_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const uint32_t n = row / p.output_height;
    const uint32_t oy = row - n * p.output_height;
    const int32_t y0 = static_cast<int32_t>(oy * p.stride_height) - static_cast<int32_t>(p.pad_top);
    int32_t ty_begin, ty_end;
    max_taps(y0, p.kernel_height, p.dilation_height, p.input_height, ty_begin, ty_end);
    const uint8_t* image = p.input + static_cast<uint64_t>(n) * p.input_height * p.input_width * p.input_stride + c;
    uint8_t* out = p.output + (static_cast<uint64_t>(row) * p.output_width + ox) * p.output_stride + c;

    if constexpr (VEC == 1) {
      uint32_t m = 0;
      for (int32_t ty = ty_begin; ty < ty_end; ty++) {
        const uint8_t* line = image + static_cast<uint64_t>(clamp_coord(y0 + ty * static_cast<int32_t>(p.dilation_height), p.input_height)) * p.input_width * p.input_stride;
        for (int32_t tx = tx_begin; tx < tx_end; tx++) {
          const uint32_t ix = clamp_coord(x0 + tx * static_cast<int32_t>(p.dilation_width), p.input_width);
          m = max(m, static_cast<uint32_t>(line[static_cast<uint64_t>(ix) * p.input_stride]));
        }
      }
      out[0] = static_cast<uint8_t>(max(min(m, p.output_max), p.output_min));   // u8maxpool sse2: max(min(v, max), min)
    } else {
      constexpr int D = VEC / 4;
      uint32_t odd[D], even[D];
#pragma unroll
      for (int i = 0; i < D; i++) odd[i] = even[i] = 0;
      for (int32_t ty = ty_begin; ty < ty_end; ty++) {
        const uint8_t* line = image + static_cast<uint64_t>(clamp_coord(y0 + ty * static_cast<int32_t>(p.dilation_height), p.input_height)) * p.input_width * p.input_stride;
        const auto column = [&](int32_t tx) {
          return line + static_cast<uint64_t>(clamp_coord(x0 + tx * static_cast<int32_t>(p.dilation_width), p.input_width)) * p.input_stride;
        };
        int32_t tx = tx_begin;
        for (; tx + 3 <= tx_end; tx += 3) {     // three taps' loads in flight before the first max
          uint32_t v[3][D];
#pragma unroll
          for (int j = 0; j < 3; j++) load_taps<VEC>(column(tx + j), v[j]);
#pragma unroll
          for (int j = 0; j < 3; j++) {
#pragma unroll
            for (int i = 0; i < D; i++) max_step(odd[i], even[i], v[j][i]);
          }
        }
        for (; tx < tx_end; tx++) {
          uint32_t v[D];
          load_taps<VEC>(column(tx), v);
#pragma unroll
          for (int i = 0; i < D; i++) max_step(odd[i], even[i], v[i]);
        }
      }
      if constexpr (VEC == 16) {
        uint4 r;
        r.x = max_finish(odd[0], even[0], clamp_hi, clamp_lo);
        r.y = max_finish(odd[1], even[1], clamp_hi, clamp_lo);
        r.z = max_finish(odd[2], even[2], clamp_hi, clamp_lo);
        r.w = max_finish(odd[3], even[3], clamp_hi, clamp_lo);
        *reinterpret_cast<uint4*>(out) = r;
      } else {
        *reinterpret_cast<uint32_t*>(out) = max_finish(odd[0], even[0], clamp_hi, clamp_lo);
      }
    }
  }
}

/* running 16-bit sums of one dword: bytes 0 / 2 in `even`, bytes 1 / 3 in `odd` */
__device__ __forceinline__ void sum_step(uint32_t& even, uint32_t& odd, uint32_t x)
{
  even = as_u32(as_u16x2(even) + as_u16x2(__builtin_amdgcn_perm(0u, x, 0x0c020c00u)));
  odd = as_u32(as_u16x2(odd) + as_u16x2(__builtin_amdgcn_perm(0u, x, 0x0c030c01u)));
}

template <int VEC>
__global__ __launch_bounds__(kThreads)
void q8_avgpool_kernel(const qnnp_hip_pool_args p, const uint32_t cvecs, const uint32_t rows)
{
  const uint32_t item = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t ox = item / cvecs;
  if (ox >= p.output_width) return;
  const uint32_t c = (item - ox * cvecs) * VEC;
  const int32_t x0 = static_cast<int32_t>(ox * p.stride_width) - static_cast<int32_t>(p.pad_left);
  int32_t tx_begin, tx_end;
  in_image_taps(x0, p.kernel_width, 1, p.input_width, tx_begin, tx_end);

  for (uint32_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const uint32_t n = row / p.output_height;
    const uint32_t oy = row - n * p.output_height;
    const int32_t y0 = static_cast<int32_t>(oy * p.stride_height) - static_cast<int32_t>(p.pad_top);
    int32_t ty_begin, ty_end;
    in_image_taps(y0, p.kernel_height, 1, p.input_height, ty_begin, ty_end);
    const uint8_t* image = p.input + static_cast<uint64_t>(n) * p.input_height * p.input_width * p.input_stride + c;
    uint8_t* out = p.output + (static_cast<uint64_t>(row) * p.output_width + ox) * p.output_stride + c;
    const uint32_t taps = static_cast<uint32_t>(ty_end - ty_begin) * static_cast<uint32_t>(tx_end - tx_begin);
    // sum (x - izp) over the in-image taps, in 32-bit wrap-around like the reference's int32 accumulators
    const uint32_t bias = 0u - taps * static_cast<uint32_t>(p.input_zero_point);

    uint32_t acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) acc[i] = 0;
    bool packed = false;
    if constexpr (VEC > 1) {
      if (taps <= kPackedTaps) {
        packed = true;
        constexpr int D = VEC / 4;
        uint32_t even[D], odd[D];
#pragma unroll
        for (int i = 0; i < D; i++) even[i] = odd[i] = 0;
        for (int32_t ty = ty_begin; ty < ty_end; ty++) {
          const uint8_t* line = image + static_cast<uint64_t>(y0 + ty) * p.input_width * p.input_stride;
          int32_t tx = tx_begin;
          for (; tx + 3 <= tx_end; tx += 3) {     // three taps' loads in flight before the first add
            uint32_t v[3][D];
#pragma unroll
            for (int j = 0; j < 3; j++) load_taps<VEC>(line + static_cast<uint64_t>(x0 + tx + j) * p.input_stride, v[j]);
#pragma unroll
            for (int j = 0; j < 3; j++) {
#pragma unroll
              for (int i = 0; i < D; i++) sum_step(even[i], odd[i], v[j][i]);
            }
          }
          for (; tx < tx_end; tx++) {
            uint32_t v[D];
            load_taps<VEC>(line + static_cast<uint64_t>(x0 + tx) * p.input_stride, v);
#pragma unroll
            for (int i = 0; i < D; i++) sum_step(even[i], odd[i], v[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < D; i++) {
          acc[4 * i + 0] = even[i] & 0xFFFFu;
          acc[4 * i + 1] = odd[i] & 0xFFFFu;
          acc[4 * i + 2] = even[i] >> 16;
          acc[4 * i + 3] = odd[i] >> 16;
        }
      }
    }
    if (!packed) {
      for (int32_t ty = ty_begin; ty < ty_end; ty++) {
        const uint8_t* line = image + static_cast<uint64_t>(y0 + ty) * p.input_width * p.input_stride;
        for (int32_t tx = tx_begin; tx < tx_end; tx++) {
          const uint8_t* px = line + static_cast<uint64_t>(x0 + tx) * p.input_stride;
          if constexpr (VEC == 1) {
            acc[0] += px[0];
          } else {
#pragma unroll
            for (int i = 0; i < VEC / 4; i++) {
              const uint32_t x = reinterpret_cast<const uint32_t*>(px)[i];
              acc[4 * i + 0] += x & 0xFFu;
              acc[4 * i + 1] += (x >> 8) & 0xFFu;
              acc[4 * i + 2] += (x >> 16) & 0xFFu;
              acc[4 * i + 3] += x >> 24;
            }
          }
        }
      }
    }
    if constexpr (VEC == 1) {
      out[0] = static_cast<uint8_t>(avgpool_quantize(static_cast<int32_t>(acc[0] + bias), p.params));
    } else {
      uint32_t r[VEC / 4];
#pragma unroll
      for (int i = 0; i < VEC / 4; i++) {
        r[i] = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) r[i] |= avgpool_quantize(static_cast<int32_t>(acc[4 * i + j] + bias), p.params) << (8 * j);
      }
      if constexpr (VEC == 16) {
        *reinterpret_cast<uint4*>(out) = make_uint4(r[0], r[1], r[2], r[3]);
      } else {
        *reinterpret_cast<uint32_t*>(out) = r[0];
      }
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

inline int vector_width(const qnnp_hip_pool_args& a)
{
  const auto fits = [&a](uint32_t v) {
    return a.channels % v == 0 && a.input_stride % v == 0 && a.output_stride % v == 0 && aligned(a.input, v) &&
        aligned(a.output, v);
  };
  return fits(16) ? 16 : (fits(4) ? 4 : 1);
}

/* grid: x = the (ox, channel vector) items of one output row, y = output rows (looped past the cap) */
inline bool plan(const qnnp_hip_pool_args& a, int vec, uint32_t& cvecs, uint32_t& rows, dim3& grid)
{
  cvecs = a.channels / static_cast<uint32_t>(vec);
  const uint64_t items = static_cast<uint64_t>(a.output_width) * cvecs;
  const uint64_t all_rows = static_cast<uint64_t>(a.batch) * a.output_height;
  if (items == 0 || items > 0x7FFFFFFFull || all_rows > 0xFFFFFFFFull) return false;
  const uint64_t gx = (items + kThreads - 1) / kThreads;
  uint64_t gy = all_rows < 65535u ? all_rows : 65535u;
  const uint64_t gy_cap = 0x7FFFFFFFull / (gx * kThreads);      // total work-items below 2^31
  if (gy > gy_cap) gy = gy_cap > 0 ? gy_cap : 1;
  rows = static_cast<uint32_t>(all_rows);
  grid = dim3(static_cast<uint32_t>(gx), static_cast<uint32_t>(gy));
  return true;
}

inline bool valid(const qnnp_hip_pool_args* a)
{
  return a != nullptr && a->input != nullptr && a->output != nullptr && a->channels != 0 && a->input_height != 0 &&
      a->input_width != 0 && a->kernel_height != 0 && a->kernel_width != 0 && a->stride_height != 0 &&
      a->stride_width != 0 && a->dilation_height != 0 && a->dilation_width != 0;
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_maxpool_run(const struct qnnp_hip_pool_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (!valid(a)) return QNNP_HIP_EINVAL;
  if (a->batch == 0 || a->output_height == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const int vec = vector_width(*a);
  uint32_t cvecs, rows;
  dim3 grid;
  if (!plan(*a, vec, cvecs, rows, grid)) return QNNP_HIP_EINVAL;
  if (vec == 16) {
    hipLaunchKernelGGL(q8_maxpool_kernel<16>, grid, dim3(kThreads), 0, stream, *a, cvecs, rows);
    if (kernel_name != nullptr) *kernel_name = "q8_maxpool_x16";
  } else if (vec == 4) {
    hipLaunchKernelGGL(q8_maxpool_kernel<4>, grid, dim3(kThreads), 0, stream, *a, cvecs, rows);
    if (kernel_name != nullptr) *kernel_name = "q8_maxpool_x4";
  } else {
    hipLaunchKernelGGL(q8_maxpool_kernel<1>, grid, dim3(kThreads), 0, stream, *a, cvecs, rows);
    if (kernel_name != nullptr) *kernel_name = "q8_maxpool_x1";
  }
  return launch_status();
}

extern "C" int qnnp_hip_avgpool_run(const struct qnnp_hip_pool_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (!valid(a)) return QNNP_HIP_EINVAL;
  if (a->batch == 0 || a->output_height == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const int vec = vector_width(*a);
  uint32_t cvecs, rows;
  dim3 grid;
  if (!plan(*a, vec, cvecs, rows, grid)) return QNNP_HIP_EINVAL;
  if (vec == 16) {
    hipLaunchKernelGGL(q8_avgpool_kernel<16>, grid, dim3(kThreads), 0, stream, *a, cvecs, rows);
    if (kernel_name != nullptr) *kernel_name = "q8_avgpool_x16";
  } else if (vec == 4) {
    hipLaunchKernelGGL(q8_avgpool_kernel<4>, grid, dim3(kThreads), 0, stream, *a, cvecs, rows);
    if (kernel_name != nullptr) *kernel_name = "q8_avgpool_x4";
  } else {
    hipLaunchKernelGGL(q8_avgpool_kernel<1>, grid, dim3(kThreads), 0, stream, *a, cvecs, rows);
    if (kernel_name != nullptr) *kernel_name = "q8_avgpool_x1";
  }
  return launch_status();
}
