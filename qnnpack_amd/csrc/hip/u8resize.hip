/*
 * u8resize.hip -- bilinear resize of uint8 NHWC tensors with pixel strides, quantization unchanged. No reference
 * counterpart. The definition is integers only (include/qnnpack_gfx950.h): the host builds one table per axis
 * (resize-table.h) -- for every output row / column the first of the two input rows / columns it blends, whether the
 * second is the next one, and a Q11 weight -- and the kernels compute, for every channel c of output pixel (oy, ox),
 *   top = x[y0][x0][c] * (2048 - wx) + x[y0][x1][c] * wx;   bot = x[y1][x0][c] * (2048 - wx) + x[y1][x1][c] * wx
 *   y   = (top * (2048 - wy) + bot * wy + 2^21) >> 22
 * Nothing is rounded before the last shift, so the kernels multiply out: with the four products of the two weight pairs
 * formed once per piece (w00 = (2048 - wx) * (2048 - wy), ..., each <= 2^22, their sum 2^22)
 *   y = (x00 * w00 + x01 * w01 + x10 * w10 + x11 * w11 + 2^21) >> 22            (<= 255 * 2^22 + 2^21 < 2^31)
 * which is the same integer: four 24-bit multiply-adds per byte (v_mad_u32_u24), one shift, one pack.
 *
 * An upsampling writes far more than it reads -- the taps of neighbouring output pixels are the same few input pixels,
 * served by L1 / L2 -- so the kernels are about coalesced stores, like q8mul.hip: 256-thread workgroups, a grid-stride
 * loop over pixel groups capped by the compute-unit count, 64-bit byte offsets. A lane's piece is 16 bytes, a dword or a
 * byte of the channels of ONE output pixel: it loads that piece of the four taps, blends and stores. Pixels with few
 * pieces share a workgroup (lane -> (pixel, piece) by one magic divide of the thread index, as row_map.hip.h does it);
 * pixels with more pieces than a workgroup span gridDim.y workgroups. The pixel's image, row and column come from two
 * more magic divides (Div31 below, exact for every pixel index below 2^31), its two 8-byte table entries from L1 / L2.
 *
 *   u8_resize_x16  channels % 16 == 0, both base addresses and both pixel strides multiples of 16: 16-byte pieces. The
 *                  output is written exactly once, so the STORE carries the streaming hint where the operator asks for
 *                  it; the loads never do (neighbouring output pixels read the same lines again).
 *   u8_resize_x4   any other tensor with channels >= 4, at ANY alignment: channels / 4 dwords per pixel at whatever
 *                  address they fall on (global memory takes unaligned dwords), then one piece of channels % 4 single
 *                  bytes. No load or store touches a byte outside the pixel's `channels` bytes.
 *   u8_resize_x1   channels < 4: byte by byte.
 * No LDS, no scratch.
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
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t __attribute__((aligned(1))) resize_u32_unaligned;

/*
 * n / d for every n < 2^31 by one multiply and one shift: with l = ceil(log2 d) and m = ceil(2^(31 + l) / d) (< 2^32
 * because d > 2^(l - 1)), m * d lies in [2^(31 + l), 2^(31 + l) + 2^l], which makes floor(n * m / 2^(31 + l)) the
 * quotient for all n < 2^31 (Granlund & Montgomery, theorem 4.2 with N = 31). m == 0 stands for d == 1.
 */
struct Div31 {
  uint32_t m, shift;
};

inline Div31 div31(uint32_t d)
{
  if (d <= 1u) return Div31{0u, 0u};
  const uint32_t l = 32u - static_cast<uint32_t>(__builtin_clz(d - 1u));
  return Div31{static_cast<uint32_t>(((UINT64_C(1) << (31u + l)) + d - 1u) / d), l - 1u};
}

__device__ __forceinline__ uint32_t div31(uint32_t n, Div31 d) { return d.m != 0u ? __umulhi(n, d.m) >> d.shift : n; }

struct ResizeParams {
  const uint8_t* input;
  uint8_t* output;
  const u32x2* row_table;      // [output_height] {y0, wy | step << 11}
  const u32x2* col_table;      // [output_width]  {x0, wx | step << 11}
  uint64_t in_stride, out_stride;
  uint64_t in_row_bytes;       // in_w * in_stride
  uint32_t pixels;             // output pixels of all images (< 2^31)
  uint32_t pieces;             // pieces per pixel
  uint32_t pieces_inv;         // reciprocal_ceil(pieces) when pieces <= kThreads
  uint32_t pixels_per_block;   // pixels of one group: kThreads / pieces, or 1 for pixels with more pieces than a workgroup
  uint32_t groups;             // ceil(pixels / pixels_per_block)
  uint32_t out_h, out_w;
  Div31 by_out_w, by_out_h;
  uint32_t in_w, in_image;     // input pixels per row and per image (batch * in_image < 2^31)
  uint32_t channels;
};

/* the four products of the two weight pairs; they sum to 2^22 */
struct Weights {
  uint32_t w00, w01, w10, w11;
};

__device__ __forceinline__ uint32_t blend_u8(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const Weights& w)
{
  return (__umul24(a, w.w00) + __umul24(b, w.w01) + __umul24(c, w.w10) + __umul24(d, w.w11) + (1u << 21)) >> 22;
}

/* four bytes of one dword of each tap (byte k of the result belongs to byte k) */
__device__ __forceinline__ uint32_t blend_u8x4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const Weights& w)
{
  const uint32_t y0 = blend_u8(a & 0xFFu, b & 0xFFu, c & 0xFFu, d & 0xFFu, w);
  const uint32_t y1 = blend_u8((a >> 8) & 0xFFu, (b >> 8) & 0xFFu, (c >> 8) & 0xFFu, (d >> 8) & 0xFFu, w);
  const uint32_t y2 = blend_u8((a >> 16) & 0xFFu, (b >> 16) & 0xFFu, (c >> 16) & 0xFFu, (d >> 16) & 0xFFu, w);
  const uint32_t y3 = blend_u8(a >> 24, b >> 24, c >> 24, d >> 24, w);
  return y0 | y1 << 8 | y2 << 16 | y3 << 24;
}

/* piece k of one output pixel: p00 .. p11 are the four tap pixels, po the output pixel */
template <int VEC, bool STREAM>
__device__ __forceinline__ void resize_piece(const uint8_t* p00, const uint8_t* p01, const uint8_t* p10, const uint8_t* p11,
                                             uint8_t* po, uint32_t k, const Weights& w, const ResizeParams& p)
{
  if constexpr (VEC == 16) {
    const uint32_t c = k * 16u;                           // < channels < 2^31
    const u32x4 a = *reinterpret_cast<const u32x4*>(p00 + c);
    const u32x4 b = *reinterpret_cast<const u32x4*>(p01 + c);
    const u32x4 e = *reinterpret_cast<const u32x4*>(p10 + c);
    const u32x4 f = *reinterpret_cast<const u32x4*>(p11 + c);
    u32x4 y;
    y.x = blend_u8x4(a.x, b.x, e.x, f.x, w);
    y.y = blend_u8x4(a.y, b.y, e.y, f.y, w);
    QNNP_PIN();   // two dwords' values in flight, not four: interleaving all sixteen bytes takes the kernel past 64 VGPRs
    y.z = blend_u8x4(a.z, b.z, e.z, f.z, w);
    y.w = blend_u8x4(a.w, b.w, e.w, f.w, w);
    if constexpr (STREAM) {
      __builtin_nontemporal_store(y, reinterpret_cast<u32x4*>(po + c));
    } else {
      *reinterpret_cast<u32x4*>(po + c) = y;
    }
  } else if constexpr (VEC == 4) {
    const uint32_t c = k * 4u;
    if (c + 4u <= p.channels) {
      const uint32_t a = *reinterpret_cast<const resize_u32_unaligned*>(p00 + c);
      const uint32_t b = *reinterpret_cast<const resize_u32_unaligned*>(p01 + c);
      const uint32_t e = *reinterpret_cast<const resize_u32_unaligned*>(p10 + c);
      const uint32_t f = *reinterpret_cast<const resize_u32_unaligned*>(p11 + c);
      *reinterpret_cast<resize_u32_unaligned*>(po + c) = blend_u8x4(a, b, e, f, w);
    } else {
      // the tail: channels % 4 single bytes
      for (uint32_t i = c; i < p.channels; i++) {
        po[i] = static_cast<uint8_t>(blend_u8(p00[i], p01[i], p10[i], p11[i], w));
      }
    }
  } else {
    po[k] = static_cast<uint8_t>(blend_u8(p00[k], p01[k], p10[k], p11[k], w));
  }
}

/* grid x: pixel groups (grid-stride); grid y: the kThreads-piece chunks of a pixel with more pieces than a workgroup
 * (grid-stride) */
template <int VEC, bool STREAM>
__global__ __launch_bounds__(kThreads)
void u8_resize_kernel(const ResizeParams p)
{
  uint32_t pl = 0, k0 = blockIdx.y * kThreads + threadIdx.x;
  if (p.pieces <= static_cast<uint32_t>(kThreads)) {
    pl = div_magic(threadIdx.x, p.pieces_inv);
    k0 = threadIdx.x - pl * p.pieces;
    if (pl >= p.pixels_per_block) return;
  }
  const uint32_t k_step = gridDim.y * kThreads;
  for (uint32_t grp = blockIdx.x; grp < p.groups; grp += gridDim.x) {
    const uint32_t r = grp * p.pixels_per_block + pl;       // < pixels + kThreads: no wrap
    if (r >= p.pixels || k0 >= p.pieces) continue;          // (the last group; a lane past the pixel's last piece)
    const uint32_t t = div31(r, p.by_out_w);                // image * out_h + oy
    const uint32_t ox = r - t * p.out_w;
    const uint32_t n = div31(t, p.by_out_h);
    const uint32_t oy = t - n * p.out_h;
    const u32x2 row = p.row_table[oy], col = p.col_table[ox];
    const uint32_t wy = row.y & 2047u, wx = col.y & 2047u;
    Weights w;
    w.w00 = (2048u - wx) * (2048u - wy);
    w.w01 = wx * (2048u - wy);
    w.w10 = (2048u - wx) * wy;
    w.w11 = wx * wy;
    // the second tap of an axis is the next input row / column, or the same one (the weight is 0 then)
    const uint64_t step_y = (row.y >> 11) != 0u ? p.in_row_bytes : 0u, step_x = (col.y >> 11) != 0u ? p.in_stride : 0u;
    const uint32_t i00 = n * p.in_image + row.x * p.in_w + col.x;             // < batch * in_image < 2^31
    const uint8_t* p00 = p.input + static_cast<uint64_t>(i00) * p.in_stride;
    const uint8_t* p01 = p00 + step_x;
    const uint8_t* p10 = p00 + step_y;
    const uint8_t* p11 = p10 + step_x;
    uint8_t* po = p.output + static_cast<uint64_t>(r) * p.out_stride;
    for (uint32_t k = k0; k < p.pieces; k += k_step) {
      resize_piece<VEC, STREAM>(p00, p01, p10, p11, po, k, w, p);
    }
  }
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_resize_run(const struct qnnp_hip_resize_args* a, const char** kernel_name)
{
  using namespace qnnp;
  constexpr uint32_t kSizeLimit = 1u << 24;
  if (a == nullptr || a->input == nullptr || a->output == nullptr || a->table == nullptr || !aligned(address(a->table), 8) ||
      a->channels == 0 || a->channels > 0x7FFFFFFFu || a->input_stride < a->channels || a->output_stride < a->channels ||
      a->input_height == 0 || a->input_width == 0 || a->output_height == 0 || a->output_width == 0 ||
      a->input_height >= kSizeLimit || a->input_width >= kSizeLimit || a->output_height >= kSizeLimit ||
      a->output_width >= kSizeLimit) {
    return QNNP_HIP_EINVAL;
  }
  const uint64_t in_image = static_cast<uint64_t>(a->input_height) * a->input_width;
  const uint64_t pixels = static_cast<uint64_t>(a->batch) * a->output_height * a->output_width;
  if (a->batch > 0x7FFFFFFFu || a->batch * in_image > 0x7FFFFFFFu || pixels > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;
  if (a->batch == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());

  const bool all16 = aligned(a->channels, 16) && aligned(address(a->input), 16) && aligned(address(a->output), 16) &&
      aligned(a->input_stride, 16) && aligned(a->output_stride, 16);
  const uint32_t vec = all16 ? 16u : (a->channels >= 4u ? 4u : 1u);

  ResizeParams p;
  p.input = a->input;
  p.output = a->output;
  p.row_table = static_cast<const u32x2*>(a->table);
  p.col_table = p.row_table + a->output_height;
  p.in_stride = a->input_stride;
  p.out_stride = a->output_stride;
  p.in_row_bytes = static_cast<uint64_t>(a->input_width) * a->input_stride;
  p.pixels = static_cast<uint32_t>(pixels);
  p.pieces = (a->channels + vec - 1u) / vec;              // x4: the dwords, and one piece for a tail of 1 .. 3 bytes
  const bool shared = p.pieces <= static_cast<uint32_t>(kThreads);
  p.pieces_inv = shared ? reciprocal_ceil(p.pieces) : 0u;
  p.pixels_per_block = shared ? kThreads / p.pieces : 1u;
  p.groups = static_cast<uint32_t>((pixels + p.pixels_per_block - 1) / p.pixels_per_block);
  p.out_h = a->output_height;
  p.out_w = a->output_width;
  p.by_out_w = div31(a->output_width);
  p.by_out_h = div31(a->output_height);
  p.in_w = a->input_width;
  p.in_image = static_cast<uint32_t>(in_image);
  p.channels = a->channels;

  // beyond the cap the grid-stride loops take further passes
  const uint32_t cap = active_cu_count() * 16u;
  const uint32_t chunks = shared ? 1u : (p.pieces + kThreads - 1) / kThreads;
  const uint32_t gy = chunks < kMaxGridY ? (chunks < cap ? chunks : cap) : (cap < kMaxGridY ? cap : kMaxGridY);
  const uint32_t cap_x = cap / gy > 0 ? cap / gy : 1u;
  const dim3 grid(p.groups < cap_x ? p.groups : cap_x, gy);

  const bool hint = a->streaming_mode == 0 ? qnnp_hip_streaming_stores() != 0 : a->streaming_mode == 2;
  const char* name = nullptr;
  if (vec == 16) {
    if (hint) {
      hipLaunchKernelGGL((u8_resize_kernel<16, true>), grid, dim3(kThreads), 0, stream, p);
    } else {
      hipLaunchKernelGGL((u8_resize_kernel<16, false>), grid, dim3(kThreads), 0, stream, p);
    }
    name = "u8_resize_x16";
  } else if (vec == 4) {
    hipLaunchKernelGGL((u8_resize_kernel<4, false>), grid, dim3(kThreads), 0, stream, p);
    name = "u8_resize_x4";
  } else {
    hipLaunchKernelGGL((u8_resize_kernel<1, false>), grid, dim3(kThreads), 0, stream, p);
    name = "u8_resize_x1";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
