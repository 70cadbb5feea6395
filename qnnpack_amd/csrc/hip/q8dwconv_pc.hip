/*
 * q8dwconv_pc.hip -- uint8 depthwise convolution, NHWC, with PER-CHANNEL requantization
 * (include/qnnpack_gfx950_perchannel.h): every depthwise operator made by
 * qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel runs here, whatever its window, stride, dilation, padding,
 * channel count (>= 1), pixel strides and base addresses. The per-tensor operators never come here (q8dwconv.hip).
 *
 * Arithmetic: the accumulator of q8dwconv.hip on the same packed images,
 *   acc[c] = bias1[c] + sum_taps a(tap, c) * wadj[tap][c],       padding taps read a = input zero point,
 * then qnnp_requant_pc (requant_pc.h) with channel c's (multiplier, shift) and the operator's clamp and zero point.
 *
 * q8_dwconv_pc_kernel<KW, SW>: a thread owns FOUR CONSECUTIVE CHANNELS and loads their four table entries and biases
 * ONCE; it then walks kPcWalk consecutive output pixels of one output row -- this is where per-channel costs nothing
 * extra, the constants do not change along the walk. Per kernel row:
 *   KW in {3, 5}, SW in {1, 2}, column dilation 1: the (kPcWalk - 1) * SW + KW input columns the walk touches are
 *     fetched once into registers and every output pixel takes its KW of them (3x3 stride 1: 6 fetches for 12 taps);
 *   <0, 0>: any window, stride and dilation -- a tap's four weights are loaded once and meet the tap's column of every
 *     pixel of the walk.
 * A column is one unaligned dword (a pixel of 6 or 58 bytes starts anywhere; gfx950 takes unaligned global dwords),
 * fetched bytewise only where the dword would pass the tensor's last byte. Bytes of channels past C are computed with
 * the table's pad entries and not stored. Stores: one dword where the address allows it, else halves, else bytes.
 * No LDS, no scratch: every array is indexed by unrolled constants.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "per_device.h"
#include "qnnp_hip.h"
#include "requant_pc.h"

namespace {

using qnnp::launch_status;

constexpr int kPcThreads = 256;
constexpr int kPcWalk = 4;            // output pixels of a row per thread
typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

struct DwPcParams {
  const uint8_t* input;
  const uint8_t* input_end;   // one past the last input byte the operator may read
  uint8_t* output;
  const int16_t* wadj;        // [taps][c_pad]
  const int32_t* bias1;       // [c_pad]
  const qnnp_requant_pc_entry* table;   // [c_pad]
  uint32_t H, W, OH, OW;
  uint32_t C, c_pad;
  uint32_t KH, KW;
  uint32_t sh, sw, dh, dw;
  uint32_t pad_top, pad_left;
  uint32_t in_stride, out_stride;
  uint32_t izp4;              // input zero point in all four bytes
  uint32_t q4;                // channel groups of four: ceil(C / 4)
  uint32_t row_items;         // threads' worth of work in one output row: ceil(OW / kPcWalk) * q4
  uint32_t bpr;               // workgroups per output row
  uint64_t units;             // batch * OH * bpr
  int32_t lo, hi, zp;         // clamp less the zero point, zero point
};

// four bytes from `src` (src < end); bytes at or past `end` read 0
__device__ __forceinline__ uint32_t fetch4(const uint8_t* src, const uint8_t* end)
{
  if (src + 4 <= end) return *reinterpret_cast<const u32_unaligned*>(src);
  uint32_t v = src[0];
  if (src + 1 < end) v |= static_cast<uint32_t>(src[1]) << 8;
  if (src + 2 < end) v |= static_cast<uint32_t>(src[2]) << 16;
  return v;
}

// acc[j] += byte j of a4 * int16 j of wv, in two's complement: the folded bias may sit at either end of the int32 range
// and only the finished sum is the accumulator of the definition
__device__ __forceinline__ int32_t mac(int32_t acc, uint32_t a, int16_t w)
{
  return static_cast<int32_t>(static_cast<uint32_t>(acc) + static_cast<uint32_t>(static_cast<int32_t>(a) * w));
}
__device__ __forceinline__ void mac4(int32_t (&acc)[4], uint32_t a4, uint2 wv)
{
  acc[0] = mac(acc[0], a4 & 0xFFu, static_cast<int16_t>(wv.x & 0xFFFFu));
  acc[1] = mac(acc[1], (a4 >> 8) & 0xFFu, static_cast<int16_t>(wv.x >> 16));
  acc[2] = mac(acc[2], (a4 >> 16) & 0xFFu, static_cast<int16_t>(wv.y & 0xFFFFu));
  acc[3] = mac(acc[3], a4 >> 24, static_cast<int16_t>(wv.y >> 16));
}

template <int KW, int SW>     // <0, 0>: window, stride and dilation from the parameters
__global__ __launch_bounds__(kPcThreads)
void q8_dwconv_pc_kernel(const DwPcParams p)
{
  for (uint64_t unit = blockIdx.x; unit < p.units; unit += gridDim.x) {
    const uint32_t row = static_cast<uint32_t>(unit / p.bpr);       // image * OH + output row (workgroup-uniform)
    const uint32_t item = static_cast<uint32_t>(unit - static_cast<uint64_t>(row) * p.bpr) * kPcThreads + threadIdx.x;
    if (item >= p.row_items) continue;
    const uint32_t seg = item / p.q4;
    const uint32_t c0 = (item - seg * p.q4) * 4u;
    const uint32_t ox0 = seg * kPcWalk;
    const uint32_t n = row / p.OH;
    const uint32_t oy = row - n * p.OH;
    const uint8_t* image = p.input + static_cast<uint64_t>(n) * p.H * p.W * p.in_stride + c0;

    // the constants of this thread's four channels, once (c_pad is a multiple of 16: whole 16-byte loads)
    const int4 e01 = *reinterpret_cast<const int4*>(p.table + c0);
    const int4 e23 = *reinterpret_cast<const int4*>(p.table + c0 + 2);
    const int4 bv = *reinterpret_cast<const int4*>(p.bias1 + c0);
    int32_t acc[kPcWalk][4];
#pragma unroll
    for (int w = 0; w < kPcWalk; w++) { acc[w][0] = bv.x; acc[w][1] = bv.y; acc[w][2] = bv.z; acc[w][3] = bv.w; }

    for (uint32_t ky = 0; ky < p.KH; ky++) {
      const uint32_t iy = oy * p.sh + ky * p.dh - p.pad_top;        // unsigned wrap = out of range
      const bool row_in = iy < p.H;
      const uint32_t row_off = iy * p.W;
      if constexpr (KW != 0) {
        constexpr int NCOL = (kPcWalk - 1) * SW + KW;
        uint32_t col[NCOL];
#pragma unroll
        for (int j = 0; j < NCOL; j++) {
          const uint32_t ix = ox0 * SW + j - p.pad_left;
          col[j] = p.izp4;
          if (row_in && ix < p.W) col[j] = fetch4(image + (row_off + ix) * p.in_stride, p.input_end);
        }
#pragma unroll
        for (int kx = 0; kx < KW; kx++) {
          const uint2 wv = *reinterpret_cast<const uint2*>(p.wadj + (ky * KW + kx) * p.c_pad + c0);
#pragma unroll
          for (int w = 0; w < kPcWalk; w++) mac4(acc[w], col[w * SW + kx], wv);
        }
      } else {
        for (uint32_t kx = 0; kx < p.KW; kx++) {
          const uint2 wv = *reinterpret_cast<const uint2*>(p.wadj + (ky * p.KW + kx) * p.c_pad + c0);
#pragma unroll
          for (int w = 0; w < kPcWalk; w++) {
            const uint32_t ox = ox0 + w;
            const uint32_t ix = ox * p.sw + kx * p.dw - p.pad_left;
            uint32_t a4 = p.izp4;
            if (row_in && ix < p.W && ox < p.OW) a4 = fetch4(image + (row_off + ix) * p.in_stride, p.input_end);
            mac4(acc[w], a4, wv);
          }
        }
      }
    }

    const uint32_t nv = min(4u, p.C - c0);
#pragma unroll
    for (int w = 0; w < kPcWalk; w++) {
      const uint32_t ox = ox0 + w;
      if (ox >= p.OW) continue;
      const uint32_t q =
          static_cast<uint32_t>(qnnp_requant_pc(acc[w][0], e01.x, static_cast<uint32_t>(e01.y), p.lo, p.hi, p.zp)) |
          (static_cast<uint32_t>(qnnp_requant_pc(acc[w][1], e01.z, static_cast<uint32_t>(e01.w), p.lo, p.hi, p.zp)) << 8) |
          (static_cast<uint32_t>(qnnp_requant_pc(acc[w][2], e23.x, static_cast<uint32_t>(e23.y), p.lo, p.hi, p.zp)) << 16) |
          (static_cast<uint32_t>(qnnp_requant_pc(acc[w][3], e23.z, static_cast<uint32_t>(e23.w), p.lo, p.hi, p.zp)) << 24);
      uint8_t* out = p.output + (static_cast<uint64_t>(row) * p.OW + ox) * p.out_stride + c0;
      const uintptr_t addr = reinterpret_cast<uintptr_t>(out);
      if (nv == 4u && (addr & 3u) == 0u) {
        *reinterpret_cast<uint32_t*>(out) = q;
      } else if (nv == 4u && (addr & 1u) == 0u) {
        *reinterpret_cast<uint16_t*>(out) = static_cast<uint16_t>(q);
        *reinterpret_cast<uint16_t*>(out + 2) = static_cast<uint16_t>(q >> 16);
      } else {
        for (uint32_t b = 0; b < nv; b++) out[b] = static_cast<uint8_t>(q >> (8 * b));
      }
    }
  }
}

template <int KW, int SW>
int launch_pc(const DwPcParams& p, hipStream_t stream)
{
  const uint64_t blocks = p.units < (UINT64_C(1) << 20) ? p.units : (UINT64_C(1) << 20);   // grid-stride beyond
  hipLaunchKernelGGL((q8_dwconv_pc_kernel<KW, SW>), dim3(static_cast<uint32_t>(blocks)), dim3(kPcThreads), 0, stream, p);
  return launch_status();
}

}  // namespace

/* the per-channel depthwise launch behind qnnp_hip_dwconv_run (q8dwconv.hip) for arguments with a table */
extern "C" int qnnp_hip_dwconv_pc_run(const struct qnnp_hip_dwconv_args* a, const char** kernel_name)
{
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  if (a == nullptr || a->batch == 0 || a->channels == 0 || a->rq_pc == nullptr || a->c_pad % 16 != 0 || a->c_pad < a->channels || a->kernel_height == 0 || a->kernel_width == 0 ||
      a->output_height == 0 || a->output_width == 0) return QNNP_HIP_EINVAL;
  DwPcParams p;
  p.input = a->input;
  p.input_end = a->input + ((static_cast<uint64_t>(a->batch) * a->input_height * a->input_width - 1u) * a->input_stride + a->channels);
  p.output = a->output;
  p.wadj = a->wadj;
  p.bias1 = a->bias1;
  p.table = a->rq_pc;
  p.H = a->input_height; p.W = a->input_width;
  p.OH = a->output_height; p.OW = a->output_width;
  p.C = a->channels; p.c_pad = a->c_pad;
  p.KH = a->kernel_height; p.KW = a->kernel_width;
  p.sh = a->stride_height; p.sw = a->stride_width;
  p.dh = a->dilation_height; p.dw = a->dilation_width;
  p.pad_top = a->pad_top; p.pad_left = a->pad_left;
  p.in_stride = a->input_stride; p.out_stride = a->output_stride;
  p.izp4 = (a->input_zero_point & 0xFFu) * 0x01010101u;
  p.q4 = (a->channels + 3u) / 4u;
  // (a row of more than 2^32 thread items -- an output row beyond 64 GiB -- is the one shape refused)
  const uint64_t row_items = static_cast<uint64_t>((a->output_width + kPcWalk - 1u) / kPcWalk) * p.q4;
  if (row_items >= (UINT64_C(1) << 32) - kPcThreads) return QNNP_HIP_EINVAL;
  p.row_items = static_cast<uint32_t>(row_items);
  p.bpr = (p.row_items + kPcThreads - 1u) / kPcThreads;
  p.units = static_cast<uint64_t>(a->batch) * a->output_height * p.bpr;
  p.lo = a->rq.output_min_less_zero_point;
  p.hi = a->rq.output_max_less_zero_point;
  p.zp = a->rq.output_zero_point;
  const bool walk = a->dilation_width == 1 && (a->kernel_width == 3 || a->kernel_width == 5) &&
                    (a->stride_width == 1 || a->stride_width == 2);
  if (!walk) {
    if (kernel_name != nullptr) *kernel_name = "q8_dwconv_pc_any";
    return launch_pc<0, 0>(p, stream);
  }
  if (a->kernel_width == 3) {
    if (kernel_name != nullptr) *kernel_name = a->stride_width == 1 ? "q8_dwconv_pc_w3s1" : "q8_dwconv_pc_w3s2";
    return a->stride_width == 1 ? launch_pc<3, 1>(p, stream) : launch_pc<3, 2>(p, stream);
  }
  if (kernel_name != nullptr) *kernel_name = a->stride_width == 1 ? "q8_dwconv_pc_w5s1" : "q8_dwconv_pc_w5s2";
  return a->stride_width == 1 ? launch_pc<5, 1>(p, stream) : launch_pc<5, 2>(p, stream);
}
