/*
 * q8dwconv.hip -- uint8 depthwise convolution, NHWC, fused Q31 requantization.
 *
 * Replaces, as whole-operator launches, the reference's per-output-row CPU
 * microkernels
 *   q8dwconv_ukernel_up8x9__sse2  (src/q8dwconv/up8x9-sse2.c:14-372, 3x3 unipass)
 *   q8dwconv_ukernel_mp8x25__sse2 (src/q8dwconv/mp8x25-sse2.c:14-742, 5x5 multipass)
 * their pthreadpool fan-out compute_dwconv_unipass / _multiipass
 * (src/operator-run.c:238-284, 675-679) and the pointer indirection buffer of
 * qnnp_indirection_init_dwconv2d (src/indirection.c:81-132), which is not needed:
 * tap coordinates are computed in-kernel.
 *
 * Arithmetic (exact int32, same folding as pack_q8dw_w, src/qnnpack/pack.h:146-159):
 *   out[c] = requant( bias1[c] + sum_taps a(tap, c) * (w(tap, c) - kzp) ),
 *   bias1 = bias + taps*izp*kzp - izp*sum_taps w,   padding taps read a = izp.
 *
 * One input channel per output channel: no dense contraction, an HBM-streaming problem whose work is the coalesced
 * NHWC traffic plus the per-element requantization.
 *
 * This file holds the two generic kernels, the plan (make_plan: which kernel takes a shape, and its launch geometry) and
 * the launch switch. Every other kernel family is a unit of its own that exports dw*_plan / dw*_launch (dwconv_params.h):
 *
 *   kernel  file            reports (q8_dwconv_...)              code  shapes
 *   B       q8dwconv.hip    direct                               1     any; one output byte per thread
 *   B4      q8dwconv.hip    direct4                              9     any window with C >= 4 and 32-bit offsets; four
 *                                                                      channels per thread. What nothing else takes
 *   A       q8dwlds.hip     lds_3x3, lds_5x5                     2     3x3 / 5x5, C % 4 == 0, dword-aligned: band staged
 *                                                                      in LDS. 3x3 / 5x5 that G / H decline
 *   C       q8dwrow.hip     row_3x3                              3     3x3, dilation 1, stride 1 | 2, dword-aligned:
 *                                                                      window sliding along a row; bands too big for A
 *           q8dwrow.hip     row_3x3_any                          8     the same for any C >= 4 at any alignment
 *   G       q8dwcol.hip     col_3x3, col_3x3_dot4,               6     3x3, stride 1 | 2, C % 4 == 0, dword-aligned,
 *                           col_3x3_dot4_dilated                       < 2 GiB: window sliding down a column. The default
 *   H       q8dwcol5.hip    col_5x5_dot4                         6     5x5, as G, weights in int8 range. The default
 *   D       q8dwmfma.hip    mfma_3x3                             4     3x3, C % 16 == 0: matrix cores, operands gathered.
 *                                                                      Forced only
 *   F       q8dwmfma.hip    mfma_lds_3x3                         5     3x3, C % 16 == 0: matrix cores on an LDS band;
 *                                                                      OW >= 56 and C <= 96 where G declines
 *   M16     q8dwmfma16.hip  mfma16_3x3                           7     3x3, stride 1, C % 16 == 0, int8-range weights:
 *                                                                      16x16x64 matrix cores. Forced only
 *
 * "code" is the value of the "dwconv_kernel" test hook (qnnp_hip_dwconv_args::variant) that forces the kernel; 0 chooses.
 * Operators with per-channel requantization run on q8dwconv_pc.hip and are not planned here.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "device_ops.hip.h"
#include "dwconv_params.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "requant.hip.h"

extern "C" void* qnnp_hip_get_stream(void);

/* q8dwconv_pc.hip: operators with per-channel requantization. Weak: that file is linked into libqnnpack_gfx950.so only
 * (see the Makefile), and a library without it refuses such an operator at run. */
extern "C" int qnnp_hip_dwconv_pc_run(const struct qnnp_hip_dwconv_args* a, const char** kernel_name) __attribute__((weak));

namespace {

using qnnp::buffer_rsrc;
using qnnp::launch_status;
using qnnp::DwParams;

// --------------------------------------------------------------------------
// Kernel B: generic direct
// --------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void q8_dwconv_direct_kernel(const DwParams p)
{
  const uint64_t total = static_cast<uint64_t>(p.batch) * p.OH * p.OW * p.C;
  for (uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
       idx += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
    const uint32_t c = static_cast<uint32_t>(idx % p.C);
    const uint64_t pix = idx / p.C;
    const uint32_t ox = static_cast<uint32_t>(pix % p.OW);
    const uint64_t t = pix / p.OW;
    const uint32_t oy = static_cast<uint32_t>(t % p.OH);
    const uint32_t n = static_cast<uint32_t>(t / p.OH);
    int32_t acc = p.bias1[c];
    for (uint32_t ky = 0; ky < p.KH; ky++) {
      const uint32_t iy = oy * p.sh + ky * p.dh - p.pad_top;   // unsigned wrap = out of range
      for (uint32_t kx = 0; kx < p.KW; kx++) {
        const uint32_t ix = ox * p.sw + kx * p.dw - p.pad_left;
        int32_t a = static_cast<int32_t>(p.izp);
        if (iy < p.H && ix < p.W) {
          a = p.input[((static_cast<uint64_t>(n) * p.H + iy) * p.W + ix) * p.in_stride + c];
        }
        acc += a * static_cast<int32_t>(p.wadj[(ky * p.KW + kx) * p.c_pad + c]);
      }
    }
    p.output[pix * p.out_stride + c] = static_cast<uint8_t>(qnnp::q31_requantize(acc, p.rq));
  }
}

// --------------------------------------------------------------------------
// Kernel B4 (round 6): generic direct, four channels per thread
// --------------------------------------------------------------------------
/*
 * What the shapes nothing else takes ran on until round 6 was kernel B: one output BYTE per thread, nine byte loads each -- ShuffleNet
 * v2's depthwise layers with 58 / 122 channels (bench/convolution.cc:335-426) at 0.03-0.07 of their bounds (28 x 28 x 122: 102 us).
 * Same arithmetic (reference: q8dwconv_ukernel_up8x9__sse2 / mp8x25, src/q8dwconv/up8x9-sse2.c:14-372), any window, stride, dilation,
 * channel count and pixel stride; a thread owns four consecutive channels of one output pixel: per tap two DWORD-ALIGNED loads around
 * its four bytes (a pixel of 58 bytes starts anywhere) joined by v_alignbyte, one 8-byte load of the four int16 tap weights. Bytes
 * past the tensor read 0 (buffer descriptor) and channels past C are computed and not stored.
 */
__global__ __launch_bounds__(256)
void q8_dwconv_direct4_kernel(const DwParams p)
{
  const uint32_t q4 = (p.C + 3u) / 4u;
  const uint64_t total = static_cast<uint64_t>(p.batch) * p.OH * p.OW * q4;
  // (the extent rounded up to whole dwords: the dword holding the tensor's last bytes must not read as out of range)
  const uint64_t in_bytes = ((static_cast<uint64_t>(p.batch) * p.H * p.W - 1u) * p.in_stride + p.C + 3u) & ~static_cast<uint64_t>(3);
  const __amdgpu_buffer_rsrc_t in_rsrc = buffer_rsrc(p.input, static_cast<int>(in_bytes));         // (make_plan: < 2^31 bytes)
  // (32-bit index arithmetic -- make_plan: fewer than 2^32 channel groups in all -- a 64-bit division costs ~100 instructions)
  const uint32_t total32 = static_cast<uint32_t>(total);
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total32; idx += gridDim.x * blockDim.x) {
    const uint32_t pix = idx / q4;
    const uint32_t cg = idx - pix * q4;
    const uint32_t t = pix / p.OW;
    const uint32_t ox = pix - t * p.OW;
    const uint32_t n = t / p.OH;
    const uint32_t oy = t - n * p.OH;
    const uint32_t c0 = cg * 4u;
    const int4 bv = *reinterpret_cast<const int4*>(p.bias1 + c0);                        // (c_pad is a multiple of four: pack.h)
    int32_t acc[4] = {bv.x, bv.y, bv.z, bv.w};
    for (uint32_t ky = 0; ky < p.KH; ky++) {
      const uint32_t iy = oy * p.sh + ky * p.dh - p.pad_top;   // unsigned wrap = out of range
      for (uint32_t kx = 0; kx < p.KW; kx++) {
        const uint32_t ix = ox * p.sw + kx * p.dw - p.pad_left;
        uint32_t a4 = p.izp * 0x01010101u;
        if (iy < p.H && ix < p.W) {
          const uint32_t off = ((n * p.H + iy) * p.W + ix) * p.in_stride + c0;
          const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, off & ~3u, 0, 0);
          const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, (off & ~3u) + 4u, 0, 0);
          a4 = __builtin_amdgcn_alignbyte(hi, lo, off & 3u);
        }
        const uint2 wv = *reinterpret_cast<const uint2*>(p.wadj + (ky * p.KW + kx) * p.c_pad + c0);
        acc[0] += static_cast<int32_t>(a4 & 0xFFu) * static_cast<int16_t>(wv.x & 0xFFFFu);
        acc[1] += static_cast<int32_t>((a4 >> 8) & 0xFFu) * static_cast<int16_t>(wv.x >> 16);
        acc[2] += static_cast<int32_t>((a4 >> 16) & 0xFFu) * static_cast<int16_t>(wv.y & 0xFFFFu);
        acc[3] += static_cast<int32_t>(a4 >> 24) * static_cast<int16_t>(wv.y >> 16);
      }
    }
    uint8_t* out = p.output + static_cast<uint64_t>(pix) * p.out_stride + c0;
    const uint32_t q = static_cast<uint32_t>(qnnp::q31_requantize(acc[0], p.rq)) | (static_cast<uint32_t>(qnnp::q31_requantize(acc[1], p.rq)) << 8) |
                       (static_cast<uint32_t>(qnnp::q31_requantize(acc[2], p.rq)) << 16) | (static_cast<uint32_t>(qnnp::q31_requantize(acc[3], p.rq)) << 24);
    const uint32_t nv = min(4u, p.C - c0);
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

enum : uint32_t { kPlanDirect = 1, kPlanLds33, kPlanLds55, kPlanRow, kPlanMfma, kPlanMfmaLds, kPlanCol, kPlanCol5, kPlanM16, kPlanDirect4, kPlanRowAny };

// The four-channel generic kernel: at least four channels, a channel pad of whole dwords and 32-bit offsets into both tensors
bool direct4_fits(const DwParams& p, const struct qnnp_hip_dwconv_args* a)
{
  const uint64_t ib = static_cast<uint64_t>(p.batch) * p.H * p.W * p.in_stride;
  const uint64_t groups4 = static_cast<uint64_t>(p.batch) * p.OH * p.OW * ((p.C + 3u) / 4u);
  return p.C >= 4 && ib + 8 < (UINT64_C(1) << 31) && groups4 + 256u * 8192u < (UINT64_C(1) << 32) && a->c_pad % 4 == 0;
}

// Kernel choice and launch geometry for one (shape, variant, alignment); fills `p` and `plan`.
int make_plan(DwParams& p, const struct qnnp_hip_dwconv_args* a, uintptr_t in_addr, uintptr_t out_addr,
              struct qnnp_hip_dwconv_plan* plan)
{
  const bool k33 = p.KH == 3 && p.KW == 3;
  const bool k55 = p.KH == 5 && p.KW == 5;
  const bool aligned4 = p.in_stride % 4 == 0 && p.out_stride % 4 == 0 && in_addr % 4 == 0 && out_addr % 4 == 0;
  p.store_mode = 0;
  if (p.C % 16 == 0 && p.out_stride % 16 == 0 && out_addr % 16 == 0) p.store_mode = 2;
  else if (p.C % 4 == 0 && p.out_stride % 4 == 0 && out_addr % 4 == 0) p.store_mode = 1;
  plan->vec16 = 0;
  plan->kernel = 0;
  if (a->variant == 8) {
    // (round 6) the sliding-window kernel on unaligned dwords, forced (auto: below, where nothing aligned takes the shape)
    if (!k33 || a->c_pad % 4 != 0 || !qnnp::dwrow_plan(p, true)) return QNNP_HIP_EINVAL;
    plan->kernel = kPlanRowAny;
  } else if (a->variant == 9) {
    // the four-channel generic kernel, forced: any window, stride and base address its offsets cover, or nothing
    if (!direct4_fits(p, a)) return QNNP_HIP_EINVAL;
    plan->kernel = kPlanDirect4;
  } else if (a->variant == 7) {
    // (round 6) the 16x16x64 matrix-core walk, forced
    if (!k33 || !qnnp::dwmfma16_plan(p, in_addr, out_addr)) return QNNP_HIP_EINVAL;
    plan->kernel = kPlanM16;
  } else if (a->variant == 6 && k55) {
    if (!aligned4 || !qnnp::dwcol5_plan(p)) return QNNP_HIP_EINVAL;
    plan->kernel = kPlanCol5;
  } else if (a->variant == 6) {
    if (!aligned4 || !qnnp::dwcol_plan(p)) return QNNP_HIP_EINVAL;
    plan->kernel = kPlanCol;
  } else if (a->variant == 5) {
    if (!qnnp::dwmfma_lds_plan(p, a)) return QNNP_HIP_EINVAL;
    plan->kernel = kPlanMfmaLds;
  } else if (a->variant == 4) {
    if (!qnnp::dwmfma_plan(p, a)) return QNNP_HIP_EINVAL;
    plan->kernel = kPlanMfma;
  } else if (a->variant == 0 && k33 && aligned4 && qnnp::dwcol_plan(p)) {
    // 3x3, dilation 1, stride 1 | 2: the column-sliding window (kernel G) -- 20-35 % ahead of the LDS-tiled and the
    // matrix-core kernels on every one of the ten MobileNetV2 depthwise layers at batch 128 (same-box A/B,
    // scripts/gpu_dwab.sh, profiles/r02/dwconv_kernel_ab_*.txt).
    plan->kernel = kPlanCol;
  } else if (a->variant == 0 && k55 && aligned4 && qnnp::dwcol5_plan(p)) {
    // 5x5, dilation 1, stride 1 | 2, weights in int8 range: the same walk with five-row windows (kernel H)
    plan->kernel = kPlanCol5;
  } else if (a->variant == 0 && k33 && p.OW >= 56 && p.C <= 96 && qnnp::dwmfma_lds_plan(p, a)) {
    // (shapes kernel G declines, e.g. tensors beyond its 32-bit offsets) large images with few channels: the
    // matrix-core kernel with the LDS-staged band
    plan->kernel = kPlanMfmaLds;
  } else {
    // Order of preference (same-box A/B over the MobileNetV2 layers: the LDS-tiled and the sliding-window
    // kernel are within +-10 % of each other, LDS ahead on the small late layers): LDS-tiled, then the
    // register sliding window (3x3 shapes whose band does not fit the LDS budget), then the direct kernel.
    const bool use_lds = a->variant != 1 && a->variant != 3 && (k33 || k55) && aligned4 && qnnp::dwlds_plan(p);
    if (a->variant == 2 && !use_lds) return QNNP_HIP_EINVAL;
    if (!use_lds && (a->variant == 0 || a->variant == 3) && k33 && aligned4 && qnnp::dwrow_plan(p)) {
      plan->kernel = kPlanRow;
    } else if (a->variant == 3) {
      return QNNP_HIP_EINVAL;
    } else if (use_lds) {
      plan->vec16 = (p.CS % 16 == 0 && p.in_stride % 16 == 0 && in_addr % 16 == 0) ? 1u : 0u;
      plan->kernel = k33 ? kPlanLds33 : kPlanLds55;
    } else {
      // (round 6) 3x3 windows of any channel count >= 4 and any alignment: the sliding-window kernel on unaligned dwords
      // ("dwconv_kernel" 8 forces it -- on aligned tensors too --, 1 keeps the generic kernel below, 9 forces its four-channel flavour)
      if (a->variant == 0 && k33 && a->c_pad % 4 == 0 && qnnp::dwrow_plan(p, true)) {
        plan->kernel = kPlanRowAny;
      } else {
        // (round 6) four channels per thread where the tensors allow 32-bit offsets; "dwconv_kernel" 1 keeps the byte-per-thread kernel
        plan->kernel = (a->variant != 1 && direct4_fits(p, a)) ? kPlanDirect4 : kPlanDirect;
      }
    }
  }
  plan->CS = p.CS; plan->TOH = p.TOH; plan->IR = p.IR; plan->IC = p.IC; plan->PP = p.PP;
  plan->bands = p.bands; plan->slabs = p.slabs; plan->store_mode = p.store_mode;
  return QNNP_HIP_OK;
}

// Everything of `p` that comes straight from the arguments; the plan's geometry fields start at zero.
void params_from_args(DwParams& p, const struct qnnp_hip_dwconv_args* a)
{
  p.input = a->input;
  p.output = a->output;
  p.wadj = a->wadj;
  p.bias1 = a->bias1;
  p.batch = a->batch;
  p.H = a->input_height; p.W = a->input_width;
  p.OH = a->output_height; p.OW = a->output_width;
  p.C = a->channels; p.c_pad = a->c_pad;
  p.KH = a->kernel_height; p.KW = a->kernel_width;
  p.sh = a->stride_height; p.sw = a->stride_width;
  p.dh = a->dilation_height; p.dw = a->dilation_width;
  p.pad_top = a->pad_top; p.pad_left = a->pad_left;
  p.in_stride = a->input_stride; p.out_stride = a->output_stride;
  p.izp = a->input_zero_point & 0xFFu;
  p.CS = p.TOH = p.IR = p.IC = p.PP = p.bands = p.slabs = 0;
  p.rq = qnnp::make_requant_dev(a->rq);
  p.stream_out = a->streaming_mode == 0 ? (qnnp_hip_streaming_stores() != 0 ? 1u : 0u) : (a->streaming_mode == 2 ? 1u : 0u);
  p.trace = nullptr;
  p.abl = 0;
  p.cu_count = qnnp::active_cu_count();
  p.dwm_x = a->dwm_x; p.dwm_bias = a->dwm_bias; p.dwm_parts = a->dwm_parts; p.c_pad32 = a->c_pad32;
  p.wrange = a->w_range;
  p.dot4 = a->dot4;
  p.inv_bands = p.inv_slabs = p.inv_q4 = p.inv_dh = 0;
  p.xcd_ranges = 0;
  p.table = nullptr;         // (the launch switch hands it to the kernels that carry it)
}

// The name a launch of plan kernel `kernel` reports.
const char* plan_kernel_name(const DwParams& p, uint32_t kernel)
{
  switch (kernel) {
    case kPlanMfmaLds: return "q8_dwconv_mfma_lds_3x3";
    case kPlanMfma: return "q8_dwconv_mfma_3x3";
    case kPlanRow: return "q8_dwconv_row_3x3";
    case kPlanRowAny: return "q8_dwconv_row_3x3_any";
    case kPlanCol:
      return (p.dh != 1 || p.dw != 1) ? "q8_dwconv_col_3x3_dot4_dilated" : (qnnp::dwcol_uses_dot4(p) ? "q8_dwconv_col_3x3_dot4" : "q8_dwconv_col_3x3");
    case kPlanCol5: return "q8_dwconv_col_5x5_dot4";
    case kPlanM16: return "q8_dwconv_mfma16_3x3";
    case kPlanDirect4: return "q8_dwconv_direct4";
    case kPlanLds33: return "q8_dwconv_lds_3x3";
    case kPlanLds55: return "q8_dwconv_lds_5x5";
    default: return "q8_dwconv_direct";
  }
}

}  // namespace

extern "C" int qnnp_hip_dwconv_plan(const struct qnnp_hip_dwconv_args* a, struct qnnp_hip_dwconv_plan* plan, const char** kernel_name)
{
  if (a == nullptr || plan == nullptr || a->batch == 0 || a->channels == 0) return QNNP_HIP_EINVAL;
  if (a->rq_pc != nullptr) return QNNP_HIP_EINVAL;   // (q8dwconv_pc.hip plans its own launches)
  DwParams p;
  params_from_args(p, a);
  plan->key = 0;
  const int rc = make_plan(p, a, reinterpret_cast<uintptr_t>(a->input), reinterpret_cast<uintptr_t>(a->output), plan);
  if (rc != QNNP_HIP_OK) return rc;
  if (kernel_name != nullptr) *kernel_name = plan_kernel_name(p, plan->kernel);
  return QNNP_HIP_OK;
}

extern "C" int qnnp_hip_dwconv_run(const struct qnnp_hip_dwconv_args* a, const char** kernel_name)
{
  if (a == nullptr || a->batch == 0 || a->channels == 0) return QNNP_HIP_EINVAL;
  // Per-channel operators (a table of multipliers and shifts): the kernels of q8dwconv_pc.hip and nothing else -- no kernel
  // of this file reads the table, so a forced one is refused, never run per tensor.
  if (a->rq_pc != nullptr) {
    if (a->variant != 0) return QNNP_HIP_EINVAL;
    if (qnnp_hip_dwconv_pc_run == nullptr) return QNNP_HIP_EINVAL;
    return qnnp_hip_dwconv_pc_run(a, kernel_name);
  }
  DwParams p;
  params_from_args(p, a);
#ifdef QNNP_ENABLE_ABLATION
  p.trace = static_cast<unsigned long long*>(qnnp_hip_trace_buffer());
  if (const char* env = getenv("QNNP_DW_ABL")) p.abl = static_cast<uint32_t>(atoi(env));
#endif

  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const uintptr_t in_addr = reinterpret_cast<uintptr_t>(a->input);
  const uintptr_t out_addr = reinterpret_cast<uintptr_t>(a->output);

  // The plan (kernel choice + band / slab geometry) depends on the shapes fixed at setup, the variant and the
  // pointers' alignment only: it is computed at the first run after a setup and kept with the operator.
  const uint32_t key = 0x80000000u | (static_cast<uint32_t>(in_addr & 15u)) | (static_cast<uint32_t>(out_addr & 15u) << 4) |
                       (static_cast<uint32_t>(a->variant & 0xFF) << 8) | ((a->batch & 0x7FFFu) << 16);
  struct qnnp_hip_dwconv_plan local_plan;
  struct qnnp_hip_dwconv_plan* plan = a->plan != nullptr ? a->plan : &local_plan;
  if (a->plan == nullptr || plan->key != key) {
    plan->key = 0;
    const int rc = make_plan(p, a, in_addr, out_addr, plan);
    if (rc != QNNP_HIP_OK) return rc;
    plan->key = key;
  } else {
    p.CS = plan->CS; p.TOH = plan->TOH; p.IR = plan->IR; p.IC = plan->IC; p.PP = plan->PP;
    p.bands = plan->bands; p.slabs = plan->slabs; p.store_mode = plan->store_mode;
  }
  if (kernel_name != nullptr) *kernel_name = plan_kernel_name(p, plan->kernel);
  switch (plan->kernel) {
    case kPlanMfmaLds: return qnnp::dwmfma_lds_launch(p, stream);
    case kPlanMfma: return qnnp::dwmfma_launch(p, stream);
    case kPlanRow: return qnnp::dwrow_launch(p, stream);
    case kPlanRowAny: return qnnp::dwrow_launch(p, stream, true);
    case kPlanCol:
    case kPlanCol5: {
      // the column walks carry an attached output table in their epilogue; it is no part of the plan
      p.table = a->table;
      const int rc = plan->kernel == kPlanCol ? qnnp::dwcol_launch(p, stream) : qnnp::dwcol5_launch(p, stream);
      if (rc == QNNP_HIP_OK && a->table != nullptr && a->table_folded != nullptr) *a->table_folded = 1;
      return rc;
    }
    case kPlanM16: return qnnp::dwmfma16_launch(p, stream);
    case kPlanDirect4: {
      const uint64_t total4 = static_cast<uint64_t>(p.batch) * p.OH * p.OW * ((p.C + 3u) / 4u);
      uint64_t blocks4 = (total4 + 255) / 256;
      if (blocks4 > 256u * 32u) blocks4 = 256u * 32u;
      hipLaunchKernelGGL(q8_dwconv_direct4_kernel, dim3(static_cast<uint32_t>(blocks4)), dim3(256), 0, stream, p);
      return launch_status();
    }
    case kPlanLds33:
    case kPlanLds55: return qnnp::dwlds_launch(p, plan->vec16 != 0, stream);
    default:
      break;
  }
  const uint64_t total = static_cast<uint64_t>(p.batch) * p.OH * p.OW * p.C;
  uint64_t blocks = (total + 255) / 256;
  if (blocks > 256u * 16u) blocks = 256u * 16u;   // grid-stride beyond 16 workgroups per CU
  hipLaunchKernelGGL(q8_dwconv_direct_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, stream, p);
  return launch_status();
}
