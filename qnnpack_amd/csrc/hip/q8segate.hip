/*
 * q8segate.hip -- the gate of a squeeze-and-excite block as ONE kernel: global average pooling -> fully connected C -> S
 * (its ReLU is the clamp of its requantization) -> fully connected S -> C -> byte table, one workgroup per image. The
 * broadcast multiply x * s that ends the block stays the kernel of q8mul.hip (squeeze-excite.c launches it behind this
 * one). No reference counterpart.
 *
 * Four of the block's five stand-alone launches work on batch x C bytes: they are launch latency and one dependent
 * memory round trip each. Here the pooled row, the hidden row and the table stay in LDS, and the only global traffic
 * between the image and the gate row is the two weight images, which every workgroup reads from L2.
 *
 * The arithmetic is the stand-alone operators', on THEIR device images (qnnp_hip.h states it):
 *   pooling  exact int32 sums + avgpool_quantize (avgpool_math.hip.h), the load shapes of q8_gavgpool_kernel
 *            (q8pointwise.hip): dwords where channels, stride and base allow, bytes otherwise, kSePoolUnroll pixels in
 *            flight per lane, pixel slices reduced through LDS;
 *   FC       matrix-vector products over the STANDARD fragment image (pack.h qnnp_pack_igemm_w): one (32 columns x 32 K)
 *            fragment is 1 KiB, lane l of a wave reads its 16 bytes -- column l % 32, K half l / 32 -- as one dwordx4, the
 *            wave 1 KiB contiguous; the activations are a 16-byte LDS read that 32 lanes share; four v_dot4_i32_i8 for
 *            the products and four more against 0x01010101 for the row sum that carries the kernel zero point. The two
 *            K halves meet through one cross-lane add. With fewer column blocks than waves the K blocks are dealt over
 *            the waves of a column block and summed through LDS;
 *   requant  the scalar exact q31_requantize (requant.hip.h).
 * The rows are kept in LDS RECENTRED (v ^ 0x80 = v - 128 as int8) and padded with zeros to k_pad, so neither the dot
 * product nor the row sum sees the padding (a raw row would be padded with 0x80).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "avgpool_math.hip.h"
#include "device_ops.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "requant.hip.h"

namespace qnnp {

namespace {

constexpr int kSeThreads = 1024;                  // one workgroup per image
constexpr int kSeWaves = kSeThreads / 64;
constexpr int kSePoolUnroll = 4;                  // pixels in flight per lane
constexpr uint32_t kSeRowBytes = (QNNP_HIP_SE_MAX_CHANNELS + 63u) / 64u * 64u;   // a row padded to k_pad
constexpr uint32_t kSeRedEntries = kSeWaves * 32; // K slices x n_pad <= waves x 32 columns

struct SeFc {
  const int8_t* w;
  const int32_t* bias2;
  uint32_t n;
  uint32_t n_pad, k_pad;
  int32_t row_coeff;
  RequantDev rq;
};

struct SeParams {
  const uint8_t* input;
  uint8_t* gate;
  uint64_t image_stride;      // bytes between images of `input`
  uint64_t input_stride;      // POOL: bytes between pixels
  uint32_t pixels;
  uint32_t channels;
  uint32_t squeeze;
  // POOL: lanes of a workgroup = [split pixel slices][1 << lanes_log2 channel vectors], `chunks` passes over the channels
  uint32_t lanes_log2;
  uint32_t split;
  uint32_t split_pow2;        // the power of two at or above split
  uint32_t chunks;
  qnnp_hip_avgpool_params pool;
  SeFc fc1, fc2;
  const uint8_t* table;
};

template <int VEC>
__device__ __forceinline__ void accumulate(int32_t (&acc)[VEC], const uint8_t* p)
{
  if constexpr (VEC == 4) {
    const uint32_t x = *reinterpret_cast<const uint32_t*>(p);
    acc[0] += x & 0xFFu;
    acc[1] += (x >> 8) & 0xFFu;
    acc[2] += (x >> 16) & 0xFFu;
    acc[3] += x >> 24;
  } else {
    acc[0] += p[0];
  }
}

/* row[c] = pooled byte ^ 0x80 for every channel of the image at `image` */
template <int VEC>
__device__ __forceinline__ void se_pool(const SeParams& p, const uint8_t* image, uint8_t* row, int32_t* partial)
{
  const uint32_t lanes = 1u << p.lanes_log2;
  const uint32_t lane_c = threadIdx.x & (lanes - 1u);       // channel vector inside the chunk
  const uint32_t slice = threadIdx.x >> p.lanes_log2;       // pixel slice
  const uint32_t split = p.split;
  for (uint32_t chunk = 0; chunk < p.chunks; chunk++) {
    const uint32_t c = (chunk * lanes + lane_c) * VEC;
    const bool live = c < p.channels && slice < split;
    int32_t acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) acc[i] = 0;
    if (live) {
      const uint8_t* px = image + c;
      uint32_t w = slice;                                   // (pixels * 255 fits an int32: no wrap below)
      for (; w + (kSePoolUnroll - 1) * split < p.pixels; w += kSePoolUnroll * split) {
        int32_t part[kSePoolUnroll][VEC];
#pragma unroll
        for (int u = 0; u < kSePoolUnroll; u++) {
#pragma unroll
          for (int i = 0; i < VEC; i++) part[u][i] = 0;
          accumulate<VEC>(part[u], px + static_cast<uint64_t>(w + u * split) * p.input_stride);
        }
#pragma unroll
        for (int u = 0; u < kSePoolUnroll; u++) {
#pragma unroll
          for (int i = 0; i < VEC; i++) acc[i] += part[u][i];
        }
      }
      for (; w < p.pixels; w += split) accumulate<VEC>(acc, px + static_cast<uint64_t>(w) * p.input_stride);
    }
    if (split > 1) {                                        // (then chunks == 1: `partial` is used once)
#pragma unroll
      for (int i = 0; i < VEC; i++) partial[threadIdx.x * VEC + i] = acc[i];
      __syncthreads();
      for (uint32_t s = p.split_pow2 >> 1; s > 0; s >>= 1) {
        if (slice < s && slice + s < split) {
#pragma unroll
          for (int i = 0; i < VEC; i++) partial[threadIdx.x * VEC + i] += partial[(threadIdx.x + s * lanes) * VEC + i];
        }
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < VEC; i++) acc[i] = partial[threadIdx.x * VEC + i];
    }
    if (live && slice == 0) {
#pragma unroll
      for (int i = 0; i < VEC; i++) {
        row[c + i] = static_cast<uint8_t>(avgpool_quantize(acc[i] + p.pool.bias, p.pool) ^ 0x80u);
      }
    }
  }
}

/* out(n, y) for every column n < f.n, y = requantize(bias2[n] + sum_k a'[k] w'(n, k) + row_coeff * sum_k a'[k]), `a` the
 * recentred row in LDS, zero padded to f.k_pad. Every thread of the workgroup calls it. */
template <typename Out>
__device__ __forceinline__ void se_fc(const SeFc& f, const uint8_t* a, int32_t* red, Out&& out)
{
  const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
  const uint32_t col = lane % 32u, half = lane / 32u;
  const uint32_t nblocks = f.n_pad / 32u, kblocks = f.k_pad / 32u;
  // this lane's share of column block nb over the K blocks kb0, kb0 + kstep, ..., both K halves added
  const auto share = [&](uint32_t nb, uint32_t kb0, uint32_t kstep) -> int32_t {
    const v4i* wp = reinterpret_cast<const v4i*>(f.w) + static_cast<size_t>(nb) * kblocks * 64u + lane;
    const uint8_t* ap = a + half * 16u;
    int32_t acc = 0, rs = 0;
#pragma unroll 4
    for (uint32_t kb = kb0; kb < kblocks; kb += kstep) {
      const v4i w = wp[static_cast<size_t>(kb) * 64u];
      const v4i x = *reinterpret_cast<const v4i*>(ap + kb * 32u);
      acc = __builtin_amdgcn_sdot4(x.x, w.x, acc, false);
      acc = __builtin_amdgcn_sdot4(x.y, w.y, acc, false);
      acc = __builtin_amdgcn_sdot4(x.z, w.z, acc, false);
      acc = __builtin_amdgcn_sdot4(x.w, w.w, acc, false);
      rs = __builtin_amdgcn_sdot4(x.x, 0x01010101, rs, false);
      rs = __builtin_amdgcn_sdot4(x.y, 0x01010101, rs, false);
      rs = __builtin_amdgcn_sdot4(x.z, 0x01010101, rs, false);
      rs = __builtin_amdgcn_sdot4(x.w, 0x01010101, rs, false);
    }
    const int32_t v = add_wrap(acc, static_cast<int32_t>(static_cast<uint32_t>(f.row_coeff) * static_cast<uint32_t>(rs)));
    return add_wrap(v, __shfl_xor(v, 32));
  };
  // K slices per column block: the waves that whole column blocks would leave idle
  uint32_t kslices = 1;
  if (nblocks < static_cast<uint32_t>(kSeWaves)) {
    kslices = static_cast<uint32_t>(kSeWaves) / nblocks;
    if (kslices > kblocks) kslices = kblocks;
  }
  if (kslices == 1) {
    for (uint32_t nb = wave; nb < nblocks; nb += kSeWaves) {
      const int32_t v = share(nb, 0, 1);
      const uint32_t n = nb * 32u + col;
      if (half == 0 && n < f.n) out(n, q31_requantize(add_wrap(f.bias2[n], v), f.rq));
    }
  } else {
    const uint32_t nb = wave / kslices, ks = wave - nb * kslices;
    if (nb < nblocks) {
      const int32_t v = share(nb, ks, kslices);
      if (half == 0) red[ks * f.n_pad + nb * 32u + col] = v;
    }
    __syncthreads();
    for (uint32_t n = threadIdx.x; n < f.n; n += kSeThreads) {
      int32_t v = f.bias2[n];
      for (uint32_t s = 0; s < kslices; s++) v = add_wrap(v, red[s * f.n_pad + n]);
      out(n, q31_requantize(v, f.rq));
    }
  }
}

/* grid x: images */
template <bool POOL, int VEC>
__global__ __launch_bounds__(kSeThreads)
void q8_se_gate_kernel(const SeParams p)
{
  __shared__ __attribute__((aligned(16))) uint8_t pooled[kSeRowBytes];   // p ^ 0x80, zero padded to fc1.k_pad
  __shared__ __attribute__((aligned(16))) uint8_t hidden[kSeRowBytes];   // h ^ 0x80, zero padded to fc2.k_pad
  __shared__ uint32_t table[64];
  __shared__ int32_t partial[POOL ? kSeThreads * VEC : 1];
  __shared__ int32_t red[kSeRedEntries];

  const uint8_t* image = p.input + static_cast<uint64_t>(blockIdx.x) * p.image_stride;
  if (threadIdx.x < 64u) table[threadIdx.x] = reinterpret_cast<const uint32_t*>(p.table)[threadIdx.x];
  for (uint32_t c = p.channels + threadIdx.x; c < p.fc1.k_pad; c += kSeThreads) pooled[c] = 0;
  for (uint32_t c = p.squeeze + threadIdx.x; c < p.fc2.k_pad; c += kSeThreads) hidden[c] = 0;
  if constexpr (POOL) {
    se_pool<VEC>(p, image, pooled, partial);
  } else {
    for (uint32_t c = threadIdx.x; c < p.channels; c += kSeThreads) pooled[c] = image[c] ^ 0x80u;
  }
  __syncthreads();
  se_fc(p.fc1, pooled, red, [&](uint32_t n, int32_t y) { hidden[n] = static_cast<uint8_t>(static_cast<uint32_t>(y) ^ 0x80u); });
  __syncthreads();
  uint8_t* gate = p.gate + static_cast<uint64_t>(blockIdx.x) * p.channels;
  const uint8_t* table8 = reinterpret_cast<const uint8_t*>(table);
  se_fc(p.fc2, hidden, red, [&](uint32_t c, int32_t y) { gate[c] = table8[static_cast<uint32_t>(y) & 0xFFu]; });
}

inline bool se_fc_valid(const qnnp_hip_se_fc& f, uint32_t k, uint32_t n)
{
  return f.w != nullptr && f.bias2 != nullptr && f.k_pad % 64u == 0 && f.n_pad % 32u == 0 && f.k_pad >= k &&
      f.k_pad <= kSeRowBytes && f.n_pad >= n && reinterpret_cast<uintptr_t>(f.w) % 16u == 0 &&
      reinterpret_cast<uintptr_t>(f.bias2) % 4u == 0;
}

inline SeFc se_fc_dev(const qnnp_hip_se_fc& f, uint32_t n)
{
  SeFc d;
  d.w = f.w;
  d.bias2 = f.bias2;
  d.n = n;
  d.n_pad = f.n_pad;
  d.k_pad = f.k_pad;
  d.row_coeff = f.row_coeff;
  d.rq = make_requant_dev(f.rq);
  return d;
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_se_gate_run(const struct qnnp_hip_se_gate_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->gate == nullptr || a->table == nullptr ||
      reinterpret_cast<uintptr_t>(a->table) % 4u != 0 || a->channels == 0 || a->squeeze == 0 ||
      a->channels > QNNP_HIP_SE_MAX_CHANNELS || a->squeeze > QNNP_HIP_SE_MAX_CHANNELS || a->batch > 0x7FFFFFFFu ||
      !se_fc_valid(a->fc1, a->channels, a->squeeze) || !se_fc_valid(a->fc2, a->squeeze, a->channels)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->pool != 0 && (a->pixels == 0 || a->pixels > 0x7FFFFFFFu / 255u || a->input_stride < a->channels ||
                       static_cast<uint64_t>(a->batch) * a->pixels > 0x7FFFFFFFu)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->batch == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());

  SeParams p;
  p.input = a->input;
  p.gate = a->gate;
  p.input_stride = a->input_stride;
  p.image_stride = a->pool != 0 ? static_cast<uint64_t>(a->pixels) * a->input_stride : a->channels;
  p.pixels = a->pixels;
  p.channels = a->channels;
  p.squeeze = a->squeeze;
  p.pool = a->pool_params;
  p.fc1 = se_fc_dev(a->fc1, a->squeeze);
  p.fc2 = se_fc_dev(a->fc2, a->channels);
  p.table = a->table;
  p.lanes_log2 = 0;
  p.split = p.split_pow2 = p.chunks = 1;

  const dim3 grid(a->batch), block(kSeThreads);
  if (a->pool == 0) {
    hipLaunchKernelGGL((q8_se_gate_kernel<false, 1>), grid, block, 0, stream, p);
    if (kernel_name != nullptr) *kernel_name = "q8_se_gate";
    return launch_status();
  }
  const bool vec4 = a->channels % 4u == 0 && a->input_stride % 4u == 0 && reinterpret_cast<uintptr_t>(a->input) % 4u == 0;
  const uint32_t cvecs = vec4 ? a->channels / 4u : a->channels;          // channel vectors per image
  while ((1u << p.lanes_log2) < cvecs && (1u << p.lanes_log2) < static_cast<uint32_t>(kSeThreads)) p.lanes_log2++;
  const uint32_t lanes = 1u << p.lanes_log2;
  p.chunks = (cvecs + lanes - 1u) / lanes;
  p.split = static_cast<uint32_t>(kSeThreads) / lanes;
  if (p.split > a->pixels) p.split = a->pixels;
  while (p.split_pow2 < p.split) p.split_pow2 *= 2u;
  if (vec4) {
    hipLaunchKernelGGL((q8_se_gate_kernel<true, 4>), grid, block, 0, stream, p);
  } else {
    hipLaunchKernelGGL((q8_se_gate_kernel<true, 1>), grid, block, 0, stream, p);
  }
  if (kernel_name != nullptr) *kernel_name = "q8_se_gate_pool";
  return launch_status();
}
