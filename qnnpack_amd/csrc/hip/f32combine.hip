/*
 * f32combine.hip -- the weighted combine behind the experts of a mixture-of-experts layer (moe.c;
 * include/qnnpack_gfx950_moe.h has the definition): output row t is the sum over a, in ascending order, of
 * weights[j] * input row j, j = t A + a, over the rows whose id lies in [0, groups), every product and every partial sum
 * flushed to a signed zero at or below 2^-126. No reference counterpart. Float32, every operation rounded once (contraction
 * is off for the file). One launch, streaming: every valid input byte is read once, every output byte written once.
 *
 * How the work is split. A workgroup owns ONE token and a run of columns, four per lane: grid (tokens, column chunks).
 *   f32_combine_wave    N <= 256: a workgroup is one wave and there is one chunk; at N = 128 half its lanes have a quad
 *   f32_combine_block   beyond: 256 lanes, 1024 columns per chunk (N = 2880: three chunks, the last 81 % full)
 * So the token's A ids and weights are uniform: they are fetched once, through the scalar cache, into scalar registers,
 * and whether row a counts is a scalar branch for the whole workgroup. A row that does not count is never addressed.
 * The loop over a is unrolled to the limit of eight: the quads of all rows that count are requested before the first
 * multiply, so up to eight 16-byte loads per lane are in flight, and the chain then runs in ascending a.
 * A lane whose quad lies wholly below N loads and stores 16 bytes; the one quad that N cuts moves dword by dword and touches
 * nothing at or past N; lanes past N leave at once. The _x4 kernels (a base, or with more than one row a stride, of the
 * input or the output that is no multiple of 16 bytes) move every quad dword by dword.
 * No LDS, no scratch memory; no matrix instruction fits an ordered sum of at most eight terms.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "per_device.h"
#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

constexpr uint32_t kMaxAssignments = 8;
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct CombineParams {
  const float* x;
  const float* weights;
  const int32_t* ids;
  float* y;
  uint64_t x_stride, y_stride;     // elements
  uint32_t assignments, groups, n;
};

__device__ __forceinline__ float flush(float v)
{
  return fabsf(v) <= 0x1.0p-126f ? copysignf(0.0f, v) : v;     // <=: what rounds to 2^-126 is a zero in either denormal mode
}

template <uint32_t THREADS, bool VEC>
__global__ __launch_bounds__(THREADS)
void f32_combine_kernel(const CombineParams p)
{
  const uint32_t c0 = (blockIdx.y * THREADS + threadIdx.x) * 4;
  if (c0 >= p.n) return;
  const uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * p.assignments;
  const bool whole = VEC && c0 + 4 <= p.n;

  bool counts[kMaxAssignments];
  float w[kMaxAssignments];
  f32x4 v[kMaxAssignments];
#pragma unroll
  for (uint32_t a = 0; a < kMaxAssignments; a++) {
    counts[a] = false;
    w[a] = 0.0f;
    v[a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (a < p.assignments) {                                    // (uniform)
      const int32_t id = p.ids[j0 + a];
      counts[a] = id >= 0 && static_cast<uint32_t>(id) < p.groups;
      if (counts[a]) {                                          // (uniform)
        w[a] = p.weights[j0 + a];
        const float* row = p.x + (j0 + a) * p.x_stride + c0;
        if (whole) {
          v[a] = *reinterpret_cast<const f32x4*>(row);
        } else {
#pragma unroll
          for (uint32_t i = 0; i < 4; i++) v[a][i] = c0 + i < p.n ? row[i] : 0.0f;
        }
      }
    }
  }

  f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (uint32_t a = 0; a < kMaxAssignments; a++) {
    if (counts[a]) {                                            // (uniform)
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) {
        const float product = flush(w[a] * v[a][i]);
        acc[i] = flush(acc[i] + product);
      }
    }
  }

  float* out = p.y + static_cast<uint64_t>(blockIdx.x) * p.y_stride + c0;
  if (whole) {
    *reinterpret_cast<f32x4*>(out) = acc;
  } else {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
      if (c0 + i < p.n) out[i] = acc[i];
    }
  }
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_weighted_combine_run(const struct qnnp_hip_weighted_combine_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->weights == nullptr || a->group_ids == nullptr || a->output == nullptr ||
      ((reinterpret_cast<uintptr_t>(a->input) | reinterpret_cast<uintptr_t>(a->weights) |
        reinterpret_cast<uintptr_t>(a->group_ids) | reinterpret_cast<uintptr_t>(a->output)) & 3u) != 0 ||
      a->channels == 0 || a->channels >= (1u << 24) || a->assignments == 0 || a->assignments > kMaxAssignments ||
      a->groups == 0 || a->groups > 1024u || a->input_stride < a->channels || a->output_stride < a->channels ||
      static_cast<uint64_t>(a->tokens) * a->assignments >= (1u << 20)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->tokens == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  CombineParams p;
  p.x = a->input;
  p.weights = a->weights;
  p.ids = a->group_ids;
  p.y = a->output;
  p.x_stride = a->input_stride;
  p.y_stride = a->output_stride;
  p.assignments = a->assignments;
  p.groups = a->groups;
  p.n = a->channels;
  const bool vec = (reinterpret_cast<uintptr_t>(a->input) & 15u) == 0 && (reinterpret_cast<uintptr_t>(a->output) & 15u) == 0 &&
      (static_cast<uint64_t>(a->tokens) * a->assignments == 1 || a->input_stride % 4 == 0) &&
      (a->tokens == 1 || a->output_stride % 4 == 0);
  const char* name;
  if (a->channels <= 256) {
    const dim3 grid(a->tokens, 1);
    if (vec) hipLaunchKernelGGL((f32_combine_kernel<64, true>), grid, dim3(64), 0, stream, p);
    else hipLaunchKernelGGL((f32_combine_kernel<64, false>), grid, dim3(64), 0, stream, p);
    name = vec ? "f32_combine_wave" : "f32_combine_wave_x4";
  } else {
    const dim3 grid(a->tokens, (a->channels + 1023u) / 1024u);      // at most 2^14 chunks
    if (vec) hipLaunchKernelGGL((f32_combine_kernel<256, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((f32_combine_kernel<256, false>), grid, dim3(256), 0, stream, p);
    name = vec ? "f32_combine_block" : "f32_combine_block_x4";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
