/*
 * f32topk.hip -- the top-k softmax router of a mixture-of-experts layer (moe.c; include/qnnpack_gfx950_moe.h has the
 * definition): per token the A largest of E logits, in descending order, as int32 ids minus first_group, and the softmax
 * over those A logits as float32 weights. No reference counterpart. Bit-exact: the clamp and the selection work on bit
 * patterns with integer instructions, the float operations are float32, each rounded once (contraction is off for the file),
 * and the division is the IEEE one.
 *
 * How the work is split. A token's logits live in the registers of one LANE GROUP of L lanes, V values per lane, both
 * compile-time: L * V >= E. A lane holds V / 4 quads; quad j of lane l is elements (j L + l) 4 .. + 3, so a wave's loads of
 * one j are contiguous and a quad is one 16-byte load. L and V follow from E alone:
 *   E <=   32: L =  8, V =  4    eight tokens per wave      f32_topk_l8_v4
 *   E <=   64: L = 16, V =  4    four                        f32_topk_l16_v4
 *   E <=  128: L = 32, V =  4    two                         f32_topk_l32_v4
 *   E <=  256: L = 64, V =  4    one wave per token          f32_topk_l64_v4
 *   E <=  512: L = 64, V =  8                                f32_topk_l64_v8
 *   E <= 1024: L = 64, V = 16                                f32_topk_l64_v16
 * Four values per lane at every E, not one: the per-lane part of a round is V compare-and-select pairs, which are cheap,
 * and the cross-lane part is log2(L) exchange steps, which are not; and eight lanes are the fewest that hold the A <= 8
 * results. A workgroup is four waves; the grid is the token count over the 256 / L tokens of a workgroup. Lane groups past
 * the last token load nothing and store nothing, but walk the exchanges with the others (no early exit in front of them).
 *
 * A round: every lane finds the largest (key, smallest index) among its V values (all register indices are static: the
 * loops are unrolled over V); log2(L) butterfly steps of __shfl_xor on the pair leave the group's winner in every lane;
 * the lane that holds it strikes it out by writing key 0, which is below the key of every clamped logit (the smallest,
 * that of -FLT_MAX, is 0x00800000), as are the padding positions from E on. A <= E, so a round always has a live entry.
 * Lane a of the group keeps round a's winner. After the A rounds lanes 0 .. A - 1 compute d, the exp lines and e_a; A
 * broadcasts give every lane the ordered sum S; the A ids and weights of a token leave in one contiguous store each.
 *
 * The logits are read once: whole quads below E with 16-byte loads, the one quad that E cuts (and, in the _x4 kernels --
 * base or, with more than one token, row stride no multiple of 16 bytes -- every quad) with 4-byte loads, nothing at or past
 * E. No LDS, no scratch memory; no matrix instruction fits a selection.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "per_device.h"
#include "qnnp_hip.h"

#pragma clang fp contract(off)

namespace qnnp {

namespace {

constexpr uint32_t kTopkThreads = 256;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct TopkParams {
  const uint32_t* logits;     // as bit patterns: nothing is a float before the clamp
  int32_t* ids;
  float* weights;
  uint64_t stride;            // elements
  uint32_t tokens, groups, assignments, first_group;
};

/* the header's c[e] and key, on bits: NaN and -inf -> -FLT_MAX, +inf -> FLT_MAX, everything else kept */
__device__ __forceinline__ uint32_t clamped_key(uint32_t bits)
{
  const uint32_t magnitude = bits & 0x7FFFFFFFu;
  uint32_t c = bits;
  c = magnitude == 0x7F800000u ? (bits & 0x80000000u) | 0x7F7FFFFFu : c;
  c = magnitude > 0x7F800000u ? 0xFF7FFFFFu : c;
  return c ^ ((c >> 31) != 0 ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float value_of_key(uint32_t key)
{
  return __uint_as_float(key ^ ((key >> 31) != 0 ? 0x80000000u : 0xFFFFFFFFu));
}

/* the header's e_a from y in [-80, 0]: the exp lines of the gated definition, constant for constant */
__device__ __forceinline__ float exp_of(float y)
{
  const float n = rintf(y * 0x1.715476p+0f);
  const float r1 = y - n * 0x1.62E400p-1f;               // the product is exact
  const float r2 = r1 - n * 0x1.7F7D1Cp-20f;
  float p = 0x1.0F9F9Cp-7f;
  p = p * r2;  p = p + 0x1.573A1Ap-5f;
  p = p * r2;  p = p + 0x1.555A80p-3f;
  p = p * r2;  p = p + 0x1.FFFDC6p-2f;
  p = p * r2;  p = p + 0x1.FFFFF6p-1f;
  p = p * r2;  p = p + 1.0f;
  return p * __int_as_float((static_cast<int>(n) + 127) << 23);     // n in [-116, 0]: a normal power of two
}

template <uint32_t L, uint32_t V, bool VEC>
__global__ __launch_bounds__(kTopkThreads)
void f32_topk_kernel(const TopkParams p)
{
  static_assert(L >= 8 && L <= 64 && (L & (L - 1)) == 0 && V % 4 == 0, "lane group");
  constexpr uint32_t kTokensPerBlock = kTopkThreads / L;
  const uint32_t l = threadIdx.x % L;
  const uint64_t token = static_cast<uint64_t>(blockIdx.x) * kTokensPerBlock + threadIdx.x / L;
  const bool live = token < p.tokens;
  const uint32_t* row = p.logits + (live ? token : 0) * p.stride;

  uint32_t key[V];
#pragma unroll
  for (uint32_t j = 0; j < V / 4; j++) {
    const uint32_t e0 = (j * L + l) * 4;
    if (VEC && live && e0 + 4 <= p.groups) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(row + e0);
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) key[4 * j + i] = clamped_key(q[i]);
    } else {
#pragma unroll
      for (uint32_t i = 0; i < 4; i++) key[4 * j + i] = live && e0 + i < p.groups ? clamped_key(row[e0 + i]) : 0u;
    }
  }

  uint32_t my_key = 0, my_index = 0, top_key = 0;
  for (uint32_t a = 0; a < p.assignments; a++) {
    uint32_t best_key = key[0], best_index = l * 4;
#pragma unroll
    for (uint32_t v = 1; v < V; v++) {                     // ascending index: > keeps the smallest among equals
      const uint32_t index = ((v / 4) * L + l) * 4 + v % 4;
      const bool better = key[v] > best_key;
      best_key = better ? key[v] : best_key;
      best_index = better ? index : best_index;
    }
#pragma unroll
    for (uint32_t step = L / 2; step >= 1; step /= 2) {
      const uint32_t other_key = static_cast<uint32_t>(__shfl_xor(static_cast<int>(best_key), static_cast<int>(step)));
      const uint32_t other_index = static_cast<uint32_t>(__shfl_xor(static_cast<int>(best_index), static_cast<int>(step)));
      const bool better = other_key > best_key || (other_key == best_key && other_index < best_index);
      best_key = better ? other_key : best_key;
      best_index = better ? other_index : best_index;
    }
#pragma unroll
    for (uint32_t v = 0; v < V; v++) {
      const uint32_t index = ((v / 4) * L + l) * 4 + v % 4;
      key[v] = index == best_index ? 0u : key[v];
    }
    top_key = a == 0 ? best_key : top_key;
    my_key = l == a ? best_key : my_key;
    my_index = l == a ? best_index : my_index;
  }

  // lanes from A on carry the top logit itself: d = 0, e = 1, never stored
  const float m = value_of_key(top_key);
  const float d = (l < p.assignments ? value_of_key(my_key) : m) - m;
  const float y = d < -80.0f ? -80.0f : d;
  const float e = exp_of(y);
  const int first_lane = static_cast<int>(threadIdx.x & 63u & ~(L - 1));
  float sum = 0.0f;
  for (uint32_t a = 0; a < p.assignments; a++) {
    const float e_a = __shfl(e, first_lane + static_cast<int>(a));
    sum = a == 0 ? e_a : sum + e_a;
  }
  const float w = e / sum;
  if (live && l < p.assignments) {
    const uint64_t at = token * p.assignments + l;
    p.ids[at] = static_cast<int32_t>(my_index) - static_cast<int32_t>(p.first_group);
    p.weights[at] = w;
  }
}

template <uint32_t L, uint32_t V>
void launch_topk(const TopkParams& p, bool vec, hipStream_t stream)
{
  const dim3 grid((p.tokens + kTopkThreads / L - 1) / (kTopkThreads / L));
  if (vec) hipLaunchKernelGGL((f32_topk_kernel<L, V, true>), grid, dim3(kTopkThreads), 0, stream, p);
  else hipLaunchKernelGGL((f32_topk_kernel<L, V, false>), grid, dim3(kTopkThreads), 0, stream, p);
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_topk_router_run(const struct qnnp_hip_topk_router_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->logits == nullptr || a->group_ids == nullptr || a->weights == nullptr ||
      ((reinterpret_cast<uintptr_t>(a->logits) | reinterpret_cast<uintptr_t>(a->group_ids) |
        reinterpret_cast<uintptr_t>(a->weights)) & 3u) != 0 ||
      a->groups == 0 || a->groups > 1024u || a->assignments == 0 || a->assignments > 8u || a->assignments > a->groups ||
      a->first_group >= 0x80000000u || a->logits_stride < a->groups ||
      static_cast<uint64_t>(a->tokens) * a->assignments >= (1u << 20)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->tokens == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  TopkParams p;
  p.logits = reinterpret_cast<const uint32_t*>(a->logits);
  p.ids = a->group_ids;
  p.weights = a->weights;
  p.stride = a->logits_stride;
  p.tokens = a->tokens;
  p.groups = a->groups;
  p.assignments = a->assignments;
  p.first_group = a->first_group;
  const bool vec = (reinterpret_cast<uintptr_t>(a->logits) & 15u) == 0 && (a->tokens == 1 || a->logits_stride % 4 == 0);
  const char* name;
  if (a->groups <= 32) {
    launch_topk<8, 4>(p, vec, stream);
    name = vec ? "f32_topk_l8_v4" : "f32_topk_l8_v4_x4";
  } else if (a->groups <= 64) {
    launch_topk<16, 4>(p, vec, stream);
    name = vec ? "f32_topk_l16_v4" : "f32_topk_l16_v4_x4";
  } else if (a->groups <= 128) {
    launch_topk<32, 4>(p, vec, stream);
    name = vec ? "f32_topk_l32_v4" : "f32_topk_l32_v4_x4";
  } else if (a->groups <= 256) {
    launch_topk<64, 4>(p, vec, stream);
    name = vec ? "f32_topk_l64_v4" : "f32_topk_l64_v4_x4";
  } else if (a->groups <= 512) {
    launch_topk<64, 8>(p, vec, stream);
    name = vec ? "f32_topk_l64_v8" : "f32_topk_l64_v8_x4";
  } else {
    launch_topk<64, 16>(p, vec, stream);
    name = vec ? "f32_topk_l64_v16" : "f32_topk_l64_v16_x4";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
