/*
 * q8mul.hip -- quantized multiply (q8), NC layout with row strides, with or without a broadcast of the second operand:
 *   product[r][c] = requantize((a[r][c] - a_zero_point) * (b[r / a_rows_per_b_row][c] - b_zero_point))
 * a_rows_per_b_row == 1 is the element-wise product; a_rows_per_b_row == the pixels of an image is the scale of a
 * squeeze-and-excite block (x * s, s one row per image). No reference counterpart.
 *
 * HBM-bound by construction: every byte of `a` is read once and every byte of the product written once, while the few
 * rows of `b` stay in L2 (each is re-read by every row of its image). So the kernels are about coalescing, like the add
 * of q8pointwise.hip and the table kernels of x8lut.hip: 256-thread workgroups, a grid-stride loop over row groups
 * capped by the compute-unit count, 64-bit byte offsets.
 *
 * A lane's piece is 16, 4 or 1 bytes OF ONE ROW -- a piece never straddles a row, so the row of `b` is one division per
 * piece (a host-made reciprocal), not one per byte. Short rows share a workgroup (lane -> (row, piece) by one magic
 * divide of the thread index, as row_map.hip.h does it); rows longer than a workgroup span gridDim.y workgroups.
 * The 16- and 4-byte kernels need the channel count, the three base addresses and the three strides to be multiples of
 * the piece; anything else runs byte by byte. In place (product == a, or product == b without a broadcast) a lane reads
 * and writes only its own piece.
 *
 * Arithmetic: the product of two zero-point-centred bytes is below 2^16 in magnitude (one v_mul_i32_i24), and the
 * down-convert is the convolutions' own (requant.hip.h): the rounding sequence and the clamp class are picked once per
 * launch by requant_dispatch, and the accumulator bound lets it take the bounded sequence.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "requant.hip.h"
#include "row_map.hip.h"

namespace qnnp {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct MulParams {
  const uint8_t* a;
  const uint8_t* b;
  uint8_t* product;
  uint64_t a_stride, b_stride, product_stride;
  uint32_t rows;            // rows of a and of the product (< 2^31)
  uint32_t pieces;          // pieces per row
  uint32_t pieces_inv;      // reciprocal_ceil(pieces) when pieces <= kThreads
  uint32_t rows_per_block;  // rows of one row group: kThreads / pieces, or 1 for rows longer than a workgroup
  uint32_t groups;          // ceil(rows / rows_per_block)
  uint32_t b_div;           // a_rows_per_b_row
  uint32_t b_magic;         // reciprocal_floor_plus1(b_div) when b_div > 1 and rows * b_div < 2^32, else 0: plain division
  int32_t a_zero_point, b_zero_point;
  RequantDev rq;
};

/* four products of one dword of a and one of b, requantized and packed (byte c of the result belongs to byte c) */
template <int SEQ, bool FULL>
__device__ __forceinline__ uint32_t mul_u8x4(uint32_t x, uint32_t y, const MulParams& p)
{
  const int32_t az = p.a_zero_point, bz = p.b_zero_point;
  const int32_t n0 = __mul24(static_cast<int32_t>(x & 0xFFu) - az, static_cast<int32_t>(y & 0xFFu) - bz);
  const int32_t n1 = __mul24(static_cast<int32_t>((x >> 8) & 0xFFu) - az, static_cast<int32_t>((y >> 8) & 0xFFu) - bz);
  const int32_t n2 = __mul24(static_cast<int32_t>((x >> 16) & 0xFFu) - az, static_cast<int32_t>((y >> 16) & 0xFFu) - bz);
  const int32_t n3 = __mul24(static_cast<int32_t>(x >> 24) - az, static_cast<int32_t>(y >> 24) - bz);
  return q31_requantize_pack4<SEQ, FULL>(n0, n1, n2, n3, p.rq);
}

/* one VEC-byte piece. STREAM (16-byte pieces, product not in place): `a` and the product are pure streams -- every line
 * read or written exactly once -- and carry the hint; `b` is re-read by every row of its image and never does. */
template <int VEC, bool STREAM, int SEQ, bool FULL>
__device__ __forceinline__ void mul_piece(const uint8_t* pa, const uint8_t* pb, uint8_t* pp, const MulParams& p)
{
  if constexpr (VEC == 16) {
    u32x4 x;
    if constexpr (STREAM) {
      x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pa));
    } else {
      x = *reinterpret_cast<const u32x4*>(pa);
    }
    const u32x4 y = *reinterpret_cast<const u32x4*>(pb);
    u32x4 z;
    z.x = mul_u8x4<SEQ, FULL>(x.x, y.x, p);
    z.y = mul_u8x4<SEQ, FULL>(x.y, y.y, p);
    QNNP_PIN();   // two dwords' values in flight, not four: interleaving all sixteen takes the kernel past 64 VGPRs
    z.z = mul_u8x4<SEQ, FULL>(x.z, y.z, p);
    z.w = mul_u8x4<SEQ, FULL>(x.w, y.w, p);
    if constexpr (STREAM) {
      __builtin_nontemporal_store(z, reinterpret_cast<u32x4*>(pp));
    } else {
      *reinterpret_cast<u32x4*>(pp) = z;
    }
  } else if constexpr (VEC == 4) {
    const uint32_t x = *reinterpret_cast<const uint32_t*>(pa);
    const uint32_t y = *reinterpret_cast<const uint32_t*>(pb);
    *reinterpret_cast<uint32_t*>(pp) = mul_u8x4<SEQ, FULL>(x, y, p);
  } else {
    const int32_t n = __mul24(static_cast<int32_t>(*pa) - p.a_zero_point, static_cast<int32_t>(*pb) - p.b_zero_point);
    *pp = static_cast<uint8_t>(q31_requantize_pack4<SEQ, FULL>(n, n, n, n, p.rq));
  }
}

/* grid x: row groups (grid-stride); grid y: the kThreads-piece chunks of a row longer than a workgroup (grid-stride) */
template <int VEC, bool STREAM>
__global__ __launch_bounds__(kThreads)
void q8_mul_kernel(const MulParams p)
{
  uint32_t rl = 0, k0 = blockIdx.y * kThreads + threadIdx.x;
  if (p.pieces <= static_cast<uint32_t>(kThreads)) {
    rl = div_magic(threadIdx.x, p.pieces_inv);
    k0 = threadIdx.x - rl * p.pieces;
    if (rl >= p.rows_per_block) return;
  }
  const uint32_t k_step = gridDim.y * kThreads;
  requant_dispatch(p.rq, [&](auto seq, auto full) {
    constexpr int SEQ = decltype(seq)::value;
    constexpr bool FULL = decltype(full)::value;
    for (uint32_t grp = blockIdx.x; grp < p.groups; grp += gridDim.x) {
      const uint32_t r = grp * p.rows_per_block + rl;       // < rows + kThreads: no wrap
      if (r >= p.rows) continue;                            // (the last group)
      const uint32_t br = p.b_div == 1u ? r : (p.b_magic != 0u ? __umulhi(r, p.b_magic) : r / p.b_div);
      const uint8_t* pa = p.a + static_cast<uint64_t>(r) * p.a_stride;
      const uint8_t* pb = p.b + static_cast<uint64_t>(br) * p.b_stride;
      uint8_t* pp = p.product + static_cast<uint64_t>(r) * p.product_stride;
      for (uint32_t k = k0; k < p.pieces; k += k_step) {
        const uint32_t c = k * VEC;                         // < channels < 2^31
        mul_piece<VEC, STREAM, SEQ, FULL>(pa + c, pb + c, pp + c, p);
      }
    }
  });
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_mul_run(const struct qnnp_hip_mul_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->a == nullptr || a->b == nullptr || a->product == nullptr || a->channels == 0 ||
      a->channels > 0x7FFFFFFFu || a->a_stride < a->channels || a->b_stride < a->channels ||
      a->product_stride < a->channels) {
    return QNNP_HIP_EINVAL;
  }
  const uint64_t rows = static_cast<uint64_t>(a->b_rows) * a->a_rows_per_b_row;
  if (rows > 0x7FFFFFFFu) return QNNP_HIP_EINVAL;
  if (rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());

  const auto all_aligned = [&](uint64_t n) {
    return aligned(a->channels, n) && aligned(address(a->a), n) && aligned(address(a->b), n) &&
        aligned(address(a->product), n) && aligned(a->a_stride, n) && aligned(a->b_stride, n) && aligned(a->product_stride, n);
  };
  const uint32_t vec = all_aligned(16) ? 16u : (all_aligned(4) ? 4u : 1u);

  MulParams p;
  p.a = a->a;
  p.b = a->b;
  p.product = a->product;
  p.a_stride = a->a_stride;
  p.b_stride = a->b_stride;
  p.product_stride = a->product_stride;
  p.rows = static_cast<uint32_t>(rows);
  p.pieces = a->channels / vec;
  const bool shared = p.pieces <= static_cast<uint32_t>(kThreads);
  p.pieces_inv = shared ? reciprocal_ceil(p.pieces) : 0u;
  p.rows_per_block = shared ? kThreads / p.pieces : 1u;
  p.groups = static_cast<uint32_t>((rows + p.rows_per_block - 1) / p.rows_per_block);
  p.b_div = a->a_rows_per_b_row;
  p.b_magic = (p.b_div > 1u && rows * p.b_div < (UINT64_C(1) << 32)) ? reciprocal_floor_plus1(p.b_div) : 0u;
  p.a_zero_point = a->a_zero_point;
  p.b_zero_point = a->b_zero_point;
  p.rq = make_requant_dev(a->rq);

  // beyond the cap the grid-stride loops take further passes
  const uint32_t cap = active_cu_count() * 16u;
  const uint32_t chunks = shared ? 1u : (p.pieces + kThreads - 1) / kThreads;
  const uint32_t gy = chunks < kMaxGridY ? (chunks < cap ? chunks : cap) : (cap < kMaxGridY ? cap : kMaxGridY);
  const uint32_t cap_x = cap / gy > 0 ? cap / gy : 1u;
  const dim3 grid(p.groups < cap_x ? p.groups : cap_x, gy);

  const bool in_place = a->product == a->a || a->product == a->b;
  const bool hint = a->streaming_mode == 0 ? qnnp_hip_streaming_stores() != 0 : a->streaming_mode == 2;
  const char* name = nullptr;
  if (vec == 16) {
    if (hint && !in_place) {
      hipLaunchKernelGGL((q8_mul_kernel<16, true>), grid, dim3(kThreads), 0, stream, p);
    } else {
      hipLaunchKernelGGL((q8_mul_kernel<16, false>), grid, dim3(kThreads), 0, stream, p);
    }
    name = "q8_mul_x16";
  } else if (vec == 4) {
    hipLaunchKernelGGL((q8_mul_kernel<4, false>), grid, dim3(kThreads), 0, stream, p);
    name = "q8_mul_x4";
  } else {
    hipLaunchKernelGGL((q8_mul_kernel<1, false>), grid, dim3(kThreads), 0, stream, p);
    name = "q8_mul_x1";
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
