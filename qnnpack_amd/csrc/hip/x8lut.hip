/*
 * x8lut.hip -- byte lookup table (x8), NC layout with pixel strides: y[c] = table[x[c]] for every byte of every pixel.
 *
 * Replaces x8lut_ukernel__scalar (reference src/x8lut/scalar.c) and the lut case of qnnp_run_operator
 * (src/operator-run.c:1017-1052), which serves the reference's sigmoid and leaky ReLU operators (their 256-byte tables
 * are built on the host at create: sigmoid.c, leaky-relu.c) and the generic table operator (lut.c).
 *
 * The kernels move bytes like the clamp kernels of x8shuffle.hip and keep their structure: contiguous tensors
 * (strides == channels, or one pixel) are one flat range; otherwise each row is walked on its own (row_map.hip.h).
 * Pieces are 16, 4 or 1 bytes, the largest size that divides both the distance between input and output and the
 * difference of their strides, so input and output pieces are aligned alike. Whole aligned pieces are loaded (an
 * aligned 16-byte piece never crosses a page, so the bytes beside a range's ends are readable; they are not used);
 * partial pieces at the ends of a range are stored byte by byte, so the bytes between strided pixels are never written.
 * In place (input == output, equal strides) a lane reads and writes only its own piece.
 *
 * The lookup: every workgroup copies the table into 256 bytes of LDS (64 lanes, one dword each) and meets at one
 * barrier BEFORE any lane leaves -- a lane without an item still takes part. A lane then reads one LDS byte per input
 * byte (ds_read_u8) and packs four of them into each dword it stores. No per-lane table, no scratch, no gather from
 * global memory. A lane issues the load of its first piece before the table is staged, and of each later piece before
 * it looks the current one up, so neither the table fetch and the barrier nor the LDS reads stand between a workgroup
 * and its global loads (measured: profiles/lut/README.md).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "lut_lookup.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "row_map.hip.h"

namespace qnnp {

namespace {

/* Tensors are addressed as integers (aligned pieces start before a row does), which hides from the compiler that they
 * are global memory; it would emit flat loads and stores, which it can only wait for all at once (a flat access may go
 * to LDS), so a load issued ahead would be waited for at once. These say what the addresses are. */
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ T global_load(uintptr_t a)
{
  return *reinterpret_cast<const __attribute__((address_space(1))) T*>(a);
}
template <typename T>
__device__ __forceinline__ void global_store(uintptr_t a, T v)
{
  *reinterpret_cast<__attribute__((address_space(1))) T*>(a) = v;
}

/* (stage_table and lut_u8x4: lut_lookup.hip.h, shared with the table flavours of the convolution kernels) */

/* one VEC-byte input piece in registers (VEC == 1: the byte) */
template <int VEC>
struct Piece {
  uint32_t v[VEC >= 4 ? VEC / 4 : 1];
};

/* the aligned input piece at in_a */
template <int VEC>
__device__ __forceinline__ Piece<VEC> load_piece(uintptr_t in_a)
{
  Piece<VEC> x;
  if constexpr (VEC == 16) {
    const u32x4 q = global_load<u32x4>(in_a);
    x.v[0] = q.x; x.v[1] = q.y; x.v[2] = q.z; x.v[3] = q.w;
  } else if constexpr (VEC == 4) {
    x.v[0] = global_load<uint32_t>(in_a);
  } else {
    x.v[0] = global_load<uint8_t>(in_a);
  }
  return x;
}

/* the VEC-byte piece of output at address a (VEC-aligned) from the input piece x; only bytes in [lo, hi) are stored */
template <int VEC>
__device__ __forceinline__ void store_piece(const uint8_t (&lds)[256], Piece<VEC> x, uintptr_t a, uintptr_t lo, uintptr_t hi)
{
  if constexpr (VEC == 1) {
    global_store<uint8_t>(a, lds[x.v[0]]);
  } else {
    constexpr int D = VEC / 4;
#pragma unroll
    for (int i = 0; i < D; i++) x.v[i] = lut_u8x4(lds, x.v[i]);
    if (a >= lo && a + VEC <= hi) {
      if constexpr (VEC == 16) {
        u32x4 q;
        q.x = x.v[0]; q.y = x.v[1]; q.z = x.v[2]; q.w = x.v[3];
        global_store<u32x4>(a, q);
      } else {
        global_store<uint32_t>(a, x.v[0]);
      }
    } else {
#pragma unroll
      for (int b = 0; b < VEC; b++) {
        if (a + b >= lo && a + b < hi) global_store<uint8_t>(a + b, static_cast<uint8_t>(x.v[b / 4] >> (8 * (b % 4))));
      }
    }
  }
}

/* contiguous tensors: the bytes [output, output + bytes) in VEC-aligned pieces, grid-stride */
template <int VEC>
__global__ __launch_bounds__(kThreads)
void x8_lut_flat_kernel(const qnnp_hip_lut_args p, const uint64_t bytes, const uint64_t pieces)
{
  __shared__ alignas(16) uint8_t lds[256];
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p.output);
  const uintptr_t delta = reinterpret_cast<uintptr_t>(p.input) - lo;      // a multiple of VEC (mod 2^64)
  const uintptr_t base = lo & ~static_cast<uintptr_t>(VEC - 1);
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  Piece<VEC> cur = {};
  if (i < pieces) cur = load_piece<VEC>(base + i * VEC + delta);          // in flight while the table is staged
  stage_table(lds, p.table);
  while (i < pieces) {
    const uint64_t next = i + step;
    // unconditional (the last pass fetches its own piece again), so that the wait below can leave this load in flight
    const Piece<VEC> ahead = load_piece<VEC>(base + (next < pieces ? next : i) * VEC + delta);
    store_piece<VEC>(lds, cur, base + i * VEC, lo, lo + bytes);
    cur = ahead;
    i = next;
  }
}

/* strided tensors: item k of a row = the k-th VEC-aligned piece touching the output row */
template <int VEC>
__global__ __launch_bounds__(kThreads)
void x8_lut_rows_kernel(const qnnp_hip_lut_args p, const RowMap m)
{
  __shared__ alignas(16) uint8_t lds[256];
  uint32_t rl, k;
  const bool has = row_item(m, rl, k);
  struct Where {
    uintptr_t a, in_a, lo, hi;
    bool live;
  };
  /* this lane's piece in row group grp; not live: no such row, or the piece lies past the row's end */
  const auto locate = [&](uint32_t grp) {
    Where w = {0, 0, 0, 0, false};
    const uint32_t r = grp * m.rows_per_block + rl;
    if (has && grp < m.groups && r < m.rows) {
      const uintptr_t orow = reinterpret_cast<uintptr_t>(p.output + static_cast<uint64_t>(r) * p.output_stride);
      const uintptr_t irow = reinterpret_cast<uintptr_t>(p.input + static_cast<uint64_t>(r) * p.input_stride);
      w.a = (orow & ~static_cast<uintptr_t>(VEC - 1)) + static_cast<uintptr_t>(k) * VEC;
      w.in_a = w.a + (irow - orow);
      w.lo = orow;
      w.hi = orow + p.channels;
      w.live = w.a < w.hi;
    }
    return w;
  };
  uint32_t grp = blockIdx.y;
  Where w = locate(grp);
  Piece<VEC> cur = {};
  if (w.live) cur = load_piece<VEC>(w.in_a);                              // in flight while the table is staged
  stage_table(lds, p.table);
  if (!has) return;                                                       // after the barrier
  while (grp < m.groups) {
    const uint32_t next = grp + gridDim.y;
    const Where wn = locate(next);
    Piece<VEC> ahead = {};
    if (wn.live) ahead = load_piece<VEC>(wn.in_a);
    if (w.live) store_piece<VEC>(lds, cur, w.a, w.lo, w.hi);
    w = wn;
    cur = ahead;
    grp = next;
  }
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_lut_run(const struct qnnp_hip_lut_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->output == nullptr || a->table == nullptr || a->channels == 0 ||
      a->channels > 0x7FFFFFFFu || a->input_stride < a->channels || a->output_stride < a->channels ||
      a->pixels > 0x7FFFFFFFu || !aligned(address(a->table), 4)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->pixels == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const uint64_t delta = address(a->input) - address(a->output);
  // the reference takes its contiguous path under the same condition (src/operator-run.c:1024)
  const bool flat = a->pixels == 1 || (a->input_stride == a->channels && a->output_stride == a->channels);
  const uint64_t stride_delta = flat ? 0 : a->input_stride - a->output_stride;
  const int vec = aligned(delta, 16) && aligned(stride_delta, 16) ? 16 : (aligned(delta, 4) && aligned(stride_delta, 4) ? 4 : 1);
  const char* name = nullptr;
  if (flat) {
    const uint64_t bytes = static_cast<uint64_t>(a->pixels) * a->channels;
    const uint64_t pieces = (address(a->output) % vec + bytes + vec - 1) / vec;
    const uint64_t want = (pieces + kThreads - 1) / kThreads;
    const uint32_t cap = active_cu_count() * 16u;      // beyond it the grid-stride loop takes further passes
    const dim3 grid(static_cast<uint32_t>(want < cap ? want : cap));
    if (vec == 16) {
      hipLaunchKernelGGL(x8_lut_flat_kernel<16>, grid, dim3(kThreads), 0, stream, *a, bytes, pieces);
      name = "x8_lut_flat_x16";
    } else if (vec == 4) {
      hipLaunchKernelGGL(x8_lut_flat_kernel<4>, grid, dim3(kThreads), 0, stream, *a, bytes, pieces);
      name = "x8_lut_flat_x4";
    } else {
      hipLaunchKernelGGL(x8_lut_flat_kernel<1>, grid, dim3(kThreads), 0, stream, *a, bytes, pieces);
      name = "x8_lut_flat_x1";
    }
  } else {
    const uint32_t items = vec == 1 ? a->channels : (a->channels + 2u * vec - 2u) / vec;
    dim3 grid;
    const RowMap m = row_map(a->pixels, items, grid);
    if (vec == 16) {
      hipLaunchKernelGGL(x8_lut_rows_kernel<16>, grid, dim3(kThreads), 0, stream, *a, m);
      name = "x8_lut_rows_x16";
    } else if (vec == 4) {
      hipLaunchKernelGGL(x8_lut_rows_kernel<4>, grid, dim3(kThreads), 0, stream, *a, m);
      name = "x8_lut_rows_x4";
    } else {
      hipLaunchKernelGGL(x8_lut_rows_kernel<1>, grid, dim3(kThreads), 0, stream, *a, m);
      name = "x8_lut_rows_x1";
    }
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
