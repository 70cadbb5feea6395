/*
 * q8softargmax.hip -- softargmax over rows of uint8 (NC layout with row strides). For each row, all in uint32_t:
 *
 *   m    = max_c x[c]
 *   t_c  = table[x[c] + (255 - m)]                        table: 256 uint32_t made on the host at create (softargmax.c)
 *   vsum = sum_c t_c  (mod 2^32)                          the reference's sum WRAPS for rows of more than 512 channels
 *   y[c] = min(((t_c << 8) + (vsum >> 1)) / vsum, 255)    exact floor division (softargmax_math.h)
 *
 * Replaces u8rmax_ukernel__sse2, u8lut32norm_ukernel__scalar (reference src/u8lut32norm/scalar.c) and the softargmax
 * case of qnnp_run_operator (src/operator-run.c:625-637, 1091-1108), bit for bit, wrapped sums included: the sums here
 * are uint32_t additions, which are associative modulo 2^32, so the order of a reduction does not matter.
 *
 * vsum == 0 (mod 2^32) is where the reference is undefined: it divides by zero and dies (its assert is compiled out).
 * Here such a row's output is all 0. The sum can only be 0 modulo 2^32 by being at least 2^32, and every t_c << 8 is
 * below 2^31, so that is the quotient of the sum that did not wrap. The kernels test for it and never divide by zero.
 *
 * Which channel count takes which kernel (the thresholds are the two macros below and appear in the kernel names):
 *   1 .. 1024        q8_softargmax_group1024_x{16,1}: the row lives in registers. A power-of-two group of 1 .. 64 lanes
 *                    serves a row -- the smallest group whose lanes hold the row's pieces, 2 pieces of 16 bytes or 16
 *                    single bytes a lane -- so a wave carries 1 .. 64 rows and a workgroup 4 .. 256. With 16-byte
 *                    pieces (a row of c channels touches up to (c + 30) / 16 of them): 1 lane up to 17 channels, 2 up to
 *                    49, 4 up to 113, 8 up to 241, 16 up to 497, 32 up to 1009, 64 beyond; with single bytes: 16
 *                    channels a lane. Max and sum are reduced inside the group with
 *                    __shfl_xor; there is no barrier in the loop over the rows.
 *   1025 .. 32768    q8_softargmax_lds32768_x{16,1}: a workgroup serves a row and keeps it in LDS (each lane its own
 *                    pieces, so the row itself needs no barrier); max and sum cross the four waves through LDS.
 *   beyond           q8_softargmax_stream_x{16,1}: the same kernel without the row in LDS: the row is read three times
 *                    (max, sum, output), the second and third time from L2 for any realistic row.
 * In the first two every input byte is read from memory once; in all three every output byte is written once.
 *
 * Pieces are 16 bytes where the distance between input and output and the difference of their strides are multiples
 * of 16, single bytes otherwise, aligned as in x8lut.hip: whole aligned pieces are loaded (an aligned 16-byte piece
 * never crosses a page, so the bytes beside a row's ends are readable; they are masked off), partial pieces at the ends
 * of a row are stored byte by byte, so the bytes between strided rows are never written. In place (input == output,
 * equal strides) a lane writes only pieces it alone has read, after its row's sum is complete.
 *
 * The table: every workgroup copies the 1 KiB table into LDS (256 lanes, one dword each) and meets at one barrier
 * before any lane leaves; a lane issues the global loads of its first pieces before that. Lookups are ds_read_b32 at
 * x + (255 - m).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_ops.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "row_map.hip.h"
#include "softargmax_math.h"

/* the row-size thresholds, here and nowhere else; the kernel names carry them (tests/_softargmax.py reads them there) */
#define QNNP_SOFTARGMAX_GROUP_MAX 1024    /* channels up to which a row lives in the registers of a lane group */
#define QNNP_SOFTARGMAX_LDS_MAX 32768     /* channels up to which a workgroup keeps the row in LDS */
#define QNNP_STR2(x) #x
#define QNNP_STR(x) QNNP_STR2(x)

namespace qnnp {

namespace {

constexpr uint32_t kGroupMax = QNNP_SOFTARGMAX_GROUP_MAX;
constexpr uint32_t kLdsMax = QNNP_SOFTARGMAX_LDS_MAX;
constexpr uint32_t kWave = 64;
constexpr uint32_t kWaves = kThreads / kWave;

/* pieces a lane of the group kernel holds */
template <int VEC>
constexpr uint32_t kLanePieces = VEC == 16 ? 2u : 16u;

/* pieces of VEC bytes that can touch a row of `channels` bytes at any alignment */
constexpr uint32_t row_pieces(uint32_t channels, uint32_t vec)
{
  return vec == 1 ? channels : (channels + 2u * vec - 2u) / vec;
}
static_assert(row_pieces(kGroupMax, 16) <= kWave * kLanePieces<16> && row_pieces(kGroupMax, 1) <= kWave * kLanePieces<1>,
              "a wave must hold the longest row of the group kernel");
static_assert(kLdsMax % 16 == 0 && kLdsMax + 16 + 1024 + 64 <= 65536, "table, row and reduction words within 64 KiB of LDS");

/* Tensors are addressed as integers (aligned pieces start before a row does); these say that the addresses are global
 * memory, as in x8lut.hip. */
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

/* the workgroup's copy of the table; every lane of the workgroup must call this (one barrier) */
__device__ __forceinline__ void stage_table(uint32_t (&lds)[256], const uint32_t* table)
{
  lds[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
}

/* one VEC-byte input piece in registers (VEC == 1: the byte) */
template <int VEC>
struct Piece {
  uint32_t v[VEC >= 4 ? VEC / 4 : 1];
};

template <int VEC>
__device__ __forceinline__ Piece<VEC> load_piece(uintptr_t in_a)
{
  Piece<VEC> x;
  if constexpr (VEC == 16) {
    const u32x4 q = global_load<u32x4>(in_a);
    x.v[0] = q.x; x.v[1] = q.y; x.v[2] = q.z; x.v[3] = q.w;
  } else {
    x.v[0] = global_load<uint8_t>(in_a);
  }
  return x;
}

/* One row: output bytes [lo, hi), the input `delta` bytes away, pieces counted from `base` = lo rounded down to VEC. */
struct Row {
  uintptr_t base, delta, lo, hi;
  bool live;
};

__device__ __forceinline__ Row locate_row(const qnnp_hip_softargmax_args& p, uint32_t r, bool live, uint32_t vec)
{
  Row w = {0, 0, 0, 0, live};
  if (live) {
    const uintptr_t orow = reinterpret_cast<uintptr_t>(p.output + static_cast<uint64_t>(r) * p.output_stride);
    const uintptr_t irow = reinterpret_cast<uintptr_t>(p.input + static_cast<uint64_t>(r) * p.input_stride);
    w.base = orow & ~static_cast<uintptr_t>(vec - 1);
    w.delta = irow - orow;
    w.lo = orow;
    w.hi = orow + p.channels;
  }
  return w;
}

/* The bytes [first, last) of the piece at output address a belong to the row (a < hi). */
template <int VEC>
__device__ __forceinline__ void piece_bounds(const Row& w, uintptr_t a, uint32_t& first, uint32_t& last)
{
  first = a < w.lo ? static_cast<uint32_t>(w.lo - a) : 0u;
  last = w.hi - a < static_cast<uintptr_t>(VEC) ? static_cast<uint32_t>(w.hi - a) : static_cast<uint32_t>(VEC);
}

/* the piece with the bytes outside [first, last) set to 0: they do not raise the max, and piece_sum knows of them */
template <int VEC>
__device__ __forceinline__ void mask_piece(Piece<VEC>& x, uint32_t first, uint32_t last)
{
  if constexpr (VEC > 1) {
    if (first != 0u || last != static_cast<uint32_t>(VEC)) {
#pragma unroll
      for (int i = 0; i < VEC / 4; i++) {
        const int s = static_cast<int>(first) - 4 * i;   // bytes of this dword below s are outside
        const int e = static_cast<int>(last) - 4 * i;    // bytes of this dword from e on are outside
        const uint32_t keep_from = s <= 0 ? 0xFFFFFFFFu : (s >= 4 ? 0u : 0xFFFFFFFFu << (8 * s));
        const uint32_t keep_to = e >= 4 ? 0xFFFFFFFFu : (e <= 0 ? 0u : ~(0xFFFFFFFFu << (8 * e)));
        x.v[i] &= keep_from & keep_to;
      }
    }
  }
}

template <int VEC>
__device__ __forceinline__ uint32_t piece_max(const Piece<VEC>& x)
{
  if constexpr (VEC == 1) {
    return x.v[0];
  } else {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < VEC / 4; i++) {
      const uint32_t v = x.v[i];
      m = max(max(m, v & 0xFFu), max((v >> 8) & 0xFFu, max((v >> 16) & 0xFFu, v >> 24)));
    }
    return m;
  }
}

/* sum of table[x + adj] over the bytes [first, last) of a masked piece: the masked bytes look table[adj] (= t0) up */
template <int VEC>
__device__ __forceinline__ uint32_t piece_sum(const uint32_t (&table)[256], const Piece<VEC>& x, uint32_t adj, uint32_t t0,
                                              uint32_t first, uint32_t last)
{
  if constexpr (VEC == 1) {
    return table[x.v[0] + adj];
  } else {
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < VEC / 4; i++) {
      const uint32_t v = x.v[i];
      s += table[(v & 0xFFu) + adj] + table[((v >> 8) & 0xFFu) + adj] + table[((v >> 16) & 0xFFu) + adj] + table[(v >> 24) + adj];
    }
    return s - (static_cast<uint32_t>(VEC) - (last - first)) * t0;
  }
}

/* what a row's lanes need to turn table entries into output bytes */
struct Norm {
  uint32_t adj;        // 255 - m
  uint32_t rounding;   // vsum >> 1
  uint32_t keep;       // 0xFF, or 0 for a row whose sum is 0 modulo 2^32: its output is all 0
  qnnp_softargmax_divisor div;
};

__device__ __forceinline__ Norm make_norm(uint32_t adj, uint32_t vsum)
{
  Norm n;
  n.adj = adj;
  n.rounding = vsum >> 1;
  n.keep = vsum != 0u ? 0xFFu : 0u;
  n.div = qnnp_softargmax_divisor_init(vsum != 0u ? vsum : 1u);   // never a division by zero
  return n;
}

__device__ __forceinline__ uint32_t output_byte(const uint32_t (&table)[256], uint32_t x, const Norm& n)
{
  return qnnp_softargmax_normalize(table[x + n.adj], n.rounding, n.div) & n.keep;
}

/* the output piece at address a from the masked input piece x; only the bytes [first, last) are stored */
template <int VEC>
__device__ __forceinline__ void store_piece(const uint32_t (&table)[256], const Piece<VEC>& x, const Norm& n, uintptr_t a,
                                            uint32_t first, uint32_t last)
{
  if constexpr (VEC == 1) {
    global_store<uint8_t>(a, static_cast<uint8_t>(output_byte(table, x.v[0], n)));
  } else {
    uint32_t y[VEC / 4];
#pragma unroll
    for (int i = 0; i < VEC / 4; i++) {
      const uint32_t v = x.v[i];
      y[i] = output_byte(table, v & 0xFFu, n) | output_byte(table, (v >> 8) & 0xFFu, n) << 8 |
             output_byte(table, (v >> 16) & 0xFFu, n) << 16 | output_byte(table, v >> 24, n) << 24;
    }
    if (first == 0u && last == static_cast<uint32_t>(VEC)) {
      u32x4 q;
      q.x = y[0]; q.y = y[1]; q.z = y[2]; q.w = y[3];
      global_store<u32x4>(a, q);
    } else {
#pragma unroll
      for (int b = 0; b < VEC; b++) {
        if (static_cast<uint32_t>(b) >= first && static_cast<uint32_t>(b) < last) {
          global_store<uint8_t>(a + b, static_cast<uint8_t>(y[b / 4] >> (8 * (b % 4))));
        }
      }
    }
  }
}

/*
 * Rows of up to kGroupMax channels: `lanes` (a power of two, 1 << lanes_log2) lanes per row, piece j * lanes + g of the
 * row in slot j of lane g. Workgroup `grp` takes the kThreads / lanes rows from grp * (kThreads / lanes) on; the grid
 * strides over the `groups` of them. Every lane stays in the loop (a lane without a row or a piece takes part in the
 * shuffles with 0), and the pieces of the next group are in flight while this one is worked on.
 */
template <int VEC>
__global__ __launch_bounds__(kThreads)
void q8_softargmax_group_kernel(const qnnp_hip_softargmax_args p, const uint32_t lanes, const uint32_t lanes_log2,
                                const uint32_t groups)
{
  constexpr int P = static_cast<int>(kLanePieces<VEC>);
  __shared__ uint32_t table[256];
  const uint32_t rows_per_block = static_cast<uint32_t>(kThreads) >> lanes_log2;
  const uint32_t rl = threadIdx.x >> lanes_log2;
  const uint32_t g = threadIdx.x & (lanes - 1u);
  const auto locate = [&](uint32_t grp) {
    const uint32_t r = grp * rows_per_block + rl;          // below 2^31 + kThreads
    return locate_row(p, r, grp < groups && r < p.rows, VEC);
  };
  const auto address_of = [&](const Row& w, int j) {
    return w.base + static_cast<uintptr_t>((static_cast<uint32_t>(j) * lanes + g) * static_cast<uint32_t>(VEC));
  };
  const auto fetch = [&](const Row& w, Piece<VEC> (&x)[P]) {
#pragma unroll
    for (int j = 0; j < P; j++) {
      const uintptr_t a = address_of(w, j);
      x[j] = Piece<VEC>{};
      if (w.live && a < w.hi) x[j] = load_piece<VEC>(a + w.delta);
    }
  };
  uint32_t grp = blockIdx.x;
  Row w = locate(grp);
  Piece<VEC> x[P];
  fetch(w, x);                                             // in flight while the table is staged
  stage_table(table, p.table);
  while (grp < groups) {
    const uint32_t next = grp + gridDim.x;
    const Row wn = locate(next);
    Piece<VEC> ahead[P];
    fetch(wn, ahead);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < P; j++) {
      const uintptr_t a = address_of(w, j);
      if (w.live && a < w.hi) {
        uint32_t first, last;
        piece_bounds<VEC>(w, a, first, last);
        mask_piece<VEC>(x[j], first, last);
        m = max(m, piece_max<VEC>(x[j]));
      }
    }
    for (uint32_t off = 1; off < lanes; off <<= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(m, off)));
    const uint32_t adj = 255u - m;
    const uint32_t t0 = table[adj];
    uint32_t vsum = 0;
#pragma unroll
    for (int j = 0; j < P; j++) {
      const uintptr_t a = address_of(w, j);
      if (w.live && a < w.hi) {
        uint32_t first, last;
        piece_bounds<VEC>(w, a, first, last);
        vsum += piece_sum<VEC>(table, x[j], adj, t0, first, last);
      }
    }
    for (uint32_t off = 1; off < lanes; off <<= 1) vsum += static_cast<uint32_t>(__shfl_xor(vsum, off));
    const Norm n = make_norm(adj, vsum);
#pragma unroll
    for (int j = 0; j < P; j++) {
      const uintptr_t a = address_of(w, j);
      if (w.live && a < w.hi) {
        uint32_t first, last;
        piece_bounds<VEC>(w, a, first, last);
        store_piece<VEC>(table, x[j], n, a, first, last);
      }
    }
    w = wn;
#pragma unroll
    for (int j = 0; j < P; j++) x[j] = ahead[j];
    grp = next;
  }
}

/* max / wrapping sum over the workgroup: __shfl_xor inside each wave, then the four waves' words through LDS. One
 * barrier; every lane must call it. `red` must not be written again before the workgroup's next barrier. */
template <bool MAX>
__device__ __forceinline__ uint32_t block_reduce(uint32_t v, uint32_t (&red)[kWaves])
{
#pragma unroll
  for (uint32_t off = kWave / 2; off != 0; off >>= 1) {
    const uint32_t o = static_cast<uint32_t>(__shfl_xor(v, off));
    v = MAX ? max(v, o) : v + o;
  }
  if ((threadIdx.x & (kWave - 1u)) == 0u) red[threadIdx.x / kWave] = v;
  __syncthreads();
  return MAX ? max(max(red[0], red[1]), max(red[2], red[3])) : red[0] + red[1] + red[2] + red[3];
}

/*
 * Rows beyond kGroupMax channels: a workgroup per row, the grid strides over the rows; lane t takes the pieces t,
 * t + kThreads, ... of the row. STAGE: the masked pieces are kept in LDS between the passes -- slot k of the row buffer
 * is written and read by the lane that owns piece k only, so the buffer needs no barrier; without STAGE the pieces are
 * loaded again from memory. The two barriers of a row are those of the reductions: red_max is read before the second
 * and written again after it (in the next row), red_sum is read before the next row's first and written after it.
 */
template <int VEC, bool STAGE>
__global__ __launch_bounds__(kThreads)
void q8_softargmax_block_kernel(const qnnp_hip_softargmax_args p)
{
  __shared__ uint32_t table[256];
  __shared__ uint32_t red_max[kWaves], red_sum[kWaves];
  __shared__ alignas(16) uint8_t staged[STAGE ? kLdsMax + 16u : 16u];
  const uint32_t tid = threadIdx.x;
  const auto items_of = [&](const Row& w) { return static_cast<uint32_t>((w.hi - w.base + (VEC - 1)) / VEC); };
  const auto keep = [&](uint32_t k, const Piece<VEC>& x) {
    if constexpr (VEC == 16) {
      u32x4 q;
      q.x = x.v[0]; q.y = x.v[1]; q.z = x.v[2]; q.w = x.v[3];
      *reinterpret_cast<u32x4*>(&staged[k * 16u]) = q;
    } else {
      staged[k] = static_cast<uint8_t>(x.v[0]);
    }
  };
  /* the masked piece k of row w: from LDS, or (not STAGE) from memory again */
  const auto again = [&](const Row& w, uint32_t k, uint32_t first, uint32_t last) {
    Piece<VEC> x;
    if constexpr (STAGE) {
      if constexpr (VEC == 16) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(&staged[k * 16u]);
        x.v[0] = q.x; x.v[1] = q.y; x.v[2] = q.z; x.v[3] = q.w;
      } else {
        x.v[0] = staged[k];
      }
    } else {
      x = load_piece<VEC>(w.base + static_cast<uintptr_t>(k) * VEC + w.delta);
      mask_piece<VEC>(x, first, last);
    }
    return x;
  };
  /* this lane's first piece of row r (none: zeros), loaded ahead: for the workgroup's first row before the table is
   * staged, for every later row as soon as the pieces of the row before it have been fetched */
  const auto first_piece = [&](uint32_t r) {
    Piece<VEC> x = {};
    if (r < p.rows) {
      const Row w = locate_row(p, r, true, VEC);
      if (tid < items_of(w)) x = load_piece<VEC>(w.base + static_cast<uintptr_t>(tid) * VEC + w.delta);
    }
    return x;
  };
  Piece<VEC> head = first_piece(blockIdx.x);                // in flight while the table is staged
  stage_table(table, p.table);
  for (uint32_t r = blockIdx.x; r < p.rows; r += gridDim.x) {
    const Row w = locate_row(p, r, true, VEC);
    const uint32_t items = items_of(w);
    uint32_t m = 0;
    Piece<VEC> x = head;
    for (uint32_t k = tid; k < items; k += kThreads) {
      const uintptr_t a = w.base + static_cast<uintptr_t>(k) * VEC;
      // the next piece is in flight while this one is worked on
      Piece<VEC> ahead = {};
      if (k + kThreads < items) ahead = load_piece<VEC>(a + static_cast<uintptr_t>(kThreads) * VEC + w.delta);
      uint32_t first, last;
      piece_bounds<VEC>(w, a, first, last);
      mask_piece<VEC>(x, first, last);
      if constexpr (STAGE) keep(k, x);
      m = max(m, piece_max<VEC>(x));
      x = ahead;
    }
    head = first_piece(r + gridDim.x);                      // in flight during the reductions and the two passes below
    m = block_reduce<true>(m, red_max);
    const uint32_t adj = 255u - m;
    const uint32_t t0 = table[adj];
    uint32_t vsum = 0;
    for (uint32_t k = tid; k < items; k += kThreads) {
      const uintptr_t a = w.base + static_cast<uintptr_t>(k) * VEC;
      uint32_t first, last;
      piece_bounds<VEC>(w, a, first, last);
      vsum += piece_sum<VEC>(table, again(w, k, first, last), adj, t0, first, last);
    }
    vsum = block_reduce<false>(vsum, red_sum);
    const Norm n = make_norm(adj, vsum);
    for (uint32_t k = tid; k < items; k += kThreads) {
      const uintptr_t a = w.base + static_cast<uintptr_t>(k) * VEC;
      uint32_t first, last;
      piece_bounds<VEC>(w, a, first, last);
      store_piece<VEC>(table, again(w, k, first, last), n, a, first, last);
    }
  }
}

}  // namespace

}  // namespace qnnp

extern "C" int qnnp_hip_softargmax_run(const struct qnnp_hip_softargmax_args* a, const char** kernel_name)
{
  using namespace qnnp;
  if (a == nullptr || a->input == nullptr || a->output == nullptr || a->table == nullptr || a->channels == 0 ||
      a->channels > 0x7FFFFFFFu || a->input_stride < a->channels || a->output_stride < a->channels ||
      a->rows > 0x7FFFFFFFu || !aligned(address(a->table), 4)) {
    return QNNP_HIP_EINVAL;
  }
  if (a->rows == 0) return QNNP_HIP_OK;
  hipStream_t stream = reinterpret_cast<hipStream_t>(qnnp_hip_get_stream());
  const uint64_t delta = address(a->input) - address(a->output);
  const uint64_t stride_delta = a->rows == 1 ? 0 : a->input_stride - a->output_stride;
  const uint32_t vec = aligned(delta, 16) && aligned(stride_delta, 16) ? 16u : 1u;
  const uint32_t cus = active_cu_count();
  const char* name = nullptr;
  if (a->channels <= kGroupMax) {
    const uint32_t items = row_pieces(a->channels, vec);
    const uint32_t lane_pieces = vec == 16 ? kLanePieces<16> : kLanePieces<1>;
    uint32_t lanes = 1, lanes_log2 = 0;
    while (lanes * lane_pieces < items) {
      lanes <<= 1;
      lanes_log2++;
    }
    const uint32_t rows_per_block = static_cast<uint32_t>(kThreads) / lanes;
    const uint32_t groups = (a->rows + rows_per_block - 1) / rows_per_block;
    const uint32_t cap = cus * 8u;                         // beyond it the loop over the row groups takes further passes
    const dim3 grid(groups < cap ? groups : cap);
    if (vec == 16) {
      hipLaunchKernelGGL(q8_softargmax_group_kernel<16>, grid, dim3(kThreads), 0, stream, *a, lanes, lanes_log2, groups);
      name = "q8_softargmax_group" QNNP_STR(QNNP_SOFTARGMAX_GROUP_MAX) "_x16";
    } else {
      hipLaunchKernelGGL(q8_softargmax_group_kernel<1>, grid, dim3(kThreads), 0, stream, *a, lanes, lanes_log2, groups);
      name = "q8_softargmax_group" QNNP_STR(QNNP_SOFTARGMAX_GROUP_MAX) "_x1";
    }
  } else {
    const uint32_t cap = cus * 4u;                         // beyond it the loop over the rows takes further passes
    const dim3 grid(a->rows < cap ? a->rows : cap);
    const bool stage = a->channels <= kLdsMax;
    if (stage && vec == 16) {
      hipLaunchKernelGGL((q8_softargmax_block_kernel<16, true>), grid, dim3(kThreads), 0, stream, *a);
      name = "q8_softargmax_lds" QNNP_STR(QNNP_SOFTARGMAX_LDS_MAX) "_x16";
    } else if (stage) {
      hipLaunchKernelGGL((q8_softargmax_block_kernel<1, true>), grid, dim3(kThreads), 0, stream, *a);
      name = "q8_softargmax_lds" QNNP_STR(QNNP_SOFTARGMAX_LDS_MAX) "_x1";
    } else if (vec == 16) {
      hipLaunchKernelGGL((q8_softargmax_block_kernel<16, false>), grid, dim3(kThreads), 0, stream, *a);
      name = "q8_softargmax_stream_x16";
    } else {
      hipLaunchKernelGGL((q8_softargmax_block_kernel<1, false>), grid, dim3(kThreads), 0, stream, *a);
      name = "q8_softargmax_stream_x1";
    }
  }
  if (kernel_name != nullptr) *kernel_name = name;
  return launch_status();
}
