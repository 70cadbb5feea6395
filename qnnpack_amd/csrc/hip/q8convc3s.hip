/*
 * q8convc3s.hip -- convolutions over 3-channel images on the streaming scheme: q8_conv_stream_c3_kernel and, for 16-byte
 * aligned output rows, q8_conv_stream_c3s_kernel<SEQ, FULL>. Network first layers in 4-byte tap slots (pack.h "channel
 * slots"), at most 16 taps, one group, any stride, dilation and padding: the offset-table sibling of q8convc3.hip's row-slot
 * kernels, which take dense undilated windows first. Plan and launch: convstream_c3_plan / convstream_c3_launch
 * (igemm_params.h); q8igemm.hip decides when it runs ("gemm_kernel" 7 forces it).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "pwstream_common.hip.h"

namespace qnnp {

namespace {

/*
 * Third flavour: convolutions over 3-channel images (network first layers, e.g. 3x3 stride 2, 3 -> 32). The
 * reduction is tiny (taps x 4-byte slots <= 64 bytes, pack.h "channel slots"), so the same barrier-free
 * scheme applies with an in-register gather: a lane fetches the (at most 8) taps of its K half with one
 * unaligned dword each -- addresses from the operator's offset table, padding taps and the slot's 4th byte
 * replaced in registers -- and multiplies against the LDS-resident weights. One wave = 32 consecutive
 * output pixels of the flattened (image, row, column) space.
 */
typedef uint32_t __attribute__((aligned(1))) pw_u32_unaligned;

__global__ __launch_bounds__(kThreads, 4)
void q8_conv_stream_c3_kernel(const IgemmParams p)
{
  constexpr int KB = 2;                                    // k_pad == 64: up to 16 taps of 4-byte slots
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  const uint32_t row_in_block = lane & 31u;
  const uint32_t khalf = lane >> 5;
  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;
  {
    const uint32_t frags = nblocks * KB;
    for (uint32_t f = wave; f < frags; f += kWaves) {
      const uint32_t nb = f / KB;
      const uint32_t kb = f - nb * KB;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (p.packed_w + (static_cast<uint64_t>(nb) * kblocks + kb) * 1024 + lane * 16),
          (__attribute__((address_space(3))) void*) (lds + f * 1024), 16, 0, 0);
    }
    uint8_t* lds_bias = lds + frags * 1024;
    const uint32_t bias_chunks = p.n_pad / 4;
    for (uint32_t c0 = wave * 64; c0 < bias_chunks; c0 += kThreads) {
      const uint32_t c = min(c0 + lane, bias_chunks - 1);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (reinterpret_cast<const uint8_t*>(p.bias2) + c * 16),
          (__attribute__((address_space(3))) void*) (lds_bias + c0 * 16), 16, 0, 0);
    }
    // (no wait here: the first unit's gather is issued first, so the latencies overlap)
  }
  const uint8_t* lds_w = lds + lane * 16;
  const int4* lds_bias4 = reinterpret_cast<const int4*>(lds + nblocks * KB * 1024);

  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t unit_stride = gridDim.x * kWaves;
  const uint32_t fillpix = p.izp_fill;                     // {izp, izp, izp, 0x80}: padding tap, 4th byte = K padding
  const uint32_t raw_to_centred = 128u * 32u * KB;

  // The gather is two dependent loads (offset-table entry, then the pixel). They are split so that the table
  // entries of unit u+2 and the pixels of unit u+1 are in flight while unit u is multiplied: no load waits on
  // another one issued in the same iteration.
  struct Taps { int32_t off[KB * 4]; const uint8_t* base; };
  auto load_offsets = [&](uint32_t unit, Taps& t) __attribute__((always_inline)) {
    uint32_t m = unit * 32u + row_in_block;
    if (m >= p.rows) m = p.rows - 1;                       // clamped rows are never stored
    const uint32_t img = m / p.rows_per_image;
    const uint32_t pix = m - img * p.rows_per_image;
    t.base = p.input + static_cast<uint64_t>(img) * p.image_stride;
    const int32_t* offs = p.offsets + static_cast<uint64_t>(pix) * p.ks;
#pragma unroll
    for (int i = 0; i < KB * 4; i++) {
      const uint32_t tap = (i >> 2) * 8 + khalf * 4 + (i & 3);     // kb*8 + khalf*4 + j
      t.off[i] = tap < p.ks ? offs[tap] : -2;                      // -2: beyond the kernel (K padding), -1: padding tap
    }
  };
  auto load_pixels = [&](const Taps& t, v4i (&a)[KB]) __attribute__((always_inline)) {
#pragma unroll
    for (int kb = 0; kb < KB; kb++) {
      uint32_t v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int32_t off = t.off[kb * 4 + j];
        const bool inside = off >= 0;
        const uint8_t* src = t.base + (inside ? off : 0);
        uint32_t x;
        if (src + 4 <= p.input_end) {
          x = *reinterpret_cast<const pw_u32_unaligned*>(src);
        } else {                                           // the very last pixel of the tensor: bytewise
          x = static_cast<uint32_t>(src[0]) | (static_cast<uint32_t>(src[1]) << 8) | (static_cast<uint32_t>(src[2]) << 16);
        }
        x = (x & 0x00FFFFFFu) | 0x80000000u;               // the slot's 4th byte is K padding: a' == 0
        v[j] = inside ? x : (off == -1 ? fillpix : 0x80808080u);
      }
      a[kb] = v4i{static_cast<int>(v[0]), static_cast<int>(v[1]), static_cast<int>(v[2]), static_cast<int>(v[3])};
    }
  };

  uint32_t unit = blockIdx.x * kWaves + wave;
  v4i a_next[KB];
  Taps t_next;
  if (unit < units) {
    load_offsets(unit, t_next);
    load_pixels(t_next, a_next);
    if (unit + unit_stride < units) load_offsets(unit + unit_stride, t_next);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // weights + bias are in LDS
  __syncthreads();

  requant_dispatch_ofs(p.rq, [&](auto shift0, auto full) {
    for (; unit < units; unit += unit_stride) {
      v4i a[KB];
#pragma unroll
      for (int kb = 0; kb < KB; kb++) a[kb] = a_next[kb];
      if (unit + unit_stride < units) {
        load_pixels(t_next, a_next);                       // offsets landed one iteration ago
        if (unit + 2 * unit_stride < units) load_offsets(unit + 2 * unit_stride, t_next);
      }

      uint32_t rs = 0;
#pragma unroll
      for (int kb = 0; kb < KB; kb++) {
        rs = __builtin_amdgcn_sad_u8(a[kb].x, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].y, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].z, 0u, rs);
        rs = __builtin_amdgcn_sad_u8(a[kb].w, 0u, rs);
        a[kb].x ^= static_cast<int>(kFlip);
        a[kb].y ^= static_cast<int>(kFlip);
        a[kb].z ^= static_cast<int>(kFlip);
        a[kb].w ^= static_cast<int>(kFlip);
      }
      rs += __shfl_xor(rs, 32);
      const int32_t rowterm = with_rq_offset<decltype(shift0)::value>(p.row_coeff * static_cast<int32_t>(rs - raw_to_centred));

      const uint32_t m = unit * 32u + row_in_block;
      uint8_t* out_row = p.output + static_cast<uint64_t>(m) * p.output_stride;
      const bool row_ok = m < p.rows;
      for (uint32_t nb = 0; nb < nblocks; nb++) {
        v16i acc;
        // (read per block, beside the weight fragment: carried over from the previous trip it cost 16 v_mov_b64 per block)
        int4 bias4[4];
#pragma unroll
        for (int rg = 0; rg < 4; rg++) bias4[rg] = lds_bias4[nb * 8 + rg * 2 + khalf];
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          acc[rg * 4 + 0] = bias4[rg].x; acc[rg * 4 + 1] = bias4[rg].y;
          acc[rg * 4 + 2] = bias4[rg].z; acc[rg * 4 + 3] = bias4[rg].w;
        }
        const uint8_t* wf = lds_w + nb * (KB * 1024);
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
          const v4i w = *reinterpret_cast<const v4i*>(wf + kb * 1024);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w, a[kb], acc, 0, 0, 0);
        }
        igemm_store_tile<decltype(shift0)::value, decltype(full)::value, false, 2>(
            acc, bias4, rowterm, out_row, nb * 32, khalf, row_ok, p);
      }
    }
  });
}

/*
 * The same gather for 16-byte aligned output rows (n % 16 == 0: every real first layer), built like the staged
 * pointwise kernel: every load of the loop is issued unconditionally (buffer loads: 32-bit offsets, clamped unit
 * index), the unit's block is requantized into a per-wave LDS image, and the one vmcnt wait sits between the
 * multiply phase and the unit's stores. Per unit and lane: 8 table entries + 8 pixel dwords (two units / one unit
 * ahead), ~4 vector instructions per tap -- the first version spent ~22 per tap on 64-bit addresses, per-load
 * branches and the bytewise tail, and waited for its "prefetched" loads at once (vmcnt(0) behind them: the branch
 * around each load made the outstanding count path-dependent).
 * The last pixel of the tensor cannot be read as a dword: units that may touch the last image take a flavour of the
 * gather that clamps the offset to the last whole dword and shifts (wave-uniform choice, both flavours issue the
 * same loads).
 */
template <int SEQ, bool FULL>       // the requantization flavour, chosen on the host (as the staged pointwise kernel)
__global__ __launch_bounds__(kThreads, 5)
void q8_conv_stream_c3s_kernel(const IgemmParams p, const uint32_t log_cpr)
{
  constexpr int KB = 2;                                    // k_pad == 64: up to 16 taps of 4-byte slots
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  const uint32_t row_in_block = lane & 31u;
  const uint32_t khalf = lane >> 5;
  const uint32_t nblocks = p.n_pad / 32;
  const uint32_t kblocks = p.k_pad / 32;
  const bool whole_dense = p.output_stride == p.n;
  const uint32_t pitch = whole_dense ? p.n : (16u << log_cpr);
  {
    const uint32_t frags = nblocks * KB;
    for (uint32_t f = wave; f < frags; f += kWaves) {
      const uint32_t nb = f / KB;
      const uint32_t kb = f - nb * KB;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (p.packed_w + (static_cast<uint64_t>(nb) * kblocks + kb) * 1024 + lane * 16),
          (__attribute__((address_space(3))) void*) (lds + f * 1024), 16, 0, 0);
    }
    uint8_t* lds_bias = lds + frags * 1024;
    const uint32_t bias_chunks = p.n_pad / 4;
    for (uint32_t c0 = wave * 64; c0 < bias_chunks; c0 += kThreads) {
      const uint32_t c = min(c0 + lane, bias_chunks - 1);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*) (reinterpret_cast<const uint8_t*>(p.bias2) + c * 16),
          (__attribute__((address_space(3))) void*) (lds_bias + c0 * 16), 16, 0, 0);
    }
  }
  const uint8_t* lds_w = lds + lane * 16;
  const uint32_t bias_bytes = (p.n_pad * 4u + 1023u) & ~1023u;
  const int4* lds_bias4 = reinterpret_cast<const int4*>(lds + nblocks * KB * 1024);
  uint8_t* stage = lds + nblocks * KB * 1024 + bias_bytes + wave * (32u * pitch);

  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t unit_stride = gridDim.x * kWaves;
  const uint32_t raw_to_centred = 128u * 32u * KB;
  const uint32_t in_bytes = static_cast<uint32_t>(p.input_end - p.input);          // (launcher: < 2^31)
  const __amdgpu_buffer_rsrc_t in_rsrc = buffer_rsrc(p.input, static_cast<int>(in_bytes));
  const __amdgpu_buffer_rsrc_t off_rsrc = buffer_rsrc(
      p.offsets, static_cast<int>(p.rows_per_image * p.ks * 4u + 16u));   // (+16: convolution.c allocates the slack)
  // first output row (flattened) whose window may hold the tensor's last pixel: conservatively the last image
  const uint32_t tail_first = p.rows - p.rows_per_image;

  // what a slot that is not a pixel multiplies with: the padding pixel {izp, izp, izp, 0x80} for a tap of the
  // kernel, a' == 0 for a slot beyond it (K padding)
  uint32_t fill[KB * 4];
  bool is_tap[KB * 4];
#pragma unroll
  for (int i = 0; i < KB * 4; i++) {
    const uint32_t tap = (i >> 2) * 8 + khalf * 4 + (i & 3);       // kb*8 + khalf*4 + j
    is_tap[i] = tap < p.ks;
    fill[i] = is_tap[i] ? p.izp_fill : 0x80808080u;
  }

  struct Taps { int32_t off[KB * 4]; uint32_t img_off; };
  // table entries of the lane's 8 slots; slots beyond the kernel read the neighbouring entries (or 0 beyond the
  // table) and are replaced by `fill`
  auto load_offsets = [&](uint32_t unit, Taps& t) __attribute__((always_inline)) {
    uint32_t m = unit * 32u + row_in_block;
    if (m >= p.rows) m = p.rows - 1;                       // clamped rows are never stored
    const uint32_t img = m / p.rows_per_image;
    const uint32_t pix = m - img * p.rows_per_image;
    t.img_off = img * static_cast<uint32_t>(p.image_stride);
    const uint32_t voff = pix * p.ks * 4u + khalf * 16u;
    // one 16-byte load per K block (the lane's four consecutive entries): with a dword per load every instruction
    // walked the same ~18 cache lines again (36 bytes between the pixels of neighbouring lanes)
#pragma unroll
    for (int kb = 0; kb < KB; kb++) {
      const v4i e = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(off_rsrc, voff + kb * 32, 0, 0));
      t.off[kb * 4 + 0] = e.x; t.off[kb * 4 + 1] = e.y; t.off[kb * 4 + 2] = e.z; t.off[kb * 4 + 3] = e.w;
    }
  };
  // pixel dwords of the slots: offsets < 0 (padding, K padding) read some other in-range dword or 0; replaced later
  auto load_pixels = [&](auto tail_tag, const Taps& t, uint32_t (&x)[KB * 4]) __attribute__((always_inline)) {
    constexpr bool TAIL = decltype(tail_tag)::value;
#pragma unroll
    for (int i = 0; i < KB * 4; i++) {
      const uint32_t voff = t.img_off + static_cast<uint32_t>(t.off[i]);
      if constexpr (TAIL) {
        const uint32_t vc = min(voff, in_bytes - 4u);      // (negative offsets wrap to huge values: clamped too)
        const uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, vc, 0, 0);
        x[i] = v >> (((voff - vc) & 3u) * 8u);
      } else {
        x[i] = __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, voff, 0, 0);
      }
    }
  };
  // slots -> MFMA operand (raw bytes), row sum, re-centred at 128
  auto finish_rows = [&](const uint32_t (&x)[KB * 4], const Taps& t, v4i (&a)[KB]) __attribute__((always_inline)) -> uint32_t {
    uint32_t rs = 0;
#pragma unroll
    for (int kb = 0; kb < KB; kb++) {
      uint32_t v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int i = kb * 4 + j;
        const uint32_t pixel = (x[i] & 0x00FFFFFFu) | 0x80000000u;   // the slot's 4th byte is K padding: a' == 0
        v[j] = (is_tap[i] && t.off[i] >= 0) ? pixel : fill[i];
        rs = __builtin_amdgcn_sad_u8(v[j], 0u, rs);
        v[j] ^= kFlip;
      }
      a[kb] = v4i{static_cast<int>(v[0]), static_cast<int>(v[1]), static_cast<int>(v[2]), static_cast<int>(v[3])};
    }
    rs += __shfl_xor(rs, 32);
    return rs;
  };
  auto gather = [&](uint32_t unit, const Taps& t, uint32_t (&x)[KB * 4]) __attribute__((always_inline)) {
    if (unit * 32u + 32u > tail_first) {                   // wave-uniform
      load_pixels(std::true_type{}, t, x);
    } else {
      load_pixels(std::false_type{}, t, x);
    }
  };

  uint32_t unit = blockIdx.x * kWaves + wave;
  const uint32_t last = units - 1u;
  Taps t_cur, t_next;
  uint32_t x[KB * 4];
  v4i a[KB];
  load_offsets(min(unit, last), t_cur);
  load_offsets(min(unit + unit_stride, last), t_next);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // weights + bias are in LDS, the table entries landed
  gather(min(unit, last), t_cur, x);
  __syncthreads();
  if (unit >= units) return;

  {
    const std::integral_constant<int, SEQ> shift0{};
    const std::integral_constant<bool, FULL> full{};
    (void) shift0; (void) full;
    uint32_t rs = finish_rows(x, t_cur, a);
    for (;;) {
      const uint32_t next = unit + unit_stride;
      // pixels of the next unit (its table entries landed one iteration ago), table entries of the one after
      gather(min(next, last), t_next, x);
      Taps t_after;
      load_offsets(min(next + unit_stride, last), t_after);

      const int32_t rowterm = with_rq_offset<decltype(shift0)::value>(p.row_coeff * static_cast<int32_t>(rs - raw_to_centred));
      uint8_t* img = stage + row_in_block * pitch;
      for (uint32_t nb = 0; nb < nblocks; nb++) {
        v16i acc;
        // (read per block, beside the weight fragment: carried over from the previous trip it cost 16 v_mov_b64 per block)
        int4 bias4[4];
#pragma unroll
        for (int rg = 0; rg < 4; rg++) bias4[rg] = lds_bias4[nb * 8 + rg * 2 + khalf];
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          acc[rg * 4 + 0] = bias4[rg].x; acc[rg * 4 + 1] = bias4[rg].y;
          acc[rg * 4 + 2] = bias4[rg].z; acc[rg * 4 + 3] = bias4[rg].w;
        }
        const uint8_t* wf = lds_w + nb * (KB * 1024);
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
          const v4i w = *reinterpret_cast<const v4i*>(wf + kb * 1024);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w, a[kb], acc, 0, 0, 0);
        }
        igemm_stage_tile<decltype(shift0)::value, decltype(full)::value, false, 2>(
            acc, bias4, rowterm, img, nb * 32, khalf, p, nb * 32 + khalf * 16 < p.n);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // image complete before it is read back
      __builtin_amdgcn_sched_barrier(0);
      rs = finish_rows(x, t_next, a);                            // first use of the loads: the wait lands here
      t_next = t_after;
      __builtin_amdgcn_sched_barrier(0);
      stream_copy_out(stage, whole_dense, log_cpr, unit, 0u, p.n, p, lane);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // read back before the next unit overwrites it
      if (next >= units) break;
      unit = next;
    }
  }
}

}  // namespace

/* offset-table convolution in 4-byte tap slots, at most 16 taps, one group, weights + bias <= 64 KiB */
bool convstream_c3_plan(const IgemmParams& p, uint32_t groups, PwPlan* plan)
{
  if (p.offsets == nullptr || groups != 1 || p.kc != 4 || p.ks == 0 || p.ks > 16 || p.k_pad != 64) return false;
  if (p.rows == 0 || p.rows_per_image == 0) return false;
  const uint32_t lds_bytes = (p.n_pad / 32u) * 2u * 1024u + ((p.n_pad * 4u + 1023u) & ~1023u);
  if (lds_bytes > kMaxLds) return false;
  *plan = PwPlan{};
  plan->family = PwFamily::C3;
  plan->kb = 2;
  plan->vec = 4;
  plan->seq = plan->full = -1;                             // the kernel dispatches itself
  plan->grid_y = 1;
  // 16-byte aligned output rows, tensors addressable with 32-bit offsets: the staged flavour
  const uint64_t in_bytes = static_cast<uint64_t>(p.input_end - p.input);
  const uint64_t table_bytes = static_cast<uint64_t>(p.rows_per_image) * p.ks * 4u;
  if (p.store_mode == 2 && p.n % 16u == 0 && in_bytes >= 4 && in_bytes < (UINT64_C(1) << 31) &&
      table_bytes < (UINT64_C(1) << 31) && p.rows >= p.rows_per_image) {
    uint32_t log_cpr = 1;
    while ((16u << log_cpr) < p.n_pad) log_cpr++;
    const uint32_t pitch = p.output_stride == p.n ? p.n : (16u << log_cpr);
    const uint32_t staged_bytes = lds_bytes + kWaves * 32u * pitch;
    if (staged_bytes <= kMaxLds) {
      plan->c3_staged = true;
      plan->log_cpr = log_cpr;
      plan->lds_bytes = staged_bytes;
      plan->per_cu = resident_per_cu(5, staged_bytes);       // 5: what the kernel's registers allow
      plan->grid_x = persistent_grid(p, plan->per_cu);
      requant_dispatch_ofs(p.rq, [&](auto seq, auto full) { plan->seq = decltype(seq)::value; plan->full = decltype(full)::value; });
      return true;
    }
  }
  plan->lds_bytes = lds_bytes;
  plan->per_cu = 4;
  plan->grid_x = persistent_grid(p, plan->per_cu);
  return true;
}

int convstream_c3_launch(const IgemmParams& p, const PwPlan& plan, hipStream_t stream, const char** name)
{
  *name = pwstream_kernel_name(plan);
  if (!plan.c3_staged) return launch_planned<&q8_conv_stream_c3_kernel>(kMaxLds, plan, stream, p);
  int rc = QNNP_HIP_EINVAL;
  requant_dispatch_ofs(p.rq, [&](auto seq, auto full) {
    rc = launch_planned<q8_conv_stream_c3s_kernel<decltype(seq)::value, decltype(full)::value>>(kMaxLds, plan, stream, p, plan.log_cpr);
  });
  return rc;
}

}  // namespace qnnp
