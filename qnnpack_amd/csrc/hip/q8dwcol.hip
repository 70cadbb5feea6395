/*
 * q8dwcol.hip -- depthwise kernel G: the column-sliding register window, q8_dwconv_col3x3_kernel<S, SEQ, FULL, DEEP, QUAD,
 * DIL> (3x3, stride 1 | 2, C % 4 == 0, dword-aligned tensors; dilated windows on its int8 flavour at stride 1). The
 * default for every 3x3 layer it takes. One family, no device code shared with another unit (kernel H in q8dwcol5.hip
 * is the same walk written out for five-row windows). Plan and launch: dwcol_plan / dwcol_launch, and dwcol_uses_dot4
 * for the flavour a launch picks (dwconv_params.h); "dwconv_kernel" 6 forces it.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "device_ops.hip.h"
#include "dwconv_params.h"
#include "lut_lookup.hip.h"
#include "per_device.h"
#include "qnnp_hip.h"
#include "requant.hip.h"

namespace {

using qnnp::buffer_rsrc;
using qnnp::div_magic;
using qnnp::DwParams;

typedef short v2s __attribute__((ext_vector_type(2)));

// --------------------------------------------------------------------------
// Kernel G: column-sliding register window, 3x3, dilation 1, stride 1 or 2 (both axes), C % 4 == 0
// --------------------------------------------------------------------------
/*
 * What bounds the depthwise kernels is VALU issue (PMC: 24.5 VALU instructions per output, 78 % VALU-active at a third
 * of the HBM rate), and ten of those instructions are the tap arithmetic: five v_perm_b32 that pair two taps' bytes as
 * int16 x 2 and five v_dot2_i32_i16. tools/ubench_valu.hip prices both at 3.2 cycles per wave-instruction (every
 * 8-byte-encoded VALU op; the 4-byte VOP2 ones take 2.0), so the lever is the COUNT. This kernel shares the pairing:
 *
 *   a thread owns one 4-channel dword column j = ox * (C/4) + c/4 of the flattened output row and walks DOWN the output
 *   rows of a segment. Per step it loads one new input row (stride 2: two) -- the three dwords at columns
 *   ix0..ix0+2 -- and pairs
 *       H[r] = (col0, col1) of input row r        (per channel: v_perm -> two int16)   used by the THREE output rows
 *       Q[r] = (col2 @ r, col2 @ r+1)                                                  whose windows contain row r
 *   so an output costs 2 x 4 new v_perm (stride 2: 3 x 4) instead of 5 x 4, and 5 x 4 v_dot2:
 *       out(t) = sum_r H[t+r] . (w_r0, w_r1)  +  Q[t-1] . (0, w_02)  +  Q[t+1] . (w_12, w_22)        (stride 1)
 *   Everything the window re-uses vertically stays in registers; the horizontal overlap (a dword is col0 / col1 / col2
 *   of three neighbouring threads) is served by L1, and because consecutive lanes are consecutive dwords of the NHWC
 *   row, every load and store instruction of a wave covers one contiguous run of memory (256 bytes for dense tensors).
 *   No LDS, no barrier; the rows two steps ahead are in flight while a step computes.
 * Padding: rows outside the image are wave-uniform (a wave = one image, one row segment) and replaced by the zero
 * point without touching memory; columns outside the image exist only in the waves at the ends of a row (FIX flavour).
 */
constexpr int kColThreads = 256;

/* DIL (the int8 walk at stride 1 only): dilated windows. Columns: the three taps sit p.dw pixels apart -- other lane
 * offsets, nothing else. Rows: output rows of one residue class `rho` mod p.dh form an UNDILATED walk over every
 * p.dh-th input row, so a wave takes (image, residue, segment of that residue's rows, chunk) and walks with a row
 * stride of p.dh rows: `oy0` / `oy1` then count the residue's rows (output row rho + p.dh * t), a row index `iy` of the
 * walk is input row rho - pad_top + p.dh * iy, valid for v_lo <= iy < v_hi. */
/* TAB: the output table flavour (qnnpack_gfx950_output_table.h): every packed output dword goes through the LDS copy of
 * p.table (`tab`, lut_lookup.hip.h) before its store. The kernel has no barrier and its waves leave early, so every wave
 * writes the table itself (stage_table_wave): it requests its dword of the table in front of its weights and writes it to
 * LDS where it has waited for the weights anyway. */
template <int S, bool FIX, int SEQ, bool FULL, bool DEEP, bool QUAD, bool DIL = false, bool TAB = false>
__device__ __forceinline__ void dwconv_col3x3_body(
    const DwParams& p, const uint32_t n, const uint32_t oy0, const uint32_t oy1, const uint32_t ox, const uint32_t cg,
    const bool ok0, const bool ok1, const bool ok2, const uint32_t rho = 0, uint8_t (*tab)[256] = nullptr)
{
  static_assert(!DIL || (S == 1 && QUAD), "the dilated walk exists for the int8 flavour at stride 1");
  uint32_t tab_dword = 0;
  if constexpr (TAB) tab_dword = qnnp::table_dword(p.table);
  // kLate: the walks of the default path (int8 dot-product walk at stride 1, pair walk at stride 2) replace padding
  // where a row is CONSUMED, not where it is requested; the int16 pair walks at stride 1 (weights outside the int8
  // classes) keep the round-2 scheme
  constexpr bool kLate = QUAD || S == 2;
  // tap weights: W01[r] = (w_r0, w_r1) pairs, WQA = (0, w_02), WQB = (w_12, w_22); per channel of the group
  uint32_t w01[3][4], wqa[4], wqb[4];
  // QUAD flavour: W4[r] = (x_r0, x_r1, x_r2, 0) as int8, x = +-(w - kzp) (see the step below)
  uint32_t w4[3][4];
  const uint32_t kx = p.wrange == 2u ? 0x7f7f7f7fu : 0x80808080u;    // wave-uniform
  int32_t bias[4];
  // The tap weights and the bias are REQUESTED here; the int8 walk moves them to their registers only after the first
  // input rows have been requested too (unpack_weights()): traced on MobileNetV2 layer 8, a wave spent 5.3k cycles
  // until its weights were in registers and another 2.9k until its first rows had arrived -- one round trip behind
  // the other.
  uint2 tw[9];
  int4 bv;
  uint4 wv[3];
  if constexpr (QUAD) {
    // host-made register image: W4[r] for the thread's four channels, and the bias that goes with a ^ kx
#pragma unroll
    for (int r = 0; r < 3; r++) wv[r] = *reinterpret_cast<const uint4*>(p.dot4 + r * p.c_pad + cg);
    bv = *reinterpret_cast<const int4*>(p.dot4 + 3u * p.c_pad + cg);
  } else {
#pragma unroll
    for (int i = 0; i < 9; i++) tw[i] = *reinterpret_cast<const uint2*>(p.wadj + i * p.c_pad + cg);   // 4 x int16
    bv = *reinterpret_cast<const int4*>(p.bias1 + cg);
  }
  auto unpack_weights = [&]() __attribute__((always_inline)) {
    if constexpr (QUAD) __builtin_amdgcn_sched_barrier(0);             // behind the row loads issued so far
    auto lo16 = [](uint2 v, int c) -> uint32_t { return ((c < 2 ? v.x : v.y) >> ((c & 1) * 16)) & 0xFFFFu; };
    if constexpr (TAB) qnnp::stage_table_wave(*tab, tab_dword);
    bias[0] = bv.x; bias[1] = bv.y; bias[2] = bv.z; bias[3] = bv.w;
    if constexpr (QUAD) {
#pragma unroll
      for (int r = 0; r < 3; r++) { w4[r][0] = wv[r].x; w4[r][1] = wv[r].y; w4[r][2] = wv[r].z; w4[r][3] = wv[r].w; }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if constexpr (!QUAD) {
#pragma unroll
        for (int r = 0; r < 3; r++) w01[r][c] = lo16(tw[r * 3 + 0], c) | (lo16(tw[r * 3 + 1], c) << 16);
        wqa[c] = lo16(tw[2], c) << 16;
        wqb[c] = lo16(tw[5], c) | (lo16(tw[8], c) << 16);
      }
      // the offset rounding sequences (requant.hip.h) take accumulator + 2^31: folded into the bias, once per thread
      bias[c] = qnnp::with_rq_offset<SEQ>(bias[c]);
    }
    if constexpr (kLate && FIX) {
      // Padding COLUMNS of this lane are never loaded (out-of-range offsets: the buffer returns 0) and never selected:
      // reading 0 where the input zero point belongs is a per-lane constant -- izp * (the column's weights) -- that goes
      // into the bias here, once, instead of three v_cndmask per step on registers just requested (which made every step
      // of a border wave wait for its newest row: s_waitcnt vmcnt(3) / vmcnt(0) in the loop, ISA of the round-2 build).
      const bool okc[3] = {ok0, ok1, ok2};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        int32_t sum = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            int32_t x;
            if constexpr (QUAD) x = static_cast<int8_t>(w4[r][c] >> (8 * k));            // +-(w - kzp), as multiplied
            else x = static_cast<int16_t>(lo16(tw[r * 3 + k], c));                       // w - kzp
            sum += okc[k] ? 0 : x;
          }
        }
        // QUAD multiplies a' = a ^ kx: a' (izp) - a'(0) = izp (kx = 0x80) or -izp (0x7f); the pair walks multiply a itself
        const int32_t step = (QUAD && p.wrange == 2u) ? -static_cast<int32_t>(p.izp) : static_cast<int32_t>(p.izp);
        bias[c] = qnnp::add_wrap(bias[c], step * sum);
      }
    }
  };
  // (the pair walks unpack at once: with the raw taps live across the first row requests they need 93-98 VGPRs
  //  instead of 79-82, a wave per SIMD less, and the stride-2 layers measured no better for the overlap)
  if constexpr (!QUAD) unpack_weights();
  QNNP_DW_TRACE(p, 1);
  const uint32_t fill = p.izp * 0x01010101u;
  const uint32_t row_bytes = p.W * p.in_stride;
#ifdef QNNP_ENABLE_ABLATION
  // measurement knobs that leave the instruction stream alone: bit 2 = every step re-reads the segment's first row
  // (loads served by L1 / L2), bit 3 = every step stores to the segment's first output row (writes combine in L2)
  const uint32_t row_adv = (p.abl & 4u) ? 0u : row_bytes;
#else
  const uint32_t row_adv = row_bytes;
#endif
  // Buffer addressing: a descriptor over the whole tensor (built from kernel arguments only, so it stays in SGPRs),
  // per lane a constant 32-bit byte offset inside a row, per row a SCALAR offset -- no vector address arithmetic in
  // the loop. Invalid columns are clamped to column 0 (their value is replaced below).
  const __amdgpu_buffer_rsrc_t in_rsrc = buffer_rsrc(p.input, static_cast<int>(p.batch * p.H * row_bytes));
  const int32_t ix0 = static_cast<int32_t>(ox * S) - static_cast<int32_t>(p.pad_left);
  uint32_t coff[3];
  coff[0] = cg + (ok0 ? static_cast<uint32_t>(ix0) : 0u) * p.in_stride;
  const int32_t dcol = DIL ? static_cast<int32_t>(p.dw) : 1;
  coff[1] = cg + (ok1 ? static_cast<uint32_t>(ix0 + dcol) : 0u) * p.in_stride;
  coff[2] = cg + (ok2 ? static_cast<uint32_t>(ix0 + 2 * dcol) : 0u) * p.in_stride;
  // what a padding ROW reads at this lane's columns: the input zero point -- or 0 at a padding column of a kLate walk
  uint32_t fillk[3] = {fill, fill, fill};
  if constexpr (kLate && FIX) {
    // (beyond the descriptor's extent -- dwcol_plan keeps the tensor below 2^31 bytes: the load returns 0)
    if (!ok0) { coff[0] = 0x80000000u; fillk[0] = 0u; }
    if (!ok1) { coff[1] = 0x80000000u; fillk[1] = 0u; }
    if (!ok2) { coff[2] = 0x80000000u; fillk[2] = 0u; }
  }
  const uint32_t img_off = n * p.H * row_bytes;                     // wave-uniform
  int32_t iy_first = static_cast<int32_t>(oy0 * S) - static_cast<int32_t>(p.pad_top);
  // DIL: the walk's row index -> input row base + dh * iy (scalars)
  int32_t v_lo = 0, v_hi = static_cast<int32_t>(p.H);
  uint32_t row_org = img_off, row_adv_w = row_adv, out_rows = 1u;
  if constexpr (DIL) {
    const int32_t d = static_cast<int32_t>(p.dh);
    const int32_t base = static_cast<int32_t>(rho) - static_cast<int32_t>(p.pad_top);
    v_lo = base >= 0 ? 0 : (-base + d - 1) / d;
    v_hi = static_cast<int32_t>(p.H) - 1 - base >= 0 ? (static_cast<int32_t>(p.H) - 1 - base) / d + 1 : 0;
    row_org = img_off + static_cast<uint32_t>(base) * row_bytes;    // (wraps for base < 0: rows iy >= v_lo bring it back)
    row_adv_w = row_adv * p.dh;
    out_rows = p.dh;
    iy_first = static_cast<int32_t>(oy0);
  }

  struct Row { uint32_t c[3]; bool ok; };
  // One input row: three dwords. The loads are ALWAYS issued (a row outside the image is clamped to a valid one and
  // its values replaced afterwards, wave-uniformly): a branch around the loads makes the number of outstanding
  // operations path-dependent, and hipcc then falls back to s_waitcnt vmcnt(<3) right behind the newest loads --
  // the rows "in flight" were waited for at once (measured: 17 of 45 us on MobileNetV2 layer 8).
  // CHECK = false: the caller knows the row is inside the image (the steady state of a segment).
  auto load_row = [&](auto check, int32_t iy) __attribute__((always_inline)) -> Row {
    constexpr bool CHECK = decltype(check)::value;
    Row r;
    bool row_ok = true;
    // (kLate walks: always -- the clamp is scalar work, and a steady-state step may request a row below the image for the
    //  checked steps behind it; what makes a step "steady" there is that the row it CONSUMES is inside)
    uint32_t ro;
    if constexpr (DIL) {
      row_ok = iy >= v_lo && iy < v_hi;
      iy = iy >= v_hi ? v_hi - 1 : iy;
      iy = iy < v_lo ? v_lo : iy;                 // (no valid row at all: a row below the image, or beyond the tensor -- the buffer answers 0)
      ro = row_org + static_cast<uint32_t>(iy) * row_adv_w;
    } else {
    if constexpr (CHECK || kLate) {
      row_ok = iy >= 0 && iy < static_cast<int32_t>(p.H);
      iy = iy < 0 ? 0 : (iy >= static_cast<int32_t>(p.H) ? static_cast<int32_t>(p.H) - 1 : iy);
    }
    ro = img_off + static_cast<uint32_t>(iy) * row_adv;        // scalar
    }
    r.ok = row_ok;
    r.c[0] = __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, coff[0], ro, 0);
    r.c[1] = __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, coff[1], ro, 0);
    r.c[2] = __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, coff[2], ro, 0);
    if constexpr (!kLate) {
      // (a select on a register just requested is a wait for it: the kLate walks do this in settle(), at the use)
      if constexpr (FIX) {
        r.c[0] = ok0 ? r.c[0] : fill;
        r.c[1] = ok1 ? r.c[1] : fill;
        r.c[2] = ok2 ? r.c[2] : fill;
      }
      if constexpr (CHECK) {
        r.c[0] = row_ok ? r.c[0] : fill;
        r.c[1] = row_ok ? r.c[1] : fill;
        r.c[2] = row_ok ? r.c[2] : fill;
      }
    }
    return r;
  };
  // kLate walks: a padding ROW becomes the zero point where it is consumed (CHECK = false: the caller knows the row is
  // inside the image -- the steady-state steps, whose rows lie between the first trip's and the ones they request)
  auto settle = [&](auto check, Row& r) __attribute__((always_inline)) {
    if constexpr (kLate && decltype(check)::value) {
      r.c[0] = r.ok ? r.c[0] : fillk[0];
      r.c[1] = r.ok ? r.c[1] : fillk[1];
      r.c[2] = r.ok ? r.c[2] : fillk[2];
    }
  };
  constexpr std::true_type kChecked{};
  constexpr std::false_type kInside{};
  struct Pair { uint32_t v[4]; };
  // per channel c: (lo.byte c, hi.byte c) as two zero-extended int16
  auto pair = [](uint32_t lo, uint32_t hi) __attribute__((always_inline)) -> Pair {
    Pair q;
    q.v[0] = __builtin_amdgcn_perm(hi, lo, 0x0c040c00u);
    q.v[1] = __builtin_amdgcn_perm(hi, lo, 0x0c050c01u);
    q.v[2] = __builtin_amdgcn_perm(hi, lo, 0x0c060c02u);
    q.v[3] = __builtin_amdgcn_perm(hi, lo, 0x0c070c03u);
    return q;
  };
  auto dot = [](const Pair& a, const uint32_t (&w)[4], int32_t (&acc)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      acc[c] = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, a.v[c]), __builtin_bit_cast(v2s, w[c]), acc[c], false);
    }
  };
  // QUAD flavour: per channel c the bytes (col0, col1, col2, 0) of one input row, re-centred to int8
  struct Quad { uint32_t v[4]; };
  auto quad = [kx](const Row& r) __attribute__((always_inline)) -> Quad {
    const uint32_t d0 = r.c[0] ^ kx, d1 = r.c[1] ^ kx, d2 = r.c[2] ^ kx;
    const uint32_t lo = __builtin_amdgcn_perm(d1, d0, 0x05010400u);      // (d0.b0, d1.b0, d0.b1, d1.b1)
    const uint32_t hi = __builtin_amdgcn_perm(d1, d0, 0x07030602u);      // (d0.b2, d1.b2, d0.b3, d1.b3)
    Quad q;
    q.v[0] = __builtin_amdgcn_perm(d2, lo, 0x0c040100u);
    q.v[1] = __builtin_amdgcn_perm(d2, lo, 0x0c050302u);
    q.v[2] = __builtin_amdgcn_perm(d2, hi, 0x0c060100u);
    q.v[3] = __builtin_amdgcn_perm(d2, hi, 0x0c070302u);
    return q;
  };
  auto dot4 = [](const Quad& a, const uint32_t (&w)[4], int32_t (&acc)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      acc[c] = __builtin_amdgcn_sdot4(static_cast<int32_t>(a.v[c]), static_cast<int32_t>(w[c]), acc[c], false);
    }
  };
  auto dot4_first = [](const Quad& a, const uint32_t (&w)[4], const int32_t (&b)[4], int32_t (&acc)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      asm("v_dot4_i32_i8 %0, %1, %2, %3" : "=v"(acc[c]) : "v"(a.v[c]), "v"(w[c]), "v"(b[c]));
    }
  };
  // first product of an output: the three-operand form takes the bias as its addend (the two-operand accumulate
  // form the compiler prefers would need a copy of the bias per output first)
  auto dot_first = [](const Pair& a, const uint32_t (&w)[4], const int32_t (&b)[4], int32_t (&acc)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(acc[c]) : "v"(a.v[c]), "v"(w[c]), "v"(b[c]));
    }
  };

  const __amdgpu_buffer_rsrc_t out_rsrc = buffer_rsrc(p.output, static_cast<int>(p.batch * p.OH * p.OW * p.out_stride));
  const uint32_t out_voff = ox * p.out_stride + cg;
  uint32_t out_soff = (n * p.OH + (DIL ? rho + out_rows * oy0 : oy0)) * p.OW * p.out_stride;   // scalar, advances one output row (DIL: p.dh rows) per step
#ifdef QNNP_ENABLE_ABLATION
  const uint32_t out_step = (p.abl & 8u) ? 0u : p.OW * p.out_stride * out_rows;
#else
  const uint32_t out_step = p.OW * p.out_stride * out_rows;
#endif

  {
    auto finish = [&](int32_t (&acc)[4]) __attribute__((always_inline)) {
      uint32_t packed = qnnp::q31_requantize_pack4<SEQ, FULL>(
          acc[0], acc[1], acc[2], acc[3], p.rq);
      if constexpr (TAB) packed = qnnp::lut_u8x4(*tab, packed);
      // (a wave's 64 dwords of an output row are contiguous: whole lines, written once -- the streaming hint, under the
      //  "streaming_stores" option; the two builtins differ in an immediate, so hipcc cannot merge them)
      if (p.stream_out) __builtin_amdgcn_raw_buffer_store_b32(packed, out_rsrc, out_voff, out_soff, 2);
      else __builtin_amdgcn_raw_buffer_store_b32(packed, out_rsrc, out_voff, out_soff, 0);
      out_soff += out_step;
    };
    const uint32_t steps = oy1 - oy0;
    if constexpr (S == 1 && QUAD) {
      // The int8 dot-product flavour (weights whose x = w - kzp, or -x, fit int8: DwParams::wrange). An input row is
      // transposed ONCE into per-channel quads T[r] = (col0, col1, col2, 0) -- two v_perm over (col0, col1), four that
      // append col2 -- and serves the three output rows whose windows contain it:
      //     out(t) = T[t] . W4[0] + T[t+1] . W4[1] + T[t+2] . W4[2]               (v_dot4_i32_i8, 3 per channel)
      // i.e. 6 v_perm + 3 v_xor + 12 dot products per output dword against 8 v_perm + 20 v_dot2 of the pair walk.
      // a' = a ^ 0x80 = a - 128 pairs with x, a' = a ^ 0x7f = 127 - a with -x; the difference to sum a * x is a
      // constant per channel, folded into the bias above. A row buffer is dead as soon as its quad is built, so
      // NBUF buffers keep NBUF rows in flight: row r lives in buffer r % NBUF, T[.] rotate with period three.
      constexpr int NBUF = DEEP ? 6 : 3;
      Row r0 = load_row(kChecked, iy_first);
      Row r1 = load_row(kChecked, iy_first + 1);
      Row r2 = load_row(kChecked, iy_first + 2);
      Row r3, r4, r5;
      if constexpr (DEEP) {
        r3 = load_row(kChecked, iy_first + 3);
        r4 = load_row(kChecked, iy_first + 4);
        r5 = load_row(kChecked, iy_first + 5);
      }
      unpack_weights();
      settle(kChecked, r0);
      Quad q0 = quad(r0);
      r0 = load_row(kChecked, iy_first + NBUF);
      settle(kChecked, r1);
      Quad q1 = quad(r1);
      r1 = load_row(kChecked, iy_first + NBUF + 1);
      Quad q2;
      uint32_t t = 0;
      QNNP_DW_TRACE(p, 2);
      // steps whose newest window row (iy_first + t + 2) is inside the image: t < t_inside
      const int32_t inside = (DIL ? v_hi : static_cast<int32_t>(p.H)) - 2 - iy_first;
      const uint32_t t_inside = inside <= 0 ? 0u : (static_cast<uint32_t>(inside) < steps ? static_cast<uint32_t>(inside) : steps);
#define QNNP_DW_COL_STEPQ(CHECK, TA, TB, TC, RC)                                      \
      {                                                                             \
        settle(CHECK, RC);                                                          \
        TC = quad(RC);                                      /* T[t+2] */            \
        RC = load_row(CHECK, iy_first + static_cast<int32_t>(t) + 2 + NBUF);        \
        __builtin_amdgcn_sched_barrier(0);                                          \
        int32_t acc[4];                                                             \
        dot4_first(TA, w4[0], bias, acc);                                           \
        dot4(TB, w4[1], acc);                                                       \
        dot4(TC, w4[2], acc);                                                       \
        finish(acc);                                                                \
        t++;                                                                        \
      }
      // (a steady-state step consumes row iy_first + t + 2 >= 0 -- dwcol_plan: pad_top <= 2, the rows above the image
      //  were settled above -- and requests a row inside the image: what it consumes lies between the two)
      if constexpr (DEEP) {
        while (t + 6 <= t_inside) {                // steady state: straight-line body, counted waits
          QNNP_DW_COL_STEPQ(kInside, q0, q1, q2, r2)
          QNNP_DW_COL_STEPQ(kInside, q1, q2, q0, r3)
          QNNP_DW_COL_STEPQ(kInside, q2, q0, q1, r4)
          QNNP_DW_COL_STEPQ(kInside, q0, q1, q2, r5)
          QNNP_DW_COL_STEPQ(kInside, q1, q2, q0, r0)
          QNNP_DW_COL_STEPQ(kInside, q2, q0, q1, r1)
        }
        QNNP_DW_TRACE(p, 3);
        while (t < steps) {                        // the last steps of a segment (and of the image: padding rows)
          QNNP_DW_COL_STEPQ(kChecked, q0, q1, q2, r2)
          if (t >= steps) break;
          QNNP_DW_COL_STEPQ(kChecked, q1, q2, q0, r3)
          if (t >= steps) break;
          QNNP_DW_COL_STEPQ(kChecked, q2, q0, q1, r4)
          if (t >= steps) break;
          QNNP_DW_COL_STEPQ(kChecked, q0, q1, q2, r5)
          if (t >= steps) break;
          QNNP_DW_COL_STEPQ(kChecked, q1, q2, q0, r0)
          if (t >= steps) break;
          QNNP_DW_COL_STEPQ(kChecked, q2, q0, q1, r1)
        }
      } else {
        while (t + 3 <= t_inside) {
          QNNP_DW_COL_STEPQ(kInside, q0, q1, q2, r2)
          QNNP_DW_COL_STEPQ(kInside, q1, q2, q0, r0)
          QNNP_DW_COL_STEPQ(kInside, q2, q0, q1, r1)
        }
        while (t < steps) {
          QNNP_DW_COL_STEPQ(kChecked, q0, q1, q2, r2)
          if (t >= steps) break;
          QNNP_DW_COL_STEPQ(kChecked, q1, q2, q0, r0)
          if (t >= steps) break;
          QNNP_DW_COL_STEPQ(kChecked, q2, q0, q1, r1)
        }
      }
      QNNP_DW_TRACE(p, 4);
#undef QNNP_DW_COL_STEPQ
    } else if constexpr (S == 1 && DEEP) {
      // The same walk with FOUR rows in flight instead of two: six row buffers (row r lives in buffer r % 6), the pair
      // registers keep their period of three, so six steps are written out per trip. PMC on the two-rows-ahead loop
      // (MobileNetV2 layers 8 / 13, batch 128): waves parked on s_waitcnt for 60 / 50 % of their lifetime, VALU busy
      // 59 / 50 % -- a step of 4-5 waves sharing a SIMD takes ~850 cycles, two of them are less than an HBM round trip.
      // State entering step t: HA = H[t], HB = H[t+1], QA = Q[t-1], QB = Q[t], RP = row t+1, RC = row t+2,
      // RL = the buffer of row t (dead: both its pairs are built), reloaded with row t+6.
      Row r0 = load_row(kChecked, iy_first);
      Row r1 = load_row(kChecked, iy_first + 1);
      Row r2 = load_row(kChecked, iy_first + 2);
      Row r3 = load_row(kChecked, iy_first + 3);
      Row r4 = load_row(kChecked, iy_first + 4);
      Row r5 = load_row(kChecked, iy_first + 5);
      Pair h0 = pair(r0.c[0], r0.c[1]);
      Pair h1 = pair(r1.c[0], r1.c[1]);
      Pair qa = pair(r0.c[2], r0.c[2]);            // Q[-1] = (don't care, col2 @ 0)
      Pair qb = pair(r0.c[2], r1.c[2]);            // Q[0]
      Pair h2, qc;
      uint32_t t = 0;
      // steps whose prefetched row (iy_first + t + 6) is inside the image: t < t_inside
      const int32_t inside = static_cast<int32_t>(p.H) - 6 - iy_first;
      const uint32_t t_inside = inside <= 0 ? 0u : (static_cast<uint32_t>(inside) < steps ? static_cast<uint32_t>(inside) : steps);
#define QNNP_DW_COL_STEP6(CHECK, HA, HB, HC, QA, QB, QC, RP, RC, RL)                 \
      {                                                                             \
        HC = pair(RC.c[0], RC.c[1]);                        /* H[t+2] */            \
        QC = pair(RP.c[2], RC.c[2]);                        /* Q[t+1] */            \
        RL = load_row(CHECK, iy_first + static_cast<int32_t>(t) + 6);               \
        __builtin_amdgcn_sched_barrier(0);   /* (left alone the scheduler sinks the loads towards their uses) */ \
        int32_t acc[4];                                                             \
        dot_first(HA, w01[0], bias, acc);                                           \
        dot(HB, w01[1], acc);                                                       \
        dot(HC, w01[2], acc);                                                       \
        dot(QA, wqa, acc);                                                          \
        dot(QC, wqb, acc);                                                          \
        finish(acc);                                                                \
        t++;                                                                        \
      }
      while (t + 6 <= t_inside) {                  // steady state: straight-line body, counted waits
        QNNP_DW_COL_STEP6(kInside, h0, h1, h2, qa, qb, qc, r1, r2, r0)
        QNNP_DW_COL_STEP6(kInside, h1, h2, h0, qb, qc, qa, r2, r3, r1)
        QNNP_DW_COL_STEP6(kInside, h2, h0, h1, qc, qa, qb, r3, r4, r2)
        QNNP_DW_COL_STEP6(kInside, h0, h1, h2, qa, qb, qc, r4, r5, r3)
        QNNP_DW_COL_STEP6(kInside, h1, h2, h0, qb, qc, qa, r5, r0, r4)
        QNNP_DW_COL_STEP6(kInside, h2, h0, h1, qc, qa, qb, r0, r1, r5)
      }
      while (t < steps) {                          // the last steps of a segment (and of the image: padding rows)
        QNNP_DW_COL_STEP6(kChecked, h0, h1, h2, qa, qb, qc, r1, r2, r0)
        if (t >= steps) break;
        QNNP_DW_COL_STEP6(kChecked, h1, h2, h0, qb, qc, qa, r2, r3, r1)
        if (t >= steps) break;
        QNNP_DW_COL_STEP6(kChecked, h2, h0, h1, qc, qa, qb, r3, r4, r2)
        if (t >= steps) break;
        QNNP_DW_COL_STEP6(kChecked, h0, h1, h2, qa, qb, qc, r4, r5, r3)
        if (t >= steps) break;
        QNNP_DW_COL_STEP6(kChecked, h1, h2, h0, qb, qc, qa, r5, r0, r4)
        if (t >= steps) break;
        QNNP_DW_COL_STEP6(kChecked, h2, h0, h1, qc, qa, qb, r0, r1, r5)
      }
#undef QNNP_DW_COL_STEP6
    } else if constexpr (S == 1) {
      // window rows of output t: t, t+1, t+2 (relative to iy_first). State entering step t:
      //   HA = H[t], HB = H[t+1], QA = Q[t-1] (only its high half matters), QB = Q[t],
      //   RP = row t+1 (its col2 is still needed), RC = row t+2, third row buffer = row t+3 (in flight).
      // The step pairs row t+2, then re-uses RP for row t+4: two rows are always in flight. Roles rotate through
      // the same registers with period three, so three steps are written out per trip and nothing is copied.
      const Row r0 = load_row(kChecked, iy_first);
      Row b1 = load_row(kChecked, iy_first + 1);
      Row b2 = load_row(kChecked, iy_first + 2);
      Row b3 = load_row(kChecked, iy_first + 3);
      Pair h0 = pair(r0.c[0], r0.c[1]);
      Pair h1 = pair(b1.c[0], b1.c[1]);
      Pair qa = pair(r0.c[2], r0.c[2]);            // Q[-1] = (don't care, col2 @ 0)
      Pair qb = pair(r0.c[2], b1.c[2]);            // Q[0]
      Pair h2, qc;
      uint32_t t = 0;
      // steps whose prefetched row (iy_first + t + 4) is inside the image: t < t_inside
      const int32_t inside = static_cast<int32_t>(p.H) - 4 - iy_first;
      const uint32_t t_inside = inside <= 0 ? 0u : (static_cast<uint32_t>(inside) < steps ? static_cast<uint32_t>(inside) : steps);
#define QNNP_DW_COL_STEP(CHECK, HA, HB, HC, QA, QB, QC, RP, RC)                      \
      {                                                                             \
        HC = pair(RC.c[0], RC.c[1]);                        /* H[t+2] */            \
        QC = pair(RP.c[2], RC.c[2]);                        /* Q[t+1] */            \
        RP = load_row(CHECK, iy_first + static_cast<int32_t>(t) + 4);               \
        int32_t acc[4];                                                             \
        dot_first(HA, w01[0], bias, acc);                                           \
        dot(HB, w01[1], acc);                                                       \
        dot(HC, w01[2], acc);                                                       \
        dot(QA, wqa, acc);                                                          \
        dot(QC, wqb, acc);                                                          \
        finish(acc);                                                                \
        t++;                                                                        \
      }
      while (t + 3 <= t_inside) {                  // steady state: straight-line body, counted waits
        QNNP_DW_COL_STEP(kInside, h0, h1, h2, qa, qb, qc, b1, b2)
        QNNP_DW_COL_STEP(kInside, h1, h2, h0, qb, qc, qa, b2, b3)
        QNNP_DW_COL_STEP(kInside, h2, h0, h1, qc, qa, qb, b3, b1)
      }
      while (t < steps) {                          // the last steps of a segment (and of the image: padding rows)
        QNNP_DW_COL_STEP(kChecked, h0, h1, h2, qa, qb, qc, b1, b2)
        if (t < steps) {
          QNNP_DW_COL_STEP(kChecked, h1, h2, h0, qb, qc, qa, b2, b3)
          if (t < steps) {
            QNNP_DW_COL_STEP(kChecked, h2, h0, h1, qc, qa, qb, b3, b1)
          }
        }
      }
#undef QNNP_DW_COL_STEP
    } else {
      // stride 2: window rows of output t: 2t, 2t+1, 2t+2. State entering step t:
      //   HA = H[2t], QA = (don't care, col2 @ 2t), (RA, RB) = rows 2t+1 / 2t+2, the other row pair = rows 2t+3 / 2t+4
      //   (in flight). Period two: two steps per trip.
      const Row r0 = load_row(kChecked, iy_first);
      Row a1 = load_row(kChecked, iy_first + 1);
      Row a2 = load_row(kChecked, iy_first + 2);
      Row c1 = load_row(kChecked, iy_first + 3);
      Row c2 = load_row(kChecked, iy_first + 4);
      // steps whose window rows (iy_first + 2t + 1, + 2) are inside the image: t < t_inside
      const int32_t inside = (static_cast<int32_t>(p.H) - 1 - iy_first) / 2;
      const uint32_t t_inside = (static_cast<int32_t>(p.H) - 1 - iy_first) <= 0 ? 0u :
          (static_cast<uint32_t>(inside) < steps ? static_cast<uint32_t>(inside) : steps);
      Row r0s = r0;
      settle(kChecked, r0s);
      Pair ha = pair(r0s.c[0], r0s.c[1]);
      Pair qa = pair(r0s.c[2], r0s.c[2]);
      Pair hb, qb;
      uint32_t t = 0;
#define QNNP_DW_COL_STEP2(CHECK, HA, HC, QA, QC, RA, RB)                            \
      {                                                                             \
        settle(CHECK, RA);                                                          \
        settle(CHECK, RB);                                                          \
        const Pair hmid = pair(RA.c[0], RA.c[1]);           /* H[2t+1] */           \
        HC = pair(RB.c[0], RB.c[1]);                        /* H[2t+2] = H[2(t+1)] */ \
        QC = pair(RA.c[2], RB.c[2]);                        /* (col2 @ 2t+1, col2 @ 2t+2) */ \
        RA = load_row(CHECK, iy_first + 2 * static_cast<int32_t>(t) + 5);           \
        RB = load_row(CHECK, iy_first + 2 * static_cast<int32_t>(t) + 6);           \
        __builtin_amdgcn_sched_barrier(0);   /* (left alone the scheduler sinks the loads to the end of the trip) */ \
        int32_t acc[4];                                                             \
        dot_first(HA, w01[0], bias, acc);                                           \
        dot(hmid, w01[1], acc);                                                     \
        dot(HC, w01[2], acc);                                                       \
        dot(QA, wqa, acc);                                                          \
        dot(QC, wqb, acc);                                                          \
        finish(acc);                                                                \
        t++;                                                                        \
      }
      if (iy_first + 1 < 0) {                      // padding 2: row 1 of the walk is above the image -- one checked trip
        QNNP_DW_COL_STEP2(kChecked, ha, hb, qa, qb, a1, a2)
        if (t >= steps) return;
        QNNP_DW_COL_STEP2(kChecked, hb, ha, qb, qa, c1, c2)
      }
      if (t + 2 <= t_inside) {
        // (hipcc sizes the waits at a loop header for the fewest operations in flight over all ways in; entered from the
        //  checked first trip that came out as vmcnt(1) on every trip. With the queue drained once on the way in, the back
        //  edge alone decides)
        __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0)
        do {
          QNNP_DW_COL_STEP2(kInside, ha, hb, qa, qb, a1, a2)
          QNNP_DW_COL_STEP2(kInside, hb, ha, qb, qa, c1, c2)
        } while (t + 2 <= t_inside);
      }
      while (t < steps) {
        QNNP_DW_COL_STEP2(kChecked, ha, hb, qa, qb, a1, a2)
        if (t < steps) {
          QNNP_DW_COL_STEP2(kChecked, hb, ha, qb, qa, c1, c2)
        }
      }
#undef QNNP_DW_COL_STEP2
    }
  }
}

/* SEQ / FULL: the requantization flavour (requant.hip.h), chosen on the host -- one kernel per flavour, so that the
 * common one is not charged the registers of the rare ones (83 against 77 VGPRs: 5 instead of 6 waves per SIMD) */
template <int S, int SEQ, bool FULL, bool DEEP, bool QUAD, bool DIL = false, bool TAB = false>
__global__ __launch_bounds__(kColThreads)
void q8_dwconv_col3x3_kernel(const DwParams p)
{
  // wave -> (image, row segment, 64-dword chunk of the flattened output row); `slabs` = row segments, `TOH` = rows
  // per segment, `bands` = chunks per row here
  const uint32_t lane = threadIdx.x & 63u;
  QNNP_DW_TRACE(p, 0);
#ifdef QNNP_ENABLE_ABLATION
  if (p.trace != nullptr && threadIdx.x == 0 && blockIdx.x < 4096) {
    p.trace[(blockIdx.x * 4 + 3) * 8 + 0] = wall_clock64();
    // where the workgroup's wave 0 runs: HW_REG_HW_ID (wave 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13) and HW_REG_XCC_ID
    p.trace[(blockIdx.x * 4 + 2) * 8 + 0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    p.trace[(blockIdx.x * 4 + 2) * 8 + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
  }
#endif
  // Workgroup b runs on XCD b % 8 (observed, MI355X_MICROARCH.md "Workgroup dispatch"; a speed assumption only). For
  // tensors that more or less live in the caches (dwcol_launch: <= 96 MiB in + out) every XCD takes a CONTIGUOUS range of
  // the flattened (image, segment, chunk) space, so that the halo pixels either side of a chunk are found in that XCD's
  // L2 by the neighbouring workgroups: same box, batch 128, 28x28x192 s2 8.8 -> 8.2 us, 14x14x576 s2 7.1 -> 6.9,
  // 56x56x144 s2 19.3 -> 18.9. The big HBM-streaming layers keep the round-robin order, where the eight XCDs sweep
  // neighbouring addresses at the same time: 112x112x96 s2 41.9 -> 43.8 us with the ranges, 112x112x32 +0.3.
  uint32_t b = blockIdx.x;
  if (p.xcd_ranges != 0u) {
    const uint32_t q = gridDim.x >> 3, r = gridDim.x & 7u, xcd = b & 7u;
    b = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (b >> 3);
  }
  uint32_t w = __builtin_amdgcn_readfirstlane(b * (kColThreads / 64) + (threadIdx.x >> 6));
  // (divisions by run-time values through host-made reciprocals: ~40 instructions each otherwise, on every wave's way
  //  to its first load; exact while dividend * divisor < 2^32, which dwcol_plan checks)
  const uint32_t wb = div_magic(w, p.inv_bands);
  const uint32_t chunk = w - wb * p.bands;
  const uint32_t n = div_magic(wb, p.inv_slabs);
  const uint32_t seg = wb - n * p.slabs;
  if (n >= p.batch) return;
  const uint32_t q4 = p.C >> 2;
  const uint32_t cols = p.OW * q4;
  // lanes past the end of the row repeat its last dword column: same loads, same results, same stores -- harmless
  uint32_t j = chunk * 64u + lane;
  if (j >= cols) j = cols - 1u;
  const uint32_t ox = div_magic(j, p.inv_q4);
  const uint32_t cg = (j - ox * q4) * 4u;
  // DIL: segment index -> (segment of a residue class of the output rows, residue); `slabs` counts both
  uint32_t rho = 0, rows = p.OH, sidx = seg;
  if constexpr (DIL) {
    sidx = div_magic(seg, p.inv_dh);
    rho = seg - sidx * p.dh;
    rows = rho < p.OH ? div_magic(p.OH - rho + p.dh - 1u, p.inv_dh) : 0u;       // output rows rho, rho + dh, ...
  }
  const uint32_t oy0 = sidx * p.TOH;
  if (DIL && oy0 >= rows) return;
  const uint32_t oy1 = min(rows, oy0 + p.TOH);
  const int32_t dcol = DIL ? static_cast<int32_t>(p.dw) : 1;
  const int32_t ix0 = static_cast<int32_t>(ox * S) - static_cast<int32_t>(p.pad_left);
  const bool ok0 = ix0 >= 0 && ix0 < static_cast<int32_t>(p.W);
  const bool ok1 = ix0 + dcol >= 0 && ix0 + dcol < static_cast<int32_t>(p.W);
  const bool ok2 = ix0 + 2 * dcol >= 0 && ix0 + 2 * dcol < static_cast<int32_t>(p.W);
  uint8_t (*tab)[256] = nullptr;
  if constexpr (TAB) {
    __shared__ alignas(16) uint8_t tab_lds[256];   // written whole by every wave that reads it (lut_lookup.hip.h)
    tab = &tab_lds;
  }
  if (__builtin_amdgcn_ballot_w64(!(ok0 && ok1 && ok2)) != 0) {
    dwconv_col3x3_body<S, true, SEQ, FULL, DEEP, QUAD, DIL, TAB>(p, n, oy0, oy1, ox, cg, ok0, ok1, ok2, rho, tab);
  } else {
    dwconv_col3x3_body<S, false, SEQ, FULL, DEEP, QUAD, DIL, TAB>(p, n, oy0, oy1, ox, cg, true, true, true, rho, tab);
  }
  QNNP_DW_TRACE(p, 5);
#ifdef QNNP_ENABLE_ABLATION
  if (p.trace != nullptr && threadIdx.x == 0 && blockIdx.x < 4096) p.trace[(blockIdx.x * 4 + 3) * 8 + 1] = wall_clock64();
#endif
}

}  // namespace

namespace qnnp {

// geometry of kernel G: `bands` = 64-dword chunks per flattened output row, `slabs` = row segments, `TOH` = rows each
bool dwcol_plan(DwParams& p)
{
  if (p.C % 4 != 0 || p.KH != 3 || p.KW != 3) return false;
  if (p.sh != p.sw || (p.sw != 1 && p.sw != 2)) return false;
  // dilated windows: the int8 walk at stride 1 only (its residue-class form, see the body); up to 64 rows apart
  const bool dilated = p.dh != 1 || p.dw != 1;
  if (dilated && !(p.sw == 1 && dwcol_uses_dot4(p) && p.dh <= 64 && p.dw <= 64)) return false;
  // The walk's steady-state steps fetch row iy_first + t + 2 + NBUF with no lower bound (only the start-up steps
  // check it): any API-legal padding beyond the window's own reach (top / left > 2 [x the dilation], which no 3x3 layer
  // of a real network has) would index rows before the image. Those shapes take the generic kernels.
  if (p.pad_top > 2 * p.dh || p.pad_left > 2 * p.dw) return false;
  // 32-bit byte offsets into both tensors
  const uint64_t in_bytes = static_cast<uint64_t>(p.batch) * p.H * p.W * p.in_stride;
  const uint64_t out_bytes = static_cast<uint64_t>(p.batch) * p.OH * p.OW * p.out_stride;
  if (in_bytes >= (UINT64_C(1) << 31) || out_bytes >= (UINT64_C(1) << 32)) return false;
  const uint32_t cols = p.OW * (p.C / 4);
  const uint32_t chunks = (cols + 63u) / 64u;
  // Row segments: each re-loads its halo (two rows at stride 1) and builds the first pairs again, so as few as
  // still give every SIMD several waves' worth of work (the tail of the last round is what it buys back).
  // (dilated: a "segment" here is one segment of EVERY residue class of the output rows, rows_v rows each at most)
  const uint32_t rows_v = dilated ? (p.OH + p.dh - 1) / p.dh : p.OH;
  const uint32_t classes = dilated ? p.dh : 1u;
  const uint64_t waves_per_seg = static_cast<uint64_t>(p.batch) * chunks * classes;
  // (measured on the MobileNetV2 layers, batch 128: 1.3-2 rounds of waves beat 3-4 -- 35.6 against 39.6 us on
  //  layer 8 -- now that the rows in flight are really in flight; shorter segments only add start-ups and halo rows)
  // wave slots the segment count is sized for: 6 per SIMD at stride 2, 5 at stride 1 (what the 79- and 82-VGPR kernels
  // of the time allowed; today's 70-72 VGPRs would admit 7, but a rows-per-segment sweep of the present kernels --
  // QNNP_GFX950_DW_COL_ROWS, same box -- found this choice at or within 3 % of the best on all ten MobileNetV2 layers:
  // more, shorter segments pay the ~8k-cycle start-up of a wave again)
  const uint64_t slots = static_cast<uint64_t>(p.cu_count) * 4u * (p.sw == 1 ? 5u : 6u);
  const uint64_t target = slots * 3u / 2u;                                         // ~1.5 rounds
  uint32_t segs = static_cast<uint32_t>((target + waves_per_seg - 1) / waves_per_seg);
  // Stride 1 with enough columns to give every SIMD a few waves: at most ONE round (28x28x192, batch 128: two
  // segments 15.2 us, four 16.6; 14x14x576: one 12.5, two 14.3 -- a second, partly filled round costs more than it
  // hides; the stride-2 layers are HBM-bound and keep the deeper queue)
  if (p.sw == 1 && waves_per_seg * 5u >= slots * 2u) {
    const uint32_t one_round = static_cast<uint32_t>(slots / waves_per_seg);
    segs = one_round < 1u ? 1u : one_round;
  }
  const uint32_t min_rows = 7;
  uint32_t max_segs = rows_v / min_rows;
  if (max_segs < 1) max_segs = 1;
  if (segs > max_segs) segs = max_segs;
  if (segs < 1) segs = 1;
  uint32_t toh = (rows_v + segs - 1) / segs;
  if (const uint32_t forced = col_rows_override()) toh = forced < rows_v ? forced : rows_v;
  p.TOH = toh;
  p.slabs = ((rows_v + toh - 1) / toh) * classes;
  p.bands = chunks;
  const uint64_t waves = static_cast<uint64_t>(p.batch) * p.slabs * chunks;
  // (the kernel divides wave and column indices through 32-bit reciprocals: exact while dividend * divisor < 2^32)
  const uint64_t dmax = chunks > p.slabs ? chunks : p.slabs;
  if ((waves + 8u * (kColThreads / 64)) * dmax >= (UINT64_C(1) << 32)) return false;
  if (static_cast<uint64_t>(cols) * (p.C / 4) >= (UINT64_C(1) << 32)) return false;
  return waves < (UINT64_C(1) << 31);
}

// stride 1 with weights in int8 range (DwParams::wrange): the v_dot4_i32_i8 flavour of kernel G
bool dwcol_uses_dot4(const DwParams& p)
{
  bool quad = p.sw == 1u && (p.wrange == 1u || p.wrange == 2u) && p.dot4 != nullptr;
#ifdef QNNP_ENABLE_ABLATION
  if (const char* env = getenv("QNNP_GFX950_DW_COL_QUAD")) quad = quad && atoi(env) != 0;
#endif
  return quad;
}

int dwcol_launch(const DwParams& geometry, hipStream_t stream)
{
  DwParams p = geometry;
  p.inv_dh = reciprocal_ceil(p.dh);
  p.inv_bands = reciprocal_ceil(p.bands);
  p.inv_slabs = reciprocal_ceil(p.slabs);
  p.inv_q4 = reciprocal_ceil(p.C / 4u);
  p.xcd_ranges = (static_cast<uint64_t>(p.batch) * p.H * p.W * p.in_stride +
                  static_cast<uint64_t>(p.batch) * p.OH * p.OW * p.out_stride) <= (UINT64_C(96) << 20) ? 1u : 0u;
  const uint64_t waves = static_cast<uint64_t>(p.batch) * p.slabs * p.bands;
  const uint32_t blocks = static_cast<uint32_t>((waves + (kColThreads / 64) - 1) / (kColThreads / 64));
  // every flavour twice: plain, and with the output table in its epilogue (p.table, the TAB flavour of the kernel)
#define QNNP_DW_COL_LAUNCH(...)                                                                                        \
  do {                                                                                                               \
    if (p.table != nullptr) {                                                                                        \
      hipLaunchKernelGGL((q8_dwconv_col3x3_kernel<__VA_ARGS__, true>), dim3(blocks), dim3(kColThreads), 0, stream, p); \
    } else {                                                                                                         \
      hipLaunchKernelGGL((q8_dwconv_col3x3_kernel<__VA_ARGS__, false>), dim3(blocks), dim3(kColThreads), 0, stream, p); \
    }                                                                                                                \
  } while (0)
  qnnp::requant_dispatch_ofs(p.rq, [&](auto seq, auto full) {
    constexpr int kSeq = decltype(seq)::value;
    constexpr bool kFull = decltype(full)::value;
    if (p.dh != 1 || p.dw != 1) {                  // (dwcol_plan: stride 1, the int8 flavour)
      if (p.TOH >= 12u) {
        QNNP_DW_COL_LAUNCH(1, kSeq, kFull, true, true, true);
      } else {
        QNNP_DW_COL_LAUNCH(1, kSeq, kFull, false, true, true);
      }
    } else if (p.sw == 1) {
      // four rows in flight (see the kernel) when a segment is long enough to use them: 112x112x32 30.7 -> 29.1 us,
      // 56x56x144 33.4 -> 32.3, 14-row segments level, 7x7x960 8.25 -> 8.55 with its six-row start-up
      bool deep = p.TOH >= 12u;
#ifdef QNNP_ENABLE_ABLATION
      if (const char* env = getenv("QNNP_GFX950_DW_COL_DEEP")) deep = atoi(env) != 0;
#endif
      const bool quad = dwcol_uses_dot4(p);
      if (quad && deep) {
        QNNP_DW_COL_LAUNCH(1, kSeq, kFull, true, true, false);
      } else if (quad) {
        QNNP_DW_COL_LAUNCH(1, kSeq, kFull, false, true, false);
      } else if (deep) {
        QNNP_DW_COL_LAUNCH(1, kSeq, kFull, true, false, false);
      } else {
        QNNP_DW_COL_LAUNCH(1, kSeq, kFull, false, false, false);
      }
    } else {
      QNNP_DW_COL_LAUNCH(2, kSeq, kFull, false, false, false);
    }
  });
#undef QNNP_DW_COL_LAUNCH
  return launch_status();
}

}  // namespace qnnp
