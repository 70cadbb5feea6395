/*
 * q8pwconv.hip -- the pointwise streaming kernels' launch plan and launch switch. The kernels themselves live in one unit
 * per family and share pwstream_common.hip.h; each unit exposes its launch entry only (igemm_params.h). Every family works
 * on 32-row x 32-channel blocks of a pointwise (1x1) convolution or fully-connected layer, one wave per block, MFMA operands
 * in registers, no barrier in the loop.
 *
 *   family   unit             kernel                          code  shapes
 *   Stream   q8pwstream.hip   q8_pw_stream_mfma_kernel        5     K <= 256, weights + bias <= 64 KiB in LDS; rows of one channel
 *                                                                   block or not 16-byte aligned; depth-to-space stores (D2S)
 *   Staged   q8pwstaged.hip   q8_pw_stream_staged_kernel      5     K <= 256, 16-byte aligned rows (or dense 8 mod 16), any N in
 *                                                                   workgroup columns; strided 1x1 through a table row per pixel
 *   LongK    q8pwlongk.hip    q8_pw_stream_longk_kernel       9     256 < K <= 1024, 16-byte aligned rows, weights of a column
 *                                                                   <= 96 KiB in LDS
 *   Gw       q8pwgw.hip       q8_pw_stream_gw_kernel          6     any K and N, 16-byte aligned input rows, weights from L2
 *   Gwk      q8pwgw.hip       q8_pw_stream_gwk_kernel         6     the same with K >= 256 and few blocks: K split over the waves
 *
 * ("code": the "gemm_kernel" value that forces the family's plan, include/qnnpack_gfx950_test.h. The 3-channel streaming kernels
 * are no part of this: q8convc3s.hip plans and launches them.)
 *
 * A plan (PwPlan, igemm_params.h) is everything a launch decides: the instantiation -- K blocks, load width, the RES / TAB / PF /
 * D2S flavour --, the grid, the dynamic LDS, the staged kernels' channel columns. q8igemm.hip asks for it once per run, when it
 * asks whether the family takes the layer, and hands it back to pwstream_launch. The plan decides speed, not bytes;
 * tests/test_igemm_plan_host.py holds it to a record.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "pwstream_common.hip.h"

namespace qnnp {

namespace {

/* the table flavour takes a launch planned for `lds_bytes` when the table fits the kernel's budget behind them and the
 * launch stays as resident as it was: never a lower occupancy for the fold */
bool table_fits(uint32_t by_registers, uint32_t lds_bytes, uint32_t budget)
{
  return lds_bytes + kTableLds <= budget &&
         resident_per_cu(by_registers, lds_bytes + kTableLds) == resident_per_cu(by_registers, lds_bytes);
}

/* the stream kernel's LDS: the whole weight matrix and the bias */
uint32_t pw_lds_bytes(const IgemmParams& p)
{
  const uint32_t kb = (p.k_total + 31u) / 32u;
  // the bias region is rounded up to whole 1 KiB LDS-DMA rows (a wave-instruction always writes 64 x 16 B)
  return (p.n_pad / 32u) * kb * 1024u + ((p.n_pad * 4u + 1023u) & ~1023u);
}

/* the staged kinds' LDS: a column's weights and bias, and the four waves' images */
uint32_t staged_lds_bytes(uint32_t kb, uint32_t nbp, uint32_t pitch)
{
  return nbp * kb * 1024u + ((nbp * 128u + 1023u) & ~1023u) + kWaves * 32u * pitch;
}

uint32_t log2_pieces(uint32_t row_bytes)       // log2(16-byte pieces per image row) of a chunked image: pitch = 2^k * 16 >= row_bytes
{
  uint32_t lg = 1;
  while ((16u << lg) < row_bytes) lg++;
  return lg;
}

/* How a staged kernel covers an N: whole rows per unit when that fills the chip (and fits `lds_limit`), else columns of 8 / 4 /
 * 2 channel blocks -- the widest that still gives every wave slot `fill` units (the staged kernel about two: it prefetches
 * the next one; the long-K kernel one). Fills nbp, grid_y, log_cpr, lds_bytes and per_cu. */
bool plan_columns(const IgemmParams& p, uint32_t kb, uint32_t lds_limit, uint32_t fill, uint32_t base_per_cu, bool nbp_knob, PwPlan* plan)
{
  const uint32_t nblocks = p.n_pad / 32u;
  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t slots = p.cu_count * base_per_cu * kWaves;
  const bool dense = p.output_stride == p.n;
  const uint32_t log_whole = log2_pieces(nblocks * 32u);
  const uint32_t whole_pitch = dense ? p.n : (16u << log_whole);
  const uint32_t whole_lds = staged_lds_bytes(kb, nblocks, whole_pitch);
  const bool whole_fits = whole_lds <= lds_limit;
  uint32_t nbp = 0;
  if (whole_fits && (units >= slots || nblocks < 4u)) {
    nbp = nblocks;
  } else {
    // (columns of a single block measured worse: 7x7x960 -> 320 12.7 -> 14.3 us)
    for (uint32_t cand = 8; cand >= 2; cand >>= 1) {
      if (cand >= nblocks || staged_lds_bytes(kb, cand, cand * 32u) > lds_limit) continue;
      nbp = cand;
      if (static_cast<uint64_t>(units) * ((nblocks + cand - 1) / cand) >= static_cast<uint64_t>(fill) * slots) break;
    }
    if (nbp == 0) {
      if (!whole_fits) return false;
      nbp = nblocks;
    }
  }
#ifdef QNNP_ENABLE_ABLATION
  if (const char* env = nbp_knob ? getenv("QNNP_PW_NBP") : nullptr) {   // measurement builds: channel blocks per workgroup column
    const uint32_t forced = static_cast<uint32_t>(atoi(env));
    if (forced >= 1 && forced <= nblocks && staged_lds_bytes(kb, forced, forced >= nblocks ? whole_pitch : forced * 32u) <= lds_limit) {
      nbp = forced >= nblocks ? nblocks : forced;
    }
  }
#endif
  plan->nbp = nbp;
  plan->grid_y = (nblocks + nbp - 1) / nbp;
  plan->log_cpr = plan->grid_y == 1 ? log_whole : log2_pieces(nbp * 32u);
  plan->lds_bytes = plan->grid_y == 1 ? whole_lds : staged_lds_bytes(kb, nbp, nbp * 32u);
  plan->per_cu = resident_per_cu(base_per_cu, plan->lds_bytes);
  return true;
}

/* The staged kernel's plan: dense8 in front of the column search. */
bool plan_staged(const IgemmParams& p, uint32_t kb, uint32_t vec, PwPlan* plan)
{
  const uint32_t base_per_cu = static_cast<uint32_t>(staged_waves(static_cast<int>(kb)));
  // dense rows of 8 (mod 16) bytes from a 16-byte aligned base: every 32-row block starts 16-byte aligned
  const bool dense8 = p.n % 16u == 8u && p.output_stride == p.n && reinterpret_cast<uintptr_t>(p.output) % 16u == 0 &&
      p.d2s_sh == 0 && p.rows >= 32u &&
      // (a residual rides in the 16-byte-load flavour only: pw_staged_launch)
      (p.residual == nullptr || (vec == 16 && p.residual_stride == p.n && reinterpret_cast<uintptr_t>(p.residual) % 16u == 0));
  if (dense8) {
    const uint32_t nb = p.n_pad / 32u;
    const uint32_t lg = log2_pieces(nb * 32u);
    const uint32_t lds = staged_lds_bytes(kb, nb, 16u << lg);
    if (lds > kMaxLds) return false;
    plan->nbp = nb;
    plan->grid_y = 1;
    plan->log_cpr = lg | 0x80000000u;                          // stream_copy_out's third mode
    plan->lds_bytes = lds;
    plan->per_cu = resident_per_cu(base_per_cu, lds);
    return true;
  }
  if (p.store_mode != 2 || p.n % 16u != 0 || p.d2s_sh != 0) return false;
  return plan_columns(p, kb, kMaxLds, 2u, base_per_cu, true, plan);
}

/* which instantiation the host's requantization dispatch picks (the units' launch entries make the same call) */
void lane_flavour(const IgemmParams& p, PwPlan* plan)
{
  requant_dispatch_lane(p.rq, p.lane, [&](auto seq, auto full) { plan->seq = decltype(seq)::value; plan->full = decltype(full)::value; });
}

uint32_t per_cu_knob(uint32_t per_cu)
{
#ifdef QNNP_ENABLE_ABLATION
  if (const char* env = getenv("QNNP_PW_BLOCKS")) per_cu = static_cast<uint32_t>(atoi(env));
#endif
  return per_cu;
}

}  // namespace

/* The short-K kernels. Pointwise / fully-connected form (no offset table, or the table of a strided 1x1 convolution), one
 * group, K <= 256; the stream kernel where one of its conditions holds and weights + bias fit 64 KiB, else the staged one. */
bool pwstream_plan(const IgemmParams& p, uint32_t groups, uint32_t vec, bool want_table, PwPlan* plan)
{
  if ((p.offsets != nullptr && p.offsets_dense == 0) || groups != 1 || (vec != 16 && vec != 8)) return false;
  if (p.fill_table == nullptr || p.rows == 0 || p.k_total == 0 || p.k_total > 256u) return false;
  if (p.k_total % vec != 0) return false;
  const uint32_t kb = (p.k_total + 31u) / 32u;
  const bool table = want_table && p.residual == nullptr;
  *plan = PwPlan{};
  plan->kb = kb;
  plan->vec = vec;
  // 16-byte aligned rows wider than one channel block: the staged flavour (whole-line stores, N in columns)
  // (one 32-channel block per row: the first kernel keeps it -- 28x28x192 -> 32 measured 7.1 us there, 8.1 here)
  if (p.d2s_sh == 0 && p.n != 32 && plan_staged(p, kb, vec, plan)) {
    plan->family = PwFamily::Staged;
    plan->res = vec == 16 && p.residual != nullptr;          // (a residual implies 16-byte aligned rows: q8igemm.hip)
    plan->tab = table && table_fits(static_cast<uint32_t>(staged_waves(static_cast<int>(kb))), plan->lds_bytes, kMaxLds);
    if (plan->tab) plan->lds_bytes += kTableLds;               // (at the same residency: per_cu stands)
    plan->grid_x = persistent_grid(p, per_cu_knob(plan->per_cu), plan->grid_y);
    lane_flavour(p, plan);
    return true;
  }
  // the stream kernel: the whole matrix in LDS, no offset table; depth-to-space stores with 16-byte loads only
  const uint32_t lds_bytes = pw_lds_bytes(p);
  if (p.offsets != nullptr || lds_bytes > kMaxLds || (p.d2s_sh != 0 && vec != 16)) return false;
  const uint32_t by_registers = kb <= 5 ? 4u : 2u;             // LDS bounds the residency: kMaxLds -> 2 per CU, half of that -> 4
  plan->family = PwFamily::Stream;
  plan->d2s = p.d2s_sh != 0;
  plan->res = !plan->d2s && p.residual != nullptr;
  plan->tab = !plan->d2s && table && table_fits(by_registers, lds_bytes, kMaxLds);
  plan->lds_bytes = lds_bytes + (plan->tab ? kTableLds : 0u);
  plan->per_cu = per_cu_knob(resident_per_cu(by_registers, plan->lds_bytes));
  plan->grid_x = persistent_grid(p, plan->per_cu);
  plan->grid_y = 1;
  plan->seq = plan->full = -1;                                 // the kernel dispatches itself
  return true;
}

/* The long-K kernel: pointwise / fully-connected form, one group, 16-byte aligned rows both sides, 256 < K <= 1024. Like the
 * staged plan with the run-time K block count and its own LDS limit. */
bool pwstream_longk_plan(const IgemmParams& p, uint32_t groups, uint32_t vec, bool want_table, PwPlan* plan)
{
  if (p.offsets != nullptr || groups != 1 || vec != 16) return false;
  if (p.fill_table == nullptr || p.rows == 0 || p.k_total <= 256u) return false;
  if (p.store_mode != 2 || p.n % 16u != 0 || p.d2s_sh != 0 || p.k_total % 16u != 0) return false;
  const uint32_t kb = (p.k_total + 31u) / 32u;
  if (kb <= 8 || kb > 32) return false;
  const uint32_t kbmax = kb <= 12 ? 12 : (kb <= 20 ? 20 : 32);
  const uint32_t base_per_cu = static_cast<uint32_t>(longk_waves(static_cast<int>(kbmax)));
  *plan = PwPlan{};
  if (!plan_columns(p, kb, kMaxLdsLongK, 1u, base_per_cu, false, plan)) return false;
  plan->family = PwFamily::LongK;
  plan->kb = kbmax;
  plan->vec = 16;
  plan->res = p.residual != nullptr;
  // more units than waves: the flavour that requests the next unit's rows before it multiplies the current one
  // (PF: 2 waves per SIMD by its registers)
  const uint32_t units = (p.rows + 31u) / 32u;
  const uint32_t per_cu_pf = plan->per_cu < 2u ? plan->per_cu : 2u;
  const uint32_t gx_pf = (p.cu_count * per_cu_pf + plan->grid_y - 1) / plan->grid_y;
  plan->pf = !plan->res && kbmax <= 20 && static_cast<uint64_t>(gx_pf) * kWaves * 5u <= static_cast<uint64_t>(units) * 4u;   // >= 1.25 units per wave
  // (behind the choice of PF: the table changes nothing about it)
  plan->tab = want_table && !plan->res && table_fits(base_per_cu, plan->lds_bytes, kMaxLdsLongK);
  if (plan->tab) plan->lds_bytes += kTableLds;
  if (plan->pf) plan->per_cu = per_cu_pf;
  plan->grid_x = persistent_grid(p, plan->per_cu, plan->grid_y);
  lane_flavour(p, plan);
  return true;
}

/* The global-weights kernels: pointwise / fully-connected form, one group, 16-byte aligned rows, any K and N */
bool pwstream_gw_plan(const IgemmParams& p, uint32_t groups, uint32_t vec, bool want_table, PwPlan* plan)
{
  if (p.offsets != nullptr || groups != 1 || vec != 16) return false;
  if (p.fill_table == nullptr || p.rows == 0 || p.k_total == 0 || p.k_total % 16 != 0) return false;
  const uint64_t units64 = static_cast<uint64_t>((p.rows + 31u) / 32u) * (p.n_pad / 32u);
  const uint64_t in_bytes = static_cast<uint64_t>(p.rows - 1u) * p.input_stride + p.k_total;   // buffer addressing
  if (units64 >= (UINT64_C(1) << 31) || in_bytes >= (UINT64_C(1) << 31)) return false;
  const uint32_t units = static_cast<uint32_t>(units64);
  // long reductions: K split over the four waves of a workgroup (one workgroup per block)
  // (only when the blocks alone cannot fill the chip -- classifier heads: with ~2000 blocks the one-wave-per-block
  //  kernel was 7-25 % faster, same box: the split costs three more waves' loads of the row block and a barrier)
  bool split_k = p.k_total >= 256u && units <= 2u * p.cu_count;
#ifdef QNNP_ENABLE_ABLATION
  if (const char* env = getenv("QNNP_GW_SPLITK")) split_k = atoi(env) != 0;
#endif
  *plan = PwPlan{};
  plan->family = split_k ? PwFamily::Gwk : PwFamily::Gw;
  plan->vec = 16;
  if (split_k) plan->depth = ((p.k_total + 31u) / 32u + kWaves - 1) / kWaves <= 4 ? 4 : 8;
  plan->res = p.residual != nullptr;
  // (no dynamic LDS to compete with: the table's 256 B stand alone or beside the 12 KiB of partial sums)
  plan->tab = want_table && !plan->res;
  plan->grid_x = split_k ? units : (units + kWaves - 1) / kWaves;
  plan->grid_y = 1;
  plan->seq = plan->full = -1;                                 // the kernels dispatch themselves
  return true;
}

const char* pwstream_kernel_name(const PwPlan& plan)
{
  switch (plan.family) {
    case PwFamily::Stream: return plan.d2s ? "q8_pw_stream_d2s_mfma" : "q8_pw_stream_mfma";
    case PwFamily::Staged: return "q8_pw_stream_mfma";
    case PwFamily::LongK: return "q8_pw_stream_longk_mfma";
    case PwFamily::Gw: return "q8_pw_stream_gw_mfma";
    case PwFamily::Gwk: return "q8_pw_stream_gwk_mfma";
    case PwFamily::C3: return "q8_conv_stream_c3_mfma";
    default: return nullptr;
  }
}

/* p: the parameters the plan was made from, with the table where the plan folds it */
int pwstream_launch(const IgemmParams& p, const PwPlan& plan, hipStream_t stream, const char** name)
{
  *name = pwstream_kernel_name(plan);
  switch (plan.family) {
    case PwFamily::Stream: return pw_stream_launch(p, plan, stream);
    case PwFamily::Staged: return pw_staged_launch(p, plan, stream);
    case PwFamily::LongK: return pw_longk_launch(p, plan, stream);
    case PwFamily::Gw: case PwFamily::Gwk: return pw_gw_launch(p, plan, stream);
    default: return QNNP_HIP_EINVAL;
  }
}

}  // namespace qnnp
