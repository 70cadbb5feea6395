/*
 * dwconv_params.h -- kernel-argument block shared by the depthwise kernels, and what each kernel unit exports
 * (q8dwconv.hip: the generic kernels, the plan and the launch switch; q8dwlds.hip, q8dwrow.hip, q8dwcol.hip, q8dwcol5.hip,
 * q8dwmfma.hip, q8dwmfma16.hip: one kernel family each).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "qnnp_hip.h"
#include "requant.hip.h"

namespace qnnp {

struct DwParams {
  const uint8_t* input;
  uint8_t* output;
  const int16_t* wadj;
  const int32_t* bias1;
  uint32_t batch;
  uint32_t H, W, OH, OW;
  uint32_t C, c_pad;
  uint32_t KH, KW;
  uint32_t sh, sw, dh, dw;
  uint32_t pad_top, pad_left;
  uint32_t in_stride, out_stride;
  uint32_t izp;
  // LDS-tiled kernel geometry
  uint32_t CS;        // channels per slab (multiple of 4, divides C)
  uint32_t TOH;       // output rows per band
  uint32_t IR, IC;    // staged input rows / columns per band
  uint32_t PP;        // LDS dwords per (row, 4-channel group) line: IC padded for bank spread
  uint32_t bands;     // ceil(OH / TOH)
  uint32_t slabs;     // C / CS
  uint32_t cu_count;  // compute units of the bound device
  // matrix-core kernel
  const int8_t* dwm_x;
  const int32_t* dwm_bias;
  uint32_t dwm_parts, c_pad32;
  uint32_t wrange;       // qnnp_dwconv_weight_range of wadj (pack.h): 1 / 2 = the int8 dot-product flavour of kernel G applies
  const uint32_t* dot4;  // [4][c_pad] register image of that flavour (pack.h qnnp_pack_dwconv_dot4), or null
  uint32_t xcd_ranges;   // kernel G: 1 = contiguous ranges of the work per XCD (dwcol_launch)
  uint32_t inv_bands, inv_slabs, inv_q4;   // kernel G: ceil(2^32 / d) of its three divisors (0 when d == 1), dwcol_launch
  uint32_t inv_dh;       // kernel G, dilated flavour: the same for the row dilation
  uint32_t store_mode;   // as igemm_epilogue.hip.h: 2 = 16-byte stores, 1 = dword stores, 0 = byte stores
  uint32_t abl;          // measurement builds only: bit 0 = no stores, bit 1 = no global loads (kernel F)
  unsigned long long* trace;   // measurement builds only (QNNP_ENABLE_ABLATION + env QNNP_GFX950_TRACE)
  qnnp::RequantDev rq;
  uint32_t stream_out;       // 1: the column-walk kernels mark their output stores as streaming ("streaming_stores")
  const uint8_t* table;      // kernels G and H: the output table their TAB flavour applies (qnnp_hip_dwconv_args::table), or null
};

// cycle stamp of thread 0 of the first 4096 workgroups into trace[blockIdx.x * 32 + slot]; compiled out of the product
#ifdef QNNP_ENABLE_ABLATION
#define QNNP_DW_TRACE(p, slot)                                                                      \
  do {                                                                                              \
    if ((p).trace != nullptr && threadIdx.x == 0 && blockIdx.x < 4096)                              \
      (p).trace[(blockIdx.x * 4) * 8 + (slot)] = __builtin_readcyclecounter();                     \
  } while (0)
#else
#define QNNP_DW_TRACE(p, slot) do { } while (0)
#endif

// measurement knob, read once: output rows per segment of kernels G, H and M16 (0 = automatic)
inline uint32_t col_rows_override()
{
  static const uint32_t rows = [] {
    if (const char* env = getenv("QNNP_GFX950_DW_COL_ROWS")) {
      const int v = atoi(env);
      if (v >= 1 && v <= 4096) return static_cast<uint32_t>(v);
    }
    return 0u;
  }();
  return rows;
}

/* A unit's dw*_plan answers whether its kernel takes the shape and, when it does, writes the launch geometry into the
 * plan fields of `p` (CS .. slabs; each unit says what they mean for its kernel). A plan that REFUSES may have written
 * some of them already: make_plan's order of calls decides what a later kernel finds there (tests/golden/dwconv_plans.txt
 * pins it). dw*_launch launches `p` as planned on `stream` and returns the launch status. */

/* q8dwlds.hip: kernel A */
bool dwlds_plan(DwParams& p);
int dwlds_launch(const DwParams& p, bool vec16, hipStream_t stream);

/* q8dwrow.hip: kernel C; `unaligned` = its flavour for any channel count >= 4 and any alignment */
bool dwrow_plan(DwParams& p, bool unaligned = false);
int dwrow_launch(const DwParams& p, hipStream_t stream, bool unaligned = false);

/* q8dwcol.hip: kernel G */
bool dwcol_plan(DwParams& p);
bool dwcol_uses_dot4(const DwParams& p);
int dwcol_launch(const DwParams& p, hipStream_t stream);

/* q8dwcol5.hip: kernel H */
bool dwcol5_plan(DwParams& p);
int dwcol5_launch(const DwParams& p, hipStream_t stream);

/* q8dwmfma.hip: kernels D and F */
bool dwmfma_plan(const DwParams& p, const struct qnnp_hip_dwconv_args* a);
int dwmfma_launch(const DwParams& p, hipStream_t stream);
bool dwmfma_lds_plan(DwParams& p, const struct qnnp_hip_dwconv_args* a);
int dwmfma_lds_launch(const DwParams& p, hipStream_t stream);

/* q8dwmfma16.hip: kernel M16 */
bool dwmfma16_plan(DwParams& p, uintptr_t in_addr, uintptr_t out_addr);
int dwmfma16_launch(const DwParams& p, hipStream_t stream);

}  // namespace qnnp
