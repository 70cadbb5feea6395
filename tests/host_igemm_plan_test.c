/*
 * host_igemm_plan_test.c -- TEST INFRASTRUCTURE: the kernel choice of the implicit-GEMM dispatcher and the launch plan of
 * the pointwise streaming kernels, as text.
 *
 * A stand-alone program (Makefile target igemm-plan) linked against libqnnpack_gfx950.so itself: no sanitizer, no stub.
 * It calls qnnp_hip_igemm_plan (hip/qnnp_hip.h) on a fixed list of argument blocks and prints one line per case: the
 * case, the status, the kernel a run would report and every field of the plan. tests/test_igemm_plan_host.py compares
 * the output with tests/golden/igemm_plans.txt line for line. The plan decides speed, not bytes -- which kernel, which
 * flavour, grid, LDS, channel columns -- so no parity test sees it change; this file does.
 *
 * The library is never initialised: qnnp::active_cu_count() answers its no-device value of 256 on every machine (the
 * MI355X's own count), and nothing touches a device. The pointers are made-up addresses, chosen for their low bits
 * and never dereferenced.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hip/qnnp_hip.h"

/* the enumerators of q8igemm.hip's Kernel and Image BY VALUE: this order is those enums' order, and a new or moved
 * enumerator there needs the same edit here (the golden then differs in every line it touches) */
static const char* const kKernelNames[] = {"Generic", "Wave", "Ws16s", "Patch", "Lds", "Rows16", "Rows32", "C3",
                                           "Mid", "U", "Pw", "LongK", "Gw", "Big", "BigC", "BigX"};
static const char* const kImageNames[] = {"Standard", "Centred", "Rows", "Rowsum"};
static const char* const kFamilyNames[] = {"none", "stream", "staged", "longk", "gw", "gwk", "c3"};

#define IN_BASE UINT64_C(0x7f1000000000)
#define OUT_BASE UINT64_C(0x7f5000000000)
#define RES_BASE UINT64_C(0x7f7000000000)
#define TABLE_BASE UINT64_C(0x7f9000000000)

enum { kResNone = 0, kResMatching, kResOtherStride, kResMisaligned };

/* one convolution or fully connected operator as convolution.c / fully-connected.c hand it to qnnp_hip_igemm_run */
struct layer {
  uint32_t batch, h, w, kh, kw, s, d, groups, gic, goc;
  uint32_t kzp;                    /* kernel zero point: 127 has the centred images where convolution.c packs them */
  int variant;
  uint32_t in_off, out_off;        /* added to the base addresses */
  uint32_t in_extra, out_extra;    /* pixel strides = channels + extra */
  int residual;                    /* kRes* */
  int table;                       /* 1: an output table is attached */
  uint32_t d2s;                    /* depth-to-space stride (deconvolution with kernel == stride), 0 = off */
  int per_channel;
  int rq;                          /* 0: shift 1, full clamp; 1: shift 0; 2: shift 1, clamp [1, 254] */
};

static struct layer pointwise(uint32_t batch, uint32_t hw, uint32_t gic, uint32_t goc)
{
  struct layer l;
  memset(&l, 0, sizeof(l));
  l.batch = batch; l.h = hw; l.w = hw; l.kh = 1; l.kw = 1; l.s = 1; l.d = 1; l.groups = 1; l.gic = gic; l.goc = goc; l.kzp = 127;
  return l;
}

static uint32_t round_up(uint32_t x, uint32_t q) { return (x + q - 1) / q * q; }

static void plan_line(const char* name, const struct layer* l)
{
  static const struct qnnp_hip_add_params add;             /* copied into the kernel arguments, never looked at */
  uint32_t residual_folded = 0, table_folded = 0;
  const uint32_t eh = (l->kh - 1) * l->d + 1, ew = (l->kw - 1) * l->d + 1;
  const uint32_t pad_top = eh / 2, pad_left = ew / 2;      /* bench.py's conv_geometry */
  const uint32_t oh = (pad_top + l->h + (eh - 1 - eh / 2) - eh) / l->s + 1, ow = (pad_left + l->w + (ew - 1 - ew / 2) - ew) / l->s + 1;
  const int is_conv = !(l->kh == 1 && l->kw == 1 && l->s == 1);
  const uint32_t taps = l->kh * l->kw;
  const uint32_t kc_slot = (is_conv && l->groups == 1 && l->gic == 3) ? 4u : l->gic;
  const uint32_t k_total = taps * kc_slot;
  const uint32_t in_channels = l->groups * l->gic, out_channels = l->groups * l->goc;
  struct qnnp_hip_igemm_args a;
  memset(&a, 0, sizeof(a));
  a.input = (const uint8_t*) (uintptr_t) (IN_BASE + l->in_off);
  a.output = (uint8_t*) (uintptr_t) (OUT_BASE + l->out_off);
  a.packed_w = (const int8_t*) (uintptr_t) TABLE_BASE;
  a.bias2 = (const int32_t*) (uintptr_t) (TABLE_BASE + 0x100000);
  a.bias2_pair = 1;
  a.offsets = is_conv ? (const int32_t*) (uintptr_t) (TABLE_BASE + 0x200000) : NULL;
  a.rows = l->batch * oh * ow;
  a.rows_per_image = oh * ow;
  a.input_stride = in_channels + l->in_extra;
  a.output_stride = out_channels + l->out_extra;
  a.image_stride = (uint64_t) l->h * l->w * a.input_stride;
  a.input_bytes = ((uint64_t) l->batch * l->h * l->w - 1) * a.input_stride + in_channels;
  a.groups = l->groups;
  a.n = l->goc;
  a.n_pad = round_up(l->goc, 32);
  a.kc = l->gic;
  a.kc_slot = kc_slot;
  a.ks = taps;
  a.k_total = k_total;
  a.k_pad = round_up(k_total, 64);
  a.row_coeff = 128 - (int32_t) l->kzp;
  a.input_zero_point = 127;
  a.variant = l->variant;
  a.input_height = l->h; a.input_width = l->w; a.output_height = oh; a.output_width = ow;
  a.kernel_height = l->kh; a.kernel_width = l->kw; a.stride_height = l->s; a.stride_width = l->s;
  a.dilation_height = l->d; a.dilation_width = l->d; a.pad_top = is_conv ? pad_top : 0; a.pad_left = is_conv ? pad_left : 0;
  a.streaming_mode = 1;
  /* any valid requantization: it selects the SEQ / FULL instantiation and nothing else */
  a.rq.multiplier = 0x40000000;
  a.rq.shift = l->rq == 1 ? 0 : 1;
  a.rq.remainder_mask = l->rq == 1 ? 0 : 1;
  a.rq.remainder_threshold = 0;
  a.rq.output_min_less_zero_point = l->rq == 2 ? -126 : -127;
  a.rq.output_max_less_zero_point = l->rq == 2 ? 127 : 128;
  a.rq.output_zero_point = 127;
  /* convolution.c pack_gemm: the centred image exists for one group, whole 32-deep K blocks and kernel zero point 128, or 127
   * where a kernel takes a second image (1x1 with K % 64 == 0 and channels % 4 == 0; the small 3x3 windows are no part of
   * this list) */
  a.packed_w_centred = a.packed_w;
  a.bias2_centred = a.bias2;
  if (l->groups == 1 && kc_slot == l->gic && k_total % 32 == 0) {
    if (l->kzp == 128) {
      a.centre_flip = 0x80;
    } else if (l->kzp == 127 && taps == 1 && k_total % 64 == 0 && l->goc % 4 == 0) {
      a.centre_flip = 0x7F;
      a.packed_w_centred = (const int8_t*) (uintptr_t) (TABLE_BASE + 0x300000);
      a.bias2_centred = (const int32_t*) (uintptr_t) (TABLE_BASE + 0x400000);
    }
  }
  /* convolution.c pack_rows: the row-slot image of 3-channel first layers, centred where the kernel zero point is 127 */
  if (kc_slot == 4 && l->d == 1 &&
      ((l->kh <= 4 && l->kw * 3 <= 16 && a.n_pad <= 64) || ((l->kh == 5 || l->kh == 7) && l->kw * 3 <= 32 && a.n_pad <= (l->kh == 7 ? 96u : 64u)))) {
    a.packed_w_rows16 = (const int8_t*) (uintptr_t) (TABLE_BASE + 0x500000);
    if (l->kzp == 127) a.bias2_rows = (const int32_t*) (uintptr_t) (TABLE_BASE + 0x600000);
  }
  /* convolution.c launch_igemm_kernel: grouped 1x1 over many rows runs on the dense image */
  if (!is_conv && l->groups > 1 && in_channels <= 1024 && out_channels <= 1024 && l->residual == kResNone && l->variant == 0 &&
      a.rows >= 65536u) {
    a.groups = 1;
    a.n = out_channels;
    a.n_pad = round_up(out_channels, 32);
    a.kc = a.kc_slot = a.k_total = in_channels;
    a.k_pad = round_up(in_channels, 64);
    a.centre_flip = 0;
  }
  if (l->d2s != 0) {               /* deconvolution.c: stride x stride phases of round_up(n, 32) packed columns */
    a.d2s_stride_h = a.d2s_stride_w = l->d2s;
    a.d2s_input_h = l->h;
    a.d2s_input_w = l->w;
    a.n_pad = l->d2s * l->d2s * round_up(l->goc, 32);
    a.centre_flip = 0;
  }
  if (l->residual != kResNone) {
    a.residual = (const uint8_t*) (uintptr_t) (RES_BASE + (l->residual == kResMisaligned ? 1u : 0u));
    a.residual_stride = a.output_stride + (l->residual == kResOtherStride ? 16u : 0u);
    a.residual_add = &add;
    a.residual_folded = &residual_folded;
  }
  if (l->table) {
    a.table = (const uint8_t*) (uintptr_t) (TABLE_BASE + 0x800000);
    a.table_folded = &table_folded;
  }
  if (l->per_channel) a.rq_pc = (const struct qnnp_requant_pc_entry*) (uintptr_t) (TABLE_BASE + 0x900000);

  struct qnnp_hip_igemm_plan p;
  memset(&p, 0, sizeof(p));
  const char* kernel_name = NULL;
  const int rc = qnnp_hip_igemm_plan(&a, &p, &kernel_name);
  if (rc != QNNP_HIP_OK) {
    /* a refusal promises nothing about the plan */
    memset(&p, 0, sizeof(p));
    kernel_name = NULL;
  }
  /* A refusal: the status alone. A kernel without a streaming plan: the dispatcher's choice. A streaming kernel: its launch,
   * the fields that are not zero (seq / full: not -1). flags are the flavours that are on (d2s res tab pf, staged = the staged
   * 3-channel kernel, dense8 = bit 31 of log_cpr), folded what a run would report as carried by the kernel. */
  if (rc != QNNP_HIP_OK) {
    printf("%s rc=%d\n", name, rc);
    return;
  }
  printf("%s rc=%d kernel=%s image=%s option=%u vec=%u store_mode=%u", name, rc,
         p.kernel < sizeof(kKernelNames) / sizeof(kKernelNames[0]) ? kKernelNames[p.kernel] : "unknown",
         p.image < sizeof(kImageNames) / sizeof(kImageNames[0]) ? kImageNames[p.image] : "unknown", p.option, p.vec, p.store_mode);
  if (p.family != 0) {
    char flags[64];
    snprintf(flags, sizeof(flags), "%s%s%s%s%s%s", p.d2s ? "+d2s" : "", p.res ? "+res" : "", p.tab ? "+tab" : "", p.pf ? "+pf" : "",
             p.c3_staged ? "+staged" : "", (p.log_cpr >> 31) ? "+dense8" : "");
    printf(" name=%s family=%s kvec=%u grid=%ux%u", kernel_name != NULL ? kernel_name : "-",
           p.family < sizeof(kFamilyNames) / sizeof(kFamilyNames[0]) ? kFamilyNames[p.family] : "unknown", p.kvec, p.grid_x, p.grid_y);
    if (p.kb != 0) printf(" kb=%u", p.kb);
    if (p.depth != 0) printf(" depth=%u", p.depth);
    if (flags[0] != 0) printf(" flags=%s", flags + 1);
    if (p.seq >= 0) printf(" seq=%d full=%d", p.seq, p.full);
    if (p.lds_bytes != 0) printf(" lds=%u", p.lds_bytes);
    if (p.nbp != 0) printf(" nbp=%u log_cpr=%u", p.nbp, p.log_cpr & 31u);
    else if (p.log_cpr != 0) printf(" log_cpr=%u", p.log_cpr & 31u);
    if (p.per_cu != 0) printf(" per_cu=%u", p.per_cu);
    if (p.residual_folded || p.table_folded) printf(" folded=%s", p.residual_folded ? "residual" : "table");
  }
  printf("\n");
}

/* (a) the networks of tests/golden/reference_bench_shapes.json: every distinct 1x1 / fully connected layer
 * {H, W, stride, groups, group input channels, group output channels}, sorted, and every distinct 3-channel first layer
 * {H, W, window, stride, dilation, output channels}. tests/test_igemm_plan_host.py holds this list to that file. */
static const uint32_t kNetPointwise[][6] = {
  {1, 1, 1, 1, 1280, 1000}, {7, 7, 1, 1, 96, 96}, {7, 7, 1, 1, 144, 288}, {7, 7, 1, 1, 144, 576}, {7, 7, 1, 1, 160, 960},
  {7, 7, 1, 1, 192, 1024}, {7, 7, 1, 1, 232, 232}, {7, 7, 1, 1, 320, 1280}, {7, 7, 1, 1, 352, 352},
  {7, 7, 1, 1, 464, 1024}, {7, 7, 1, 1, 488, 488}, {7, 7, 1, 1, 512, 1024}, {7, 7, 1, 1, 512, 2048},
  {7, 7, 1, 1, 576, 144}, {7, 7, 1, 1, 576, 160}, {7, 7, 1, 1, 704, 1024}, {7, 7, 1, 1, 960, 160}, {7, 7, 1, 1, 960, 320},
  {7, 7, 1, 1, 976, 2048}, {7, 7, 1, 1, 1024, 1024}, {7, 7, 1, 1, 2048, 512}, {7, 7, 1, 2, 100, 200},
  {7, 7, 1, 2, 100, 400}, {7, 7, 1, 2, 400, 100}, {7, 7, 1, 3, 80, 160}, {7, 7, 1, 3, 80, 320}, {7, 7, 1, 3, 320, 80},
  {7, 7, 1, 4, 68, 136}, {7, 7, 1, 4, 68, 272}, {7, 7, 1, 4, 272, 68}, {7, 7, 1, 8, 48, 96}, {7, 7, 1, 8, 48, 192},
  {7, 7, 1, 8, 192, 48}, {13, 13, 1, 1, 48, 192}, {13, 13, 1, 1, 64, 256}, {13, 13, 1, 1, 256, 48},
  {13, 13, 1, 1, 384, 48}, {13, 13, 1, 1, 384, 64}, {13, 13, 1, 1, 512, 64}, {13, 13, 1, 1, 512, 1000},
  {14, 14, 1, 1, 48, 48}, {14, 14, 1, 1, 64, 384}, {14, 14, 1, 1, 72, 144}, {14, 14, 1, 1, 72, 288},
  {14, 14, 1, 1, 96, 96}, {14, 14, 1, 1, 96, 576}, {14, 14, 1, 1, 116, 116}, {14, 14, 1, 1, 176, 176},
  {14, 14, 1, 1, 192, 64}, {14, 14, 1, 1, 232, 232}, {14, 14, 1, 1, 244, 244}, {14, 14, 1, 1, 256, 512},
  {14, 14, 1, 1, 256, 1024}, {14, 14, 1, 1, 288, 72}, {14, 14, 1, 1, 288, 144}, {14, 14, 1, 1, 352, 352},
  {14, 14, 1, 1, 384, 64}, {14, 14, 1, 1, 384, 96}, {14, 14, 1, 1, 488, 488}, {14, 14, 1, 1, 512, 512},
  {14, 14, 1, 1, 576, 96}, {14, 14, 1, 1, 1024, 256}, {14, 14, 1, 1, 1024, 512}, {14, 14, 1, 2, 50, 100},
  {14, 14, 1, 2, 50, 200}, {14, 14, 1, 2, 200, 50}, {14, 14, 1, 2, 200, 100}, {14, 14, 1, 3, 40, 80},
  {14, 14, 1, 3, 40, 160}, {14, 14, 1, 3, 160, 40}, {14, 14, 1, 3, 160, 80}, {14, 14, 1, 4, 34, 68},
  {14, 14, 1, 4, 34, 136}, {14, 14, 1, 4, 136, 34}, {14, 14, 1, 4, 136, 68}, {14, 14, 1, 8, 24, 48},
  {14, 14, 1, 8, 24, 96}, {14, 14, 1, 8, 96, 24}, {14, 14, 1, 8, 96, 48}, {14, 14, 2, 1, 256, 512},
  {14, 14, 2, 1, 1024, 2048}, {27, 27, 1, 1, 32, 128}, {27, 27, 1, 1, 48, 192}, {27, 27, 1, 1, 64, 256},
  {27, 27, 1, 1, 128, 32}, {27, 27, 1, 1, 256, 32}, {27, 27, 1, 1, 256, 48}, {27, 27, 1, 1, 384, 48},
  {27, 27, 1, 1, 384, 64}, {28, 28, 1, 1, 24, 24}, {28, 28, 1, 1, 24, 58}, {28, 28, 1, 1, 24, 88}, {28, 28, 1, 1, 24, 122},
  {28, 28, 1, 1, 32, 192}, {28, 28, 1, 1, 36, 120}, {28, 28, 1, 1, 36, 144}, {28, 28, 1, 1, 48, 48},
  {28, 28, 1, 1, 58, 58}, {28, 28, 1, 1, 88, 88}, {28, 28, 1, 1, 116, 116}, {28, 28, 1, 1, 122, 122},
  {28, 28, 1, 1, 128, 256}, {28, 28, 1, 1, 128, 512}, {28, 28, 1, 1, 144, 32}, {28, 28, 1, 1, 144, 36},
  {28, 28, 1, 1, 144, 72}, {28, 28, 1, 1, 176, 176}, {28, 28, 1, 1, 192, 32}, {28, 28, 1, 1, 244, 244},
  {28, 28, 1, 1, 256, 256}, {28, 28, 1, 1, 512, 128}, {28, 28, 1, 1, 512, 256}, {28, 28, 1, 1, 512, 512},
  {28, 28, 1, 2, 25, 88}, {28, 28, 1, 2, 25, 100}, {28, 28, 1, 2, 100, 25}, {28, 28, 1, 2, 100, 50},
  {28, 28, 1, 3, 20, 72}, {28, 28, 1, 3, 20, 80}, {28, 28, 1, 3, 80, 20}, {28, 28, 1, 3, 80, 40}, {28, 28, 1, 4, 17, 62},
  {28, 28, 1, 4, 17, 68}, {28, 28, 1, 4, 68, 17}, {28, 28, 1, 4, 68, 34}, {28, 28, 1, 8, 12, 45}, {28, 28, 1, 8, 12, 48},
  {28, 28, 1, 8, 48, 12}, {28, 28, 1, 8, 48, 24}, {28, 28, 2, 1, 128, 256}, {28, 28, 2, 1, 512, 1024},
  {55, 55, 1, 1, 16, 64}, {55, 55, 1, 1, 32, 128}, {55, 55, 1, 1, 64, 16}, {55, 55, 1, 1, 96, 16}, {55, 55, 1, 1, 128, 16},
  {55, 55, 1, 1, 128, 32}, {56, 55, 1, 1, 128, 16}, {56, 56, 1, 1, 24, 24}, {56, 56, 1, 1, 24, 36}, {56, 56, 1, 1, 24, 50},
  {56, 56, 1, 1, 24, 58}, {56, 56, 1, 1, 24, 60}, {56, 56, 1, 1, 24, 68}, {56, 56, 1, 1, 24, 88}, {56, 56, 1, 1, 24, 96},
  {56, 56, 1, 1, 24, 122}, {56, 56, 1, 1, 24, 144}, {56, 56, 1, 1, 64, 64}, {56, 56, 1, 1, 64, 128},
  {56, 56, 1, 1, 64, 256}, {56, 56, 1, 1, 96, 24}, {56, 56, 1, 1, 128, 128}, {56, 56, 1, 1, 144, 24},
  {56, 56, 1, 1, 256, 64}, {56, 56, 1, 1, 256, 128}, {56, 56, 1, 1, 256, 256}, {56, 56, 2, 1, 64, 128},
  {56, 56, 2, 1, 256, 512}, {112, 112, 1, 1, 16, 96}, {112, 112, 1, 1, 32, 16}, {112, 112, 1, 1, 32, 64},
};
static const uint32_t kNetFirst[][6] = {
  {224, 224, 3, 1, 1, 64}, {224, 224, 3, 2, 1, 24}, {224, 224, 3, 2, 1, 32}, {224, 224, 3, 2, 1, 64},
  {224, 224, 7, 2, 1, 64}, {224, 224, 7, 2, 1, 96},
};

int main(void)
{
  char name[160];

  for (size_t i = 0; i < sizeof(kNetPointwise) / sizeof(kNetPointwise[0]); i++) {
    const uint32_t* t = kNetPointwise[i];
    for (uint32_t batch = 1; batch <= 128; batch *= 128) {
      struct layer l = pointwise(batch, t[0], t[4], t[5]);
      l.w = t[1]; l.s = t[2]; l.groups = t[3];
      snprintf(name, sizeof(name), "net_%ux%u_s%u_g%u_%uto%u_b%u", t[0], t[1], t[2], t[3], t[4], t[5], batch);
      plan_line(name, &l);
    }
  }
  for (size_t i = 0; i < sizeof(kNetFirst) / sizeof(kNetFirst[0]); i++) {
    const uint32_t* t = kNetFirst[i];
    for (uint32_t batch = 1; batch <= 128; batch *= 128) {
      struct layer l = pointwise(batch, t[0], 3, t[5]);
      l.w = t[1]; l.kh = l.kw = t[2]; l.s = t[3]; l.d = t[4];
      snprintf(name, sizeof(name), "net_first_%ux%u_k%u_s%u_d%u_3to%u_b%u", t[0], t[1], t[2], t[3], t[4], t[5], batch);
      plan_line(name, &l);
    }
  }
  /* a dilated first layer has no row-slot image: the automatic path's way to the 3-channel streaming kernel */
  {
    struct layer l = pointwise(8, 224, 3, 32);
    l.kh = l.kw = 3; l.s = 2; l.d = 2;
    plan_line("first_dilated_224x224_k3_s2_d2_3to32_b8", &l);
  }

  /* (b) the stream kernel: KB 1 to 8 with 16-byte loads, 1 / 3 / 8 with 8-byte loads (one channel block per row keeps it),
   * depth-to-space stores, and a channel count the staged plan refuses */
  for (uint32_t kb = 1; kb <= 8; kb++) {
    struct layer l = pointwise(128, 28, 32 * kb, 32);
    snprintf(name, sizeof(name), "stream_kb%u_vec16_28x28x%uto32_b128", kb, l.gic);
    plan_line(name, &l);
  }
  {
    static const uint32_t k8[3] = {24, 88, 248};
    for (int i = 0; i < 3; i++) {
      struct layer l = pointwise(128, 28, k8[i], 32);
      snprintf(name, sizeof(name), "stream_kb%u_vec8_28x28x%uto32_b128", (k8[i] + 31) / 32, k8[i]);
      plan_line(name, &l);
    }
    struct layer l = pointwise(8, 14, 64, 32);
    l.variant = 5; l.d2s = 2;
    plan_line("stream_d2s_forced5_14x14x64to32_s2_b8", &l);
    l.variant = 0;
    plan_line("stream_d2s_auto_refused", &l);
    l = pointwise(128, 56, 24, 36);
    plan_line("stream_dword_stores_56x56x24to36_b128", &l);
    l = pointwise(128, 56, 24, 36);
    l.rq = 1;
    plan_line("stream_dword_stores_56x56x24to36_b128_shift0", &l);
  }

  /* (c) the staged kernel: whole rows (dense and strided output), columns of 8 / 4 / 2 blocks, dense8, a strided 1x1
   * convolution, both load widths */
  {
    struct layer l = pointwise(128, 112, 16, 96);
    plan_line("staged_whole_dense_112x112x16to96_b128", &l);
    l.out_extra = 32;
    plan_line("staged_whole_strided_112x112x16to96_b128", &l);
    l = pointwise(128, 56, 96, 576);
    plan_line("staged_columns_56x56x96to576_b128", &l);
    l = pointwise(128, 25, 96, 576);
    plan_line("staged_columns_25x25x96to576_b128", &l);
    l = pointwise(128, 14, 96, 576);
    plan_line("staged_columns_14x14x96to576_b128", &l);
    l = pointwise(16, 14, 96, 576);
    plan_line("staged_columns_14x14x96to576_b16", &l);
    l = pointwise(128, 56, 144, 24);
    plan_line("staged_dense8_56x56x144to24_b128", &l);
    l.out_extra = 8;
    plan_line("staged_dense8_not_dense_56x56x144to24_b128", &l);
    l = pointwise(128, 56, 64, 128);
    l.s = 2;
    plan_line("staged_strided1x1_56x56_s2_64to128_b128", &l);
    l = pointwise(128, 56, 24, 144);
    plan_line("staged_vec8_56x56x24to144_b128", &l);
    l = pointwise(128, 56, 144, 48);
    l.rq = 1;
    plan_line("staged_56x56x144to48_b128_shift0", &l);
    l.rq = 2;
    plan_line("staged_56x56x144to48_b128_clamp", &l);
  }

  /* (d) the long-K kernel (forced: where a centred image exists the automatic path has a GEMM for these): KBMAX 12 / 20 /
   * 32, the two-row-set flavour taken and not, whole rows and columns */
  {
    struct layer l = pointwise(128, 14, 384, 96);
    l.variant = 9;
    plan_line("longk_kbmax12_14x14x384to96_b128", &l);
    l = pointwise(128, 14, 576, 96);
    l.variant = 9;
    plan_line("longk_kbmax20_14x14x576to96_b128", &l);
    l = pointwise(128, 28, 512, 128);
    l.variant = 9;
    plan_line("longk_kbmax20_pf_28x28x512to128_b128", &l);
    l = pointwise(128, 7, 960, 320);
    l.variant = 9;
    plan_line("longk_kbmax32_columns_7x7x960to320_b128", &l);
    l = pointwise(128, 7, 320, 1280);
    l.variant = 9;
    plan_line("longk_kbmax12_columns_7x7x320to1280_b128", &l);
    l = pointwise(128, 14, 384, 96);
    l.kzp = 120;
    plan_line("longk_auto_14x14x384to96_b128_kzp120", &l);
  }

  /* (e) the global-weights kernels: one wave per block, and the split reduction at depth 4 and 8 */
  {
    struct layer l = pointwise(128, 7, 960, 160);
    plan_line("gw_auto_7x7x960to160_b128", &l);
    l = pointwise(32, 1, 512, 1000);
    l.variant = 6;
    plan_line("gwk_depth4_fc_512to1000_b32", &l);
    l = pointwise(32, 1, 1024, 1000);
    l.variant = 6;
    plan_line("gwk_depth8_fc_1024to1000_b32", &l);
    l = pointwise(32, 1, 1024, 100);
    plan_line("gwk_auto_fc_1024to100_b32", &l);
  }

  /* (f) the 3-channel streaming kernel, forced: staged (16-byte output rows) and not */
  {
    struct layer l = pointwise(8, 224, 3, 32);
    l.kh = l.kw = 3; l.s = 2; l.variant = 7;
    plan_line("c3_staged_forced7_224x224_k3_s2_3to32_b8", &l);
    l.out_extra = 16;
    plan_line("c3_staged_strided_forced7_224x224_k3_s2_3to32_b8", &l);
    l.out_extra = 0; l.goc = 24;
    plan_line("c3_unstaged_forced7_224x224_k3_s2_3to24_b8", &l);
    l.goc = 32; l.rq = 1;
    plan_line("c3_staged_forced7_shift0", &l);
  }

  /* (g) flavours. Per table-carrying family: a residual, a table that folds. Stream, staged and long-K: a table that does
   * not fold because one resident workgroup would be lost (LDS at exactly 160 KiB / k), and one that does not because the
   * kernel's LDS budget is full. */
  {
    struct layer l = pointwise(128, 28, 192, 32);
    l.residual = kResMatching;
    plan_line("flavour_stream_residual_28x28x192to32_b128", &l);
    l.residual = kResNone; l.table = 1;
    plan_line("flavour_stream_table_28x28x192to32_b128", &l);
    l = pointwise(128, 28, 32, 1100);                     /* 35 blocks: 40 KiB, residency 4; 256 bytes more make it 3 */
    l.variant = 5; l.table = 1;
    plan_line("flavour_stream_table_residency_28x28x32to1100_b128", &l);
    l = pointwise(128, 28, 64, 956);                      /* 30 blocks x 2 + 4 KiB of bias: 64 KiB */
    l.variant = 5; l.table = 1;
    plan_line("flavour_stream_table_budget_28x28x64to956_b128", &l);

    l = pointwise(128, 56, 144, 48);
    l.residual = kResMatching;
    plan_line("flavour_staged_residual_56x56x144to48_b128", &l);
    l.residual = kResNone; l.table = 1;
    plan_line("flavour_staged_table_56x56x144to48_b128", &l);
    l = pointwise(128, 56, 24, 144);
    l.table = 1;
    plan_line("flavour_staged_vec8_table_56x56x24to144_b128", &l);
    l.table = 0; l.residual = kResMatching;
    plan_line("flavour_staged_vec8_residual_56x56x24to144_b128", &l);
    l = pointwise(128, 56, 144, 24);
    l.residual = kResMatching;
    plan_line("flavour_staged_dense8_residual_56x56x144to24_b128", &l);
    l.residual = kResNone; l.table = 1;
    plan_line("flavour_staged_dense8_table_56x56x144to24_b128", &l);
    l = pointwise(128, 56, 32, 224);                      /* 7 + 1 + 32 KiB: residency 4 of 7; 256 bytes more make it 3 */
    l.out_extra = 32; l.table = 1;
    plan_line("flavour_staged_table_residency_56x56x32to224_b128", &l);
    l = pointwise(128, 56, 160, 224);                     /* 35 + 1 + 28 KiB: 64 KiB */
    l.table = 1;
    plan_line("flavour_staged_table_budget_56x56x160to224_b128", &l);

    l = pointwise(128, 14, 384, 96);
    l.variant = 9; l.residual = kResMatching;
    plan_line("flavour_longk_residual_14x14x384to96_b128", &l);
    l.residual = kResNone; l.table = 1;
    plan_line("flavour_longk_table_14x14x384to96_b128", &l);
    l = pointwise(128, 28, 512, 128);
    l.variant = 9; l.table = 1;
    plan_line("flavour_longk_pf_table_28x28x512to128_b128", &l);
    l.table = 0; l.residual = kResMatching;
    plan_line("flavour_longk_pf_residual_28x28x512to128_b128", &l);
    l = pointwise(128, 14, 736, 80);                      /* 69 + 1 + 10 KiB: residency 2; 256 bytes more make it 1 */
    l.variant = 9; l.table = 1;
    plan_line("flavour_longk_table_residency_14x14x736to80_b128", &l);
    l = pointwise(128, 28, 480, 160);                     /* 75 + 1 + 20 KiB: 96 KiB */
    l.variant = 9; l.table = 1;
    plan_line("flavour_longk_table_budget_28x28x480to160_b128", &l);

    l = pointwise(128, 7, 960, 160);
    l.residual = kResMatching;
    plan_line("flavour_gw_residual_7x7x960to160_b128", &l);
    l.residual = kResNone; l.table = 1;
    plan_line("flavour_gw_table_7x7x960to160_b128", &l);
    l = pointwise(32, 1, 1024, 100);
    l.residual = kResMatching;
    plan_line("flavour_gwk_residual_fc_1024to100_b32", &l);
    l.residual = kResNone; l.table = 1;
    plan_line("flavour_gwk_table_fc_1024to100_b32", &l);
    l = pointwise(32, 1, 512, 1000);
    l.variant = 6; l.table = 1;
    plan_line("flavour_gwk_depth4_table_fc_512to1000_b32", &l);

    /* a residual the kernels do not carry (another stride, an odd address), and a table beside a residual */
    l = pointwise(128, 56, 144, 48);
    l.residual = kResOtherStride;
    plan_line("flavour_residual_other_stride_56x56x144to48_b128", &l);
    l.residual = kResMisaligned;
    plan_line("flavour_residual_misaligned_56x56x144to48_b128", &l);
    l.residual = kResMatching; l.table = 1;
    plan_line("flavour_table_with_residual_refused", &l);
    /* a table on a kernel that carries none */
    l = pointwise(128, 14, 1024, 256);
    l.table = 1;
    plan_line("flavour_table_not_carried_14x14x1024to256_b128", &l);
  }

  /* (h) alignments: the output side for store_mode 2 / 1 / 0, the input side for 16 / 8 / 4-byte loads (and single bytes) */
  {
    static const uint32_t offs[4] = {0, 8, 4, 1};
    for (int o = 0; o < 4; o++) {
      struct layer l = pointwise(128, 28, 192, 64);
      l.out_off = offs[o];
      snprintf(name, sizeof(name), "align_out%u_28x28x192to64_b128", offs[o]);
      plan_line(name, &l);
    }
    for (int i = 1; i < 4; i++) {
      struct layer l = pointwise(128, 28, 192, 64);
      l.in_off = offs[i];
      snprintf(name, sizeof(name), "align_in%u_28x28x192to64_b128", offs[i]);
      plan_line(name, &l);
    }
    struct layer l = pointwise(128, 28, 192, 64);
    l.in_extra = 8; l.out_extra = 4;
    plan_line("align_strides_in+8_out+4_28x28x192to64_b128", &l);
  }

  /* (i) the forced streaming codes on shapes they refuse, and per-channel requantization under one of them */
  {
    struct layer l = pointwise(128, 14, 512, 128);
    l.variant = 5;
    plan_line("forced5_k512_refused", &l);
    l = pointwise(128, 28, 192, 64);
    l.variant = 6; l.in_off = 8;
    plan_line("forced6_in8_refused", &l);
    l = pointwise(128, 28, 192, 64);
    l.variant = 7;
    plan_line("forced7_pointwise_refused", &l);
    l = pointwise(128, 28, 128, 64);
    l.variant = 9;
    plan_line("forced9_k128_refused", &l);
    l = pointwise(128, 28, 192, 64);
    l.variant = 5; l.per_channel = 1;
    plan_line("forced5_per_channel_refused", &l);
    l.variant = 0;
    plan_line("per_channel_auto_28x28x192to64_b128", &l);
    l = pointwise(128, 28, 192, 64);
    l.variant = 5;
    plan_line("forced5_28x28x192to64_b128", &l);
    l.variant = 6;
    plan_line("forced6_28x28x192to64_b128", &l);
    l = pointwise(0, 28, 192, 64);
    plan_line("empty_batch_refused", &l);
  }
  return 0;
}
