/*
 * host_dwconv_plan_test.c -- TEST INFRASTRUCTURE: the launch plan of the depthwise kernels, as text.
 *
 * A stand-alone program (Makefile target dwconv-plan) linked against libqnnpack_gfx950.so itself: no sanitizer, no stub.
 * It calls qnnp_hip_dwconv_plan (hip/qnnp_hip.h) on a fixed list of argument blocks and prints one line per case: the
 * case, the status, the kernel a run would report and every field of the plan. tests/test_dwconv_plan_host.py compares
 * the output with tests/golden/dwconv_plans.txt line for line. The plan decides speed, not bytes -- rows per segment,
 * bands, slabs -- so no parity test sees it change; this file does.
 *
 * The library is never initialised: qnnp::active_cu_count() answers its no-device value of 256 on every machine (the
 * MI355X's own count), and nothing touches a device. The pointers are made-up addresses, chosen for their low bits
 * and never dereferenced.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hip/qnnp_hip.h"

/* the enumerators of q8dwconv.hip (kPlanDirect = 1, ...) BY VALUE: this order is that enum's order, and a new or moved
 * enumerator there needs the same edit here (the golden then differs in the `kernel` column of every line it touches) */
static const char* const kPlanNames[] = {"none", "kPlanDirect", "kPlanLds33", "kPlanLds55", "kPlanRow", "kPlanMfma", "kPlanMfmaLds",
                                         "kPlanCol", "kPlanCol5", "kPlanM16", "kPlanDirect4", "kPlanRowAny"};

#define IN_BASE UINT64_C(0x7f1000000000)
#define OUT_BASE UINT64_C(0x7f5000000000)
#define TABLE_BASE UINT64_C(0x7f9000000000)

struct shape {
  uint32_t batch, h, w, c;
  uint32_t kh, kw, sh, sw, dh, dw;
  uint32_t pad_top, pad_left;
  uint32_t w_range;
  int variant;
  uint32_t in_off, out_off;        /* added to the base addresses */
  uint32_t stride_extra;           /* pixel strides = c + stride_extra */
};

/* square window, one stride and dilation, padding as bench.py's conv_geometry (half the window's extent) */
static struct shape conv(uint32_t batch, uint32_t hw, uint32_t c, uint32_t k, uint32_t s, uint32_t d, uint32_t w_range)
{
  struct shape sh = {batch, hw, hw, c, k, k, s, s, d, d, ((k - 1) * d + 1) / 2, ((k - 1) * d + 1) / 2, w_range, 0, 0, 0, 0};
  return sh;
}

static void plan_line(const char* name, const struct shape* s)
{
  const uint32_t eh = (s->kh - 1) * s->dh + 1, ew = (s->kw - 1) * s->dw + 1;
  const uint32_t c_pad = (s->c + 15u) / 16u * 16u;
  struct qnnp_hip_dwconv_args a;
  memset(&a, 0, sizeof(a));
  a.input = (const uint8_t*) (uintptr_t) (IN_BASE + s->in_off);
  a.output = (uint8_t*) (uintptr_t) (OUT_BASE + s->out_off);
  a.wadj = (const int16_t*) (uintptr_t) TABLE_BASE;
  a.bias1 = (const int32_t*) (uintptr_t) (TABLE_BASE + 0x100000);
  a.dwm_x = (const int8_t*) (uintptr_t) (TABLE_BASE + 0x200000);
  a.dwm_bias = (const int32_t*) (uintptr_t) (TABLE_BASE + 0x300000);
  a.dwm_parts = 2;
  a.w_range = s->w_range;
  /* convolution.c: the dot-product image exists for 3x3 and 5x5 windows with weights in one of the int8 ranges */
  a.dot4 = (s->w_range != 0 && s->kh == s->kw && (s->kh == 3 || s->kh == 5)) ? (const uint32_t*) (uintptr_t) (TABLE_BASE + 0x400000) : NULL;
  a.c_pad32 = (s->c + 31u) / 32u * 32u;
  a.batch = s->batch;
  a.input_height = s->h;
  a.input_width = s->w;
  /* padding below / right as bench.py's conv_geometry: what half the window's extent leaves */
  const uint32_t pad_bottom = eh - 1 - eh / 2, pad_right = ew - 1 - ew / 2;
  a.output_height = (s->pad_top + s->h + pad_bottom - eh) / s->sh + 1;
  a.output_width = (s->pad_left + s->w + pad_right - ew) / s->sw + 1;
  a.channels = s->c;
  a.c_pad = c_pad;
  a.kernel_height = s->kh;
  a.kernel_width = s->kw;
  a.stride_height = s->sh;
  a.stride_width = s->sw;
  a.dilation_height = s->dh;
  a.dilation_width = s->dw;
  a.pad_top = s->pad_top;
  a.pad_left = s->pad_left;
  a.input_stride = s->c + s->stride_extra;
  a.output_stride = s->c + s->stride_extra;
  a.input_zero_point = 127;
  /* any valid requantization: it never enters the plan */
  a.rq.multiplier = 0x40000000;
  a.rq.shift = 1;
  a.rq.remainder_mask = 1;
  a.rq.remainder_threshold = 0;
  a.rq.output_min_less_zero_point = -127;
  a.rq.output_max_less_zero_point = 128;
  a.rq.output_zero_point = 127;
  a.variant = s->variant;
  a.streaming_mode = 1;

  struct qnnp_hip_dwconv_plan plan;
  memset(&plan, 0, sizeof(plan));
  const char* kernel_name = "-";
  const int rc = qnnp_hip_dwconv_plan(&a, &plan, &kernel_name);
  if (rc != QNNP_HIP_OK) {
    /* a refusal promises nothing about the plan */
    memset(&plan, 0, sizeof(plan));
    kernel_name = "-";
  }
  const char* plan_name = plan.kernel < sizeof(kPlanNames) / sizeof(kPlanNames[0]) ? kPlanNames[plan.kernel] : "unknown";
  printf("%s rc=%d name=%s kernel=%s vec16=%u CS=%u TOH=%u IR=%u IC=%u PP=%u bands=%u slabs=%u store_mode=%u\n", name, rc,
         kernel_name, plan_name, plan.vec16, plan.CS, plan.TOH, plan.IR, plan.IC, plan.PP, plan.bands, plan.slabs, plan.store_mode);
}

int main(void)
{
  char name[160];

  /* (a) the ten depthwise layers of MobileNetV2 (bench.py MOBILENETV2): input side, channels, stride */
  static const uint32_t mnv2[10][3] = {{112, 32, 1}, {112, 96, 2}, {56, 144, 1}, {56, 144, 2}, {28, 192, 1},
                                       {28, 192, 2}, {14, 384, 1}, {14, 576, 1}, {14, 576, 2}, {7, 960, 1}};
  static const uint32_t batches[3] = {1, 8, 128};
  for (int l = 0; l < 10; l++) {
    for (int b = 0; b < 3; b++) {
      for (uint32_t wr = 0; wr < 3; wr++) {
        const struct shape s = conv(batches[b], mnv2[l][0], mnv2[l][1], 3, mnv2[l][2], 1, wr);
        snprintf(name, sizeof(name), "mnv2_%ux%ux%u_s%u_b%u_wr%u", s.h, s.w, s.c, s.sh, s.batch, wr);
        plan_line(name, &s);
      }
    }
  }

  /* (b) 5x5: input side, channels, stride (bench.py's MobileNetV3 rows and the first MobileNetV2 shape) */
  static const uint32_t k5[4][3] = {{56, 72, 2}, {28, 240, 1}, {14, 672, 1}, {112, 32, 1}};
  for (int l = 0; l < 4; l++) {
    for (uint32_t wr = 0; wr < 2; wr++) {
      const struct shape s = conv(128, k5[l][0], k5[l][1], 5, k5[l][2], 1, wr);
      snprintf(name, sizeof(name), "dw5x5_%ux%ux%u_s%u_b128_wr%u", s.h, s.w, s.c, s.sh, wr);
      plan_line(name, &s);
    }
  }

  /* (c) dilated 3x3: dilation 2 with and without the int8 image, dilation 65 (beyond the column walk's 64) */
  {
    struct shape s = conv(128, 28, 192, 3, 1, 2, 1);
    plan_line("dil2_28x28x192_b128_wr1", &s);
    s.w_range = 0;
    plan_line("dil2_28x28x192_b128_wr0", &s);
    s = conv(8, 160, 32, 3, 1, 65, 1);
    plan_line("dil65_160x160x32_b8_wr1", &s);
  }

  /* (d) channel counts that are no multiple of four (c_pad 16, 16, 64, 128) */
  static const uint32_t odd_c[4] = {3, 6, 58, 122};
  for (int i = 0; i < 4; i++) {
    const struct shape s = conv(8, 28, odd_c[i], 3, 1, 1, 1);
    snprintf(name, sizeof(name), "channels_28x28x%u_b8", s.c);
    plan_line(name, &s);
  }

  /* (e) base addresses off the 16-byte grid, (f) pixel strides beyond the channel count */
  static const uint32_t offs[4] = {0, 1, 4, 8};
  for (int i = 0; i < 4; i++) {
    for (int o = 0; o < 4; o++) {
      struct shape s = conv(8, 28, 64, 3, 1, 1, 1);
      s.in_off = offs[i];
      s.out_off = offs[o];
      snprintf(name, sizeof(name), "offset_28x28x64_b8_in%u_out%u", s.in_off, s.out_off);
      plan_line(name, &s);
    }
  }
  static const uint32_t extra[4] = {0, 1, 4, 16};
  for (int i = 0; i < 4; i++) {
    struct shape s = conv(8, 28, 64, 3, 1, 1, 1);
    s.stride_extra = extra[i];
    snprintf(name, sizeof(name), "stride_28x28x64_b8_c+%u", extra[i]);
    plan_line(name, &s);
  }

  /* (g) padding beyond the window's reach, other windows, other strides */
  {
    struct shape s = conv(8, 28, 64, 3, 1, 1, 1);
    s.pad_top = 3;
    plan_line("pad_top3_28x28x64_b8", &s);
    s = conv(8, 28, 64, 3, 1, 1, 1);
    s.pad_left = 3;
    plan_line("pad_left3_28x28x64_b8", &s);
    s = conv(8, 28, 64, 7, 1, 1, 0);
    plan_line("window_7x7_28x28x64_b8", &s);
    s = conv(8, 28, 64, 3, 1, 1, 0);
    s.kw = 5; s.pad_left = 2;
    plan_line("window_3x5_28x28x64_b8", &s);
    s = conv(8, 28, 64, 3, 1, 1, 0);
    s.kh = 1; s.pad_top = 0;
    plan_line("window_1x3_28x28x64_b8", &s);
    s = conv(8, 28, 64, 3, 3, 1, 1);
    plan_line("stride3_28x28x64_b8", &s);
    s = conv(8, 28, 64, 3, 1, 1, 1);
    s.sw = 2;
    plan_line("stride1x2_28x28x64_b8", &s);
  }

  /* (h) tensors of at least 2^31 and 2^32 bytes: wide with few channels (OW >= 56, C <= 96), many channels, and images
   * too wide for a band in LDS */
  {
    struct shape s = conv(2048, 112, 96, 3, 1, 1, 1);     /* 2.3 GiB */
    plan_line("huge_2g_112x112x96_b2048", &s);
    s = conv(4096, 112, 96, 3, 1, 1, 1);                  /* 4.6 GiB */
    plan_line("huge_4g_112x112x96_b4096", &s);
    s = conv(8192, 56, 144, 3, 1, 1, 1);                  /* 3.4 GiB */
    plan_line("huge_2g_56x56x144_b8192", &s);
    s = conv(16384, 56, 144, 3, 1, 1, 1);                 /* 6.9 GiB */
    plan_line("huge_4g_56x56x144_b16384", &s);
    s = conv(4, 2048, 128, 3, 1, 1, 1);                   /* 2 GiB, rows of 2048 pixels */
    plan_line("huge_2g_2048x2048x128_b4", &s);
    s = conv(8, 2048, 128, 3, 1, 1, 1);                   /* 4 GiB */
    plan_line("huge_4g_2048x2048x128_b8", &s);
    s = conv(2048, 56, 240, 5, 1, 1, 1);                  /* 5x5, 2.8 GiB */
    plan_line("huge_2g_dw5x5_56x56x240_b2048", &s);
  }

  /* (i) small outputs: 1x1, 7x7 (in (a) too), fewer than eight columns */
  {
    struct shape s = conv(8, 1, 64, 3, 1, 1, 1);
    plan_line("out_1x1_c64_b8", &s);
    s = conv(1, 1, 1280, 3, 1, 1, 0);
    plan_line("out_1x1_c1280_b1", &s);
    s = conv(8, 7, 64, 3, 1, 1, 1);
    plan_line("out_7x7_c64_b8", &s);
    s = conv(8, 14, 64, 3, 2, 1, 0);
    plan_line("out_7x7_s2_c64_b8", &s);
    s = conv(8, 5, 64, 3, 1, 1, 1);
    plan_line("out_5x5_c64_b8", &s);
    s = conv(8, 14, 64, 3, 1, 1, 1);
    s.w = 6;
    plan_line("out_14x6_c64_b8", &s);
    s = conv(8, 5, 64, 5, 1, 1, 1);
    plan_line("out_5x5_dw5x5_c64_b8", &s);
  }

  /* (j) every forced code on a shape it takes and on one it refuses. Code 1 (the byte-per-thread kernel) takes every
   * shape: what it refuses is what every code refuses, an empty batch. */
  {
    struct shape s = conv(8, 56, 144, 3, 1, 1, 1);
    s.variant = 1;
    plan_line("forced1_56x56x144_b8", &s);
    s.batch = 0;
    plan_line("forced1_empty_batch", &s);

    s = conv(8, 14, 576, 3, 1, 1, 1);
    s.variant = 2;
    plan_line("forced2_14x14x576_b8", &s);
    s = conv(8, 28, 240, 5, 1, 1, 1);
    s.variant = 2;
    plan_line("forced2_dw5x5_28x28x240_b8", &s);
    s = conv(8, 28, 60, 3, 1, 1, 1);
    s.variant = 2;
    plan_line("forced2_28x28x60_b8", &s);
    s = conv(8, 28, 64, 7, 1, 1, 0);
    s.variant = 2;
    plan_line("forced2_window_7x7_refused", &s);

    s = conv(8, 56, 144, 3, 1, 1, 1);
    s.variant = 3;
    plan_line("forced3_56x56x144_b8", &s);
    s = conv(128, 56, 144, 3, 2, 1, 0);
    s.variant = 3;
    plan_line("forced3_56x56x144_s2_b128", &s);
    s = conv(8, 28, 240, 5, 1, 1, 1);
    s.variant = 3;
    plan_line("forced3_dw5x5_refused", &s);

    s = conv(8, 56, 144, 3, 1, 1, 1);
    s.variant = 4;
    plan_line("forced4_56x56x144_b8", &s);
    s = conv(8, 28, 58, 3, 1, 1, 1);
    s.variant = 4;
    plan_line("forced4_58_channels_refused", &s);

    s = conv(128, 112, 32, 3, 1, 1, 1);
    s.variant = 5;
    plan_line("forced5_112x112x32_b128", &s);
    s = conv(1, 14, 576, 3, 2, 1, 0);
    s.variant = 5;
    plan_line("forced5_14x14x576_s2_b1", &s);
    s = conv(8, 28, 240, 5, 1, 1, 1);
    s.variant = 5;
    plan_line("forced5_dw5x5_refused", &s);

    s = conv(128, 28, 192, 3, 1, 1, 0);
    s.variant = 6;
    plan_line("forced6_28x28x192_b128_wr0", &s);
    s = conv(128, 28, 240, 5, 1, 1, 2);
    s.variant = 6;
    plan_line("forced6_dw5x5_28x28x240_b128_wr2", &s);
    s = conv(8, 28, 64, 3, 1, 1, 1);
    s.variant = 6;
    s.pad_top = 3;
    plan_line("forced6_pad_top3_refused", &s);
    s = conv(8, 28, 240, 5, 1, 1, 0);
    s.variant = 6;
    plan_line("forced6_dw5x5_wr0_refused", &s);
    s = conv(8, 28, 64, 3, 1, 1, 1);
    s.variant = 6;
    s.out_off = 1;
    plan_line("forced6_out_offset1_refused", &s);

    s = conv(128, 28, 192, 3, 1, 1, 1);
    s.variant = 7;
    plan_line("forced7_28x28x192_b128_wr1", &s);
    s = conv(128, 56, 144, 3, 1, 1, 2);
    s.variant = 7;
    plan_line("forced7_56x56x144_b128_wr2", &s);
    s = conv(8, 112, 32, 3, 1, 1, 1);
    s.variant = 7;
    plan_line("forced7_112x112x32_b8_wr1", &s);
    s = conv(128, 28, 192, 3, 1, 1, 0);
    s.variant = 7;
    plan_line("forced7_wr0_refused", &s);

    s = conv(8, 28, 58, 3, 1, 1, 1);
    s.variant = 8;
    plan_line("forced8_28x28x58_b8", &s);
    s = conv(128, 28, 192, 3, 2, 1, 1);
    s.variant = 8;
    plan_line("forced8_28x28x192_s2_b128", &s);
    s = conv(8, 28, 240, 5, 1, 1, 1);
    s.variant = 8;
    plan_line("forced8_dw5x5_refused", &s);

    s = conv(8, 28, 58, 7, 1, 1, 0);
    s.variant = 9;
    plan_line("forced9_window_7x7_28x28x58_b8", &s);
    s = conv(8, 28, 3, 3, 1, 1, 0);
    s.variant = 9;
    plan_line("forced9_3_channels_refused", &s);
  }
  return 0;
}
