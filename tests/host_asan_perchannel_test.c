/*
 * host_asan_perchannel_test.c -- TEST INFRASTRUCTURE: the host code of the per-channel creates
 * (include/qnnpack_gfx950_perchannel.h; convolution.c, fully-connected.c, per-channel.h) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, against tests/hip_stub.c (Makefile target asan-perchannel; run by
 * tests/test_perchannel_host.py). Walks create / setup / run / delete of both operators at 1, 3 and 33 output channels
 * (dense, grouped, depthwise, 3-channel inputs), the table each create uploads -- entry by entry against
 * qnnp_compute_requant, the pad entries included --, every refused create in the documented order, a create whose n-th
 * allocation or upload fails (nothing stays allocated), and the refusals of the fused block and the residual attach.
 * Prints "host-sanitizers-perchannel-ok" on success.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>
#include <qnnpack_gfx950_perchannel.h>

#include "hip/qnnp_hip.h"
#include "hip/requant_pc.h"
#include "operator.h"
#include "requantization.h"

/* tests/hip_stub.c test controls */
void qnnp_stub_fail_nth(long n);
int qnnp_stub_fail_pending(void);
size_t qnnp_stub_live_allocs(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static const float IS = 0.75f, OS = 1.5f;

/* exactly `n` floats (ASan sees a read past them): ks[c] = 2^-(6 + c % 9) * (1 + ((37 c) % 64) / 64) */
static float* scales(size_t n)
{
  float* ks = (float*) malloc(n * sizeof(float));
  CHECK(ks != NULL);
  for (size_t c = 0; c < n; c++) ks[c] = ldexpf(1.0f + (float) ((37 * c) % 64) / 64.0f, -(int) (6 + c % 9));
  return ks;
}

static uint8_t* bytes(size_t n, unsigned salt)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t) (i * 37u + salt);
  return p;
}

static int32_t* biases(size_t n)
{
  int32_t* b = (int32_t*) malloc(n * sizeof(int32_t));
  CHECK(b != NULL);
  for (size_t i = 0; i < n; i++) b[i] = (int32_t) (i * 1001u) - 5000;
  return b;
}

/* the table of `op` against qnnp_compute_requant, channel by channel, and its pad entries */
static void check_table(qnnp_operator_t op, uint32_t runs, size_t run_channels, uint32_t pad, const float* ks)
{
  CHECK(op->per_channel == 1 && op->d_requant_pc != NULL);
  CHECK(pad >= run_channels);
  const struct qnnp_requant_pc_entry* t = (const struct qnnp_requant_pc_entry*) op->d_requant_pc;
  for (uint32_t g = 0; g < runs; g++) {
    for (uint32_t c = 0; c < pad; c++) {
      const struct qnnp_requant_pc_entry e = t[(size_t) g * pad + c];
      if (c < run_channels) {
        const float scale = IS * ks[g * run_channels + c] / OS;
        const struct qnnp_hip_requant rq = qnnp_compute_requant(scale, 0, 0, 255);
        CHECK(e.multiplier == rq.multiplier && e.shift == rq.shift);
        CHECK(e.multiplier >= 0x40000000 && e.shift <= 31);
      } else {
        CHECK(e.multiplier == 0x40000000 && e.shift == 0);
      }
    }
  }
  CHECK(op->requant.output_zero_point == 9 && op->requant.output_min_less_zero_point == 1 - 9 &&
        op->requant.output_max_less_zero_point == 250 - 9);
}

static void convolution_walk(uint32_t groups, size_t gic, size_t goc, uint32_t kh, uint32_t kw, uint32_t pad_hw, uint32_t stride)
{
  const size_t cin = groups * gic, cout = groups * goc;
  float* ks = scales(cout);
  uint8_t* kernel = bytes(cout * kh * kw * gic, 3);
  int32_t* bias = biases(cout);
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(pad_hw, pad_hw, pad_hw, pad_hw, kh, kw, stride, stride, 1, 1,
      groups, gic, goc, 127, IS, 128, ks, kernel, bias, 9, OS, 1, 250, 0, &op) == qnnp_status_success);
  CHECK(op != NULL);
  const int depthwise = groups > 1 && gic == 1 && goc == 1;
  CHECK((op->ukernel_type == qnnp_ukernel_type_dwconv) == depthwise);
  if (depthwise) {
    CHECK(op->c_pad % 16 == 0);
    check_table(op, 1, cout, op->c_pad, ks);
    CHECK(op->d_dw_dot4 == NULL && op->d_dwm_x == NULL);
  } else {
    CHECK(op->n_pad % 32 == 0);
    check_table(op, groups, goc, op->n_pad, ks);
    CHECK(op->d_weights_dense == NULL && op->d_weights_centred == NULL && op->d_weights_rows16 == NULL);   /* never those images */
  }
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  const size_t batch = 2, h = 7, w = 6, si = cin + 3, so = cout + 5;
  const size_t oh = (h + 2 * pad_hw - kh) / stride + 1, ow = (w + 2 * pad_hw - kw) / stride + 1;
  uint8_t* x = bytes((batch * h * w - 1) * si + cin, 11);
  uint8_t* y = bytes((batch * oh * ow - 1) * so + cout, 0);
  CHECK(qnnp_setup_convolution2d_nhwc_q8(op, batch, h, w, x, si, y, so, NULL) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), depthwise ? "stub_dwconv" : "stub_igemm") == 0);
  /* a second setup at another shape, and an empty batch */
  CHECK(qnnp_setup_convolution2d_nhwc_q8(op, 1, h, w, x, si, y, so, NULL) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(qnnp_setup_convolution2d_nhwc_q8(op, 0, h, w, x, si, y, so, NULL) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  /* the fully connected setup takes no convolution with a window, per-channel or not */
  if (kh * kw > 1 || depthwise) {
    CHECK(qnnp_setup_fully_connected_nc_q8(op, 1, x, cin, y, cout) != qnnp_status_success || op->ukernel_type == qnnp_ukernel_type_gemm);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);

  /* every allocation and upload of the create failing in turn: out_of_memory (or a warning-only optional image),
   * no handle, nothing left allocated */
  for (long nth = 0; nth < 64; nth++) {
    const size_t live = qnnp_stub_live_allocs();
    qnnp_operator_t none = NULL;
    qnnp_stub_fail_nth(nth);
    const enum qnnp_status st = qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(pad_hw, pad_hw, pad_hw, pad_hw, kh, kw,
        stride, stride, 1, 1, groups, gic, goc, 127, IS, 128, ks, kernel, bias, 9, OS, 1, 250, 0, &none);
    const int fired = !qnnp_stub_fail_pending();
    qnnp_stub_fail_nth(-1);
    if (!fired) {
      CHECK(st == qnnp_status_success);
      CHECK(qnnp_delete_operator(none) == qnnp_status_success);
      CHECK(nth >= 6);                       /* weights, bias pair and table: two calls each */
      break;
    }
    CHECK(st == qnnp_status_out_of_memory && none == NULL);
    CHECK(qnnp_stub_live_allocs() == live);
  }
  free(x);
  free(y);
  free(ks);
  free(kernel);
  free(bias);
}

static void fully_connected_walk(size_t k, size_t n)
{
  float* ks = scales(n);
  uint8_t* kernel = bytes(n * k, 5);
  int32_t* bias = biases(n);
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_fully_connected_nc_q8_per_channel(k, n, 127, IS, 128, ks, kernel, bias, 9, OS, 1, 250, 0, &op) ==
        qnnp_status_success);
  CHECK(op != NULL && op->ukernel_type == qnnp_ukernel_type_gemm);
  check_table(op, 1, n, op->n_pad, ks);
  CHECK(op->d_weights_centred == NULL && op->centre_flip == 0);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
  const size_t batch = 5, si = k + 2, so = n + 7;
  uint8_t* x = bytes((batch - 1) * si + k, 1);
  uint8_t* y = bytes((batch - 1) * so + n, 2);
  CHECK(qnnp_setup_fully_connected_nc_q8(op, batch, x, si, y, so) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_igemm") == 0);
  CHECK(qnnp_setup_fully_connected_nc_q8(op, 1, x, si, y, so) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(qnnp_setup_fully_connected_nc_q8(op, batch, x, k - 1, y, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);   /* a refused setup leaves the last one runnable */
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  for (long nth = 0; nth < 64; nth++) {
    const size_t live = qnnp_stub_live_allocs();
    qnnp_operator_t none = NULL;
    qnnp_stub_fail_nth(nth);
    const enum qnnp_status st = qnnp_gfx950_create_fully_connected_nc_q8_per_channel(k, n, 127, IS, 128, ks, kernel, bias, 9, OS,
        1, 250, 0, &none);
    const int fired = !qnnp_stub_fail_pending();
    qnnp_stub_fail_nth(-1);
    if (!fired) {
      CHECK(st == qnnp_status_success && nth == 6);
      CHECK(qnnp_delete_operator(none) == qnnp_status_success);
      break;
    }
    CHECK(st == qnnp_status_out_of_memory && none == NULL);
    CHECK(qnnp_stub_live_allocs() == live);
  }
  free(x);
  free(y);
  free(ks);
  free(kernel);
  free(bias);
}

#define CONV(groups, gic, goc, is, ks_, kernel_, bias_, os, out) \
  qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, groups, gic, goc, 127, is, 128, ks_, kernel_, \
      bias_, 9, os, 0, 255, 0, out)
#define FC(k, n, is, ks_, kernel_, bias_, os, out) \
  qnnp_gfx950_create_fully_connected_nc_q8_per_channel(k, n, 127, is, 128, ks_, kernel_, bias_, 9, os, 0, 255, 0, out)

static void statuses(void)
{
  const size_t n = 33;
  float* ks = scales(n);
  uint8_t* kernel = bytes(n * 9 * 8, 3);
  int32_t* bias = biases(n);
  qnnp_operator_t op = NULL;
  const size_t live = qnnp_stub_live_allocs();
  /* invalid_parameter, in the order of the per-tensor create: window, subsampling, dilation, input scale, kernel
   * scales (NULL), output scale, counts / kernel / bias, then the scales themselves */
  CHECK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(0, 0, 0, 0, 0, 3, 1, 1, 1, 1, 1, 8, n, 0, 0.0f, 0, NULL, NULL, NULL, 0,
      0.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(0, 0, 0, 0, 3, 3, 0, 1, 1, 1, 1, 8, n, 0, IS, 0, ks, kernel, bias, 0,
      OS, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(0, 0, 0, 0, 3, 3, 1, 1, 1, 0, 1, 8, n, 0, IS, 0, ks, kernel, bias, 0,
      OS, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, n, 0.0f, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, n, INFINITY, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, n, IS, NULL, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, n, IS, ks, kernel, bias, -1.0f, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, n, IS, ks, kernel, bias, NAN, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(0, 8, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 0, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, 0, IS, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, n, IS, ks, NULL, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(CONV(1, 8, n, IS, ks, kernel, NULL, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(FC(0, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(FC(8, 0, IS, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(FC(8, n, IS, NULL, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(FC(8, n, 1.0e-40f, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
  CHECK(FC(8, n, IS, ks, NULL, bias, OS, &op) == qnnp_status_invalid_parameter);
  const float bad[6] = {0.0f, -0.5f, NAN, INFINITY, 1.0e-40f, -0.0f};
  for (int b = 0; b < 6; b++) {
    for (size_t at = 0; at < n; at += 16) {          /* first, middle and last channel */
      const float keep = ks[at];
      ks[at] = bad[b];
      CHECK(CONV(1, 8, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
      CHECK(FC(8, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_invalid_parameter);
      /* ... before any unsupported_parameter: with an output scale that puts every other channel out of range */
      CHECK(CONV(1, 8, n, IS, ks, kernel, bias, 1.0e-9f, &op) == qnnp_status_invalid_parameter);
      ks[at] = keep;
    }
  }
  /* unsupported_parameter: one scale_c at or above 1, or below 2^-32 */
  for (size_t at = 0; at < n; at += 16) {
    const float keep = ks[at];
    ks[at] = OS / IS;                                 /* scale_c == 1 */
    CHECK(CONV(1, 8, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_unsupported_parameter);
    CHECK(FC(8, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_unsupported_parameter);
    ks[at] = 0x1.0p-34f;                              /* scale_c == 2^-35 */
    CHECK(CONV(1, 8, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_unsupported_parameter);
    CHECK(FC(8, n, IS, ks, kernel, bias, OS, &op) == qnnp_status_unsupported_parameter);
    ks[at] = keep;
  }
  CHECK(op == NULL);                                  /* a refused create writes no handle */
  CHECK(qnnp_stub_live_allocs() == live);
  /* both ends of the range are inside it */
  {
    float edge[2] = {0x1.0p-32f, 0x1.fffffep-1f};
    uint8_t k2[2] = {1, 2};
    int32_t b2[2] = {0, 0};
    CHECK(qnnp_gfx950_create_fully_connected_nc_q8_per_channel(1, 2, 0, 1.0f, 0, edge, k2, b2, 0, 1.0f, 0, 255, 7, &op) ==
          qnnp_status_success);
    const struct qnnp_requant_pc_entry* t = (const struct qnnp_requant_pc_entry*) op->d_requant_pc;
    CHECK(t[0].multiplier == 0x40000000 && t[0].shift == 31 && t[1].multiplier == 0x7FFFFF80 && t[1].shift == 0);
    CHECK(qnnp_delete_operator(op) == qnnp_status_success);
    op = NULL;
  }

  /* the fused block and the residual attach refuse a per-channel member; the per-tensor twins pass */
  {
    const size_t c = 16;
    float* ksc = scales(c);
    uint8_t* kdw = bytes(c * 9, 1);
    uint8_t* kpw = bytes(c * c, 2);
    int32_t* b = biases(c);
    qnnp_operator_t dw = NULL, pw = NULL, dw_pc = NULL, pw_pc = NULL, add = NULL, fused = NULL;
    CHECK(qnnp_create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, c, 1, 1, 127, IS, 128, 0.01f, kdw, b, 9, OS, 0, 255, 0, &dw) == qnnp_status_success);
    CHECK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, c, c, 127, IS, 128, 0.01f, kpw, b, 9, OS, 0, 255, 0, &pw) == qnnp_status_success);
    CHECK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, c, 1, 1, 127, IS, 128, ksc, kdw, b, 9, OS, 0, 255, 0, &dw_pc) == qnnp_status_success);
    CHECK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, c, c, 127, IS, 128, ksc, kpw, b, 9, OS, 0, 255, 0, &pw_pc) == qnnp_status_success);
    CHECK(qnnp_create_add_nc_q8(c, 9, 1.0f, 9, 1.0f, 9, 2.0f, 0, 255, 0, &add) == qnnp_status_success);
    CHECK(dw->per_channel == 0 && dw->d_requant_pc == NULL && pw->per_channel == 0);
    CHECK(qnnp_gfx950_create_fused_block(NULL, dw_pc, pw, NULL, &fused) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_gfx950_create_fused_block(NULL, dw, pw_pc, NULL, &fused) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_gfx950_create_fused_block(pw_pc, dw, pw, NULL, &fused) == qnnp_status_unsupported_parameter);
    CHECK(fused == NULL);
    CHECK(qnnp_gfx950_create_fused_block(pw, dw, pw, NULL, &fused) == qnnp_status_success);
    CHECK(qnnp_delete_operator(fused) == qnnp_status_success);
    uint8_t* x = bytes(4 * 4 * c, 7);
    uint8_t* y = bytes(4 * 4 * c, 8);
    CHECK(qnnp_setup_convolution2d_nhwc_q8(pw_pc, 1, 4, 4, x, c, y, c, NULL) == qnnp_status_success);
    CHECK(qnnp_gfx950_attach_residual_add(pw_pc, add, x, c) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_setup_convolution2d_nhwc_q8(dw_pc, 1, 4, 4, x, c, y, c, NULL) == qnnp_status_success);
    CHECK(qnnp_gfx950_attach_residual_add(dw_pc, add, x, c) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_run_operator(pw_pc, NULL) == qnnp_status_success);
    CHECK(qnnp_gfx950_operator_residual_folded(pw_pc) == -1);
    CHECK(qnnp_delete_operator(dw) == qnnp_status_success);
    CHECK(qnnp_delete_operator(pw) == qnnp_status_success);
    CHECK(qnnp_delete_operator(dw_pc) == qnnp_status_success);
    CHECK(qnnp_delete_operator(pw_pc) == qnnp_status_success);
    CHECK(qnnp_delete_operator(add) == qnnp_status_success);
    free(x);
    free(y);
    free(ksc);
    free(kdw);
    free(kpw);
    free(b);
  }
  free(ks);
  free(kernel);
  free(bias);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized, whatever the arguments */
  CHECK(CONV(0, 0, 0, 0.0f, NULL, NULL, NULL, 0.0f, &op) == qnnp_status_uninitialized);
  CHECK(FC(0, 0, 0.0f, NULL, NULL, NULL, 0.0f, &op) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  statuses();
  const size_t counts[3] = {1, 3, 33};
  for (int i = 0; i < 3; i++) {
    const size_t n = counts[i];
    fully_connected_walk(1, n);
    fully_connected_walk(70, n);
    convolution_walk(1, 8, n, 1, 1, 0, 1);                 /* 1x1: the GEMM form */
    convolution_walk(1, 5, n, 3, 3, 1, 2);                 /* KxK */
    convolution_walk(1, 3, n, 3, 3, 1, 1);                 /* 3-channel inputs: slots of four */
    convolution_walk(2, 4, n, 1, 1, 0, 1);                 /* grouped 1x1: never the dense image */
    convolution_walk(3, 2, n, 3, 3, 1, 1);                 /* grouped KxK */
    if (n > 1) convolution_walk((uint32_t) n, 1, 1, 3, 3, 1, 1);     /* depthwise */
    if (n > 1) convolution_walk((uint32_t) n, 1, 1, 5, 5, 2, 2);
  }
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-perchannel-ok\n");
  return 0;
}
