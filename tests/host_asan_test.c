/*
 * host_asan_test.c -- TEST INFRASTRUCTURE: drives the product's plain-C host code (compiled with
 * -fsanitize=address,undefined against tests/hip_stub.c) through the public API of include/qnnpack.h the way the
 * reference's operator testers do (test/convolution-operator-tester.h:415-449): create -> setup -> run -> re-setup with
 * another geometry -> run -> delete, over the operator types and the shapes that take different packing / table paths.
 * Any heap overflow, use-after-free, leak or undefined arithmetic in the packers, offset tables, phase splitting,
 * staging logic or error paths aborts the program. Prints "host-sanitizers-ok" on success.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "operator.h"   /* (qnnpack_amd/csrc: the sweeps below check which device images a create built) */

/* tests/hip_stub.c test controls */
void qnnp_stub_fail_nth(long n);
int qnnp_stub_fail_pending(void);
void qnnp_stub_set_capturing(int on);
size_t qnnp_stub_live_allocs(void);

static uint32_t rng_state = 0x1234567u;
static uint8_t rnd8(void) { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t) (rng_state >> 24); }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static uint8_t* random_bytes(size_t n)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = rnd8();
  return p;
}

static int32_t* random_bias(size_t n)
{
  int32_t* p = (int32_t*) malloc(sizeof(int32_t) * (n ? n : 1));
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = (int32_t) (rnd8() * 79) - 10000;
  return p;
}

static size_t out_dim(size_t in, uint32_t pad, uint32_t k, uint32_t d, uint32_t s)
{
  const size_t eff = (size_t) (k - 1) * d + 1;
  return (in + pad - eff) / s + 1;
}

static void conv_case(uint32_t pad, uint32_t kh, uint32_t kw, uint32_t stride, uint32_t dil, uint32_t groups,
                      size_t gic, size_t goc, size_t batch, size_t h, size_t w, size_t extra_stride)
{
  const size_t cin = groups * gic, cout = groups * goc;
  uint8_t* kernel = random_bytes((size_t) groups * goc * kh * kw * gic);
  int32_t* bias = random_bias(cout);
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_convolution2d_nhwc_q8(pad, pad, pad, pad, kh, kw, stride, stride, dil, dil, groups, gic, goc,
      127, 0.5f, 121, 0.5f, kernel, bias, 130, 0.75f, 3, 250, 0, &op) == qnnp_status_success);
  free(kernel);   /* reference ownership: create copied (packed) them */
  free(bias);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  for (int round = 0; round < 3; round++) {
    const size_t hh = h + (size_t) round * 3, ww = w + (size_t) round;
    const size_t in_stride = cin + extra_stride, out_stride = cout + extra_stride;
    const size_t oh = out_dim(hh, 2 * pad, kh, dil, stride), ow = out_dim(ww, 2 * pad, kw, dil, stride);
    uint8_t* in = random_bytes((batch * hh * ww - 1) * in_stride + cin);
    uint8_t* out = random_bytes((batch * oh * ow - 1) * out_stride + cout);
    CHECK(qnnp_setup_convolution2d_nhwc_q8(op, batch, hh, ww, in, in_stride, out, out_stride, NULL) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    /* invalid geometry must not disturb the operator */
    CHECK(qnnp_setup_convolution2d_nhwc_q8(op, batch, 0, ww, in, in_stride, out, out_stride, NULL) == qnnp_status_invalid_parameter);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(in);
    free(out);
  }
  CHECK(qnnp_setup_convolution2d_nhwc_q8(op, 0, 5, 5, NULL, cin, NULL, cout, NULL) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);   /* empty batch */
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void deconv_case(uint32_t pad, uint32_t adj, uint32_t k, uint32_t stride, uint32_t groups, size_t gic, size_t goc,
                        size_t batch, size_t h, size_t w)
{
  uint8_t* kernel = random_bytes((size_t) groups * gic * k * k * goc);
  int32_t* bias = random_bias(groups * goc);
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_deconvolution2d_nhwc_q8(pad, pad, pad, pad, adj, adj, k, k, stride, stride, 1, 1, groups, gic, goc,
      127, 0.5f, 127, 0.5f, kernel, bias, 127, 0.5f, 0, 255, 0, &op) == qnnp_status_success);
  free(kernel);
  free(bias);
  for (int round = 0; round < 2; round++) {
    const size_t hh = h + (size_t) round * 2, ww = w + (size_t) round * 3;
    const size_t oh = stride * (hh - 1) + adj + k - 2 * pad, ow = stride * (ww - 1) + adj + k - 2 * pad;
    uint8_t* in = random_bytes(batch * hh * ww * groups * gic);
    uint8_t* out = random_bytes(batch * oh * ow * groups * goc);
    CHECK(qnnp_setup_deconvolution2d_nhwc_q8(op, batch, hh, ww, in, groups * gic, out, groups * goc, NULL) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(in);
    free(out);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

/* ---- failure injection: every device allocation and upload a create or setup makes may fail ------------------------
 * For n = 0, 1, 2, ... the n-th qnnp_hip_alloc / qnnp_hip_h2d fails (tests/hip_stub.c) until a create no longer reaches
 * it. A create must then answer success or out_of_memory; out_of_memory leaves the handle alone and nothing allocated
 * (ASan reports leaked host memory at exit); a successful create -- optional images may be missing -- must set up, run
 * and delete. */
enum sweep_kind { SWEEP_CONV, SWEEP_DECONV, SWEEP_FC, SWEEP_FUSED };
struct sweep_case {
  enum sweep_kind kind;
  uint32_t pad, kh, kw, stride, dil, groups;
  size_t gic, goc;
  uint8_t kzp;
  size_t h, w;        /* input extent of the setup (fully connected: h = batch) */
  size_t image;       /* offsetof(struct qnnp_operator, <device image>) the case is there to reach, 0: none */
};

static qnnp_operator_t const UNTOUCHED = (qnnp_operator_t) (uintptr_t) 0x5A5A5A5A;

static enum qnnp_status sweep_create(const struct sweep_case* c, const uint8_t* kernel, const int32_t* bias,
                                     qnnp_operator_t* op, qnnp_operator_t members[4])
{
  switch (c->kind) {
    case SWEEP_CONV:
      return qnnp_create_convolution2d_nhwc_q8(c->pad, c->pad, c->pad, c->pad, c->kh, c->kw, c->stride, c->stride, c->dil,
          c->dil, c->groups, c->gic, c->goc, 121, 0.5f, c->kzp, 0.5f, kernel, bias, 130, 0.75f, 0, 255, 0, op);
    case SWEEP_DECONV:
      return qnnp_create_deconvolution2d_nhwc_q8(c->pad, c->pad, c->pad, c->pad, 0, 0, c->kh, c->kw, c->stride, c->stride,
          1, 1, c->groups, c->gic, c->goc, 121, 0.5f, c->kzp, 0.5f, kernel, bias, 130, 0.75f, 0, 255, 0, op);
    case SWEEP_FC:
      return qnnp_create_fully_connected_nc_q8(c->gic, c->goc, 121, 0.5f, c->kzp, 0.5f, kernel, bias, 130, 0.75f, 0, 255,
          0, op);
    case SWEEP_FUSED:
    {
      /* 16 -> 96 expand, 3x3 depthwise, 96 -> 16 project, + input: the members' creates are swept as well */
      enum qnnp_status s;
      s = qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 16, 96, 127, 0.5f, c->kzp, 0.5f, kernel, bias,
          127, 0.5f, 0, 255, 0, &members[0]);
      if (s == qnnp_status_success) {
        s = qnnp_create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 96, 1, 1, 127, 0.5f, c->kzp, 0.5f, kernel, bias,
            127, 0.5f, 0, 255, 0, &members[1]);
      }
      if (s == qnnp_status_success) {
        s = qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 96, 16, 127, 0.5f, c->kzp, 0.5f, kernel, bias,
            127, 0.5f, 0, 255, 0, &members[2]);
      }
      if (s == qnnp_status_success) {
        s = qnnp_create_add_nc_q8(16, 127, 0.5f, 127, 0.5f, 127, 0.75f, 0, 255, 0, &members[3]);
      }
      if (s == qnnp_status_success) {
        s = qnnp_gfx950_create_fused_block(members[0], members[1], members[2], members[3], op);
      }
      return s;
    }
  }
  return qnnp_status_invalid_parameter;
}

static size_t sweep_out_dim(const struct sweep_case* c, size_t in)
{
  if (c->kind == SWEEP_DECONV) return c->stride * (in - 1) + c->kh - 2 * c->pad;
  return out_dim(in, 2 * c->pad, c->kh, c->dil, c->stride);
}

static enum qnnp_status sweep_setup(const struct sweep_case* c, qnnp_operator_t op, size_t h, size_t w, const uint8_t* in,
                                    uint8_t* out)
{
  const size_t cin = c->groups * c->gic, cout = c->groups * c->goc;
  switch (c->kind) {
    case SWEEP_CONV: return qnnp_setup_convolution2d_nhwc_q8(op, 2, h, w, in, cin, out, cout, NULL);
    case SWEEP_DECONV: return qnnp_setup_deconvolution2d_nhwc_q8(op, 2, h, w, in, cin, out, cout, NULL);
    case SWEEP_FC: return qnnp_setup_fully_connected_nc_q8(op, h, in, cin, out, cout);
    case SWEEP_FUSED: return qnnp_gfx950_setup_fused_block(op, 2, h, w, in, 16, out, 16);
  }
  return qnnp_status_invalid_parameter;
}

static size_t sweep_in_bytes(const struct sweep_case* c, size_t h, size_t w)
{
  if (c->kind == SWEEP_FC) return h * c->gic;
  return 2 * h * w * (c->kind == SWEEP_FUSED ? 16 : c->groups * c->gic);
}

static size_t sweep_out_bytes(const struct sweep_case* c, size_t h, size_t w)
{
  if (c->kind == SWEEP_FC) return h * c->goc;
  if (c->kind == SWEEP_FUSED) return 2 * h * w * 16;
  return 2 * sweep_out_dim(c, h) * sweep_out_dim(c, w) * c->groups * c->goc;
}

static void delete_all(qnnp_operator_t op, qnnp_operator_t members[4])
{
  if (op != UNTOUCHED) CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  for (int i = 0; i < 4; i++) {
    if (members[i] != NULL) CHECK(qnnp_delete_operator(members[i]) == qnnp_status_success);
    members[i] = NULL;
  }
}

/* set up at (h, w) with the n-th device call failing (n < 0: none; *reached: that call happened); a failed setup must
 * leave the operator unrunnable. Returns 1 for out_of_memory. */
static int setup_and_run(const struct sweep_case* c, qnnp_operator_t op, size_t h, size_t w, long n, int* reached)
{
  uint8_t* in = random_bytes(sweep_in_bytes(c, h, w));
  uint8_t* out = random_bytes(sweep_out_bytes(c, h, w));
  qnnp_stub_fail_nth(n);
  const enum qnnp_status s = sweep_setup(c, op, h, w, in, out);
  const int failed = !qnnp_stub_fail_pending() && n >= 0;
  qnnp_stub_fail_nth(-1);
  if (reached != NULL) *reached = failed;
  if (s == qnnp_status_success) {
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  } else {
    CHECK(s == qnnp_status_out_of_memory && failed);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
  }
  free(in);
  free(out);
  return s == qnnp_status_out_of_memory;
}

static void sweep(const struct sweep_case* c)
{
  const size_t kernel_bytes = c->kind == SWEEP_FUSED ? 96 * 16 : c->kind == SWEEP_FC ? c->gic * c->goc :
      c->groups * c->gic * c->kh * c->kw * c->goc;
  uint8_t* kernel = random_bytes(kernel_bytes);
  int32_t* bias = random_bias(c->kind == SWEEP_FUSED ? 96 : c->groups * c->goc);
  if (c->kind == SWEEP_CONV && c->gic == 1 && c->goc == 1) {
    for (size_t i = 0; i < kernel_bytes; i++) kernel[i] = (uint8_t) (c->kzp - 100 + kernel[i] % 200);   /* w - kzp fits int8 */
  }
  int create_ooms = 0, setup_ooms = 0;
  for (long n = 0; ; n++) {
    const size_t live = qnnp_stub_live_allocs();
    qnnp_operator_t op = UNTOUCHED, members[4] = {NULL, NULL, NULL, NULL};
    qnnp_stub_fail_nth(n);
    const enum qnnp_status s = sweep_create(c, kernel, bias, &op, members);
    const int reached = !qnnp_stub_fail_pending();
    qnnp_stub_fail_nth(-1);
    if (s == qnnp_status_out_of_memory) {
      CHECK(op == UNTOUCHED);
      delete_all(op, members);
      CHECK(qnnp_stub_live_allocs() == live);
      create_ooms++;
    } else {
      CHECK(s == qnnp_status_success && op != UNTOUCHED);
      if (!reached && c->image != 0) {
        CHECK(*(void**) ((char*) op + c->image) != NULL);   /* the case reaches the image it is there for */
      }
      CHECK(setup_and_run(c, op, c->h, c->w, -1, NULL) == 0);
      delete_all(op, members);
      CHECK(qnnp_stub_live_allocs() == live);
    }
    if (!reached) break;
  }
  CHECK(create_ooms > 0);

  /* setup: small geometry first, then a larger one (the device tables and staging grow) with the n-th call failing,
   * then that geometry again without failures */
  for (long n = 0; ; n++) {
    const size_t live = qnnp_stub_live_allocs();
    qnnp_operator_t op = UNTOUCHED, members[4] = {NULL, NULL, NULL, NULL};
    CHECK(sweep_create(c, kernel, bias, &op, members) == qnnp_status_success);
    CHECK(setup_and_run(c, op, c->h, c->w, -1, NULL) == 0);
    const size_t h2 = c->h + 5, w2 = c->w + 3;
    int reached = 0;
    setup_ooms += setup_and_run(c, op, h2, w2, n, &reached);
    CHECK(setup_and_run(c, op, h2, w2, -1, NULL) == 0);
    delete_all(op, members);
    CHECK(qnnp_stub_live_allocs() == live);
    if (!reached) break;
  }
  CHECK(setup_ooms > 0);
  free(kernel);
  free(bias);
}

/* Inside a graph capture every create and setup refuses with invalid_parameter, writes no handle and allocates nothing. */
static void capture_refusals(void)
{
  uint8_t* k = random_bytes(96 * 16);
  int32_t* b = random_bias(96);
  uint8_t* x = random_bytes(2 * 8 * 8 * 96);
  uint8_t* y = random_bytes(2 * 8 * 8 * 96);
  qnnp_operator_t conv = NULL, dw = NULL, project = NULL, deconv = NULL, fc = NULL, add = NULL, gap = NULL, fused = NULL;
  CHECK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 16, 96, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &conv) == qnnp_status_success);
  CHECK(qnnp_create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 96, 1, 1, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &dw) == qnnp_status_success);
  CHECK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 96, 16, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &project) == qnnp_status_success);
  CHECK(qnnp_create_deconvolution2d_nhwc_q8(0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 16, 8, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &deconv) == qnnp_status_success);
  CHECK(qnnp_create_fully_connected_nc_q8(16, 16, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &fc) == qnnp_status_success);
  CHECK(qnnp_create_add_nc_q8(96, 127, 0.5f, 127, 0.5f, 127, 0.75f, 0, 255, 0, &add) == qnnp_status_success);
  CHECK(qnnp_create_global_average_pooling_nwc_q8(16, 127, 0.5f, 127, 0.75f, 0, 255, 0, &gap) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_fused_block(conv, dw, project, NULL, &fused) == qnnp_status_success);
  CHECK(qnnp_setup_convolution2d_nhwc_q8(dw, 2, 8, 8, x, 96, y, 96, NULL) == qnnp_status_success);

  const size_t live = qnnp_stub_live_allocs();
  qnnp_operator_t op = UNTOUCHED;
  qnnp_stub_set_capturing(1);
  CHECK(qnnp_create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 1, 16, 16, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_deconvolution2d_nhwc_q8(0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 16, 8, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_fully_connected_nc_q8(16, 16, 127, 0.5f, 127, 0.5f, k, b, 127, 0.5f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_add_nc_q8(96, 127, 0.5f, 127, 0.5f, 127, 0.75f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_global_average_pooling_nwc_q8(16, 127, 0.5f, 127, 0.75f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_fused_block(conv, dw, project, NULL, &op) == qnnp_status_invalid_parameter);
  CHECK(op == UNTOUCHED);
  CHECK(qnnp_setup_convolution2d_nhwc_q8(conv, 2, 8, 8, x, 16, y, 96, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_deconvolution2d_nhwc_q8(deconv, 2, 8, 8, x, 16, y, 8, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_fully_connected_nc_q8(fc, 4, x, 16, y, 16) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_add_nc_q8(add, 4, x, 96, x, 96, y, 96) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_global_average_pooling_nwc_q8(gap, 2, 8, x, 16, y, 16) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_fused_block(fused, 2, 8, 8, x, 16, y, 16) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_residual_add(dw, add, x, 96) == qnnp_status_invalid_parameter);
  CHECK(qnnp_stub_live_allocs() == live);
  qnnp_stub_set_capturing(0);

  qnnp_operator_t ops[] = {conv, dw, project, deconv, fc, add, gap, fused};
  for (size_t i = 0; i < sizeof(ops) / sizeof(ops[0]); i++) CHECK(qnnp_delete_operator(ops[i]) == qnnp_status_success);
  free(k); free(b); free(x); free(y);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  uint8_t k4[16] = {0};
  int32_t b4[4] = {0};
  /* before initialization everything answers uninitialized (reference convolution.c:69-72) */
  CHECK(qnnp_create_fully_connected_nc_q8(4, 4, 0, 1.0f, 0, 1.0f, k4, b4, 0, 2.0f, 0, 255, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_initialize() == qnnp_status_success);
  CHECK(qnnp_initialize() == qnnp_status_success);
  CHECK(qnnp_gfx950_set_device(0) == qnnp_status_success);
  CHECK(qnnp_gfx950_set_device(3) == qnnp_status_invalid_parameter);

  /* parameter validation (reference convolution.c:74-176) */
  CHECK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 4, 4, 0, 1.0f, 0, 1.0f, k4, b4, 0, 2.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 4, 4, 0, 1.0f, 0, 1.0f, k4, b4, 0, 0.5f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_delete_operator(NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_run_operator(NULL, NULL) == qnnp_status_invalid_parameter);

  /*        pad kh kw s  d  groups gic goc batch h   w  extra-stride */
  conv_case(0, 1, 1, 1, 1, 1,    23, 19, 2,   7,  9, 0);    /* pointwise GEMM, ragged channels */
  conv_case(0, 1, 1, 1, 1, 2,    17, 19, 1,   6,  5, 3);    /* grouped, padded pixel strides */
  conv_case(1, 3, 3, 1, 1, 1,    15, 17, 3,   10, 9, 0);    /* offset table */
  conv_case(1, 3, 3, 2, 1, 1,     3, 32, 2,   17, 19, 2);   /* 3-channel first layer (4-wide tap slots) */
  conv_case(2, 3, 3, 1, 2, 2,    14, 13, 1,   11, 12, 0);   /* dilated, grouped */
  conv_case(1, 3, 3, 1, 1, 27,    1,  1, 2,   15, 14, 0);   /* depthwise, ragged channels */
  conv_case(1, 3, 3, 2, 1, 96,    1,  1, 2,   15, 14, 0);   /* depthwise, matrix-core weight image */
  conv_case(2, 5, 5, 1, 1, 40,    1,  1, 1,   12, 13, 8);   /* depthwise 5x5 */
  conv_case(1, 3, 3, 1, 1, 1,    64, 64, 2,   14, 14, 0);   /* power-of-two channels (LDS-tiled kernel image) */

  /*          pad adj k stride groups gic goc batch h  w */
  deconv_case(0,  0,  2, 2,    1,     16, 8,  2,    5, 6);  /* kernel == stride: depth-to-space GEMM */
  deconv_case(1,  1,  3, 2,    1,     8,  12, 2,    5, 4);  /* phase split */
  deconv_case(1,  0,  3, 1,    2,     6,  5,  1,    6, 7);  /* single table, grouped */
  deconv_case(0,  1,  4, 3,    1,     4,  4,  1,    3, 3);  /* 9 phases, some without taps */

  /* fully connected */
  for (int round = 0; round < 2; round++) {
    const size_t kc = round ? 1024 : 37, n = round ? 1000 : 29, batch = round ? 1 : 5;
    uint8_t* kernel = random_bytes(n * kc);
    int32_t* bias = random_bias(n);
    CHECK(qnnp_create_fully_connected_nc_q8(kc, n, 127, 0.5f, 127, 0.5f, kernel, bias, 127, 0.5f, 0, 255, 0, &op) == qnnp_status_success);
    free(kernel);
    free(bias);
    uint8_t* in = random_bytes(batch * (kc + 3));
    uint8_t* out = random_bytes(batch * (n + 5));
    CHECK(qnnp_setup_fully_connected_nc_q8(op, batch, in, kc + 3, out, n + 5) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    float ms = 0.0f;
    CHECK(qnnp_gfx950_time_operator(op, 1, 3, &ms) == qnnp_status_invalid_parameter);   /* host tensors cannot be timed */
    free(in);
    free(out);
    CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  }

  /* add + global average pooling */
  {
    CHECK(qnnp_create_add_nc_q8(24, 121, 0.75f, 127, 1.25f, 133, 0.96875f, 0, 255, 0, &op) == qnnp_status_success);
    uint8_t* a = random_bytes(9 * 31), * b = random_bytes(9 * 29), * s = random_bytes(9 * 24);
    CHECK(qnnp_setup_add_nc_q8(op, 9, a, 31, b, 29, s, 24) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_setup_add_nc_q8(op, 9, a, 3, b, 29, s, 24) == qnnp_status_invalid_parameter);   /* stride < channels */
    free(a); free(b); free(s);
    CHECK(qnnp_delete_operator(op) == qnnp_status_success);
    CHECK(qnnp_create_global_average_pooling_nwc_q8(77, 121, 1.0f, 133, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
    uint8_t* x = random_bytes(3 * 49 * 80), * y = random_bytes(3 * 77);
    CHECK(qnnp_setup_global_average_pooling_nwc_q8(op, 3, 49, x, 80, y, 77) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(x); free(y);
    CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  }

  /* the same three parameter builders over their whole accepted ranges (requantization.h): an add at one ratio pair per
   * exponent of the larger ratio, -14 ... 7 (its right shift is 21 - exponent: beyond 31 below 2^-10), and the two
   * average poolings at both ends of [2^-8, 2^8) */
  {
    uint8_t* a = random_bytes(9 * 31), * b = random_bytes(9 * 29), * s = random_bytes(9 * 24);
    for (int e = -14; e <= 7; e++) {
      const float larger = ldexpf(1.37f, e);
      const float smaller = e > -14 ? ldexpf(1.0f, -14) : larger;
      for (int swap = 0; swap < 2; swap++) {
        CHECK(qnnp_create_add_nc_q8(24, 121, swap ? smaller : larger, 127, swap ? larger : smaller, 133, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
        CHECK(qnnp_setup_add_nc_q8(op, 9, a, 31, b, 29, s, 24) == qnnp_status_success);
        CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
        CHECK(qnnp_delete_operator(op) == qnnp_status_success);
      }
    }
    CHECK(qnnp_create_add_nc_q8(24, 121, 1.0f, 127, 1.0f, 133, 4096.0f, 0, 255, 0, &op) == qnnp_status_success);   /* 2^-12 both */
    CHECK(qnnp_delete_operator(op) == qnnp_status_success);
    CHECK(qnnp_create_add_nc_q8(24, 121, nextafterf(256.0f, 0.0f), 127, ldexpf(1.0f, -14), 133, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
    CHECK(qnnp_delete_operator(op) == qnnp_status_success);
    CHECK(qnnp_create_add_nc_q8(24, 121, 1.0f, 127, 1.0f, 133, 32768.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);   /* 2^-15 */
    CHECK(qnnp_create_add_nc_q8(24, 121, 256.0f, 127, 1.0f, 133, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
    free(a); free(b); free(s);

    const float ends[2] = {ldexpf(1.0f, -8), nextafterf(256.0f, 0.0f)};
    uint8_t* x = random_bytes(2 * 300 * 19), * y = random_bytes(2 * 7 * 7 * 19);
    for (int i = 0; i < 2; i++) {
      CHECK(qnnp_create_global_average_pooling_nwc_q8(19, 0, ends[i], 255, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
      for (size_t width = 1; width <= 300; width *= 300) {
        CHECK(qnnp_setup_global_average_pooling_nwc_q8(op, 2, width, x, 19, y, 19) == qnnp_status_success);
        CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
      }
      CHECK(qnnp_delete_operator(op) == qnnp_status_success);
      /* 2x2 stride 2, then 7x7 over a 7x7 image with padding 1 */
      CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 2, 2, 19, 255, ends[i], 0, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
      CHECK(qnnp_setup_average_pooling2d_nhwc_q8(op, 2, 6, 6, x, 19, y, 19, NULL) == qnnp_status_success);
      CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
      CHECK(qnnp_delete_operator(op) == qnnp_status_success);
      CHECK(qnnp_create_average_pooling2d_nhwc_q8(1, 1, 1, 1, 7, 7, 1, 1, 19, 0, ends[i], 255, 1.0f, 100, 101, 0, &op) == qnnp_status_success);
      CHECK(qnnp_setup_average_pooling2d_nhwc_q8(op, 2, 7, 7, x, 19, y, 19, NULL) == qnnp_status_success);
      CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
      CHECK(qnnp_delete_operator(op) == qnnp_status_success);
    }
    CHECK(qnnp_create_global_average_pooling_nwc_q8(19, 0, 256.0f, 255, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 2, 2, 19, 0, ldexpf(1.0f, -9), 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
    free(x); free(y);
  }

  /* fused block built from stand-alone operators */
  {
    qnnp_operator_t expand = NULL, dw = NULL, project = NULL, add = NULL, fused = NULL;
    uint8_t* ke = random_bytes(96 * 16); int32_t* be = random_bias(96);
    uint8_t* kd = random_bytes(96 * 9); int32_t* bd = random_bias(96);
    uint8_t* kp = random_bytes(16 * 96); int32_t* bp = random_bias(16);
    CHECK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 16, 96, 127, 0.5f, 127, 0.5f, ke, be, 127, 0.5f, 0, 255, 0, &expand) == qnnp_status_success);
    CHECK(qnnp_create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 96, 1, 1, 127, 0.5f, 127, 0.5f, kd, bd, 127, 0.5f, 0, 255, 0, &dw) == qnnp_status_success);
    CHECK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 96, 16, 127, 0.5f, 127, 0.5f, kp, bp, 127, 0.5f, 0, 255, 0, &project) == qnnp_status_success);
    CHECK(qnnp_create_add_nc_q8(16, 127, 0.5f, 127, 0.5f, 127, 0.75f, 0, 255, 0, &add) == qnnp_status_success);
    free(ke); free(be); free(kd); free(bd); free(kp); free(bp);
    CHECK(qnnp_gfx950_create_fused_block(expand, dw, project, add, &fused) == qnnp_status_success);
    uint8_t* x = random_bytes(2 * 14 * 14 * 16), * y = random_bytes(2 * 14 * 14 * 16);
    CHECK(qnnp_gfx950_setup_fused_block(fused, 2, 14, 14, x, 16, y, 16) == qnnp_status_success);
    CHECK(qnnp_run_operator(fused, NULL) == qnnp_status_success);
    free(x); free(y);
    CHECK(qnnp_delete_operator(fused) == qnnp_status_success);
    CHECK(qnnp_delete_operator(expand) == qnnp_status_success);
    CHECK(qnnp_delete_operator(dw) == qnnp_status_success);
    CHECK(qnnp_delete_operator(project) == qnnp_status_success);
    CHECK(qnnp_delete_operator(add) == qnnp_status_success);
  }

  /* failure injection over creates and setups that take every device image path */
  {
#define IMAGE(field) offsetof(struct qnnp_operator, field)
    static const struct sweep_case cases[] = {
      /* kind        pad kh kw s  d  groups gic  goc  kzp  h   w   image */
      {SWEEP_CONV,   1, 3, 3, 1, 1, 40,    1,   1,   128, 9,  10, IMAGE(d_dw_dot4)},          /* depthwise 3x3, int8-range weights */
      {SWEEP_CONV,   2, 5, 5, 2, 1, 24,    1,   1,   127, 11, 9,  IMAGE(d_dw_dot4)},          /* depthwise 5x5, int8-range weights */
      {SWEEP_CONV,   3, 7, 7, 1, 1, 33,    1,   1,   121, 10, 12, IMAGE(d_dwm_x)},            /* depthwise 7x7 */
      {SWEEP_CONV,   1, 3, 3, 2, 1, 1,     3,   32,  127, 13, 11, IMAGE(d_bias_rows)},        /* 3 channels, 16-byte row slots */
      {SWEEP_CONV,   3, 7, 7, 2, 1, 1,     3,   64,  127, 15, 14, IMAGE(d_bias_rows)},        /* 3 channels, 32-byte row slots */
      {SWEEP_CONV,   0, 1, 1, 1, 1, 4,     24,  40,  121, 6,  7,  IMAGE(d_weights_dense)},    /* grouped 1x1, dense image */
      {SWEEP_CONV,   0, 1, 1, 1, 1, 1,     512, 256, 127, 3,  4,  IMAGE(d_weights_centred)},  /* centred 1x1 */
      {SWEEP_CONV,   1, 3, 3, 1, 1, 1,     48,  64,  127, 7,  6,  IMAGE(d_weights_centred)},  /* small 3x3 (ws16s), centred */
      {SWEEP_DECONV, 0, 2, 2, 2, 1, 1,     16,  8,   127, 5,  6,  IMAGE(d_weights)},          /* depth-to-space */
      {SWEEP_DECONV, 1, 3, 3, 2, 1, 1,     8,   12,  127, 5,  4,  IMAGE(phase[1].d_weights)}, /* phases */
      {SWEEP_DECONV, 1, 3, 3, 1, 1, 2,     6,   5,   121, 6,  7,  IMAGE(d_weights)},          /* stride 1: one table */
      {SWEEP_FC,     0, 1, 1, 1, 1, 1,     1024,256, 127, 5,  1,  IMAGE(d_weights_centred)},  /* fully connected, centred */
      {SWEEP_FUSED,  0, 3, 3, 1, 1, 1,     16,  16,  127, 8,  9,  IMAGE(d_strip)},            /* fused block */
    };
#undef IMAGE
    for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); i++) sweep(&cases[i]);
    capture_refusals();
  }

  CHECK(qnnp_deinitialize() == qnnp_status_success);
  puts("host-sanitizers-ok");
  return 0;
}
