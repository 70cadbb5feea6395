/*
 * host_asan_lifecycle_test.c -- TEST INFRASTRUCTURE: the create / setup lifecycle of EVERY operator under
 * AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and all the per-operator launch stubs (Makefile
 * target asan-lifecycle; run by tests/test_lifecycle_host.py). Where the other host programs walk one operator family in
 * depth, this one asks every public create and setup the same questions and compares the returned status with ONE
 * table (ROWS below): before qnnp_initialize, a bad argument of each class outside and inside a pretend graph capture
 * (which pins, per entry point, whether it validates before or after it enters the device), NULL and foreign handles,
 * batch 0, a staging allocation that fails, and the input / output overlap rules of the NC operators. The table is a
 * record of what the library answers, oddities included; it is not a specification. Prints "host-sanitizers-lifecycle-ok".
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

/* tests/hip_stub.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
int qnnp_stub_fail_pending(void);
size_t qnnp_stub_live_allocs(void);

static const char* g_row = "";
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: [%s] check failed: %s\n", __FILE__, __LINE__, g_row, #cond); exit(1); } } while (0)
/* a status against the table: prints both on a mismatch */
#define EXPECT(got, want) do { const int g_ = (int) (got), w_ = (int) (want); if (g_ != w_) { \
    fprintf(stderr, "%s:%d: [%s] %s answered %d, the table says %d\n", __FILE__, __LINE__, g_row, #got, g_, w_); exit(1); } } while (0)

#define OK  qnnp_status_success
#define UN  qnnp_status_uninitialized
#define INV qnnp_status_invalid_parameter
#define UNS qnnp_status_unsupported_parameter
#define OOM qnnp_status_out_of_memory
#define NA  ((enum qnnp_status) -1)   /* the create has no argument of that class / the operator no third tensor */

enum kind {
  CONV, GEMM, DWCONV, DECONV, FC, ADD, GAP, MAXPOOL, AVGPOOL, SHUFFLE, CLAMP, LUT, SIGMOID, LEAKY, HARDSWISH, HARDSIGMOID,
  SOFTARGMAX, MULTIPLY, RESIZE, FUSED, KINDS
};
enum variant { GOOD, INVALID, UNSUPPORTED };

/*
 * The record. Columns:
 *   foreign            the operator whose handle the setup is offered in place of its own
 *   invalid            create with one invalid-parameter-class argument (outside a capture)
 *   unsupported        create with one unsupported-parameter-class argument, outside a capture
 *   unsupported_cap    the same create inside a capture: invalid_parameter where the entry point enters the device before
 *                      it validates, unsupported_parameter where it validates first
 *   foreign_setup      setup of a `foreign` handle
 *   capture_setup      a valid setup inside a capture (the operator then still runs with its previous binding)
 *   batch0_setup/_run  a batch-0 setup of a FRESH operator, and the qnnp_run_operator after it (the setup marks the
 *                      operator valid, so the run succeeds and does nothing)
 *   fail[n]            a valid setup with larger tensors whose n-th device allocation / upload fails (hip_stub.c counts
 *                      both); the run after it answers invalid_parameter, the next good setup runs again
 * Every create answers uninitialized before qnnp_initialize, and so does every setup, even of a NULL handle; after it, a
 * setup of a NULL handle answers invalid_parameter: those two columns are the same for all rows and checked in main().
 */
static const struct row {
  const char* name;
  enum kind foreign;
  enum qnnp_status invalid, unsupported, unsupported_cap, foreign_setup, capture_setup, batch0_setup, batch0_run, fail[3];
} ROWS[KINDS] = {
  [CONV]        = { "convolution",       DECONV,     INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [GEMM]        = { "convolution 1x1",   DECONV,     INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [DWCONV]      = { "convolution dw",    DECONV,     INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [DECONV]      = { "deconvolution",     CONV,       INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [FC]          = { "fully connected",   ADD,        INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [ADD]         = { "add",               GAP,        INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, OOM } },
  [GAP]         = { "global avg pool",   ADD,        INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [MAXPOOL]     = { "max pooling",       AVGPOOL,    INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [AVGPOOL]     = { "average pooling",   MAXPOOL,    INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [SHUFFLE]     = { "channel shuffle",   CLAMP,      INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [CLAMP]       = { "clamp",             SHUFFLE,    INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
  [LUT]         = { "lookup table",      SOFTARGMAX, INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, NA } },
  [SIGMOID]     = { "sigmoid",           CLAMP,      INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, NA } },
  [LEAKY]       = { "leaky relu",        CLAMP,      INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, NA } },
  [HARDSWISH]   = { "hardswish",         CLAMP,      INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, NA } },
  [HARDSIGMOID] = { "hardsigmoid",       CLAMP,      INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, NA } },
  [SOFTARGMAX]  = { "softargmax",        LUT,        INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, NA } },
  [MULTIPLY]    = { "multiply",          ADD,        INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, OOM } },
  /* resize uploads its axis tables before it binds: failure 0 is that upload, 1 and 2 are the two staging buffers */
  [RESIZE]      = { "resize bilinear",   MAXPOOL,    INV, UNS, UNS, INV, INV, OK, OK, { OOM, OOM, OOM } },
  /* the fused block enters its depthwise member's device, which refuses inside a capture */
  [FUSED]       = { "fused block",       DWCONV,     INV, UNS, INV, INV, INV, OK, OK, { OOM, OOM, NA } },
};

/* The NC setups' overlap rules, batch 3 of 16 channels: exactly in place; the same pointer with another stride; spans
 * that overlap in part; disjoint spans. Channel shuffle has no in-place form. */
static const struct nc_row {
  enum kind kind;
  enum qnnp_status in_place, other_stride, partial, disjoint;
} NC_ROWS[] = {
  { CLAMP,      OK,  INV, INV, OK },
  { LUT,        OK,  INV, INV, OK },
  { SIGMOID,    OK,  INV, INV, OK },
  { SOFTARGMAX, OK,  INV, INV, OK },
  { SHUFFLE,    INV, INV, INV, OK },
};

/* qnnp_gfx950_attach_residual_add, in the table's terms. It validates before it enters the device, and the stub's
 * tensors are host memory, which the attach refuses as unsupported once it has entered. */
static const struct {
  enum qnnp_status null_handle, foreign, unsupported, unsupported_cap, host_tensors, host_tensors_cap;
} ATTACH = { INV, INV, UNS, UNS, UNS, INV };

#define ARENA ((size_t) 1 << 16)
#define MAX_BATCH 24
static uint8_t* g_in;
static uint8_t* g_in2;
static uint8_t* g_out;
static uint8_t g_kernel[2048];
static int32_t g_bias[128];
static uint8_t g_table[256];
static qnnp_operator_t const UNTOUCHED = (qnnp_operator_t) (uintptr_t) 0x5A5A5A5A;
/* the fused block's members (borrowed by every fused handle, so they live for the whole program) */
static qnnp_operator_t g_expand, g_depthwise, g_project, g_block_add;

static enum qnnp_status create_conv(uint32_t pad, uint32_t k, uint32_t groups, size_t gic, size_t goc, enum variant v,
                                    qnnp_operator_t* op)
{
  return qnnp_create_convolution2d_nhwc_q8(pad, pad, pad, pad, k, k, 1, 1, 1, 1, groups, gic, goc,
      127, v == INVALID ? 0.0f : 0.5f, 127, 0.5f, g_kernel, g_bias, 127, v == UNSUPPORTED ? 0.125f : 0.5f, 0, 255, 0, op);
}

static enum qnnp_status create(enum kind k, enum variant v, qnnp_operator_t* op)
{
  const size_t too_many = (size_t) INT32_MAX + 1;
  switch (k) {
    case CONV: return create_conv(1, 3, 1, 8, 8, v, op);
    case GEMM: return create_conv(0, 1, 1, 16, 96, v, op);
    case DWCONV: return create_conv(1, 3, 96, 1, 1, v, op);
    case DECONV:
      return qnnp_create_deconvolution2d_nhwc_q8(0, 0, 0, 0, 0, 0, v == INVALID ? 0 : 2, 2, 2, 2, 1, 1, 1, 16, 8,
          127, 0.5f, 127, 0.5f, g_kernel, g_bias, 127, v == UNSUPPORTED ? 0.25f : 0.5f, 0, 255, 0, op);
    case FC:
      return qnnp_create_fully_connected_nc_q8(16, 16, 127, 0.5f, 127, 0.5f, g_kernel, v == INVALID ? NULL : g_bias,
          127, v == UNSUPPORTED ? 0.25f : 0.5f, 0, 255, 0, op);
    case ADD:
      return qnnp_create_add_nc_q8(v == INVALID ? 0 : 16, 127, 0.5f, 127, 0.5f, 127, v == UNSUPPORTED ? 32768.0f : 0.75f,
          0, 255, 0, op);
    case GAP:
      return qnnp_create_global_average_pooling_nwc_q8(v == INVALID ? 0 : 16, 127, v == UNSUPPORTED ? 256.0f : 0.5f,
          127, v == UNSUPPORTED ? 1.0f : 0.75f, 0, 255, 0, op);
    case MAXPOOL:
      return qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, v == INVALID ? 1 : 2, v == INVALID ? 1 : 2, 2, 2, 1, 1,
          v == UNSUPPORTED ? too_many : 16, 0, 255, 0, op);
    case AVGPOOL:
      return qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, v == INVALID ? 0 : 2, 2, 16, 127,
          v == UNSUPPORTED ? ldexpf(1.0f, -9) : 0.5f, 127, v == UNSUPPORTED ? 1.0f : 0.75f, 0, 255, 0, op);
    case SHUFFLE:
      return qnnp_create_channel_shuffle_nc_x8(v == INVALID ? 1 : (v == UNSUPPORTED ? 65536 : 2),
          v == UNSUPPORTED ? 65536 : 8, 0, op);
    case CLAMP:
      return qnnp_create_clamp_nc_u8(v == UNSUPPORTED ? too_many : 16, v == INVALID ? 200 : 10, v == INVALID ? 100 : 200, 0, op);
    case LUT:
      return qnnp_gfx950_create_lut_nc_x8(v == UNSUPPORTED ? too_many : 16, v == INVALID ? NULL : g_table, 0, op);
    case SIGMOID:
      return qnnp_create_sigmoid_nc_q8(16, 127, 0.5f, 0, v == UNSUPPORTED ? 0.5f : 0x1.0p-8f, v == INVALID ? 255 : 0, 255, 0, op);
    case LEAKY:
      return qnnp_create_leaky_relu_nc_q8(16, v == INVALID ? 2.0f : 0.25f, 127, v == UNSUPPORTED ? 1024.0f : 0.5f,
          127, 0.5f, 0, 255, 0, op);
    case HARDSWISH:
      return qnnp_gfx950_create_hardswish_nc_q8(v == INVALID ? 0 : (v == UNSUPPORTED ? too_many : 16), 127, 0.0625f,
          127, 0.0625f, 0, 255, 0, op);
    case HARDSIGMOID:
      return qnnp_gfx950_create_hardsigmoid_nc_q8(v == INVALID ? 0 : 16, 127, 0.0625f, v == UNSUPPORTED ? 1 : 0,
          0x1.0p-8f, 0, 255, 0, op);
    case SOFTARGMAX:
      return qnnp_create_softargmax_nc_q8(v == INVALID ? 0 : 16, 0.0625f, v == UNSUPPORTED ? 1 : 0, 0x1.0p-8f, 0, op);
    case MULTIPLY:
      return qnnp_gfx950_create_multiply_nc_q8(16, 127, 0.5f, 127, 0.5f, 127, v == UNSUPPORTED ? 0.125f : 0.5f,
          v == INVALID ? 255 : 0, 255, 0, op);
    case RESIZE:
      return qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(v == UNSUPPORTED ? too_many : 16, v == INVALID ? 0x80u : 0, op);
    case FUSED:
      /* invalid: no depthwise member; unsupported: a 1x1 convolution in the depthwise member's place */
      return qnnp_gfx950_create_fused_block(g_expand, v == INVALID ? NULL : (v == UNSUPPORTED ? g_expand : g_depthwise),
          g_project, g_block_add, op);
    default: break;
  }
  CHECK(!"kind");
  return NA;
}

/* every 2-D operator sees batch x 4 x 4 pixels; `in` and `out` may be any pointers, the strides are the channel counts */
static enum qnnp_status setup(enum kind k, qnnp_operator_t op, size_t batch, const uint8_t* in, const uint8_t* in2, uint8_t* out)
{
  CHECK(batch <= MAX_BATCH);   /* x 6 x 6 pixels x 96 channels stays inside an arena */
  switch (k) {
    case CONV: return qnnp_setup_convolution2d_nhwc_q8(op, batch, 4, 4, in, 8, out, 8, NULL);
    case GEMM: return qnnp_setup_convolution2d_nhwc_q8(op, batch, 4, 4, in, 16, out, 96, NULL);
    case DWCONV: return qnnp_setup_convolution2d_nhwc_q8(op, batch, 4, 4, in, 96, out, 96, NULL);
    case DECONV: return qnnp_setup_deconvolution2d_nhwc_q8(op, batch, 4, 4, in, 16, out, 8, NULL);
    case FC: return qnnp_setup_fully_connected_nc_q8(op, batch, in, 16, out, 16);
    case ADD: return qnnp_setup_add_nc_q8(op, batch, in, 16, in2, 16, out, 16);
    case GAP: return qnnp_setup_global_average_pooling_nwc_q8(op, batch, 4, in, 16, out, 16);
    case MAXPOOL: return qnnp_setup_max_pooling2d_nhwc_u8(op, batch, 4, 4, in, 16, out, 16, NULL);
    case AVGPOOL: return qnnp_setup_average_pooling2d_nhwc_q8(op, batch, 4, 4, in, 16, out, 16, NULL);
    case SHUFFLE: return qnnp_setup_channel_shuffle_nc_x8(op, batch, in, 16, out, 16);
    case CLAMP: return qnnp_setup_clamp_nc_u8(op, batch, in, 16, out, 16);
    case LUT: case HARDSWISH: case HARDSIGMOID: return qnnp_gfx950_setup_lut_nc_x8(op, batch, in, 16, out, 16);
    case SIGMOID: return qnnp_setup_sigmoid_nc_q8(op, batch, in, 16, out, 16);
    case LEAKY: return qnnp_setup_leaky_relu_nc_q8(op, batch, in, 16, out, 16);
    case SOFTARGMAX: return qnnp_setup_softargmax_nc_q8(op, batch, in, 16, out, 16);
    case MULTIPLY: return qnnp_gfx950_setup_multiply_nc_q8(op, batch, 2, in, 16, in2, 16, out, 16);
    case RESIZE: return qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, batch, 4, 4, 6, 6, in, 16, out, 16);
    case FUSED: return qnnp_gfx950_setup_fused_block(op, batch, 4, 4, in, 16, out, 16);
    default: break;
  }
  CHECK(!"kind");
  return NA;
}

/* the NC setups with free pointers and strides */
static enum qnnp_status setup_nc(enum kind k, qnnp_operator_t op, const uint8_t* in, size_t in_stride, uint8_t* out, size_t out_stride)
{
  switch (k) {
    case SHUFFLE: return qnnp_setup_channel_shuffle_nc_x8(op, 3, in, in_stride, out, out_stride);
    case CLAMP: return qnnp_setup_clamp_nc_u8(op, 3, in, in_stride, out, out_stride);
    case LUT: return qnnp_gfx950_setup_lut_nc_x8(op, 3, in, in_stride, out, out_stride);
    case SIGMOID: return qnnp_setup_sigmoid_nc_q8(op, 3, in, in_stride, out, out_stride);
    case SOFTARGMAX: return qnnp_setup_softargmax_nc_q8(op, 3, in, in_stride, out, out_stride);
    default: break;
  }
  CHECK(!"kind");
  return NA;
}

static void create_columns(enum kind k)
{
  const struct row* r = &ROWS[k];
  qnnp_operator_t op = UNTOUCHED;
  EXPECT(create(k, INVALID, &op), r->invalid);
  CHECK(op == UNTOUCHED);                       /* the handle is written only on success */
  EXPECT(create(k, UNSUPPORTED, &op), r->unsupported);
  CHECK(op == UNTOUCHED);
  const size_t live = qnnp_stub_live_allocs();
  qnnp_stub_set_capturing(1);
  EXPECT(create(k, UNSUPPORTED, &op), r->unsupported_cap);
  CHECK(op == UNTOUCHED);
  EXPECT(create(k, GOOD, &op), INV);           /* no create works inside a capture */
  CHECK(op == UNTOUCHED);
  qnnp_stub_set_capturing(0);
  CHECK(qnnp_stub_live_allocs() == live);
}

static void setup_columns(enum kind k)
{
  const struct row* r = &ROWS[k];
  qnnp_operator_t op = NULL, other = NULL;
  size_t batch = 0;

  /* batch 0 on a fresh operator */
  CHECK(create(k, GOOD, &op) == OK && op != NULL && op != UNTOUCHED);
  EXPECT(qnnp_run_operator(op, NULL), INV);    /* never set up */
  EXPECT(setup(k, op, 0, NULL, NULL, NULL), r->batch0_setup);
  EXPECT(qnnp_run_operator(op, NULL), r->batch0_run);

  /* NULL and foreign handles */
  EXPECT(setup(k, NULL, 1, g_in, g_in2, g_out), INV);
  CHECK(create(r->foreign, GOOD, &other) == OK);
  EXPECT(setup(k, other, 1, g_in, g_in2, g_out), r->foreign_setup);
  CHECK(qnnp_delete_operator(other) == OK);

  /* a valid setup; then one inside a capture, refused: the first one still runs */
  EXPECT(setup(k, op, ++batch, g_in, g_in2, g_out), OK);
  EXPECT(qnnp_run_operator(op, NULL), OK);
  qnnp_stub_set_capturing(1);
  EXPECT(setup(k, op, batch + 1, g_in, g_in2, g_out), r->capture_setup);
  qnnp_stub_set_capturing(0);
  EXPECT(qnnp_run_operator(op, NULL), OK);

  /* the n-th allocation / upload of a setup with larger tensors fails */
  for (int n = 0; n < 3 && r->fail[n] != NA; n++) {
    qnnp_stub_fail_nth(n);
    EXPECT(setup(k, op, ++batch, g_in, g_in2, g_out), r->fail[n]);
    CHECK(!qnnp_stub_fail_pending());          /* the setup did reach its n-th allocation */
    qnnp_stub_fail_nth(-1);
    EXPECT(qnnp_run_operator(op, NULL), INV);
    EXPECT(setup(k, op, ++batch, g_in, g_in2, g_out), OK);
    EXPECT(qnnp_run_operator(op, NULL), OK);
  }
  CHECK(qnnp_delete_operator(op) == OK);
}

static void nc_overlap(const struct nc_row* r)
{
  qnnp_operator_t op = NULL;
  g_row = ROWS[r->kind].name;
  CHECK(create(r->kind, GOOD, &op) == OK);
  EXPECT(setup_nc(r->kind, op, g_in, 16, g_in, 16), r->in_place);
  if (r->in_place == OK) EXPECT(qnnp_run_operator(op, NULL), OK);
  EXPECT(setup_nc(r->kind, op, g_in, 16, g_in, 17), r->other_stride);
  EXPECT(setup_nc(r->kind, op, g_in, 16, g_in + 8, 16), r->partial);
  EXPECT(setup_nc(r->kind, op, g_in, 16, g_in + 1024, 16), r->disjoint);
  EXPECT(qnnp_run_operator(op, NULL), OK);
  CHECK(qnnp_delete_operator(op) == OK);
}

static void attach_columns(void)
{
  qnnp_operator_t conv = NULL, add = NULL;
  g_row = "attach residual add";
  CHECK(create(GEMM, GOOD, &conv) == OK);
  CHECK(qnnp_create_add_nc_q8(96, 127, 0.5f, 127, 0.5f, 127, 0.75f, 0, 255, 0, &add) == OK);
  CHECK(setup(GEMM, conv, 2, g_in, NULL, g_out) == OK);
  EXPECT(qnnp_gfx950_attach_residual_add(NULL, add, g_in2, 96), ATTACH.null_handle);
  EXPECT(qnnp_gfx950_attach_residual_add(conv, NULL, g_in2, 96), ATTACH.null_handle);
  EXPECT(qnnp_gfx950_attach_residual_add(add, add, g_in2, 96), ATTACH.foreign);
  EXPECT(qnnp_gfx950_attach_residual_add(conv, conv, g_in2, 96), ATTACH.foreign);
  EXPECT(qnnp_gfx950_attach_residual_add(conv, add, g_in2, (size_t) UINT32_MAX + 1), ATTACH.unsupported);
  EXPECT(qnnp_gfx950_attach_residual_add(conv, add, g_in2, 96), ATTACH.host_tensors);
  qnnp_stub_set_capturing(1);
  EXPECT(qnnp_gfx950_attach_residual_add(conv, add, g_in2, (size_t) UINT32_MAX + 1), ATTACH.unsupported_cap);
  EXPECT(qnnp_gfx950_attach_residual_add(conv, add, g_in2, 96), ATTACH.host_tensors_cap);
  qnnp_stub_set_capturing(0);
  EXPECT(qnnp_run_operator(conv, NULL), OK);   /* a refused attach leaves the convolution as it was */
  CHECK(qnnp_gfx950_operator_residual_folded(conv) == -1);
  CHECK(qnnp_delete_operator(conv) == OK);
  CHECK(qnnp_delete_operator(add) == OK);
}

int main(void)
{
  g_in = (uint8_t*) malloc(ARENA);
  g_in2 = (uint8_t*) malloc(ARENA);
  g_out = (uint8_t*) malloc(ARENA);
  CHECK(g_in != NULL && g_in2 != NULL && g_out != NULL);
  for (size_t i = 0; i < ARENA; i++) {
    g_in[i] = (uint8_t) (i * 37u + 11u);
    g_in2[i] = (uint8_t) (i * 101u + 3u);
  }
  memset(g_out, 0xA5, ARENA);
  for (size_t i = 0; i < sizeof(g_kernel); i++) g_kernel[i] = (uint8_t) (120u + i % 15u);
  for (size_t i = 0; i < 128; i++) g_bias[i] = (int32_t) i * 17 - 1000;
  for (size_t i = 0; i < 256; i++) g_table[i] = (uint8_t) (255u - i);

  /* before qnnp_initialize: every create, and every setup even of a NULL handle, answers uninitialized */
  for (int k = 0; k < KINDS; k++) {
    qnnp_operator_t op = UNTOUCHED;
    g_row = ROWS[k].name;
    EXPECT(create((enum kind) k, GOOD, &op), UN);
    CHECK(op == UNTOUCHED);
    EXPECT(setup((enum kind) k, NULL, 1, g_in, g_in2, g_out), UN);
  }
  g_row = "attach residual add";
  EXPECT(qnnp_gfx950_attach_residual_add(NULL, NULL, g_in2, 96), UN);

  CHECK(qnnp_initialize() == OK);
  g_row = "fused block members";
  CHECK(create(GEMM, GOOD, &g_expand) == OK);
  CHECK(create(DWCONV, GOOD, &g_depthwise) == OK);
  CHECK(create_conv(0, 1, 1, 96, 16, GOOD, &g_project) == OK);
  CHECK(qnnp_create_add_nc_q8(16, 127, 0.5f, 127, 0.5f, 127, 0.75f, 0, 255, 0, &g_block_add) == OK);
  for (int k = 0; k < KINDS; k++) {
    g_row = ROWS[k].name;
    create_columns((enum kind) k);
    setup_columns((enum kind) k);
  }
  for (size_t i = 0; i < sizeof(NC_ROWS) / sizeof(NC_ROWS[0]); i++) nc_overlap(&NC_ROWS[i]);
  attach_columns();

  g_row = "balance";
  CHECK(qnnp_delete_operator(g_expand) == OK);
  CHECK(qnnp_delete_operator(g_depthwise) == OK);
  CHECK(qnnp_delete_operator(g_project) == OK);
  CHECK(qnnp_delete_operator(g_block_add) == OK);
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == OK);
  free(g_in);
  free(g_in2);
  free(g_out);
  printf("host-sanitizers-lifecycle-ok\n");
  return 0;
}
