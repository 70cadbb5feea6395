/*
 * host_asan_table_test.c -- TEST INFRASTRUCTURE: the host code of the output table (output-table.c, the hand-over in
 * convolution.c, the refusals in residual.c, fused-block.c and squeeze-excite.c, the free in operator-delete.c) under
 * AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c, tests/hip_stub_table.c, tests/hip_stub_mul.c and
 * tests/hip_stub_se.c (Makefile target asan-table; run by tests/test_output_table_host.py).
 *
 * It walks every status of qnnp_gfx950_attach_output_table in the header's order, the attach / replace / detach / delete
 * lifecycles with the count of live device allocations (a leaked or doubly freed device table shows there and in ASan's
 * report), a failed allocation and a failed upload (the previous table stays in force), the three combination refusals,
 * and the in-place launch behind a convolution, a depthwise convolution and a fully connected layer: the stub's
 * convolution launches write nothing, so an output tensor prefilled with known bytes must come back as table[byte] in
 * every pixel and unchanged between strided pixels. Prints "host-sanitizers-table-ok" on success.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>
#include <qnnpack_gfx950_perchannel.h>

#include "hip/qnnp_hip.h"
#include "operator.h"

/* tests/hip_stub.c and tests/hip_stub_table.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
size_t qnnp_stub_live_allocs(void);
void qnnp_stub_set_device_pointers(int on);
extern struct qnnp_hip_lut_args qnnp_stub_lut_last;
extern unsigned qnnp_stub_lut_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define OK(call) CHECK((call) == qnnp_status_success)
#define FILL 0xA5

static uint8_t g_k[64 * 64];
static int32_t g_b[64];
static uint8_t g_table[256], g_table2[256];

static qnnp_operator_t conv1x1(size_t cin, size_t cout)
{
  qnnp_operator_t op = NULL;
  OK(qnnp_create_convolution2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, cin, cout, 4, 1.0f, 2, 1.0f, g_k, g_b, 5, 2.0f, 0, 255, 0, &op));
  return op;
}

static qnnp_operator_t depthwise3x3(uint32_t channels)
{
  qnnp_operator_t op = NULL;
  OK(qnnp_create_convolution2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, channels, 1, 1, 4, 1.0f, 2, 1.0f, g_k, g_b, 5, 2.0f, 0, 255, 0, &op));
  return op;
}

static qnnp_operator_t lut(size_t channels, const uint8_t* table)
{
  qnnp_operator_t op = NULL;
  OK(qnnp_gfx950_create_lut_nc_x8(channels, table, 0, &op));
  return op;
}

/* the 256 bytes of the operator's own device table (the stub's device memory is host memory) */
static int table_is(qnnp_operator_t op, const uint8_t* table)
{
  return op->d_output_table != NULL && memcmp(op->d_output_table, table, 256) == 0;
}

/* set up on a "device" output of `pixels` pixels of `stride` bytes prefilled with a ramp, run, and hold the result to
 * table[ramp] in the pixels and FILL between them (table == NULL: the ramp itself, nothing attached) */
static void run_and_check(qnnp_operator_t op, int kind, size_t batch, size_t h, size_t w, size_t cin, size_t cout, size_t stride,
                          const uint8_t* table)
{
  const size_t pixels = batch * h * w;
  uint8_t* in = (uint8_t*) qnnp_hip_alloc(pixels * cin);
  uint8_t* out = (uint8_t*) qnnp_hip_alloc((pixels - 1) * stride + cout);
  CHECK(in != NULL && out != NULL);
  memset(in, 7, pixels * cin);
  memset(out, FILL, (pixels - 1) * stride + cout);
  for (size_t p = 0; p < pixels; p++) {
    for (size_t c = 0; c < cout; c++) out[p * stride + c] = (uint8_t) (p * 31 + c * 7 + 3);
  }
  if (kind == 2) {
    OK(qnnp_setup_fully_connected_nc_q8(op, pixels, in, cin, out, stride));
  } else {
    OK(qnnp_setup_convolution2d_nhwc_q8(op, batch, h, w, in, cin, out, stride, NULL));
  }
  const unsigned launches = qnnp_stub_lut_launches;
  OK(qnnp_run_operator(op, NULL));
  if (table == NULL) {
    CHECK(qnnp_stub_lut_launches == launches);
    CHECK(qnnp_gfx950_operator_table_folded(op) == -1);
  } else {
    /* one launch, in place on the output, through the operator's own copy of the table */
    CHECK(qnnp_stub_lut_launches == launches + 1);
    CHECK(qnnp_stub_lut_last.input == out && qnnp_stub_lut_last.output == out);
    CHECK(qnnp_stub_lut_last.table == (const uint8_t*) op->d_output_table);
    CHECK(qnnp_stub_lut_last.pixels == pixels && qnnp_stub_lut_last.channels == cout);
    CHECK(qnnp_stub_lut_last.input_stride == stride && qnnp_stub_lut_last.output_stride == stride);
    CHECK(qnnp_gfx950_operator_table_folded(op) == 0);
  }
  CHECK(strncmp(qnnp_gfx950_operator_kernel(op), "stub_", 5) == 0 && strcmp(qnnp_gfx950_operator_kernel(op), "stub_lut") != 0);
  for (size_t p = 0; p < pixels; p++) {
    for (size_t c = 0; c < (p + 1 < pixels ? stride : cout); c++) {
      const uint8_t ramp = (uint8_t) (p * 31 + c * 7 + 3);
      const uint8_t want = c >= cout ? FILL : (table != NULL ? table[ramp] : ramp);
      if (out[p * stride + c] != want) {
        fprintf(stderr, "pixel %zu byte %zu: got %u, want %u\n", p, c, out[p * stride + c], want);
        exit(1);
      }
    }
  }
  qnnp_hip_free(in);
  qnnp_hip_free(out);
}

static void statuses(void)
{
  qnnp_operator_t conv = conv1x1(32, 16), conv2 = conv1x1(32, 16), dw = depthwise3x3(16), project = conv1x1(16, 16);
  qnnp_operator_t t16 = lut(16, g_table), t8 = lut(8, g_table), add = NULL, deconv = NULL, fused = NULL, pc = NULL;
  OK(qnnp_create_add_nc_q8(16, 1, 1.0f, 5, 1.0f, 6, 2.0f, 0, 255, 0, &add));
  OK(qnnp_create_deconvolution2d_nhwc_q8(0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 1, 1, 32, 16, 4, 1.0f, 2, 1.0f, g_k, g_b, 5, 2.0f, 0, 255, 0, &deconv));
  /* 2. a NULL convolution, whatever the table */
  CHECK(qnnp_gfx950_attach_output_table(NULL, t16) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_output_table(NULL, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_operator_table_folded(NULL) == -1);
  /* 3. the wrong kind on either side, a channel mismatch, a capture */
  CHECK(qnnp_gfx950_attach_output_table(t16, t16) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_output_table(add, t16) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_output_table(deconv, t16) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_output_table(deconv, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_output_table(conv, add) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_output_table(conv, conv2) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_attach_output_table(conv, t8) == qnnp_status_invalid_parameter);
  {
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_attach_output_table(conv, t16) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_attach_output_table(conv, NULL) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_attach_output_table(conv, t8) == qnnp_status_invalid_parameter);
    qnnp_stub_set_capturing(0);
    CHECK(qnnp_stub_live_allocs() == live && qnnp_gfx950_operator_table_folded(conv) == -1);
  }
  /* 4. a residual add on the convolution: unsupported -- behind every invalid_parameter, in front of out_of_memory */
  {
    qnnp_stub_set_device_pointers(1);
    uint8_t* in = (uint8_t*) qnnp_hip_alloc(64 * 32);
    uint8_t* out = (uint8_t*) qnnp_hip_alloc(64 * 16);
    uint8_t* res = (uint8_t*) qnnp_hip_alloc(64 * 16);
    CHECK(in != NULL && out != NULL && res != NULL);
    memset(in, 1, 64 * 32); memset(out, 2, 64 * 16); memset(res, 3, 64 * 16);
    OK(qnnp_setup_convolution2d_nhwc_q8(conv2, 1, 8, 8, in, 32, out, 16, NULL));
    OK(qnnp_gfx950_attach_residual_add(conv2, add, res, 16));
    CHECK(qnnp_gfx950_attach_output_table(conv2, t8) == qnnp_status_invalid_parameter);
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_attach_output_table(conv2, t16) == qnnp_status_invalid_parameter);
    qnnp_stub_set_capturing(0);
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_fail_nth(0);
    CHECK(qnnp_gfx950_attach_output_table(conv2, t16) == qnnp_status_unsupported_parameter);
    qnnp_stub_fail_nth(-1);
    CHECK(qnnp_stub_live_allocs() == live && qnnp_gfx950_operator_table_folded(conv2) == -1);
    CHECK(qnnp_gfx950_operator_residual_folded(conv2) == 0);
    OK(qnnp_gfx950_attach_output_table(conv2, NULL));                /* nothing attached, nothing to refuse */
    /* ... and the other order: a table on the convolution refuses the residual add, and stays */
    OK(qnnp_setup_convolution2d_nhwc_q8(conv, 1, 8, 8, in, 32, out, 16, NULL));
    OK(qnnp_gfx950_attach_output_table(conv, t16));
    CHECK(qnnp_gfx950_attach_residual_add(conv, add, res, 16) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_gfx950_attach_residual_add(conv, t16, res, 16) == qnnp_status_invalid_parameter);     /* invalid first */
    CHECK(qnnp_gfx950_operator_residual_folded(conv) == -1 && table_is(conv, g_table));
    OK(qnnp_gfx950_attach_output_table(conv, NULL));
    OK(qnnp_gfx950_attach_residual_add(conv, add, res, 16));         /* without the table the add is taken */
    /* (the next setup detaches a residual add: both convolutions go on without one) */
    OK(qnnp_setup_convolution2d_nhwc_q8(conv, 1, 8, 8, in, 32, out, 16, NULL));
    OK(qnnp_setup_convolution2d_nhwc_q8(conv2, 1, 8, 8, in, 32, out, 16, NULL));
    CHECK(qnnp_gfx950_operator_residual_folded(conv) == -1 && qnnp_gfx950_operator_residual_folded(conv2) == -1);
    qnnp_hip_free(in); qnnp_hip_free(out); qnnp_hip_free(res);
    qnnp_stub_set_device_pointers(0);
  }
  /* 5. out_of_memory: the allocation, then the upload; the previous table stays in force and nothing leaks */
  {
    OK(qnnp_gfx950_attach_output_table(dw, t16));
    const size_t live = qnnp_stub_live_allocs();
    const void* before = dw->d_output_table;
    qnnp_operator_t other = lut(16, g_table2);
    for (long nth = 0; nth < 2; nth++) {
      qnnp_stub_fail_nth(nth);
      CHECK(qnnp_gfx950_attach_output_table(dw, other) == qnnp_status_out_of_memory);
      qnnp_stub_fail_nth(-1);
      CHECK(dw->d_output_table == before && table_is(dw, g_table) && qnnp_stub_live_allocs() == live + 1);
    }
    OK(qnnp_gfx950_attach_output_table(dw, other));
    CHECK(table_is(dw, g_table2) && qnnp_stub_live_allocs() == live + 1);      /* replaced: the old table freed */
    OK(qnnp_delete_operator(other));
    CHECK(table_is(dw, g_table2));                                             /* a copy: the table operator may go */
    OK(qnnp_gfx950_attach_output_table(dw, NULL));
    CHECK(dw->d_output_table == NULL && qnnp_stub_live_allocs() == live - 1);
  }
  /* the fused operators borrow their members' parameters: a member with a table is refused, each member in turn */
  {
    qnnp_operator_t members[3] = {conv, dw, project};
    OK(qnnp_gfx950_attach_output_table(conv, NULL));
    for (int m = 0; m < 3; m++) {
      OK(qnnp_gfx950_attach_output_table(members[m], t16));
      CHECK(qnnp_gfx950_create_fused_block(conv, dw, project, NULL, &fused) == qnnp_status_unsupported_parameter);
      CHECK(qnnp_gfx950_create_fused_block(NULL, dw, project, NULL, &fused) ==
            (m == 0 ? qnnp_status_success : qnnp_status_unsupported_parameter));
      if (m == 0) { OK(qnnp_delete_operator(fused)); fused = NULL; }
      CHECK(fused == NULL);
      OK(qnnp_gfx950_attach_output_table(members[m], NULL));
    }
    OK(qnnp_gfx950_create_fused_block(conv, dw, project, NULL, &fused));
    OK(qnnp_delete_operator(fused));
  }
  {
    qnnp_operator_t pool = NULL, fc1 = NULL, fc2 = NULL, mul = NULL, se = NULL;
    OK(qnnp_create_global_average_pooling_nwc_q8(16, 4, 1.0f, 5, 1.0f, 0, 255, 0, &pool));
    OK(qnnp_create_fully_connected_nc_q8(16, 8, 4, 1.0f, 2, 1.0f, g_k, g_b, 5, 2.0f, 0, 255, 0, &fc1));
    OK(qnnp_create_fully_connected_nc_q8(8, 16, 4, 1.0f, 2, 1.0f, g_k, g_b, 5, 2.0f, 0, 255, 0, &fc2));
    OK(qnnp_gfx950_create_multiply_nc_q8(16, 4, 1.0f, 0, 0x1.0p-8f, 5, 1.0f, 0, 255, 0, &mul));
    OK(qnnp_gfx950_attach_output_table(fc1, t8));
    CHECK(qnnp_gfx950_create_squeeze_excite(pool, fc1, fc2, t16, mul, &se) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_gfx950_create_squeeze_excite(pool, fc1, fc2, t8, mul, &se) == qnnp_status_invalid_parameter);   /* invalid first */
    OK(qnnp_gfx950_attach_output_table(fc1, NULL));
    OK(qnnp_gfx950_attach_output_table(fc2, t16));
    CHECK(qnnp_gfx950_create_squeeze_excite(pool, fc1, fc2, t16, mul, &se) == qnnp_status_unsupported_parameter);
    CHECK(se == NULL);
    OK(qnnp_gfx950_attach_output_table(fc2, NULL));
    OK(qnnp_gfx950_create_squeeze_excite(pool, fc1, fc2, t16, mul, &se));
    OK(qnnp_delete_operator(se));
    OK(qnnp_delete_operator(pool)); OK(qnnp_delete_operator(fc1)); OK(qnnp_delete_operator(fc2)); OK(qnnp_delete_operator(mul));
  }
  /* a per-channel convolution takes a table like any other */
  {
    float scales[16];
    for (int i = 0; i < 16; i++) scales[i] = 0.5f + 0.01f * (float) i;
    OK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 32, 16, 4, 1.0f, 2, scales, g_k, g_b, 5, 2.0f, 0, 255, 0, &pc));
    OK(qnnp_gfx950_attach_output_table(pc, t16));
    CHECK(table_is(pc, g_table));
  }
  /* delete frees the device table */
  {
    const size_t live = qnnp_stub_live_allocs();
    OK(qnnp_gfx950_attach_output_table(project, t16));
    CHECK(qnnp_stub_live_allocs() == live + 1);
    OK(qnnp_delete_operator(project));
    OK(qnnp_delete_operator(pc));
  }
  OK(qnnp_delete_operator(conv)); OK(qnnp_delete_operator(conv2)); OK(qnnp_delete_operator(dw));
  OK(qnnp_delete_operator(t16)); OK(qnnp_delete_operator(t8)); OK(qnnp_delete_operator(add)); OK(qnnp_delete_operator(deconv));
  CHECK(qnnp_stub_live_allocs() == 0);
}

/* attach before setup, run, set up again, replace, detach -- behind each of the three operator kinds */
static void lifecycles(void)
{
  qnnp_stub_set_device_pointers(1);
  for (int kind = 0; kind < 3; kind++) {
    const size_t cin = kind == 1 ? 16 : 32, cout = 16;
    qnnp_operator_t op = NULL;
    if (kind == 0) op = conv1x1(cin, cout);
    if (kind == 1) op = depthwise3x3(16);
    if (kind == 2) OK(qnnp_create_fully_connected_nc_q8(cin, cout, 4, 1.0f, 2, 1.0f, g_k, g_b, 5, 2.0f, 0, 255, 0, &op));
    qnnp_operator_t t = lut(cout, g_table), t2 = lut(cout, g_table2), hs = NULL;
    OK(qnnp_gfx950_create_hardswish_nc_q8(cout, 5, 0.05f, 20, 0.04f, 0, 255, 0, &hs));
    run_and_check(op, kind, 2, 3, 5, cin, cout, cout, NULL);
    OK(qnnp_gfx950_attach_output_table(op, t));          /* (a valid setup exists; the first kind also attaches before any) */
    OK(qnnp_delete_operator(t));
    run_and_check(op, kind, 2, 3, 5, cin, cout, cout, g_table);
    run_and_check(op, kind, 1, 5, 7, cin, cout, cout + 5, g_table);     /* another shape, strided pixels: still attached */
    OK(qnnp_gfx950_attach_output_table(op, t2));
    run_and_check(op, kind, 1, 5, 7, cin, cout, cout + 5, g_table2);
    OK(qnnp_gfx950_attach_output_table(op, hs));         /* any table operator: hardswish's table, as that operator holds it */
    CHECK(table_is(op, (const uint8_t*) hs->d_weights));
    OK(qnnp_gfx950_attach_output_table(op, NULL));
    run_and_check(op, kind, 2, 3, 5, cin, cout, cout, NULL);
    /* batch 0 with a table attached: nothing runs */
    OK(qnnp_gfx950_attach_output_table(op, t2));
    {
      const unsigned launches = qnnp_stub_lut_launches;
      uint8_t* buf = (uint8_t*) qnnp_hip_alloc(64);
      CHECK(buf != NULL);
      if (kind == 2) OK(qnnp_setup_fully_connected_nc_q8(op, 0, buf, cin, buf, cout));
      else OK(qnnp_setup_convolution2d_nhwc_q8(op, 0, 3, 5, buf, cin, buf, cout, NULL));
      OK(qnnp_run_operator(op, NULL));
      CHECK(qnnp_stub_lut_launches == launches);
      qnnp_hip_free(buf);
    }
    OK(qnnp_delete_operator(op));                        /* with the table attached */
    OK(qnnp_delete_operator(t2));
    OK(qnnp_delete_operator(hs));
    CHECK(qnnp_stub_live_allocs() == 0);
  }
  /* host endpoints: the table walks the staged device output, and the caller's tensor gets the looked-up bytes */
  qnnp_stub_set_device_pointers(0);
  {
    qnnp_operator_t op = conv1x1(32, 16), t = lut(16, g_table);
    OK(qnnp_gfx950_attach_output_table(op, t));          /* before the first setup */
    uint8_t in[15 * 32], out[14 * 21 + 16];
    memset(in, 9, sizeof(in));
    memset(out, FILL, sizeof(out));
    OK(qnnp_setup_convolution2d_nhwc_q8(op, 1, 3, 5, in, 32, out, 21, NULL));
    const unsigned launches = qnnp_stub_lut_launches;
    OK(qnnp_run_operator(op, NULL));
    CHECK(qnnp_stub_lut_launches == launches + 1);
    CHECK(qnnp_stub_lut_last.output == (uint8_t*) op->d_stage_out && qnnp_stub_lut_last.input == qnnp_stub_lut_last.output);
    CHECK(qnnp_stub_lut_last.pixels == 15 && qnnp_stub_lut_last.channels == 16 && qnnp_stub_lut_last.output_stride == 21);
    OK(qnnp_delete_operator(op));
    OK(qnnp_delete_operator(t));
  }
  CHECK(qnnp_stub_live_allocs() == 0);
}

int main(void)
{
  for (size_t i = 0; i < sizeof(g_k); i++) g_k[i] = (uint8_t) (120 + i % 13);
  for (int i = 0; i < 256; i++) {
    g_table[i] = (uint8_t) (255 - ((i * 7 + 3) & 0xFF));
    g_table2[i] = (uint8_t) ((i * 13 + 101) & 0xFF);
  }
  /* 1. before qnnp_initialize: uninitialized, whatever the arguments */
  CHECK(qnnp_gfx950_attach_output_table(NULL, NULL) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_operator_table_folded(NULL) == -1);
  OK(qnnp_initialize());
  statuses();
  lifecycles();
  CHECK(qnnp_stub_live_allocs() == 0);
  OK(qnnp_deinitialize());
  CHECK(qnnp_gfx950_attach_output_table(NULL, NULL) == qnnp_status_uninitialized);
  printf("host-sanitizers-table-ok\n");
  return 0;
}
