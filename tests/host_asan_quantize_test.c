/*
 * host_asan_quantize_test.c -- TEST INFRASTRUCTURE: the host code of the quantize and dequantize operators (quantize.c,
 * dequantize.c) under AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and
 * tests/hip_stub_quantize.c (Makefile target asan-quantize; run by tests/test_quantize_host.py). Walks every create and
 * setup status in the documented order, launches whose stubbed kernel checks the arguments it was handed and whose
 * results follow from the definition by hand (scales that are powers of two), the switch between the rows and the planar
 * setup on one handle, a refused setup that leaves the last one runnable, and a staging allocation that fails. Prints
 * "host-sanitizers-quantize-ok" on success.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>
#include <qnnpack_gfx950_float.h>

#include "hip/qnnp_hip.h"

/* tests/hip_stub.c and tests/hip_stub_quantize.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
size_t qnnp_stub_live_allocs(void);
extern struct qnnp_hip_quantize_args qnnp_stub_quantize_last;
extern struct qnnp_hip_dequantize_args qnnp_stub_dequantize_last;
extern unsigned qnnp_stub_quantize_launches;
extern unsigned qnnp_stub_dequantize_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define FILL 0xA5

static void* filled(size_t bytes)
{
  uint8_t* p = (uint8_t*) malloc(bytes ? bytes : 1);
  CHECK(p != NULL);
  memset(p, FILL, bytes);
  return p;
}

/* Scale 1/4, zero point 100, range [90, 250]: x = i / 8 - 3 walks -3 .. in steps of 1/8, so t = x * 4 = i / 2 - 12 hits
 * every integer and every tie. By hand: round half to even, clamp to [-10, 150], add 100. */
static float x_at(size_t i) { return (float) (i % 400) * 0.125f - 3.0f; }
static uint8_t y_by_hand(size_t i)
{
  const int twice = (int) (i % 400) - 24;                 /* 2 * t */
  int r = twice >= 0 ? twice / 2 : -((-twice) / 2);        /* toward zero */
  if (twice % 2 != 0 && r % 2 != 0) r += twice > 0 ? 1 : -1;   /* a tie: to the even neighbour */
  if (r < -10) r = -10;
  if (r > 150) r = 150;
  return (uint8_t) (r + 100);
}

static void quantize_walk(size_t c, size_t batch, size_t extra_in, size_t extra_out)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(c, 100, 0.25f, 90, 250, 0, &op) == qnnp_status_success);
  CHECK(op != NULL);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  const size_t si = c + extra_in, so = c + extra_out;
  /* exact spans: ASan catches any overrun */
  const size_t n_in = (batch - 1) * si + c, n_out = (batch - 1) * so + c;
  float* x = (float*) malloc(n_in * sizeof(float));
  CHECK(x != NULL);
  for (size_t i = 0; i < n_in; i++) x[i] = x_at(i);
  uint8_t* y = (uint8_t*) filled(n_out);
  const unsigned launches = qnnp_stub_quantize_launches;
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, si, y, so) == qnnp_status_success);
  CHECK(qnnp_gfx950_operator_set_streaming_stores(op, 1) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_quantize") == 0);
  CHECK(qnnp_stub_quantize_launches == launches + 1);
  CHECK(qnnp_stub_quantize_last.planar == 0 && qnnp_stub_quantize_last.rows == batch && qnnp_stub_quantize_last.channels == c);
  CHECK(qnnp_stub_quantize_last.input_stride == si && qnnp_stub_quantize_last.output_stride == so);
  CHECK(qnnp_stub_quantize_last.inv_scale == 4.0f && qnnp_stub_quantize_last.zero_point == 100);
  CHECK(qnnp_stub_quantize_last.clamp_lo == -10.0f && qnnp_stub_quantize_last.clamp_hi == 150.0f);
  CHECK(qnnp_stub_quantize_last.streaming_mode == 2);
  CHECK((const void*) qnnp_stub_quantize_last.input != (const void*) x && qnnp_stub_quantize_last.output != y);   /* staged */
  for (size_t r = 0; r < batch; r++) {
    for (size_t k = 0; k < c; k++) CHECK(y[r * so + k] == y_by_hand(r * si + k));
    if (r + 1 < batch) for (size_t k = c; k < so; k++) CHECK(y[r * so + k] == FILL);
  }
  CHECK(qnnp_gfx950_operator_set_streaming_stores(op, -1) == qnnp_status_success);

  /* refused setups come before the operator changes: the previous setup stays runnable */
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, NULL, si, y, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, si, NULL, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, (const float*) ((const char*) x + 2), si, y, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, c - 1, y, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, si, y, c - 1) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, (size_t) INT32_MAX + 1, x, si, y, so) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, si, (uint8_t*) x, so) == qnnp_status_invalid_parameter);   /* no in-place form */
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, si, (uint8_t*) x + n_in * 4 - 1, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, 1, 0, x, y, c) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, 1, 1, x, y, c - 1) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, 1, 1, NULL, y, c) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, (size_t) 1 << 31, 1, x, y, c) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, 65536, 32768, x, y, c) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, 1, ((size_t) 1 << 31) / c + 1, x, y, c) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, SIZE_MAX, SIZE_MAX, x, y, c) == qnnp_status_unsupported_parameter);
  memset(y, FILL, n_out);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  for (size_t r = 0; r < batch; r++) for (size_t k = 0; k < c; k++) CHECK(y[r * so + k] == y_by_hand(r * si + k));

  /* the same handle, planar: x is [batch][c][pixels], y is [batch * pixels][c + extra_out] */
  {
    const size_t pixels = 5, stride = c + extra_out;
    float* px = (float*) malloc(batch * c * pixels * sizeof(float));
    CHECK(px != NULL);
    for (size_t i = 0; i < batch * c * pixels; i++) px[i] = x_at(i * 7);
    uint8_t* py = (uint8_t*) filled((batch * pixels - 1) * stride + c);
    CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, batch, pixels, px, py, stride) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_quantize_last.planar == 1 && qnnp_stub_quantize_last.pixels == pixels && qnnp_stub_quantize_last.rows == batch);
    CHECK(qnnp_stub_quantize_last.output_stride == stride);
    for (size_t n = 0; n < batch; n++) {
      for (size_t p = 0; p < pixels; p++) {
        for (size_t k = 0; k < c; k++) CHECK(py[(n * pixels + p) * stride + k] == y_by_hand(((n * c + k) * pixels + p) * 7));
        if (n * pixels + p + 1 < batch * pixels) for (size_t k = c; k < stride; k++) CHECK(py[(n * pixels + p) * stride + k] == FILL);
      }
    }
    /* and back to rows */
    memset(y, FILL, n_out);
    CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, si, y, so) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_quantize_last.planar == 0);
    for (size_t r = 0; r < batch; r++) for (size_t k = 0; k < c; k++) CHECK(y[r * so + k] == y_by_hand(r * si + k));
    free(px);
    free(py);
  }
  /* no rows: a successful no-op, whatever the pointers */
  {
    const unsigned before = qnnp_stub_quantize_launches;
    CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(op, 0, 0, NULL, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_quantize_launches == before);
  }
  /* a staging allocation that fails: out_of_memory, and the operator is not runnable until the next good setup */
  {
    /* 8 x the rows: beyond what the planar setup above had staged (5 pixels per row) */
    float* big = (float*) malloc(((8 * batch - 1) * si + c) * sizeof(float));
    CHECK(big != NULL);
    for (size_t i = 0; i < (8 * batch - 1) * si + c; i++) big[i] = x_at(i);
    uint8_t* out = (uint8_t*) filled((8 * batch - 1) * so + c);
    qnnp_stub_fail_nth(0);
    CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, 8 * batch, big, si, out, so) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
    free(big);
    free(out);
    CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(op, batch, x, si, y, so) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  free(x);
  free(y);
}

/* scale 1/8, zero point 37: y = (x - 37) / 8 exactly */
static void dequantize_walk(size_t c, size_t batch, size_t extra_in, size_t extra_out)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(c, 37, 0.125f, 0, &op) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
  const size_t si = c + extra_in, so = c + extra_out;
  const size_t n_in = (batch - 1) * si + c, n_out = (batch - 1) * so + c;
  uint8_t* x = (uint8_t*) malloc(n_in);
  CHECK(x != NULL);
  for (size_t i = 0; i < n_in; i++) x[i] = (uint8_t) (i * 37u + 11u);
  float* y = (float*) filled(n_out * sizeof(float));
  float fill;
  memset(&fill, FILL, sizeof(fill));
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, batch, x, si, y, so) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_dequantize") == 0);
  CHECK(qnnp_stub_dequantize_last.planar == 0 && qnnp_stub_dequantize_last.rows == batch && qnnp_stub_dequantize_last.channels == c);
  CHECK(qnnp_stub_dequantize_last.input_stride == si && qnnp_stub_dequantize_last.output_stride == so);
  CHECK(qnnp_stub_dequantize_last.scale == 0.125f && qnnp_stub_dequantize_last.zero_point == 37);
  CHECK(qnnp_stub_dequantize_last.input != x && qnnp_stub_dequantize_last.output != y);
  for (size_t r = 0; r < batch; r++) {
    for (size_t k = 0; k < c; k++) CHECK(y[r * so + k] == (float) ((int) x[r * si + k] - 37) / 8.0f);
    if (r + 1 < batch) for (size_t k = c; k < so; k++) CHECK(memcmp(&y[r * so + k], &fill, sizeof(fill)) == 0);
  }
  /* refused setups, then the previous one still runs */
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, batch, NULL, si, y, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, batch, x, si, NULL, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, batch, x, si, (float*) ((char*) y + 1), so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, batch, x, c - 1, y, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, batch, x, si, y, c - 1) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, (size_t) INT32_MAX + 1, x, si, y, so) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, batch, (const uint8_t*) y, si, y, so) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(op, 1, 0, x, c, y) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(op, 1, 1, x, c - 1, y) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(op, (size_t) 1 << 31, 1, x, c, y) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(op, 65536, 32768, x, c, y) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(op, 1, ((size_t) 1 << 31) / c + 1, x, c, y) == qnnp_status_unsupported_parameter);
  memset(y, FILL, n_out * sizeof(float));
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  for (size_t r = 0; r < batch; r++) for (size_t k = 0; k < c; k++) CHECK(y[r * so + k] == (float) ((int) x[r * si + k] - 37) / 8.0f);
  /* planar on the same handle: x is [batch * pixels][c + extra_in], y is [batch][c][pixels] */
  {
    const size_t pixels = 6, stride = c + extra_in;
    const size_t bytes = (batch * pixels - 1) * stride + c;
    uint8_t* px = (uint8_t*) malloc(bytes);
    CHECK(px != NULL);
    for (size_t i = 0; i < bytes; i++) px[i] = (uint8_t) (i * 29u + 3u);
    float* py = (float*) filled(batch * c * pixels * sizeof(float));
    CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(op, batch, pixels, px, stride, py) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_dequantize_last.planar == 1 && qnnp_stub_dequantize_last.pixels == pixels && qnnp_stub_dequantize_last.input_stride == stride);
    for (size_t n = 0; n < batch; n++) for (size_t k = 0; k < c; k++) for (size_t p = 0; p < pixels; p++) {
      CHECK(py[(n * c + k) * pixels + p] == (float) ((int) px[(n * pixels + p) * stride + k] - 37) / 8.0f);
    }
    free(px);
    free(py);
  }
  {
    const unsigned before = qnnp_stub_dequantize_launches;
    CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(op, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_dequantize_launches == before);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  free(x);
  free(y);
}

static void statuses(void)
{
  qnnp_operator_t op = NULL;
  /* quantize, in the documented order: channels, scale, range, then the two unsupported classes */
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(0, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 0.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, -1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 1.0e-40f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);   /* subnormal */
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, INFINITY, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, NAN, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 1.0f, 100, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 1.0f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  /* invalid before unsupported */
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8((size_t) INT32_MAX + 1, 0, 1.0f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 0x1.0p-120f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8((size_t) INT32_MAX + 1, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 0x1.fffffep-119f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 0x1.000002p+118f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(op == NULL);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8((size_t) INT32_MAX, 255, 0x1.0p-118f, 0, 1, 7, &op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(1, 0, 0x1.0p+118f, 254, 255, 0xFFFFFFFFu, &op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;
  /* dequantize */
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(0, 0, 0.0f, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, 0.0f, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, -2.0f, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, 1.0e-40f, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, INFINITY, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, NAN, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32((size_t) INT32_MAX + 1, 0, NAN, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32((size_t) INT32_MAX + 1, 0, 1.0f, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, 0x1.fffffep-119f, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, 0x1.000002p+118f, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(op == NULL);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32((size_t) INT32_MAX, 255, 0x1.0p+118f, 9, &op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;

  /* operator kinds, and graph capture */
  float x[64] = {0};
  uint8_t* y = (uint8_t*) filled(64);
  qnnp_operator_t quant = NULL, dequant = NULL, add = NULL;
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 1.0f, 0, 255, 0, &quant) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, 1.0f, 0, &dequant) == qnnp_status_success);
  CHECK(qnnp_create_add_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &add) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(NULL, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(dequant, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(add, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(dequant, 1, 1, x, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(quant, 1, y, 8, x, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(quant, 1, 1, y, 8, x) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(NULL, 1, y, 8, x, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_add_nc_q8(quant, 1, y, 8, y + 16, 8, y + 32, 8) == qnnp_status_invalid_parameter);
  {
    qnnp_operator_t none = NULL;
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(8, 0, 1.0f, 0, 255, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(8, 0, 1.0f, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(none == NULL);
    CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(quant, 2, x, 8, y, 8) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(quant, 1, 2, x, y, 8) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(dequant, 2, y, 8, x, 8) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(dequant, 1, 2, y, 8, x) == qnnp_status_invalid_parameter);
    CHECK(qnnp_stub_live_allocs() == live);
    qnnp_stub_set_capturing(0);
  }
  CHECK(qnnp_delete_operator(quant) == qnnp_status_success);
  CHECK(qnnp_delete_operator(dequant) == qnnp_status_success);
  CHECK(qnnp_delete_operator(add) == qnnp_status_success);
  free(y);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized, whatever the arguments */
  CHECK(qnnp_gfx950_create_quantize_nc_f32_q8(0, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_create_dequantize_nc_q8_f32(0, 0, 0.0f, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_quantize_nc_f32_q8(NULL, 1, NULL, 1, NULL, 1) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8(NULL, 1, 1, NULL, NULL, 1) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_dequantize_nc_q8_f32(NULL, 1, NULL, 1, NULL, 1) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32(NULL, 1, 1, NULL, 1, NULL) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  statuses();
  {
    /* channels, batch, extra stride of the input, of the output */
    const size_t shapes[5][4] = {{1, 1, 0, 0}, {17, 3, 3, 9}, {64, 2, 0, 0}, {5, 4, 11, 0}, {33, 5, 0, 7}};
    for (int k = 0; k < 5; k++) {
      quantize_walk(shapes[k][0], shapes[k][1], shapes[k][2], shapes[k][3]);
      dequantize_walk(shapes[k][0], shapes[k][1], shapes[k][2], shapes[k][3]);
    }
  }
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-quantize-ok\n");
  return 0;
}
