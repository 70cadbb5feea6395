/*
 * host_asan_se_test.c -- TEST INFRASTRUCTURE: the host code of the fused squeeze-and-excite operator (squeeze-excite.c over
 * global-average-pooling.c, fully-connected.c, lut.c and multiply.c) under AddressSanitizer + UndefinedBehaviorSanitizer,
 * against tests/hip_stub.c, tests/hip_stub_lut.c, tests/hip_stub_mul.c and tests/hip_stub_se.c (Makefile target asan-se; run
 * by tests/test_squeeze_excite_host.py).
 *
 * It builds the five members from RAW weight and bias arrays, creates, sets up and runs the fused operator over the stubs,
 * and compares the gate rows s and the output y with values computed here directly from the raw arrays by the
 * definitions -- sum (a - izp)(w - kzp) + bias, the scalar Q31 requantization with the parameters of requantization.h, the
 * pooling quantizer -- while the stub computes them from the PACKED device images as the kernel addresses them. Then it
 * walks every create and setup status in the header's order, a refused setup that leaves the previous one runnable,
 * scratch growth, and delete freeing the scratch (ASan reports leaks). Prints "host-sanitizers-se-ok" on success.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>
#include <qnnpack_gfx950_perchannel.h>
#include <qnnpack_gfx950_test.h>

#include "hip/qnnp_hip.h"
#include "requantization.h"

/* tests/hip_stub.c, tests/hip_stub_mul.c and tests/hip_stub_se.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
size_t qnnp_stub_live_allocs(void);
extern struct qnnp_hip_mul_args qnnp_stub_mul_last;
extern unsigned qnnp_stub_mul_launches;
extern struct qnnp_hip_se_gate_args qnnp_stub_se_last;
extern unsigned qnnp_stub_se_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define FILL 0xA5

static uint32_t g_rng = 12345u;
static uint32_t next_u32(void) { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static uint8_t* random_bytes(size_t n)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t) next_u32();
  return p;
}

static uint8_t* constant_bytes(size_t n, int value)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  memset(p, value, n);
  return p;
}

/* the scalar definition (reference src/qnnpack/requantization.h:464-480) over the parameters of requantization.h */
static uint8_t q31_requantize(int32_t n, const struct qnnp_hip_requant* rq)
{
  const int64_t product = (int64_t) n * (int64_t) rq->multiplier;
  const int32_t q = (int32_t) (uint32_t) ((uint64_t) (product + INT64_C(0x40000000)) >> 31);
  const int32_t remainder = (q & rq->remainder_mask) - (int32_t) (n < 0);
  const int32_t shifted = q >= 0 ? (int32_t) ((uint32_t) q >> rq->shift) : -(int32_t) (((uint32_t) -(q + 1)) >> rq->shift) - 1;
  int32_t y = shifted + (int32_t) (remainder > rq->remainder_threshold);
  if (y < rq->output_min_less_zero_point) y = rq->output_min_less_zero_point;
  if (y > rq->output_max_less_zero_point) y = rq->output_max_less_zero_point;
  return (uint8_t) (y + rq->output_zero_point);
}

/* reference src/qnnpack/requantization.h:482-498 */
static uint8_t avgpool_quantize(int32_t n, const struct qnnp_hip_avgpool_params* q)
{
  const int64_t rounded = (int64_t) n * (int64_t) q->multiplier - (int64_t) (n < 0) + q->rounding;
  int64_t y = rounded >= 0 ? (int64_t) ((uint64_t) rounded >> q->right_shift) : -(int64_t) (((uint64_t) -(rounded + 1)) >> q->right_shift) - 1;
  if (y < q->output_min_less_zero_point) y = q->output_min_less_zero_point;
  if (y > q->output_max_less_zero_point) y = q->output_max_less_zero_point;
  return (uint8_t) (y + q->output_zero_point);
}

/* one block: its quantization, its raw arrays and the five members made from them */
struct block {
  size_t c, s;
  uint8_t x_zp, pool_zp, h_zp, e_zp, y_zp, kzp1, kzp2;
  float x_scale, pool_scale, fc1_scale, fc2_scale, y_scale;
  uint8_t* k1;      /* [s][c] */
  int32_t* b1;
  uint8_t* k2;      /* [c][s] */
  int32_t* b2;
  uint8_t table[256];
  qnnp_operator_t pool, fc1, fc2, gate, mul;
};

/* weights 0 .. 255 (or all `constant` when it is >= 0), small biases */
static void make_block(struct block* b, size_t c, size_t s, uint8_t kzp1, uint8_t kzp2, int constant)
{
  memset(b, 0, sizeof(*b));
  b->c = c;
  b->s = s;
  b->x_zp = 121; b->x_scale = 0.05f;
  b->pool_zp = 119; b->pool_scale = 0.04f;
  b->h_zp = 30; b->e_zp = 140; b->y_zp = 133; b->y_scale = 0.04f;
  b->kzp1 = kzp1; b->kzp2 = kzp2;
  /* requantization scales that keep the rows inside the output range for most columns: about 1 / (40 sqrt K) */
  b->fc1_scale = 0.9f / (40.0f * (float) (c < 4 ? 2 : c) / 4.0f);
  b->fc2_scale = 0.9f / (40.0f * (float) (s < 4 ? 2 : s) / 4.0f);
  if (b->fc1_scale >= 1.0f) b->fc1_scale = 0.5f;
  if (b->fc2_scale >= 1.0f) b->fc2_scale = 0.5f;
  b->k1 = constant >= 0 ? constant_bytes(s * c, constant) : random_bytes(s * c);
  b->k2 = constant >= 0 ? constant_bytes(c * s, constant) : random_bytes(c * s);
  b->b1 = (int32_t*) malloc(sizeof(int32_t) * s);
  b->b2 = (int32_t*) malloc(sizeof(int32_t) * c);
  CHECK(b->b1 != NULL && b->b2 != NULL);
  for (size_t i = 0; i < s; i++) b->b1[i] = (int32_t) (next_u32() % 4001u) - 2000;
  for (size_t i = 0; i < c; i++) b->b2[i] = (int32_t) (next_u32() % 4001u) - 2000;
  for (int i = 0; i < 256; i++) b->table[i] = (uint8_t) (255 - ((i * 7 + 3) & 0xFF));
  CHECK(qnnp_create_global_average_pooling_nwc_q8(c, b->x_zp, b->x_scale, b->pool_zp, b->pool_scale, 0, 255, 0, &b->pool) == qnnp_status_success);
  /* fc1's ReLU is its output_min = its zero point; the scale arguments multiply out to the requantization scale */
  CHECK(qnnp_create_fully_connected_nc_q8(c, s, b->pool_zp, 1.0f, kzp1, b->fc1_scale, b->k1, b->b1, b->h_zp, 1.0f, b->h_zp, 255, 0, &b->fc1) == qnnp_status_success);
  CHECK(qnnp_create_fully_connected_nc_q8(s, c, b->h_zp, 1.0f, kzp2, b->fc2_scale, b->k2, b->b2, b->e_zp, 1.0f, 0, 255, 0, &b->fc2) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_lut_nc_x8(c, b->table, 0, &b->gate) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(c, b->x_zp, b->x_scale, 0, 0x1.0p-8f, b->y_zp, b->y_scale, 0, 255, 0, &b->mul) == qnnp_status_success);
}

static void free_block(struct block* b)
{
  CHECK(qnnp_delete_operator(b->pool) == qnnp_status_success);
  CHECK(qnnp_delete_operator(b->fc1) == qnnp_status_success);
  CHECK(qnnp_delete_operator(b->fc2) == qnnp_status_success);
  CHECK(qnnp_delete_operator(b->gate) == qnnp_status_success);
  CHECK(qnnp_delete_operator(b->mul) == qnnp_status_success);
  free(b->k1); free(b->b1); free(b->k2); free(b->b2);
}

/* s [batch][c] and y (spans as x's, stride ys) from the raw arrays, by the definitions */
static void expect(const struct block* b, size_t batch, size_t pixels, const uint8_t* x, size_t xs, uint8_t* s_out,
                   uint8_t* y, size_t ys, int* relu_hit)
{
  const float pool_scale = b->x_scale / (b->pool_scale * (float) pixels);
  const struct qnnp_hip_avgpool_params pq = qnnp_compute_avgpool_params(
      -(int32_t) pixels * (int32_t) b->x_zp, pool_scale, b->pool_zp, 0, 255);
  const struct qnnp_hip_requant rq1 = qnnp_compute_requant(1.0f * b->fc1_scale / 1.0f, b->h_zp, b->h_zp, 255);
  const struct qnnp_hip_requant rq2 = qnnp_compute_requant(1.0f * b->fc2_scale / 1.0f, b->e_zp, 0, 255);
  const float ab = b->x_scale * 0x1.0p-8f;
  const struct qnnp_hip_requant rqm = qnnp_compute_requant(ab / b->y_scale, b->y_zp, 0, 255);
  uint8_t* p = (uint8_t*) malloc(b->c);
  uint8_t* h = (uint8_t*) malloc(b->s);
  CHECK(p != NULL && h != NULL);
  for (size_t i = 0; i < batch; i++) {
    for (size_t c = 0; c < b->c; c++) {
      int32_t sum = pq.bias;
      for (size_t w = 0; w < pixels; w++) sum += x[(i * pixels + w) * xs + c];
      p[c] = avgpool_quantize(sum, &pq);
    }
    for (size_t n = 0; n < b->s; n++) {
      int64_t acc = b->b1[n];
      for (size_t k = 0; k < b->c; k++) acc += ((int32_t) p[k] - b->pool_zp) * ((int32_t) b->k1[n * b->c + k] - b->kzp1);
      CHECK(acc >= INT32_MIN && acc <= INT32_MAX);
      h[n] = q31_requantize((int32_t) acc, &rq1);
      if (h[n] == b->h_zp) *relu_hit = 1;
    }
    for (size_t n = 0; n < b->c; n++) {
      int64_t acc = b->b2[n];
      for (size_t k = 0; k < b->s; k++) acc += ((int32_t) h[k] - b->h_zp) * ((int32_t) b->k2[n * b->s + k] - b->kzp2);
      CHECK(acc >= INT32_MIN && acc <= INT32_MAX);
      s_out[i * b->c + n] = b->table[q31_requantize((int32_t) acc, &rq2)];
    }
    for (size_t w = 0; w < pixels; w++) {
      for (size_t c = 0; c < b->c; c++) {
        const int32_t acc = ((int32_t) x[(i * pixels + w) * xs + c] - b->x_zp) * (int32_t) s_out[i * b->c + c];
        y[(i * pixels + w) * ys + c] = q31_requantize(acc, &rqm);
      }
    }
  }
  free(p);
  free(h);
}

static void compare(const uint8_t* got, const uint8_t* want, size_t rows, size_t c, size_t stride, const char* what)
{
  for (size_t r = 0; r < rows; r++) {
    for (size_t o = 0; o < (r + 1 < rows ? stride : c); o++) {
      if (got[r * stride + o] != want[r * stride + o]) {
        fprintf(stderr, "%s: row %zu byte %zu: got %u, want %u\n", what, r, o, got[r * stride + o], want[r * stride + o]);
        exit(1);
      }
    }
  }
}

/* one block, out of place on strided host tensors and in place, against the raw-array expectation */
static void run_block(size_t batch, size_t pixels, size_t c, size_t s, uint8_t kzp1, uint8_t kzp2, int constant, size_t ex, size_t ey)
{
  struct block b;
  make_block(&b, c, s, kzp1, kzp2, constant);
  const size_t rows = batch * pixels, xs = c + ex, ys = c + ey;
  uint8_t* x = constant >= 0 ? constant_bytes((rows - 1) * xs + c, constant) : random_bytes((rows - 1) * xs + c);   /* exact spans */
  uint8_t* y = constant_bytes((rows - 1) * ys + c, FILL);
  uint8_t* want = constant_bytes((rows - 1) * ys + c, FILL);
  uint8_t* want_s = (uint8_t*) malloc(batch * c);
  CHECK(want_s != NULL);
  int relu_hit = 0;
  expect(&b, batch, pixels, x, xs, want_s, want, ys, &relu_hit);

  qnnp_operator_t se = NULL;
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.gate, b.mul, &se) == qnnp_status_success);
  CHECK(se != NULL);
  CHECK(qnnp_run_operator(se, NULL) == qnnp_status_invalid_parameter);    /* before setup */
  CHECK(qnnp_gfx950_test_force_kernel("se_kernel", 1) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_squeeze_excite(se, batch, pixels, x, xs, y, ys) == qnnp_status_success);
  CHECK(qnnp_gfx950_operator_set_streaming_stores(se, 1) == qnnp_status_success);
  const unsigned gates = qnnp_stub_se_launches, muls = qnnp_stub_mul_launches;
  CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
  CHECK(qnnp_stub_se_launches == gates + 1 && qnnp_stub_mul_launches == muls + 1);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(se), "stub_se_gate_pool") == 0);
  /* what the two launches were handed: the gate rows are the multiply's b, dense; the streaming mode goes to the multiply */
  CHECK(qnnp_stub_se_last.pool == 1 && qnnp_stub_se_last.batch == batch && qnnp_stub_se_last.pixels == pixels);
  CHECK(qnnp_stub_se_last.channels == c && qnnp_stub_se_last.squeeze == s && qnnp_stub_se_last.input_stride == xs);
  CHECK(qnnp_stub_se_last.fc1.row_coeff == 128 - (int32_t) kzp1 && qnnp_stub_se_last.fc2.row_coeff == 128 - (int32_t) kzp2);
  CHECK(qnnp_stub_mul_last.b == qnnp_stub_se_last.gate && qnnp_stub_mul_last.b_stride == c && qnnp_stub_mul_last.a == qnnp_stub_se_last.input);
  CHECK(qnnp_stub_mul_last.b_rows == batch && qnnp_stub_mul_last.a_rows_per_b_row == pixels && qnnp_stub_mul_last.channels == c);
  CHECK(qnnp_stub_mul_last.a_stride == xs && qnnp_stub_mul_last.product_stride == ys && qnnp_stub_mul_last.streaming_mode == 2);
  compare(qnnp_stub_se_last.gate, want_s, batch, c, c, "gate rows");      /* (the scratch is the stub's host memory) */
  compare(y, want, rows, c, ys, "output");
  if (constant < 0 && s >= 8) CHECK(relu_hit);

  /* the three-launch flavour: the stubbed pooling launch writes nothing, so only the plumbing is checked */
  CHECK(qnnp_gfx950_test_force_kernel("se_kernel", 2) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_squeeze_excite(se, batch, pixels, x, xs, y, ys) == qnnp_status_success);
  CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(se), "stub_se_gate") == 0);
  CHECK(qnnp_stub_se_last.pool == 0 && qnnp_stub_se_last.input != qnnp_stub_mul_last.a);
  CHECK(qnnp_stub_se_last.input >= qnnp_stub_se_last.gate + batch * c && (uintptr_t) qnnp_stub_se_last.input % 4 == 0);
  CHECK(qnnp_gfx950_test_force_kernel("se_kernel", 0) == qnnp_status_success);

  /* in place, automatic flavour (these images are small: the pooling inside) */
  {
    uint8_t* z = (uint8_t*) malloc((rows - 1) * xs + c);
    uint8_t* want_z = (uint8_t*) malloc((rows - 1) * xs + c);
    CHECK(z != NULL && want_z != NULL);
    memcpy(z, x, (rows - 1) * xs + c);
    memcpy(want_z, x, (rows - 1) * xs + c);
    expect(&b, batch, pixels, x, xs, want_s, want_z, xs, &relu_hit);
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, batch, pixels, z, xs, z, xs) == qnnp_status_success);
    CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
    CHECK(strcmp(qnnp_gfx950_operator_kernel(se), "stub_se_gate_pool") == 0);
    compare(z, want_z, rows, c, xs, "output in place");
    free(z);
    free(want_z);
  }
  /* the members are untouched: the chain's first operator still runs on its own */
  {
    uint8_t* p = constant_bytes(batch * c, FILL);
    CHECK(qnnp_setup_global_average_pooling_nwc_q8(b.pool, batch, pixels, x, xs, p, c) == qnnp_status_success);
    CHECK(qnnp_run_operator(b.pool, NULL) == qnnp_status_success);
    free(p);
  }
  CHECK(qnnp_delete_operator(se) == qnnp_status_success);
  free_block(&b);
  free(x); free(y); free(want); free(want_s);
}

static void statuses(void)
{
  struct block b, other;
  make_block(&b, 24, 8, 127, 127, -1);
  make_block(&other, 16, 8, 127, 127, -1);
  qnnp_operator_t se = NULL, add = NULL, pc = NULL, big_pool = NULL, big_gate = NULL, big_mul = NULL, big1 = NULL, big2 = NULL;
  /* ---- create, in the header's order: NULLs, kinds, the chain, [devices: one device here], a capture; then unsupported ---- */
  CHECK(qnnp_gfx950_create_squeeze_excite(NULL, b.fc1, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, NULL, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, NULL, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, NULL, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.gate, NULL, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.gate, b.mul, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_add_nc_q8(24, 0, 1.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &add) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_squeeze_excite(add, b.fc1, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.gate, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, add, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.mul, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.gate, b.gate, &se) == qnnp_status_invalid_parameter);
  /* the chain: each member in turn from a block of 16 channels, and the two fully connected swapped (24 -> 8 -> 24) */
  CHECK(qnnp_gfx950_create_squeeze_excite(other.pool, b.fc1, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, other.fc1, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, other.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, other.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.gate, other.mul, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc2, b.fc1, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  /* a per-channel member: unsupported -- but invalid first, and a capture is invalid */
  {
    float scales[8];
    for (int i = 0; i < 8; i++) scales[i] = b.fc1_scale * (1.0f + 0.01f * (float) i);
    CHECK(qnnp_gfx950_create_fully_connected_nc_q8_per_channel(24, 8, b.pool_zp, 1.0f, 127, scales, b.k1, b.b1, b.h_zp, 1.0f, b.h_zp, 255, 0, &pc) == qnnp_status_success);
  }
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, pc, b.fc2, b.gate, b.mul, &se) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, pc, b.fc2, b.gate, NULL, &se) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, pc, b.fc2, other.gate, b.mul, &se) == qnnp_status_invalid_parameter);
  {
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, pc, b.fc2, b.gate, b.mul, &se) == qnnp_status_invalid_parameter);
    qnnp_stub_set_capturing(0);
    CHECK(qnnp_stub_live_allocs() == live);
  }
  /* the limit: C = 4097 with S = 1, and S = 4097 with C = 1; 4096 of either is taken */
  {
    const size_t limit = QNNP_GFX950_SQUEEZE_EXCITE_MAX_CHANNELS;
    for (int which = 0; which < 2; which++) {
      for (size_t extra = 0; extra < 2; extra++) {
        const size_t c = which == 0 ? limit + extra : 1, s = which == 0 ? 1 : limit + extra;
        uint8_t* k = constant_bytes(c * s, 130);
        int32_t* bias = (int32_t*) calloc(c > s ? c : s, sizeof(int32_t));
        uint8_t table[256] = {0};
        CHECK(bias != NULL);
        CHECK(qnnp_create_global_average_pooling_nwc_q8(c, 0, 1.0f, 0, 1.0f, 0, 255, 0, &big_pool) == qnnp_status_success);
        CHECK(qnnp_create_fully_connected_nc_q8(c, s, 0, 1.0f, 128, 0.001f, k, bias, 0, 1.0f, 0, 255, 0, &big1) == qnnp_status_success);
        CHECK(qnnp_create_fully_connected_nc_q8(s, c, 0, 1.0f, 128, 0.001f, k, bias, 0, 1.0f, 0, 255, 0, &big2) == qnnp_status_success);
        CHECK(qnnp_gfx950_create_lut_nc_x8(c, table, 0, &big_gate) == qnnp_status_success);
        CHECK(qnnp_gfx950_create_multiply_nc_q8(c, 0, 1.0f, 0, 0.5f, 0, 1.0f, 0, 255, 0, &big_mul) == qnnp_status_success);
        se = NULL;
        CHECK(qnnp_gfx950_create_squeeze_excite(big_pool, big1, big2, big_gate, big_mul, &se) ==
              (extra ? qnnp_status_unsupported_parameter : qnnp_status_success));
        CHECK((se != NULL) == !extra);
        if (se != NULL) CHECK(qnnp_delete_operator(se) == qnnp_status_success);
        se = NULL;
        CHECK(qnnp_delete_operator(big_pool) == qnnp_status_success);
        CHECK(qnnp_delete_operator(big1) == qnnp_status_success);
        CHECK(qnnp_delete_operator(big2) == qnnp_status_success);
        CHECK(qnnp_delete_operator(big_gate) == qnnp_status_success);
        CHECK(qnnp_delete_operator(big_mul) == qnnp_status_success);
        free(k);
        free(bias);
      }
    }
  }
  CHECK(se == NULL);
  /* the operator structure that cannot be allocated is the only failure left */
  CHECK(qnnp_gfx950_create_squeeze_excite(b.pool, b.fc1, b.fc2, b.gate, b.mul, &se) == qnnp_status_success);

  /* ---- setup, in the header's order ---- */
  const size_t c = 24, batch = 3, pixels = 5, xs = 29, ys = 31, rows = batch * pixels;
  uint8_t* x = random_bytes((rows - 1) * xs + c);
  uint8_t* y = constant_bytes((rows - 1) * ys + c, FILL);
  uint8_t* want = constant_bytes((rows - 1) * ys + c, FILL);
  uint8_t* want_s = (uint8_t*) malloc(batch * c);
  int relu_hit = 0;
  CHECK(want_s != NULL);
  expect(&b, batch, pixels, x, xs, want_s, want, ys, &relu_hit);
  CHECK(qnnp_gfx950_setup_squeeze_excite(NULL, batch, pixels, x, xs, y, ys) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_squeeze_excite(b.mul, batch, pixels, x, xs, y, ys) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(se, batch, pixels, x, xs, x, xs, y, ys) == qnnp_status_invalid_parameter);
  /* batch 0: success whatever else, and run does nothing */
  {
    const unsigned gates = qnnp_stub_se_launches;
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, 0, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_se_launches == gates);
  }
  CHECK(qnnp_gfx950_setup_squeeze_excite(se, batch, pixels, x, xs, y, ys) == qnnp_status_success);
  CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
  compare(y, want, rows, c, ys, "output before the refused setups");
  const size_t too_wide = (size_t) INT32_MAX / 255 + 1;
  struct { size_t batch, pixels; const uint8_t* in; size_t xs; uint8_t* out; size_t ys; enum qnnp_status want; } refused[] = {
    {batch, 0, x, xs, y, ys, qnnp_status_invalid_parameter},
    {batch, 0, NULL, 0, NULL, 0, qnnp_status_invalid_parameter},
    {batch, pixels, NULL, xs, y, ys, qnnp_status_invalid_parameter},
    {batch, pixels, x, xs, NULL, ys, qnnp_status_invalid_parameter},
    {batch, pixels, x, c - 1, y, ys, qnnp_status_invalid_parameter},
    {batch, pixels, x, xs, y, c - 1, qnnp_status_invalid_parameter},
    {batch, too_wide, x, c - 1, y, ys, qnnp_status_invalid_parameter},               /* invalid before unsupported */
    {batch, too_wide, x, xs, y, ys, qnnp_status_unsupported_parameter},              /* the pooling's width bound */
    {1, too_wide, x, xs, x, xs + 1, qnnp_status_unsupported_parameter},              /* unsupported before the overlap */
    {(size_t) INT32_MAX + 1, 1, x, xs, y, ys, qnnp_status_unsupported_parameter},
    {65536, 32768, x, xs, y, ys, qnnp_status_unsupported_parameter},                 /* batch * pixels == 2^31 */
    {SIZE_MAX, pixels, x, xs, y, ys, qnnp_status_unsupported_parameter},
    {batch, pixels, x, xs, (uint8_t*) x + 1, xs, qnnp_status_invalid_parameter},     /* shifted */
    {batch, pixels, x, xs, (uint8_t*) x, xs + 1, qnnp_status_invalid_parameter},     /* the same base, another stride */
    {batch, pixels, x + xs, xs, (uint8_t*) x, xs, qnnp_status_invalid_parameter},
  };
  for (size_t i = 0; i < sizeof(refused) / sizeof(refused[0]); i++) {
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, refused[i].batch, refused[i].pixels, refused[i].in, refused[i].xs,
        refused[i].out, refused[i].ys) == refused[i].want);
    /* a refused setup leaves the previous one runnable */
    memset(y, FILL, (rows - 1) * ys + c);
    CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
    compare(y, want, rows, c, ys, "output after a refused setup");
  }
  /* (the pooling's scale range cannot be left by the pixel count alone: create holds the scale ratio in [2^-8, 2^8) and
   * the width bound holds the pixels below 2^23.01, so the width bound is the only refusal of that check) */
  CHECK(qnnp_setup_global_average_pooling_nwc_q8(b.pool, batch, too_wide, x, xs, y, c) == qnnp_status_unsupported_parameter);
  /* inside a capture: invalid, nothing allocated, the previous setup still runnable afterwards */
  {
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, batch + 1, pixels, x, xs, y, ys) == qnnp_status_invalid_parameter);
    qnnp_stub_set_capturing(0);
    CHECK(qnnp_stub_live_allocs() == live);
  }
  /* the scratch grows with the batch, and an allocation that fails -- the scratch first, then the staging -- is
   * out_of_memory and leaves the operator unrunnable until the next good setup */
  {
    const size_t big_rows = 4 * batch * pixels;
    uint8_t* bx = random_bytes((big_rows - 1) * xs + c);
    uint8_t* by = constant_bytes((big_rows - 1) * ys + c, FILL);
    uint8_t* bw = constant_bytes((big_rows - 1) * ys + c, FILL);
    uint8_t* bs = (uint8_t*) malloc(4 * batch * c);
    CHECK(bs != NULL);
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_fail_nth(0);
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, 4 * batch, pixels, bx, xs, by, ys) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(qnnp_stub_live_allocs() == live - 1);      /* the old scratch is gone, no new one */
    CHECK(qnnp_run_operator(se, NULL) == qnnp_status_invalid_parameter);
    qnnp_stub_fail_nth(1);
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, 4 * batch, pixels, bx, xs, by, ys) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(qnnp_run_operator(se, NULL) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, 4 * batch, pixels, bx, xs, by, ys) == qnnp_status_success);
    CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
    expect(&b, 4 * batch, pixels, bx, xs, bs, bw, ys, &relu_hit);
    compare(by, bw, big_rows, c, ys, "output after the scratch grew");
    /* and back to the small geometry on the larger scratch */
    memset(y, FILL, (rows - 1) * ys + c);
    CHECK(qnnp_gfx950_setup_squeeze_excite(se, batch, pixels, x, xs, y, ys) == qnnp_status_success);
    CHECK(qnnp_run_operator(se, NULL) == qnnp_status_success);
    compare(y, want, rows, c, ys, "output after re-setup to the smaller geometry");
    free(bx); free(by); free(bw); free(bs);
  }
  float ms = -1.0f;
  CHECK(qnnp_gfx950_time_operator(se, 1, 2, &ms) == qnnp_status_invalid_parameter);   /* host pointers cannot be timed */
  /* delete frees the scratch and the staging, and nothing of the members */
  {
    const size_t live = qnnp_stub_live_allocs();
    CHECK(qnnp_delete_operator(se) == qnnp_status_success);
    CHECK(qnnp_stub_live_allocs() == live - 3);      /* the scratch, the staged input, the staged output */
  }
  CHECK(qnnp_delete_operator(add) == qnnp_status_success);
  CHECK(qnnp_delete_operator(pc) == qnnp_status_success);
  free_block(&b);
  free_block(&other);
  free(x); free(y); free(want); free(want_s);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized, whatever the arguments */
  CHECK(qnnp_gfx950_create_squeeze_excite(NULL, NULL, NULL, NULL, NULL, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_squeeze_excite(NULL, 1, 1, NULL, 1, NULL, 1) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  CHECK(qnnp_gfx950_test_force_kernel("se_kernel", 3) == qnnp_status_invalid_parameter);
  statuses();
  {
    /* batch, pixels, C, S, extra stride bytes of x and y: the GPU tier's small cases */
    const size_t shapes[5][6] = {{3, 49, 24, 8, 0, 0}, {2, 1, 1, 1, 0, 0}, {2, 5, 33, 9, 3, 7}, {2, 50, 130, 40, 2, 0}, {1, 2, 260, 68, 0, 4}};
    const uint8_t zero_points[5][2] = {{128, 128}, {127, 127}, {90, 201}, {128, 127}, {127, 90}};
    for (int k = 0; k < 5; k++) {
      run_block(shapes[k][0], shapes[k][1], shapes[k][2], shapes[k][3], zero_points[k][0], zero_points[k][1], -1, shapes[k][4], shapes[k][5]);
    }
    /* the ends of the range: kernel zero points 0 and 255 against all-255 and all-0 weights and inputs */
    run_block(2, 5, 33, 9, 0, 0, 255, 3, 7);
    run_block(2, 5, 33, 9, 255, 255, 0, 3, 7);
    run_block(2, 5, 33, 9, 0, 255, 255, 0, 0);
    run_block(2, 5, 33, 9, 255, 0, 0, 0, 0);
  }
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-se-ok\n");
  return 0;
}
