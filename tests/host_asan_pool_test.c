/*
 * host_asan_pool_test.c -- TEST INFRASTRUCTURE: the host code of the windowed pooling operators (max-pooling.c,
 * average-pooling.c) under AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and
 * tests/hip_stub_pool.c (Makefile target asan-pool; run by tests/test_pooling_host.py). Walks create -> setup -> run ->
 * re-setup with another geometry -> run -> delete for both operators, and every status path of create and setup.
 * Prints "host-sanitizers-pool-ok" on success.
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
size_t qnnp_stub_live_allocs(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static uint8_t* bytes(size_t n)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t) (i * 37u + 11u);
  return p;
}

static qnnp_operator_t create(int avg, uint32_t pad, uint32_t kh, uint32_t kw, uint32_t stride, uint32_t dil, size_t c)
{
  qnnp_operator_t op = NULL;
  if (avg) {
    CHECK(qnnp_create_average_pooling2d_nhwc_q8(pad, pad, pad, pad, kh, kw, stride, stride, c, 121, 0.5f, 133, 0.75f,
        0, 255, 0, &op) == qnnp_status_success);
  } else {
    CHECK(qnnp_create_max_pooling2d_nhwc_u8(pad, pad, pad, pad, kh, kw, stride, stride, dil, dil, c, 0, 255, 0, &op) ==
        qnnp_status_success);
  }
  CHECK(op != NULL);
  return op;
}

static enum qnnp_status setup(int avg, qnnp_operator_t op, size_t n, size_t h, size_t w, const uint8_t* x, size_t si,
                              uint8_t* y, size_t so)
{
  return avg ? qnnp_setup_average_pooling2d_nhwc_q8(op, n, h, w, x, si, y, so, NULL)
             : qnnp_setup_max_pooling2d_nhwc_u8(op, n, h, w, x, si, y, so, NULL);
}

static size_t out_dim(size_t in, uint32_t pad, uint32_t k, uint32_t d, uint32_t s)
{
  return (in + 2 * pad - ((size_t) (k - 1) * d + 1)) / s + 1;
}

static void walk(int avg, uint32_t pad, uint32_t k, uint32_t stride, uint32_t dil, size_t c, size_t extra)
{
  qnnp_operator_t op = create(avg, pad, k, k, stride, avg ? 1 : dil, c);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  for (int round = 0; round < 3; round++) {
    const size_t n = 1 + (size_t) round, h = 7 + (size_t) round * 5, w = 9 + (size_t) round * 2;
    const size_t si = c + extra, so = c + 2 * extra;
    const size_t oh = out_dim(h, pad, k, avg ? 1 : dil, stride), ow = out_dim(w, pad, k, avg ? 1 : dil, stride);
    uint8_t* x = bytes((n * h * w - 1) * si + c);                 /* exact spans: ASan catches any overrun */
    uint8_t* y = bytes((n * oh * ow - 1) * so + c);
    CHECK(setup(avg, op, n, h, w, x, si, y, so) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(strcmp(qnnp_gfx950_operator_kernel(op), avg ? "stub_avgpool" : "stub_maxpool") == 0);
    /* rejected setups before the operator changes: the previous setup stays runnable */
    CHECK(setup(avg, op, n, 0, w, x, si, y, so) == qnnp_status_invalid_parameter);
    CHECK(setup(avg, op, n, h, 0, x, si, y, so) == qnnp_status_invalid_parameter);
    CHECK(setup(avg, op, n, h, w, NULL, si, y, so) == qnnp_status_invalid_parameter);
    CHECK(setup(avg, op, n, h, w, x, si, NULL, so) == qnnp_status_invalid_parameter);
    CHECK(setup(avg, op, n, h, w, x, c - 1, y, so) == qnnp_status_invalid_parameter);
    CHECK(setup(avg, op, n, h, w, x, si, y, c - 1) == qnnp_status_invalid_parameter);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    /* batch 0: a successful no-op */
    CHECK(setup(avg, op, 0, h, w, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(x);
    free(y);
  }
  /* padded input smaller than the window (the reference's output size wraps around): invalid_parameter */
  {
    uint8_t* x = bytes(c);
    uint8_t* y = bytes(c);
    const size_t tiny = 1;
    const enum qnnp_status st = setup(avg, op, 1, tiny, tiny, x, c, y, c);
    CHECK(st == (k > 1 + 2 * pad || (!avg && (size_t) (k - 1) * dil + 1 > 1 + 2 * pad) ? qnnp_status_invalid_parameter
                                                                                          : qnnp_status_success));
    if (st == qnnp_status_invalid_parameter) {
      CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);   /* the batch-0 setup before it stays in force */
    }
    free(x);
    free(y);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void create_statuses(void)
{
  qnnp_operator_t op = NULL;
  /* reference src/max-pooling.c:61-103 */
  CHECK(qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 0, 3, 1, 1, 1, 1, 8, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 8, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 65536, 65536, 1, 1, 1, 1, 8, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 2, 2, 0, 1, 1, 1, 8, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 2, 2, 1, 1, 1, 0, 8, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 2, 2, 1, 1, 1, 1, 0, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  /* reference src/average-pooling.c:61-129 */
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 3, 0, 1, 1, 8, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 1, 1, 1, 1, 8, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 0, 8, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 0, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 0.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 8, 0, NAN, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0f, 0, -1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0f, 0, 1.0e-39f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0f, 0, 512.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 256.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 4096, 4096, 1, 1, 8, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  /* setup / run of a NULL operator */
  CHECK(qnnp_setup_max_pooling2d_nhwc_u8(NULL, 1, 1, 1, NULL, 1, NULL, 1, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_average_pooling2d_nhwc_q8(NULL, 1, 1, 1, NULL, 1, NULL, 1, NULL) == qnnp_status_invalid_parameter);
  /* an operator of the other pooling type is not accepted by setup */
  op = create(1, 0, 2, 2, 2, 1, 8);
  uint8_t* x = bytes(64);
  CHECK(qnnp_setup_max_pooling2d_nhwc_u8(op, 1, 2, 2, x, 8, x, 8, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  free(x);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized (reference max-pooling.c:56-59, average-pooling.c:56-59) */
  CHECK(qnnp_create_max_pooling2d_nhwc_u8(0, 0, 0, 0, 2, 2, 1, 1, 1, 1, 8, 0, 255, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_create_average_pooling2d_nhwc_q8(0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_initialize() == qnnp_status_success);
  create_statuses();
  for (int avg = 0; avg <= 1; avg++) {
    walk(avg, 0, 2, 2, 1, 64, 0);
    walk(avg, 1, 3, 2, 1, 24, 5);
    walk(avg, 2, 3, 1, 2, 7, 1);
    walk(avg, 0, 5, 3, 1, 1, 0);
    walk(avg, 4, 3, 1, 1, 16, 3);    /* windows wholly in padding */
  }
  /* inside a graph capture (tests/hip_stub.c) create and setup refuse with invalid_parameter and allocate nothing */
  for (int avg = 0; avg <= 1; avg++) {
    qnnp_operator_t pool = create(avg, 1, 3, 3, 1, 1, 8), none = NULL;
    uint8_t* x = bytes(2 * 5 * 5 * 8), * y = bytes(2 * 5 * 5 * 8);
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK((avg ? qnnp_create_average_pooling2d_nhwc_q8(1, 1, 1, 1, 3, 3, 1, 1, 8, 121, 0.5f, 133, 0.75f, 0, 255, 0, &none)
               : qnnp_create_max_pooling2d_nhwc_u8(1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 8, 0, 255, 0, &none)) ==
          qnnp_status_invalid_parameter);
    CHECK(none == NULL);
    CHECK(setup(avg, pool, 2, 5, 5, x, 8, y, 8) == qnnp_status_invalid_parameter);
    CHECK(qnnp_stub_live_allocs() == live);
    qnnp_stub_set_capturing(0);
    CHECK(setup(avg, pool, 2, 5, 5, x, 8, y, 8) == qnnp_status_success);
    CHECK(qnnp_run_operator(pool, NULL) == qnnp_status_success);
    free(x);
    free(y);
    CHECK(qnnp_delete_operator(pool) == qnnp_status_success);
  }
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-pool-ok\n");
  return 0;
}
