/*
 * host_asan_x8_test.c -- TEST INFRASTRUCTURE: the host code of channel shuffle and clamp (channel-shuffle.c, clamp.c)
 * under AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and tests/hip_stub_x8.c (Makefile target
 * asan-x8; run by tests/test_x8_host.py). Walks create -> setup -> run -> re-setup with another batch and new buffers
 * -> run -> delete for both operators, checking the bytes that come back through the host-pointer staging, and every
 * status path of create and setup. Prints "host-sanitizers-x8-ok" on success.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

/* tests/hip_stub.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
size_t qnnp_stub_live_allocs(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define FILL 0xA5

static uint8_t* bytes(size_t n, unsigned salt)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t) (i * 37u + 11u + salt * 101u + (i >> 8));
  return p;
}

static uint8_t* filled(size_t n)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  memset(p, FILL, n);
  return p;
}

/* the output bytes of one run: every pixel's channels as the operator defines them, FILL between pixels */
static void check_shuffle(const uint8_t* x, const uint8_t* y, size_t n, size_t g, size_t gc, size_t si, size_t so)
{
  const size_t c = g * gc;
  for (size_t p = 0; p < n; p++) {
    for (size_t o = 0; o < c; o++) CHECK(y[p * so + o] == x[p * si + (o % g) * gc + o / g]);
    if (p + 1 < n) for (size_t o = c; o < so; o++) CHECK(y[p * so + o] == FILL);
  }
}

static void walk_shuffle(size_t g, size_t gc, size_t extra_in, size_t extra_out)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_channel_shuffle_nc_x8(g, gc, 0, &op) == qnnp_status_success && op != NULL);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  const size_t c = g * gc, si = c + extra_in, so = c + extra_out;
  for (int round = 0; round < 3; round++) {
    const size_t n = 1 + 4 * (size_t) round;
    uint8_t* x = bytes((n - 1) * si + c, (unsigned) round);            /* exact spans: ASan catches any overrun */
    uint8_t* y = filled((n - 1) * so + c);
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, n, x, si, y, so) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_channel_shuffle") == 0);
    check_shuffle(x, y, n, g, gc, si, so);
    /* rejected setups before the operator changes: the previous setup stays runnable */
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, n, NULL, si, y, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, n, x, si, NULL, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, n, x, c - 1, y, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, n, x, si, y, c - 1) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, n, x, si, x, si) == qnnp_status_invalid_parameter);      /* in place */
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, n, x + 1, si, x, si) == qnnp_status_invalid_parameter);  /* overlap */
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, (size_t) INT32_MAX + 1, x, si, y, so) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_shuffle(x, y, n, g, gc, si, so);
    /* batch 0: a successful no-op */
    CHECK(qnnp_setup_channel_shuffle_nc_x8(op, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(x);
    free(y);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void check_clamp(const uint8_t* x, const uint8_t* y, size_t n, size_t c, size_t si, size_t so, int lo, int hi,
                        int in_place)
{
  for (size_t p = 0; p < n; p++) {
    for (size_t o = 0; o < c; o++) {
      const int v = x[p * si + o];
      CHECK(y[p * so + o] == (v < lo ? lo : (v > hi ? hi : v)));
    }
    if (!in_place && p + 1 < n) for (size_t o = c; o < so; o++) CHECK(y[p * so + o] == FILL);
  }
}

static void walk_clamp(size_t c, size_t extra_in, size_t extra_out, uint8_t lo, uint8_t hi)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_clamp_nc_u8(c, lo, hi, 0, &op) == qnnp_status_success && op != NULL);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  const size_t si = c + extra_in, so = c + extra_out;
  for (int round = 0; round < 3; round++) {
    const size_t n = 2 + 3 * (size_t) round;
    uint8_t* x = bytes((n - 1) * si + c, (unsigned) round);
    uint8_t* y = filled((n - 1) * so + c);
    CHECK(qnnp_setup_clamp_nc_u8(op, n, x, si, y, so) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_clamp") == 0);
    check_clamp(x, y, n, c, si, so, lo, hi, 0);
    CHECK(qnnp_setup_clamp_nc_u8(op, n, NULL, si, y, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_clamp_nc_u8(op, n, x, si, NULL, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_clamp_nc_u8(op, n, x, c - 1, y, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_clamp_nc_u8(op, n, x, si, y, c - 1) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_clamp_nc_u8(op, n, x + 1, si, x, si) == qnnp_status_invalid_parameter);   /* shifted overlap */
    if (n > 1) CHECK(qnnp_setup_clamp_nc_u8(op, n, x, si, x, si + 1) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_clamp_nc_u8(op, (size_t) INT32_MAX + 1, x, si, y, so) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_clamp(x, y, n, c, si, so, lo, hi, 0);
    /* in place: the same tensor with equal strides */
    uint8_t* z = bytes((n - 1) * si + c, (unsigned) round + 7);
    uint8_t* want = bytes((n - 1) * si + c, (unsigned) round + 7);
    CHECK(qnnp_setup_clamp_nc_u8(op, n, z, si, z, si) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_clamp(want, z, n, c, si, si, lo, hi, 1);
    for (size_t p = 0; p + 1 < n; p++) CHECK(memcmp(z + p * si + c, want + p * si + c, si - c) == 0);
    CHECK(qnnp_setup_clamp_nc_u8(op, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(x);
    free(y);
    free(z);
    free(want);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void statuses(void)
{
  qnnp_operator_t op = NULL;
  /* reference src/channel-shuffle.c:35-49 */
  CHECK(qnnp_create_channel_shuffle_nc_x8(0, 4, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_channel_shuffle_nc_x8(1, 4, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_channel_shuffle_nc_x8(2, 0, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_channel_shuffle_nc_x8(1, 0, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_channel_shuffle_nc_x8(65536, 65536, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_channel_shuffle_nc_x8((size_t) INT32_MAX + 1, 1, 0, &op) == qnnp_status_unsupported_parameter);
  /* reference src/clamp.c:35-48 */
  CHECK(qnnp_create_clamp_nc_u8(0, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_clamp_nc_u8(8, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_clamp_nc_u8(0, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_clamp_nc_u8((size_t) INT32_MAX + 1, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(op == NULL);
  /* setup / run of a NULL operator, and of an operator of the other type */
  CHECK(qnnp_setup_channel_shuffle_nc_x8(NULL, 1, NULL, 1, NULL, 1) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_clamp_nc_u8(NULL, 1, NULL, 1, NULL, 1) == qnnp_status_invalid_parameter);
  uint8_t* x = bytes(64, 0), * y = filled(64);
  CHECK(qnnp_create_clamp_nc_u8(8, 0, 255, 0, &op) == qnnp_status_success);
  CHECK(qnnp_setup_channel_shuffle_nc_x8(op, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  CHECK(qnnp_create_channel_shuffle_nc_x8(2, 4, 0, &op) == qnnp_status_success);
  CHECK(qnnp_setup_clamp_nc_u8(op, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  /* a staging allocation that fails: out_of_memory, and the operator is not runnable */
  qnnp_stub_fail_nth(0);
  CHECK(qnnp_setup_channel_shuffle_nc_x8(op, 4, x, 8, y, 8) == qnnp_status_out_of_memory);
  qnnp_stub_fail_nth(-1);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_channel_shuffle_nc_x8(op, 4, x, 8, y, 8) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  check_shuffle(x, y, 4, 2, 4, 8, 8);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  free(x);
  free(y);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized (reference channel-shuffle.c:30-33, clamp.c:30-33) */
  CHECK(qnnp_create_channel_shuffle_nc_x8(2, 4, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_create_clamp_nc_u8(8, 0, 255, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_initialize() == qnnp_status_success);
  statuses();
  walk_shuffle(2, 4, 0, 0);
  walk_shuffle(3, 5, 7, 1);
  walk_shuffle(8, 12, 0, 3);
  walk_shuffle(11, 1, 2, 0);
  walk_clamp(1, 0, 0, 0, 255);
  walk_clamp(17, 3, 9, 40, 200);
  walk_clamp(64, 0, 0, 255, 255);
  walk_clamp(5, 11, 0, 0, 6);
  /* inside a graph capture (tests/hip_stub.c) create and setup refuse with invalid_parameter and allocate nothing */
  {
    qnnp_operator_t shuffle = NULL, clamp = NULL, none = NULL;
    CHECK(qnnp_create_channel_shuffle_nc_x8(2, 8, 0, &shuffle) == qnnp_status_success);
    CHECK(qnnp_create_clamp_nc_u8(16, 10, 20, 0, &clamp) == qnnp_status_success);
    uint8_t* x = bytes(5 * 16, 3), * y = filled(5 * 16);
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_create_channel_shuffle_nc_x8(2, 8, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(qnnp_create_clamp_nc_u8(16, 10, 20, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(none == NULL);
    CHECK(qnnp_setup_channel_shuffle_nc_x8(shuffle, 5, x, 16, y, 16) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_clamp_nc_u8(clamp, 5, x, 16, y, 16) == qnnp_status_invalid_parameter);
    CHECK(qnnp_stub_live_allocs() == live);
    qnnp_stub_set_capturing(0);
    CHECK(qnnp_setup_channel_shuffle_nc_x8(shuffle, 5, x, 16, y, 16) == qnnp_status_success);
    CHECK(qnnp_run_operator(shuffle, NULL) == qnnp_status_success);
    check_shuffle(x, y, 5, 2, 8, 16, 16);
    CHECK(qnnp_setup_clamp_nc_u8(clamp, 5, x, 16, y, 16) == qnnp_status_success);
    CHECK(qnnp_run_operator(clamp, NULL) == qnnp_status_success);
    check_clamp(x, y, 5, 16, 16, 16, 10, 20, 0);
    free(x);
    free(y);
    CHECK(qnnp_delete_operator(shuffle) == qnnp_status_success);
    CHECK(qnnp_delete_operator(clamp) == qnnp_status_success);
  }
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-x8-ok\n");
  return 0;
}
