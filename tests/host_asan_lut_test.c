/*
 * host_asan_lut_test.c -- TEST INFRASTRUCTURE: the host code of the lookup-table operators (lut.c, sigmoid.c,
 * leaky-relu.c) under AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and tests/hip_stub_lut.c
 * (Makefile target asan-lut; run by tests/test_lut_host.py). Walks create -> setup -> run -> re-setup with another batch
 * and new buffers -> run -> delete for the three operators, checking the bytes that come back through the host-pointer
 * staging, every status path of create and setup, and the table bytes of a few argument sets whose values follow from
 * the definition by hand. Prints "host-sanitizers-lut-ok" on success.
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
size_t qnnp_stub_live_allocs(void);

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define FILL 0xA5

typedef enum qnnp_status (*setup_fn)(qnnp_operator_t, size_t, const uint8_t*, size_t, uint8_t*, size_t);

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

/* the operator's table: its answer on the identity input */
static void read_table(qnnp_operator_t op256, setup_fn setup, uint8_t table[256])
{
  uint8_t x[256];
  for (int i = 0; i < 256; i++) x[i] = (uint8_t) i;
  CHECK(setup(op256, 1, x, 256, table, 256) == qnnp_status_success);
  CHECK(qnnp_run_operator(op256, NULL) == qnnp_status_success);
}

static void check_lut(const uint8_t* table, const uint8_t* x, const uint8_t* y, size_t n, size_t c, size_t si, size_t so,
                      int in_place)
{
  for (size_t p = 0; p < n; p++) {
    for (size_t o = 0; o < c; o++) CHECK(y[p * so + o] == table[x[p * si + o]]);
    if (!in_place && p + 1 < n) for (size_t o = c; o < so; o++) CHECK(y[p * so + o] == FILL);
  }
}

/* create -> setup -> run -> rejected setups -> run -> in place -> batch 0, three rounds, then delete */
static void walk(qnnp_operator_t op, setup_fn setup, const uint8_t table[256], size_t c, size_t extra_in, size_t extra_out)
{
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  const size_t si = c + extra_in, so = c + extra_out;
  for (int round = 0; round < 3; round++) {
    const size_t n = 2 + 3 * (size_t) round;
    uint8_t* x = bytes((n - 1) * si + c, (unsigned) round);              /* exact spans: ASan catches any overrun */
    uint8_t* y = filled((n - 1) * so + c);
    CHECK(setup(op, n, x, si, y, so) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_lut") == 0);
    check_lut(table, x, y, n, c, si, so, 0);
    /* rejected setups before the operator changes: the previous setup stays runnable */
    CHECK(setup(op, n, NULL, si, y, so) == qnnp_status_invalid_parameter);
    CHECK(setup(op, n, x, si, NULL, so) == qnnp_status_invalid_parameter);
    CHECK(setup(op, n, x, c - 1, y, so) == qnnp_status_invalid_parameter);
    CHECK(setup(op, n, x, si, y, c - 1) == qnnp_status_invalid_parameter);
    CHECK(setup(op, n, x + 1, si, x, si) == qnnp_status_invalid_parameter);   /* shifted overlap */
    CHECK(setup(op, n, x, si, x, si + 1) == qnnp_status_invalid_parameter);   /* same base, other stride */
    CHECK(setup(op, (size_t) INT32_MAX + 1, x, si, y, so) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_lut(table, x, y, n, c, si, so, 0);
    /* in place: the same tensor with equal strides */
    uint8_t* z = bytes((n - 1) * si + c, (unsigned) round + 7);
    uint8_t* was = bytes((n - 1) * si + c, (unsigned) round + 7);
    CHECK(setup(op, n, z, si, z, si) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_lut(table, was, z, n, c, si, si, 1);
    for (size_t p = 0; p + 1 < n; p++) CHECK(memcmp(z + p * si + c, was + p * si + c, si - c) == 0);
    /* batch 0: a successful no-op */
    CHECK(setup(op, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(x);
    free(y);
    free(z);
    free(was);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

/* round-half-to-even of d / 2, as lrintf gives it in the default rounding mode */
static int half_even(int d)
{
  if (d % 2 == 0) return d / 2;
  const int lo = (d - 1) / 2;   /* d odd: floor(d / 2) for either sign, since d - 1 is even */
  return lo % 2 == 0 ? lo : lo + 1;
}

static void tables(void)
{
  qnnp_operator_t op = NULL;
  uint8_t t[256];
  /* sigmoid, input 1.0 / 128, full range: 256 / (1 + e^-x) is 128 at 0, 187.1 at 1, 68.9 at -1, 0 far left, 256 -> 255 far right */
  CHECK(qnnp_create_sigmoid_nc_q8(256, 128, 1.0f, 0, 0x1.0p-8f, 0, 255, 0, &op) == qnnp_status_success);
  read_table(op, qnnp_setup_sigmoid_nc_q8, t);
  CHECK(t[128] == 128 && t[129] == 187 && t[127] == 69 && t[0] == 0 && t[255] == 255 && t[140] == 255 && t[116] == 0);
  for (int i = 1; i < 256; i++) CHECK(t[i] >= t[i - 1]);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* the same, clamped to [10, 200] */
  CHECK(qnnp_create_sigmoid_nc_q8(256, 128, 1.0f, 0, 0x1.0p-8f, 10, 200, 0, &op) == qnnp_status_success);
  read_table(op, qnnp_setup_sigmoid_nc_q8, t);
  CHECK(t[128] == 128 && t[129] == 187 && t[127] == 69 && t[0] == 10 && t[255] == 200 && t[130] == 200);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* leaky ReLU, slope 1/2, scale ratio 1, input zero point 100, output zero point 50: i - 50 right of the zero point,
   * half of (i - 100), ties to even, + 50 left of it */
  CHECK(qnnp_create_leaky_relu_nc_q8(256, 0.5f, 100, 2.0f, 50, 2.0f, 0, 255, 0, &op) == qnnp_status_success);
  read_table(op, qnnp_setup_leaky_relu_nc_q8, t);
  for (int i = 0; i < 256; i++) CHECK(t[i] == (i >= 100 ? i - 50 : half_even(i - 100) + 50));
  CHECK(t[99] == 50 && t[97] == 48 && t[95] == 48);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* the same with the output range [40, 120] */
  CHECK(qnnp_create_leaky_relu_nc_q8(256, 0.5f, 100, 2.0f, 50, 2.0f, 40, 120, 0, &op) == qnnp_status_success);
  read_table(op, qnnp_setup_leaky_relu_nc_q8, t);
  for (int i = 0; i < 256; i++) {
    int want = i >= 100 ? i - 50 : half_even(i - 100) + 50;
    want = want < 40 ? 40 : (want > 120 ? 120 : want);
    CHECK(t[i] == want);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* slope 1 and scale ratio 1 with equal zero points: the identity */
  CHECK(qnnp_create_leaky_relu_nc_q8(256, 1.0f, 7, 0.5f, 7, 0.5f, 0, 255, 0, &op) == qnnp_status_success);
  read_table(op, qnnp_setup_leaky_relu_nc_q8, t);
  for (int i = 0; i < 256; i++) CHECK(t[i] == i);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* the generic operator keeps a COPY of the caller's table */
  uint8_t mine[256];
  for (int i = 0; i < 256; i++) mine[i] = (uint8_t) (i * 167 + 13);   /* 167 is odd: a permutation */
  CHECK(qnnp_gfx950_create_lut_nc_x8(256, mine, 0, &op) == qnnp_status_success);
  memset(mine, 0, sizeof(mine));
  read_table(op, qnnp_gfx950_setup_lut_nc_x8, t);
  for (int i = 0; i < 256; i++) CHECK(t[i] == (uint8_t) (i * 167 + 13));
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void statuses(void)
{
  qnnp_operator_t op = NULL;
  const float s = 0x1.0p-8f;
  uint8_t table[256] = {0};
  /* reference src/sigmoid.c:39-80, in its order */
  CHECK(qnnp_create_sigmoid_nc_q8(0, 0, 1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 0.0f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, -1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0e-40f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);   /* subnormal */
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, INFINITY, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0f, 0, 0.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0f, 0, s, 100, 100, 0, &op) == qnnp_status_invalid_parameter);     /* min == max */
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0f, 0, s, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0f, 0, 0.5f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);  /* invalid before unsupported */
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0f, 0, 0.5f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0f, 1, s, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_sigmoid_nc_q8((size_t) INT32_MAX + 1, 0, 1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  /* reference src/leaky-relu.c:40-88, in its order */
  CHECK(qnnp_create_leaky_relu_nc_q8(0, 0.5f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 0.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, -0.5f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 1.5f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 0.5f, 0, 0.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 0.5f, 0, 1.0f, 0, 0.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 0.5f, 0, 1.0f, 0, 1.0f, 7, 7, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 0.5f, 0, 1.0f, 0, 1000.0f, 9, 7, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 0.5f, 0, 1.0f, 0, 257.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);  /* ratio < 2^-8 */
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 0.5f, 0, 256.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);  /* ratio == 2^8 */
  CHECK(qnnp_create_leaky_relu_nc_q8((size_t) INT32_MAX + 1, 0.5f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  /* the generic create */
  CHECK(qnnp_gfx950_create_lut_nc_x8(0, table, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_lut_nc_x8(8, NULL, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_lut_nc_x8((size_t) INT32_MAX + 1, table, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(op == NULL);
  /* the two edges that are still valid: ratio 2^-8 exactly, slope 1 */
  CHECK(qnnp_create_leaky_relu_nc_q8(8, 1.0f, 0, 1.0f, 0, 256.0f, 0, 255, 0, &op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;
  /* the table upload that fails (the allocation, then the copy): out_of_memory, nothing left allocated */
  const size_t live = qnnp_stub_live_allocs();
  for (long nth = 0; nth < 2; nth++) {
    qnnp_stub_fail_nth(nth);
    CHECK(qnnp_create_sigmoid_nc_q8(8, 0, 1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(op == NULL && qnnp_stub_live_allocs() == live);
  }
  /* setup of a NULL operator and of an operator of another type; any table operator takes any of the three setups */
  uint8_t* x = bytes(64, 0), * y = filled(64);
  CHECK(qnnp_setup_sigmoid_nc_q8(NULL, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_leaky_relu_nc_q8(NULL, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_lut_nc_x8(NULL, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_add_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
  CHECK(qnnp_setup_sigmoid_nc_q8(op, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_lut_nc_x8(op, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  for (int i = 0; i < 256; i++) table[i] = (uint8_t) (255 - i);
  CHECK(qnnp_gfx950_create_lut_nc_x8(8, table, 0, &op) == qnnp_status_success);
  /* a staging allocation that fails: out_of_memory, and the operator is not runnable */
  qnnp_stub_fail_nth(0);
  CHECK(qnnp_setup_leaky_relu_nc_q8(op, 4, x, 8, y, 8) == qnnp_status_out_of_memory);
  qnnp_stub_fail_nth(-1);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_sigmoid_nc_q8(op, 4, x, 8, y, 8) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  check_lut(table, x, y, 4, 8, 8, 8, 0);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  free(x);
  free(y);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  uint8_t table[256];
  for (int i = 0; i < 256; i++) table[i] = (uint8_t) (i * 59 + 200);   /* 59 is odd: a permutation */
  /* before qnnp_initialize: uninitialized (reference sigmoid.c:34-37, leaky-relu.c:35-38), whatever the arguments */
  CHECK(qnnp_create_sigmoid_nc_q8(0, 0, 0.0f, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_create_leaky_relu_nc_q8(0, 5.0f, 0, 0.0f, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_create_lut_nc_x8(0, NULL, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_setup_sigmoid_nc_q8(NULL, 1, NULL, 1, NULL, 1) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  statuses();
  tables();
  {
    const size_t shapes[4][3] = {{1, 0, 0}, {17, 3, 9}, {64, 0, 0}, {5, 11, 0}};
    for (int k = 0; k < 4; k++) {
      const size_t c = shapes[k][0];
      uint8_t t[256];
      qnnp_operator_t probe = NULL;
      CHECK(qnnp_gfx950_create_lut_nc_x8(c, table, 0, &op) == qnnp_status_success && op != NULL);
      walk(op, qnnp_gfx950_setup_lut_nc_x8, table, c, shapes[k][1], shapes[k][2]);
      CHECK(qnnp_create_sigmoid_nc_q8(256, 121, 0.75f, 0, 0x1.0p-8f, 0, 255, 0, &probe) == qnnp_status_success);
      read_table(probe, qnnp_setup_sigmoid_nc_q8, t);
      CHECK(qnnp_delete_operator(probe) == qnnp_status_success);
      CHECK(qnnp_create_sigmoid_nc_q8(c, 121, 0.75f, 0, 0x1.0p-8f, 0, 255, 0, &op) == qnnp_status_success && op != NULL);
      walk(op, qnnp_setup_sigmoid_nc_q8, t, c, shapes[k][1], shapes[k][2]);
      CHECK(qnnp_create_leaky_relu_nc_q8(256, 0.5f, 121, 1.25f, 133, 0.75f, 0, 255, 0, &probe) == qnnp_status_success);
      read_table(probe, qnnp_setup_leaky_relu_nc_q8, t);
      CHECK(qnnp_delete_operator(probe) == qnnp_status_success);
      CHECK(qnnp_create_leaky_relu_nc_q8(c, 0.5f, 121, 1.25f, 133, 0.75f, 0, 255, 0, &op) == qnnp_status_success && op != NULL);
      walk(op, qnnp_setup_leaky_relu_nc_q8, t, c, shapes[k][1], shapes[k][2]);
    }
  }
  /* inside a graph capture (tests/hip_stub.c) create and setup refuse with invalid_parameter and allocate nothing */
  {
    qnnp_operator_t lut = NULL, none = NULL;
    CHECK(qnnp_gfx950_create_lut_nc_x8(16, table, 0, &lut) == qnnp_status_success);
    uint8_t* x = bytes(5 * 16, 3), * y = filled(5 * 16);
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_create_lut_nc_x8(16, table, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(qnnp_create_sigmoid_nc_q8(16, 0, 1.0f, 0, 0x1.0p-8f, 0, 255, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(qnnp_create_leaky_relu_nc_q8(16, 0.5f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(none == NULL);
    CHECK(qnnp_gfx950_setup_lut_nc_x8(lut, 5, x, 16, y, 16) == qnnp_status_invalid_parameter);
    CHECK(qnnp_stub_live_allocs() == live);
    qnnp_stub_set_capturing(0);
    CHECK(qnnp_gfx950_setup_lut_nc_x8(lut, 5, x, 16, y, 16) == qnnp_status_success);
    CHECK(qnnp_run_operator(lut, NULL) == qnnp_status_success);
    check_lut(table, x, y, 5, 16, 16, 16, 0);
    free(x);
    free(y);
    CHECK(qnnp_delete_operator(lut) == qnnp_status_success);
  }
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-lut-ok\n");
  return 0;
}
