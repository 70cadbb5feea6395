/*
 * host_asan_mul_test.c -- TEST INFRASTRUCTURE: the host code of the multiply operator and of the hardswish and
 * hardsigmoid table builders (multiply.c, hardswish.c, hardsigmoid.c on lut.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer, against tests/hip_stub.c, tests/hip_stub_lut.c and tests/hip_stub_mul.c (Makefile target
 * asan-mul; run by tests/test_multiply_host.py). Walks every create and setup status, the overlap rules, launches whose
 * stubbed kernel checks the arguments it was handed and whose bytes follow from the definition by hand (scale ratios
 * 1/2 and 1/4), re-setup, a refused setup that leaves the last one runnable, and a few table entries of the two
 * activations. Prints "host-sanitizers-mul-ok" on success.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"

/* tests/hip_stub.c and tests/hip_stub_mul.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
size_t qnnp_stub_live_allocs(void);
extern struct qnnp_hip_mul_args qnnp_stub_mul_last;
extern unsigned qnnp_stub_mul_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define FILL 0xA5

/* bytes within `spread` of `centre`, so that products stay inside the output range */
static uint8_t* bytes(size_t n, unsigned salt, int centre, int spread)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t) (centre - spread + (int) ((i * 37u + 11u + salt * 101u + (i >> 8)) % (2u * (unsigned) spread + 1u)));
  return p;
}

static uint8_t* filled(size_t n)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  memset(p, FILL, n);
  return p;
}

static int floor_div(int n, int d) { return n >= 0 ? n / d : -((-n + d - 1) / d); }

/* the down-convert by hand for the ratios 1/2 (shift 0: the Q31 product rounds half up) and 1/4 (shift 1: that result,
 * halved, rounds half away from zero), zero point 128, full range */
static uint8_t by_hand(int acc, int quarter)
{
  int q = floor_div(acc + 1, 2);
  if (quarter) {
    const int mag = q < 0 ? -q : q;
    const int half = (mag + 1) / 2;
    q = q < 0 ? -half : half;
    /* the remainder test subtracts one for a negative ACCUMULATOR: q == 0 from acc == -1 has remainder -1, rounds to 0 */
  }
  int y = q + 128;
  return (uint8_t) (y < 0 ? 0 : (y > 255 ? 255 : y));
}

static void check_product(const uint8_t* a, const uint8_t* b, const uint8_t* y, size_t b_rows, size_t per, size_t c,
                          size_t sa, size_t sb, size_t sy, int quarter, int in_place)
{
  for (size_t r = 0; r < b_rows * per; r++) {
    for (size_t o = 0; o < c; o++) {
      const int acc = ((int) a[r * sa + o] - 128) * ((int) b[(r / per) * sb + o] - 121);
      CHECK(y[r * sy + o] == by_hand(acc, quarter));
    }
    if (!in_place && r + 1 < b_rows * per) for (size_t o = c; o < sy; o++) CHECK(y[r * sy + o] == FILL);
  }
}

static void walk(size_t c, size_t b_rows, size_t per, size_t ea, size_t eb, size_t ey, int quarter)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_multiply_nc_q8(c, 128, 1.0f, 121, quarter ? 0.25f : 0.5f, 128, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
  CHECK(op != NULL);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  const size_t sa = c + ea, sb = c + eb, sy = c + ey, rows = b_rows * per;
  /* exact spans: ASan catches any overrun */
  uint8_t* a = bytes((rows - 1) * sa + c, 1, 128, 9);
  uint8_t* b = bytes((b_rows - 1) * sb + c, 2, 121, 20);
  uint8_t* y = filled((rows - 1) * sy + c);
  const unsigned launches = qnnp_stub_mul_launches;
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, b, sb, y, sy) == qnnp_status_success);
  CHECK(qnnp_gfx950_operator_set_streaming_stores(op, 1) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_mul") == 0);
  /* what the launch was handed */
  CHECK(qnnp_stub_mul_launches == launches + 1);
  CHECK(qnnp_stub_mul_last.b_rows == b_rows && qnnp_stub_mul_last.a_rows_per_b_row == per && qnnp_stub_mul_last.channels == c);
  CHECK(qnnp_stub_mul_last.a_stride == sa && qnnp_stub_mul_last.b_stride == sb && qnnp_stub_mul_last.product_stride == sy);
  CHECK(qnnp_stub_mul_last.a_zero_point == 128 && qnnp_stub_mul_last.b_zero_point == 121);
  CHECK(qnnp_stub_mul_last.rq.multiplier == 0x40000000 && qnnp_stub_mul_last.rq.shift == (quarter ? 1u : 0u));
  CHECK(qnnp_stub_mul_last.rq.accumulator_bits == 16 && qnnp_stub_mul_last.rq.output_zero_point == 128);
  CHECK(qnnp_stub_mul_last.streaming_mode == 2);
  /* host tensors: all three are staged, none is the caller's pointer */
  CHECK(qnnp_stub_mul_last.a != a && qnnp_stub_mul_last.b != b && qnnp_stub_mul_last.product != y);
  check_product(a, b, y, b_rows, per, c, sa, sb, sy, quarter, 0);
  CHECK(qnnp_gfx950_operator_set_streaming_stores(op, -1) == qnnp_status_success);

  /* refused setups come before the operator changes: the previous setup stays runnable */
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, NULL, sa, b, sb, y, sy) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, NULL, sb, y, sy) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, b, sb, NULL, sy) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, c - 1, b, sb, y, sy) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, b, c - 1, y, sy) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, b, sb, y, c - 1) == qnnp_status_invalid_parameter);
  /* the row limit: each factor alone, the product of the two, and a product that wraps 64 bits */
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, (size_t) INT32_MAX + 1, 1, a, sa, b, sb, y, sy) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, 1, (size_t) INT32_MAX + 1, a, sa, b, sb, y, sy) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, 65536, 32768, a, sa, b, sb, y, sy) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, (size_t) 1 << 33, (size_t) 1 << 31, a, sa, b, sb, y, sy) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, SIZE_MAX, SIZE_MAX, a, sa, b, sb, y, sy) == qnnp_status_unsupported_parameter);
  /* overlaps: shifted, same base with another stride, the product on a broadcast b */
  if (rows > 1 || c > 1) {
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a + 1, sa, b, sb, a, sa) == qnnp_status_invalid_parameter);
  }
  if (rows > 1) {
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, b, sb, a, sa + 1) == qnnp_status_invalid_parameter);
  }
  if (per > 1) {
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, b, sb, (uint8_t*) b, sb) == qnnp_status_invalid_parameter);
  }
  memset(y, FILL, (rows - 1) * sy + c);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  check_product(a, b, y, b_rows, per, c, sa, sb, sy, quarter, 0);

  /* in place on a */
  {
    uint8_t* z = bytes((rows - 1) * sa + c, 1, 128, 9);
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, z, sa, b, sb, z, sa) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_product(a, b, z, b_rows, per, c, sa, sb, sa, quarter, 1);
    for (size_t r = 0; r + 1 < rows; r++) CHECK(memcmp(z + r * sa + c, a + r * sa + c, sa - c) == 0);
    free(z);
  }
  /* element-wise, in place on b; and a == b, which is only read */
  {
    uint8_t* a1 = bytes((b_rows - 1) * sb + c, 3, 128, 9);
    uint8_t* z = bytes((b_rows - 1) * sb + c, 2, 121, 20);
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, 1, a1, sb, z, sb, z, sb) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_product(a1, b, z, b_rows, 1, c, sb, sb, sb, quarter, 1);
    uint8_t* sq = filled((b_rows - 1) * sy + c);
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, 1, a1, sb, a1, sb, sq, sy) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_product(a1, a1, sq, b_rows, 1, c, sb, sb, sy, quarter, 0);
    /* a and b overlapping partially is fine too */
    if (b_rows > 1) {
      CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows - 1, 1, a1, sb, a1 + sb, sb, sq, sy) == qnnp_status_success);
      CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    }
    free(a1);
    free(z);
    free(sq);
  }
  /* no rows: a successful no-op, whatever the pointers */
  {
    const unsigned before = qnnp_stub_mul_launches;
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, 0, per, NULL, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, 0, NULL, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_mul_launches == before);
  }
  /* a staging allocation that fails: out_of_memory, and the operator is not runnable until the next good setup */
  {
    uint8_t* big = bytes((4 * rows - 1) * sa + c, 5, 128, 9);
    uint8_t* out = filled((4 * rows - 1) * sy + c);
    qnnp_stub_fail_nth(0);
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, 4 * b_rows, per, big, sa, b, sb, out, sy) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
    free(big);
    free(out);
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, b_rows, per, a, sa, b, sb, y, sy) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    check_product(a, b, y, b_rows, per, c, sa, sb, sy, quarter, 0);
  }
  float ms = -1.0f;
  CHECK(qnnp_gfx950_time_operator(op, 1, 2, &ms) == qnnp_status_invalid_parameter);   /* host pointers cannot be timed */
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  free(a);
  free(b);
  free(y);
}

static void multiply_statuses(void)
{
  qnnp_operator_t op = NULL;
  /* in the documented order */
  CHECK(qnnp_gfx950_create_multiply_nc_q8(0, 0, 0.0f, 0, 0.0f, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 0.0f, 0, 1.0f, 0, 4.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, -1.0f, 0, 1.0f, 0, 4.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0e-40f, 0, 1.0f, 0, 4.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);   /* subnormal */
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, INFINITY, 0, 4.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, NAN, 0, 4.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 0.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 4.0f, 100, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 4.0f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  /* invalid before unsupported */
  CHECK(qnnp_gfx950_create_multiply_nc_q8((size_t) INT32_MAX + 1, 0, 1.0f, 0, 1.0f, 0, 4.0f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 1.0f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8((size_t) INT32_MAX + 1, 0, 1.0f, 0, 1.0f, 0, 4.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  /* the ratio's domain is [2^-32, 1) */
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 2.0f, 0, 3.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 0x1.0p-17f, 0, 0x1.0p-17f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);   /* 2^-34 */
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 0x1.0p-80f, 0, 0x1.0p-80f, 0, 0x1.0p-100f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);   /* a * b underflows */
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 0x1.0p+80f, 0, 0x1.0p+80f, 0, 0x1.0p+100f, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);   /* a * b overflows */
  CHECK(op == NULL);
  /* both ends of the domain */
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 0x1.0p-16f, 0, 0x1.0p-16f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_multiply_nc_q8((size_t) INT32_MAX, 255, 0x1.fffffep-1f, 255, 1.0f, 255, 1.0f, 0, 1, 7, &op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;
  /* the operator structure that cannot be allocated is the only failure left; setups of other kinds */
  uint8_t* x = bytes(64, 0, 128, 9), * y = filled(64);
  qnnp_operator_t add = NULL, lut = NULL;
  uint8_t table[256] = {0};
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(NULL, 1, 1, x, 8, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_add_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &add) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_lut_nc_x8(8, table, 0, &lut) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 4.0f, 0, 255, 0, &op) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(add, 1, 1, x, 8, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(lut, 1, 1, x, 8, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_add_nc_q8(op, 1, x, 8, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_lut_nc_x8(op, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  /* inside a graph capture create and setup refuse and allocate nothing */
  {
    qnnp_operator_t none = NULL;
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 4.0f, 0, 255, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_create_hardswish_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 255, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_create_hardsigmoid_nc_q8(8, 0, 1.0f, 0, 0x1.0p-8f, 0, 255, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(none == NULL);
    CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, 2, 2, x, 8, x, 8, y, 8) == qnnp_status_invalid_parameter);
    CHECK(qnnp_stub_live_allocs() == live);
    qnnp_stub_set_capturing(0);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(add) == qnnp_status_success);
  CHECK(qnnp_delete_operator(lut) == qnnp_status_success);
  free(x);
  free(y);
}

typedef enum qnnp_status (*create_fn)(size_t, uint8_t, float, uint8_t, float, uint8_t, uint8_t, uint32_t, qnnp_operator_t*);

static void read_table(create_fn create, uint8_t izp, float is, uint8_t ozp, float os, uint8_t lo, uint8_t hi, uint8_t table[256])
{
  qnnp_operator_t op = NULL;
  uint8_t x[256];
  for (int i = 0; i < 256; i++) x[i] = (uint8_t) i;
  CHECK(create(256, izp, is, ozp, os, lo, hi, 0, &op) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_lut_nc_x8(op, 1, x, 256, table, 256) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void activation_statuses(create_fn create, int is_sigmoid)
{
  qnnp_operator_t op = NULL;
  const float s = 0x1.0p-8f;
  CHECK(create(0, 0, 1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, 0.0f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, -1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, 1.0e-40f, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, INFINITY, 0, s, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, 1.0f, 0, 0.0f, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, 1.0f, 0, NAN, 0, 255, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, 1.0f, 0, s, 100, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, 1.0f, 0, s, 200, 100, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(create(8, 0, 1.0f, 7, 0.5f, 200, 100, 0, &op) == qnnp_status_invalid_parameter);   /* invalid before unsupported */
  CHECK(create((size_t) INT32_MAX + 1, 0, 1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(create(8, 0, 1.0f, 0, 0.5f, 0, 255, 0, &op) == (is_sigmoid ? qnnp_status_unsupported_parameter : qnnp_status_success));
  if (!is_sigmoid) CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;
  CHECK(create(8, 0, 1.0f, 1, s, 0, 255, 0, &op) == (is_sigmoid ? qnnp_status_unsupported_parameter : qnnp_status_success));
  if (!is_sigmoid) CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;
  /* the table upload that fails (the allocation, then the copy): out_of_memory, nothing left allocated */
  const size_t live = qnnp_stub_live_allocs();
  for (long nth = 0; nth < 2; nth++) {
    qnnp_stub_fail_nth(nth);
    CHECK(create(8, 0, 1.0f, 0, s, 0, 255, 0, &op) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(op == NULL && qnnp_stub_live_allocs() == live);
  }
}

static void tables(void)
{
  uint8_t t[256];
  /* hardsigmoid with input 1/32 around 128: 256 * (x + 3) / 6 is 128 at 0, 0 from x = -3 (i = 32) down, saturates at 255
   * from x = 3 (i = 224) up; x = 1.5 (i = 176) gives 192 exactly, x = -1.5 gives 64 */
  read_table(qnnp_gfx950_create_hardsigmoid_nc_q8, 128, 0x1.0p-5f, 0, 0x1.0p-8f, 0, 255, t);
  CHECK(t[128] == 128 && t[32] == 0 && t[0] == 0 && t[224] == 255 && t[255] == 255 && t[176] == 192 && t[80] == 64);
  for (int i = 1; i < 256; i++) CHECK(t[i] >= t[i - 1]);
  read_table(qnnp_gfx950_create_hardsigmoid_nc_q8, 128, 0x1.0p-5f, 0, 0x1.0p-8f, 10, 200, t);
  CHECK(t[128] == 128 && t[0] == 10 && t[255] == 200 && t[176] == 192 && t[80] == 64);
  /* hardswish with input 1/16 around 128 and output 1/16 from 32: x * relu6(x + 3) / 6 is 0 at and below -3 (i = 80) and
   * at 0, x itself from 3 (i = 176) up, -0.375 at -1.5 (i = 104: -6 output steps), 3 * 6 / 6 = 3 at i = 176 (48 steps) */
  read_table(qnnp_gfx950_create_hardswish_nc_q8, 128, 0x1.0p-4f, 32, 0x1.0p-4f, 0, 255, t);
  CHECK(t[128] == 32 && t[80] == 32 && t[0] == 32 && t[104] == 26 && t[176] == 80 && t[200] == 104 && t[255] == 159);
  read_table(qnnp_gfx950_create_hardswish_nc_q8, 128, 0x1.0p-4f, 32, 0x1.0p-4f, 30, 100, t);
  CHECK(t[128] == 32 && t[104] == 30 && t[176] == 80 && t[200] == 100 && t[255] == 100);
  /* an input scale whose x overflows: the left half is 0 * -inf, a NaN, and lands on the lower bound; no trap */
  read_table(qnnp_gfx950_create_hardswish_nc_q8, 128, 0x1.0p+125f, 32, 1.0f, 3, 250, t);
  CHECK(t[0] == 3 && t[128] == 32 && t[255] == 250);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized, whatever the arguments */
  CHECK(qnnp_gfx950_create_multiply_nc_q8(0, 0, 0.0f, 0, 0.0f, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_create_hardswish_nc_q8(0, 0, 0.0f, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_create_hardsigmoid_nc_q8(0, 0, 0.0f, 0, 0.0f, 9, 1, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(NULL, 1, 1, NULL, 1, NULL, 1, NULL, 1) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  multiply_statuses();
  activation_statuses(qnnp_gfx950_create_hardswish_nc_q8, 0);
  activation_statuses(qnnp_gfx950_create_hardsigmoid_nc_q8, 1);
  tables();
  {
    /* channels, b rows, a rows per b row, extra stride bytes of a, b, product */
    const size_t shapes[6][6] = {{1, 1, 1, 0, 0, 0}, {17, 3, 5, 3, 9, 1}, {64, 2, 49, 0, 0, 0}, {5, 4, 1, 11, 0, 2},
                                 {16, 1, 7, 16, 0, 16}, {33, 5, 2, 0, 7, 0}};
    for (int k = 0; k < 6; k++) {
      for (int quarter = 0; quarter < 2; quarter++) {
        walk(shapes[k][0], shapes[k][1], shapes[k][2], shapes[k][3], shapes[k][4], shapes[k][5], quarter);
      }
    }
  }
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-mul-ok\n");
  return 0;
}
