/*
 * host_asan_softargmax_test.c -- TEST INFRASTRUCTURE: the host code of the softargmax operator (softargmax.c) under
 * AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and tests/hip_stub_softargmax.c, whose launch
 * is a no-op (Makefile target asan-softargmax; run by tests/test_softargmax_host.py). Walks every status path of create
 * and setup, the table values at a few indices against constants (from the model of tests/_softargmax.py, which the CPU
 * tier pins to the compiled reference), the overlap checks, what reaches the launch, and delete; then the per-row
 * magic division of hip/softargmax_math.h against the plain division. Prints "host-sanitizers-softargmax-ok" on success.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "hip/softargmax_math.h"
#include "operator.h"

/* tests/hip_stub.c and tests/hip_stub_softargmax.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
size_t qnnp_stub_live_allocs(void);
extern struct qnnp_hip_softargmax_args qnnp_stub_softargmax_last;
extern long qnnp_stub_softargmax_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define FILL 0xA5

static const float S = 0x1.0p-8f;
static const float X = 0.176080093f;   /* the reference tester's input scale */

static uint8_t* filled(size_t n)
{
  uint8_t* p = (uint8_t*) malloc(n ? n : 1);
  CHECK(p != NULL);
  memset(p, FILL, n);
  return p;
}

/* the operator's table: the stub's "device" memory is host memory */
static const uint32_t* table_of(qnnp_operator_t op)
{
  return (const uint32_t*) op->d_weights;
}

static void statuses(void)
{
  qnnp_operator_t op = NULL;
  /* reference src/softargmax.c:36-70, in its order */
  CHECK(qnnp_create_softargmax_nc_q8(0, X, 0, S, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, 0.0f, 0, S, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, -1.0f, 0, S, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, 1.0e-40f, 0, S, 0, &op) == qnnp_status_invalid_parameter);   /* subnormal */
  CHECK(qnnp_create_softargmax_nc_q8(8, INFINITY, 0, S, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, NAN, 0, S, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 0, 0.0f, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 0, -S, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 0, INFINITY, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(0, X, 7, 0.5f, 0, &op) == qnnp_status_invalid_parameter);        /* invalid before unsupported */
  CHECK(qnnp_create_softargmax_nc_q8(8, 0.0f, 7, 0.5f, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 0, 0.5f, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 0, S * 2, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 1, S, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 255, 0.5f, 0, &op) == qnnp_status_unsupported_parameter);
  /* the product's own limit, after the reference's checks */
  CHECK(qnnp_create_softargmax_nc_q8((size_t) INT32_MAX + 1, X, 0, S, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(qnnp_create_softargmax_nc_q8((size_t) INT32_MAX + 1, 0.0f, 0, S, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(op == NULL);
  CHECK(qnnp_create_softargmax_nc_q8((size_t) INT32_MAX, X, 0, S, 0, &op) == qnnp_status_success && op != NULL);
  CHECK(table_of(op)[255] == 2 && table_of(op)[251] == 1 && table_of(op)[250] == 1 && table_of(op)[0] == 0);   /* 2^32 / (2^31 - 1) */
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;
  /* the table upload that fails (the allocation, then the copy): out_of_memory, nothing left allocated */
  const size_t live = qnnp_stub_live_allocs();
  for (long nth = 0; nth < 2; nth++) {
    qnnp_stub_fail_nth(nth);
    CHECK(qnnp_create_softargmax_nc_q8(8, X, 0, S, 0, &op) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(op == NULL && qnnp_stub_live_allocs() == live);
  }
  /* setup of a NULL operator and of an operator of another type */
  uint8_t* x = filled(64), * y = filled(64);
  CHECK(qnnp_setup_softargmax_nc_q8(NULL, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_create_add_nc_q8(8, 0, 1.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
  CHECK(qnnp_setup_softargmax_nc_q8(op, 1, x, 8, y, 8) == qnnp_status_invalid_parameter);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* a staging allocation that fails: out_of_memory, and the operator is not runnable */
  CHECK(qnnp_create_softargmax_nc_q8(8, X, 0, S, 0, &op) == qnnp_status_success);
  qnnp_stub_fail_nth(0);
  CHECK(qnnp_setup_softargmax_nc_q8(op, 4, x, 8, y, 8) == qnnp_status_out_of_memory);
  qnnp_stub_fail_nth(-1);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_softargmax_nc_q8(op, 4, x, 8, y, 8) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  free(x);
  free(y);
}

static void tables(void)
{
  qnnp_operator_t op = NULL;
  /* qscale = min((2^32 - 1) / channels, 8388607); table[i] = lrint(qscale * exp((i - 255) * scale)) */
  CHECK(qnnp_create_softargmax_nc_q8(1000, X, 0, S, 0, &op) == qnnp_status_success);
  const uint32_t* t = table_of(op);
  CHECK(t[255] == 4294967 && t[254] == 3601548 && t[250] == 1780766 && t[200] == 267 && t[128] == 0 && t[0] == 0);
  for (int i = 1; i < 256; i++) CHECK(t[i] >= t[i - 1]);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* 4096 channels: (2^32 - 1) / 4096 rounds to 2^20, so a constant row sums to 0 modulo 2^32 */
  CHECK(qnnp_create_softargmax_nc_q8(4096, 1.0f, 0, S, 0, &op) == qnnp_status_success);
  t = table_of(op);
  CHECK(t[255] == 1048576 && t[254] == 385750 && t[250] == 7065 && t[200] == 0 && t[0] == 0);
  CHECK((uint32_t) (t[255] * 4096u) == 0);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* one channel: the cap of 2^23 - 1; a small scale keeps the whole table alive */
  CHECK(qnnp_create_softargmax_nc_q8(1, 0.01f, 0, S, 0, &op) == qnnp_status_success);
  t = table_of(op);
  CHECK(t[255] == 8388607 && t[254] == 8305139 && t[250] == 7979490 && t[200] == 4839805 && t[128] == 2355786 && t[0] == 654996);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  /* a large scale: only the maximum survives */
  CHECK(qnnp_create_softargmax_nc_q8(21, 97.0f, 0, S, 0, &op) == qnnp_status_success);
  t = table_of(op);
  CHECK(t[255] == 8388607 && t[254] == 0 && t[0] == 0);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

/* create -> setup -> run -> rejected setups -> run -> in place -> batch 0, three rounds, then delete */
static void walk(size_t c, size_t extra_in, size_t extra_out)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_softargmax_nc_q8(c, X, 0, S, 0, &op) == qnnp_status_success && op != NULL);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  const size_t si = c + extra_in, so = c + extra_out;
  for (int round = 0; round < 3; round++) {
    const size_t n = 2 + 3 * (size_t) round;
    uint8_t* x = filled((n - 1) * si + c);                               /* exact spans: ASan catches any overrun */
    uint8_t* y = filled((n - 1) * so + c);
    long launches = qnnp_stub_softargmax_launches;
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x, si, y, so) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_softargmax") == 0);
    CHECK(qnnp_stub_softargmax_launches == launches + 1);
    CHECK(qnnp_stub_softargmax_last.rows == n && qnnp_stub_softargmax_last.channels == c);
    CHECK(qnnp_stub_softargmax_last.input_stride == si && qnnp_stub_softargmax_last.output_stride == so);
    CHECK(qnnp_stub_softargmax_last.table == table_of(op));
    /* host tensors are staged: the launch sees neither of them */
    CHECK(qnnp_stub_softargmax_last.input != x && qnnp_stub_softargmax_last.output != y);
    /* rejected setups before the operator changes: the previous setup stays runnable */
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, NULL, si, y, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x, si, NULL, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x, c - 1, y, so) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x, si, y, c - 1) == qnnp_status_invalid_parameter);
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x + 1, si, x, si) == qnnp_status_invalid_parameter);   /* shifted overlap */
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x, si, x, si + 1) == qnnp_status_invalid_parameter);   /* same base, other stride */
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x, si, x + (n - 1) * si + c - 1, si) == qnnp_status_invalid_parameter);   /* one shared byte */
    CHECK(qnnp_setup_softargmax_nc_q8(op, (size_t) INT32_MAX + 1, x, si, y, so) == qnnp_status_unsupported_parameter);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_softargmax_launches == launches + 2 && qnnp_stub_softargmax_last.rows == n);
    /* in place: the same tensor with equal strides */
    CHECK(qnnp_setup_softargmax_nc_q8(op, n, x, si, x, si) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_softargmax_last.input_stride == si && qnnp_stub_softargmax_last.output_stride == si);
    /* batch 0: a successful no-op, whatever the tensors */
    launches = qnnp_stub_softargmax_launches;
    CHECK(qnnp_setup_softargmax_nc_q8(op, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_softargmax_launches == launches);
    free(x);
    free(y);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static uint32_t next_random(uint64_t* state)
{
  *state = *state * UINT64_C(6364136223846793005) + UINT64_C(1442695040888963407);
  return (uint32_t) (*state >> 32);
}

/* hip/softargmax_math.h against the plain division: every numerator class the kernels can form, divisors over the
 * whole 32-bit range, tiny wrapped sums and powers of two and their neighbours included */
static void division(void)
{
  uint64_t state = 0x50F7A26;
  uint32_t divisors[4096];
  size_t nd = 0;
  for (uint32_t d = 1; d <= 1024; d++) divisors[nd++] = d;
  for (int b = 10; b < 32; b++) {
    for (int k = -2; k <= 2; k++) divisors[nd++] = (UINT32_C(1) << b) + (uint32_t) k;
  }
  for (int k = 0; k < 8; k++) divisors[nd++] = UINT32_MAX - (uint32_t) k;
  while (nd < 4096) divisors[nd++] = next_random(&state) >> (next_random(&state) % 32);
  for (size_t i = 0; i < nd; i++) {
    const uint32_t d = divisors[i] != 0 ? divisors[i] : 1;
    const struct qnnp_softargmax_divisor div = qnnp_softargmax_divisor_init(d);
    const uint32_t edge[] = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 255 * d, 256 * d - 1, 256 * d, UINT32_MAX, UINT32_MAX - 1,
                             UINT32_C(0x80000000), UINT32_C(0x7FFFFFFF)};
    for (size_t k = 0; k < sizeof(edge) / sizeof(edge[0]); k++) CHECK(qnnp_softargmax_divide(edge[k], div) == edge[k] / d);
    for (int k = 0; k < 256; k++) {
      const uint32_t n = next_random(&state);
      CHECK(qnnp_softargmax_divide(n, div) == n / d);
      const uint32_t t = next_random(&state) >> 9;   /* a table entry: below 2^23 */
      const uint32_t q = ((t << 8) + (d >> 1)) / d;
      CHECK(qnnp_softargmax_normalize(t, d >> 1, div) == (q > 255 ? 255 : q));
    }
  }
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized (reference softargmax.c:31-34, 114-117), whatever the arguments */
  CHECK(qnnp_create_softargmax_nc_q8(0, 0.0f, 9, 0.0f, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_setup_softargmax_nc_q8(NULL, 1, NULL, 1, NULL, 1) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  statuses();
  tables();
  walk(1, 0, 0);
  walk(21, 3, 9);
  walk(1000, 0, 0);
  walk(5, 11, 0);
  /* inside a graph capture (tests/hip_stub.c) create and setup refuse with invalid_parameter and allocate nothing */
  {
    qnnp_operator_t none = NULL;
    CHECK(qnnp_create_softargmax_nc_q8(16, X, 0, S, 0, &op) == qnnp_status_success);
    uint8_t* x = filled(5 * 16), * y = filled(5 * 16);
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_create_softargmax_nc_q8(16, X, 0, S, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(none == NULL);
    CHECK(qnnp_setup_softargmax_nc_q8(op, 5, x, 16, y, 16) == qnnp_status_invalid_parameter);
    CHECK(qnnp_stub_live_allocs() == live);
    qnnp_stub_set_capturing(0);
    CHECK(qnnp_setup_softargmax_nc_q8(op, 5, x, 16, y, 16) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    free(x);
    free(y);
    CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  }
  division();
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-softargmax-ok\n");
  return 0;
}
