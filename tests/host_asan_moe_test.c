/*
 * host_asan_moe_test.c -- TEST INFRASTRUCTURE: the host code of the top-k router and the weighted combine (moe.c) under
 * AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and tests/hip_stub_moe.c (Makefile target asan-moe;
 * run by tests/test_moe_host.py). Walks every create and setup status in the documented order, a launch whose stubbed kernel
 * touches both ends of every span it was handed (tensors allocated to the byte), a refused setup that leaves the last one
 * runnable, and delete. Prints "host-sanitizers-moe-ok" on success.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>
#include <qnnpack_gfx950_moe.h>

#include "hip/qnnp_hip.h"

void qnnp_stub_set_capturing(int on);
void qnnp_stub_set_device_pointers(int on);
size_t qnnp_stub_live_allocs(void);
extern struct qnnp_hip_topk_router_args qnnp_stub_router_last;
extern struct qnnp_hip_weighted_combine_args qnnp_stub_combine_last;
extern unsigned qnnp_stub_router_launches;
extern unsigned qnnp_stub_combine_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define INV qnnp_status_invalid_parameter
#define UNS qnnp_status_unsupported_parameter
#define OK qnnp_status_success

static void* device(size_t bytes)
{
  void* p = qnnp_hip_alloc(bytes);
  CHECK(p != NULL);
  memset(p, 0, bytes);
  return p;
}

static void router_walk(size_t e, size_t a, size_t tokens, size_t extra)
{
  qnnp_operator_t op = NULL, none = NULL;
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(0, 1, 0, 0, &none) == INV);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(e, 0, 0, 0, &none) == INV);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(e, e + 1, 0, 0, &none) == INV);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(4, 9, 0, 0, &none) == INV);          /* invalid before unsupported */
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(1025, 1, 0, 0, &none) == UNS);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(16, 9, 0, 0, &none) == UNS);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(e, a, UINT32_C(1) << 31, 0, &none) == UNS);
  qnnp_stub_set_capturing(1);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(e, a, 0, 0, &none) == INV);
  qnnp_stub_set_capturing(0);
  CHECK(none == NULL);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(e, a, 3, 0xFFFFFFFFu, &op) == OK && op != NULL);
  CHECK(qnnp_run_operator(op, NULL) == INV);                                       /* before setup */

  const size_t stride = e + extra, slots = tokens * a;
  float* logits = (float*) device(((tokens - 1) * stride + e) * sizeof(float));
  int32_t* ids = (int32_t*) device(slots * sizeof(int32_t));
  float* weights = (float*) device(slots * sizeof(float));
  float* host = (float*) malloc(slots * sizeof(float));
  CHECK(host != NULL);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, ids, weights) == OK);
  CHECK(qnnp_run_operator(op, NULL) == OK);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_topk_router") == 0);
  CHECK(qnnp_stub_router_last.logits == logits && qnnp_stub_router_last.group_ids == ids && qnnp_stub_router_last.weights == weights);
  CHECK(qnnp_stub_router_last.logits_stride == stride && qnnp_stub_router_last.tokens == tokens && qnnp_stub_router_last.groups == e);
  CHECK(qnnp_stub_router_last.assignments == a && qnnp_stub_router_last.first_group == 3 && ids[slots - 1] == -3);

  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(NULL, tokens, logits, stride, ids, weights) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, NULL, stride, ids, weights) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, NULL, weights) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, ids, NULL) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, ids, (float*) ((char*) weights + 2)) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, e - 1, ids, weights) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, ((size_t) 1 << 20) / a + 1, logits, stride, ids, weights) == UNS);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, SIZE_MAX / 2, logits, stride, ids, weights) == UNS);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, ids, (float*) ids) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, (int32_t*) logits, weights) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, ids, host) == INV);          /* host memory */
  qnnp_stub_set_capturing(1);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, logits, stride, ids, weights) == INV);
  qnnp_stub_set_capturing(0);
  const unsigned launches = qnnp_stub_router_launches;
  CHECK(qnnp_run_operator(op, NULL) == OK && qnnp_stub_router_launches == launches + 1);   /* the first setup stands */
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, 0, NULL, 0, NULL, NULL) == OK);
  CHECK(qnnp_run_operator(op, NULL) == OK && qnnp_stub_router_launches == launches + 1);
  CHECK(qnnp_delete_operator(op) == OK);
  qnnp_hip_free(logits);
  qnnp_hip_free(ids);
  qnnp_hip_free(weights);
  free(host);
}

static void combine_walk(size_t n, size_t a, size_t tokens, size_t extra_in, size_t extra_out)
{
  qnnp_operator_t op = NULL, none = NULL, router = NULL;
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(0, a, 4, 0, &none) == INV);
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(n, 0, 4, 0, &none) == INV);
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(n, a, 0, 0, &none) == INV);
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(0, 9, 4, 0, &none) == INV);     /* invalid before unsupported */
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(n, 9, 4, 0, &none) == UNS);
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(n, a, 1025, 0, &none) == UNS);
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32((size_t) 1 << 24, a, 4, 0, &none) == UNS);
  CHECK(none == NULL);
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(n, a, 4, 0, &op) == OK && op != NULL);
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(8, 2, 0, 0, &router) == OK);

  const size_t si = n + extra_in, so = n + extra_out, rows = tokens * a;
  float* x = (float*) device(((rows - 1) * si + n) * sizeof(float));
  float* y = (float*) device(((tokens - 1) * so + n) * sizeof(float));
  float* w = (float*) device(rows * sizeof(float));
  int32_t* ids = (int32_t*) device(rows * sizeof(int32_t));
  int32_t* host = (int32_t*) malloc(rows * sizeof(int32_t));
  CHECK(host != NULL);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, ids, y, so) == OK);
  CHECK(qnnp_run_operator(op, NULL) == OK);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_weighted_combine") == 0);
  CHECK(qnnp_stub_combine_last.input == x && qnnp_stub_combine_last.weights == w && qnnp_stub_combine_last.group_ids == ids);
  CHECK(qnnp_stub_combine_last.output == y && qnnp_stub_combine_last.input_stride == si && qnnp_stub_combine_last.output_stride == so);
  CHECK(qnnp_stub_combine_last.tokens == tokens && qnnp_stub_combine_last.assignments == a && qnnp_stub_combine_last.groups == 4);
  CHECK(qnnp_stub_combine_last.channels == n);

  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(router, tokens, x, si, w, ids, y, so) == INV);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(op, tokens, x, si, ids, w) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, NULL, ids, y, so) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, NULL, y, so) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, (int32_t*) ((char*) ids + 1), y, so) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, n - 1, w, ids, y, so) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, ids, y, n - 1) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, ((size_t) 1 << 20) / a + 1, x, si, w, ids, y, so) == UNS);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, ids, x, so) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, (const float*) y, ids, y, so) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, (const int32_t*) y, y, so) == INV);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, host, y, so) == INV);          /* host memory */
  qnnp_stub_set_capturing(1);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, tokens, x, si, w, ids, y, so) == INV);
  qnnp_stub_set_capturing(0);
  const unsigned launches = qnnp_stub_combine_launches;
  CHECK(qnnp_run_operator(op, NULL) == OK && qnnp_stub_combine_launches == launches + 1);   /* the first setup stands */
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(op, 0, NULL, 0, NULL, NULL, NULL, 0) == OK);
  CHECK(qnnp_run_operator(op, NULL) == OK && qnnp_stub_combine_launches == launches + 1);
  CHECK(qnnp_delete_operator(op) == OK);
  CHECK(qnnp_delete_operator(router) == OK);
  qnnp_hip_free(x);
  qnnp_hip_free(y);
  qnnp_hip_free(w);
  qnnp_hip_free(ids);
  free(host);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_topk_router_nc_f32(0, 0, 0, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_create_weighted_combine_nc_f32(0, 0, 0, 0, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_topk_router_nc_f32(NULL, 1, NULL, 1, NULL, NULL) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_weighted_combine_nc_f32(NULL, 1, NULL, 1, NULL, NULL, NULL, 1) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == OK);
  qnnp_stub_set_device_pointers(1);
  router_walk(1, 1, 1, 0);
  router_walk(65, 8, 3, 3);
  router_walk(1024, 8, 2, 0);
  combine_walk(1, 1, 1, 0, 0);
  combine_walk(33, 2, 5, 3, 1);
  combine_walk(260, 8, 3, 0, 4);
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == OK);
  printf("host-sanitizers-moe-ok\n");
  return 0;
}
