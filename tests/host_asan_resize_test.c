/*
 * host_asan_resize_test.c -- TEST INFRASTRUCTURE: the host code of the bilinear resize operator (resize-bilinear.c with
 * resize-table.h) under AddressSanitizer + UndefinedBehaviorSanitizer, against tests/hip_stub.c and
 * tests/hip_stub_resize.c (Makefile target asan-resize; run by tests/test_resize_host.py). Walks create -> setup -> run ->
 * re-setup (larger, then smaller: the table grows and is reused) -> delete, every create and setup status in the
 * documented order, a refused setup that leaves the last one runnable, failing allocations, and the hand values of the
 * definition through the stubbed launch, which computes from the tables the setup uploaded. Prints
 * "host-sanitizers-resize-ok" on success.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"

/* tests/hip_stub.c and tests/hip_stub_resize.c test controls */
void qnnp_stub_set_capturing(int on);
void qnnp_stub_fail_nth(long n);
size_t qnnp_stub_live_allocs(void);
extern struct qnnp_hip_resize_args qnnp_stub_resize_last;
extern unsigned qnnp_stub_resize_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
#define FILL 0xA5
#define ALIGN QNNP_GFX950_RESIZE_ALIGN_CORNERS

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

/* the definition, straight from the header, for one axis */
static void axis(uint64_t n_in, uint64_t n_out, int align, uint64_t o, uint64_t* i0, uint64_t* i1, uint32_t* w)
{
  uint64_t f;
  if (align) {
    f = n_out == 1 ? 0 : (4096 * o * (n_in - 1) + (n_out - 1)) / (2 * (n_out - 1));
  } else {
    const int64_t num = (int64_t) ((2 * o + 1) * n_in) - (int64_t) n_out;
    f = (4096 * (uint64_t) (num > 0 ? num : 0) + 2 * n_out) / (4 * n_out);
  }
  *i0 = f >> 11 < n_in - 1 ? f >> 11 : n_in - 1;
  *i1 = *i0 + 1 < n_in - 1 ? *i0 + 1 : n_in - 1;
  *w = *i0 == *i1 ? 0 : (uint32_t) (f & 2047);
}

static void check_resized(const uint8_t* x, const uint8_t* y, size_t batch, size_t ih, size_t iw, size_t oh, size_t ow,
                          size_t c, size_t sx, size_t sy, int align)
{
  for (size_t n = 0; n < batch; n++) {
    for (size_t oy = 0; oy < oh; oy++) {
      uint64_t y0, y1, x0, x1;
      uint32_t wy, wx;
      axis(ih, oh, align, oy, &y0, &y1, &wy);
      for (size_t ox = 0; ox < ow; ox++) {
        axis(iw, ow, align, ox, &x0, &x1, &wx);
        const size_t pixel = (n * oh + oy) * ow + ox;
        for (size_t k = 0; k < c; k++) {
          const uint32_t top = x[((n * ih + y0) * iw + x0) * sx + k] * (2048u - wx) + x[((n * ih + y0) * iw + x1) * sx + k] * wx;
          const uint32_t bot = x[((n * ih + y1) * iw + x0) * sx + k] * (2048u - wx) + x[((n * ih + y1) * iw + x1) * sx + k] * wx;
          CHECK(y[pixel * sy + k] == (uint8_t) ((top * (2048u - wy) + bot * wy + (1u << 21)) >> 22));
        }
        if (pixel + 1 < batch * oh * ow) for (size_t k = c; k < sy; k++) CHECK(y[pixel * sy + k] == FILL);
      }
    }
  }
}

static void run_case(qnnp_operator_t op, size_t batch, size_t ih, size_t iw, size_t oh, size_t ow, size_t c, size_t ex,
                     size_t ey, int align)
{
  const size_t sx = c + ex, sy = c + ey;
  /* exact spans: ASan catches any overrun */
  uint8_t* x = bytes((batch * ih * iw - 1) * sx + c, (unsigned) (ih * 7 + ow));
  uint8_t* y = filled((batch * oh * ow - 1) * sy + c);
  const unsigned launches = qnnp_stub_resize_launches;
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, batch, ih, iw, oh, ow, x, sx, y, sy) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(strcmp(qnnp_gfx950_operator_kernel(op), "stub_resize") == 0);
  CHECK(qnnp_stub_resize_launches == launches + 1);
  CHECK(qnnp_stub_resize_last.batch == batch && qnnp_stub_resize_last.channels == c);
  CHECK(qnnp_stub_resize_last.input_height == ih && qnnp_stub_resize_last.input_width == iw);
  CHECK(qnnp_stub_resize_last.output_height == oh && qnnp_stub_resize_last.output_width == ow);
  CHECK(qnnp_stub_resize_last.input_stride == sx && qnnp_stub_resize_last.output_stride == sy);
  /* host tensors: both are staged, neither is the caller's pointer */
  CHECK(qnnp_stub_resize_last.input != x && qnnp_stub_resize_last.output != y);
  check_resized(x, y, batch, ih, iw, oh, ow, c, sx, sy, align);
  free(x);
  free(y);
}

static void walk(size_t c, size_t ex, size_t ey, int align)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(c, align ? ALIGN : 0, &op) == qnnp_status_success);
  CHECK(op != NULL);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);   /* before setup */
  run_case(op, 2, 3, 5, 7, 4, c, ex, ey, align);
  const size_t live = qnnp_stub_live_allocs();
  run_case(op, 3, 5, 4, 29, 16, c, ex, ey, align);     /* larger: the table and the staging grow */
  run_case(op, 1, 7, 2, 2, 3, c, ex, ey, align);       /* smaller: both are reused */
  run_case(op, 1, 1, 1, 4, 1, c, ex, ey, align);
  CHECK(qnnp_stub_resize_last.streaming_mode == 0);
  CHECK(qnnp_gfx950_operator_set_streaming_stores(op, 1) == qnnp_status_success);
  run_case(op, 2, 4, 4, 4, 4, c, ex, ey, align);       /* equal sizes */
  CHECK(qnnp_stub_resize_last.streaming_mode == 2);
  CHECK(qnnp_stub_live_allocs() == live);              /* grow-only: replaced, never added */
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void hand_values(void)
{
  const uint8_t x[4] = {0, 60, 120, 180};
  const uint8_t want4[16] = {0, 15, 45, 60, 30, 45, 75, 90, 90, 105, 135, 150, 120, 135, 165, 180};
  const uint8_t want3[9] = {0, 30, 60, 60, 90, 120, 120, 150, 180};
  uint8_t y[16];
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(1, 0, &op) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 1, 2, 2, 4, 4, x, 1, y, 1) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(memcmp(y, want4, 16) == 0);
  /* the identity */
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 1, 2, 2, 2, 2, x, 1, y, 1) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(memcmp(y, x, 4) == 0);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(1, ALIGN, &op) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 1, 2, 2, 3, 3, x, 1, y, 1) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  CHECK(memcmp(y, want3, 9) == 0);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void statuses(void)
{
  qnnp_operator_t op = NULL;
  /* create, in the documented order */
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(0, 0, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(0, 2, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(8, 2, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(8, 0x80000001u, &op) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8((size_t) INT32_MAX + 1, 2, &op) == qnnp_status_invalid_parameter);   /* invalid before unsupported */
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8((size_t) INT32_MAX + 1, 0, &op) == qnnp_status_unsupported_parameter);
  CHECK(op == NULL);
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8((size_t) INT32_MAX, ALIGN, &op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  op = NULL;

  const size_t c = 8;
  uint8_t* x = bytes(4096, 3);
  uint8_t* y = filled(4096);
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(c, 0, &op) == qnnp_status_success);
  /* batch 0: success and run does nothing, whatever the rest */
  {
    const unsigned before = qnnp_stub_resize_launches;
    CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 0, 0, 0, 0, 0, NULL, 0, NULL, 0) == qnnp_status_success);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(qnnp_stub_resize_launches == before);
  }
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 2, 3, 4, 5, 6, x, c, y, c + 3) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  check_resized(x, y, 2, 3, 4, 5, 6, c, c, c + 3, 0);
  uint8_t* keep = (uint8_t*) malloc(4096);
  CHECK(keep != NULL);
  memcpy(keep, y, 4096);
  const size_t big = (size_t) 1 << 24;
  const struct { size_t n, ih, iw, oh, ow; const uint8_t* x; size_t sx; uint8_t* y; size_t sy; enum qnnp_status want; } refused[] = {
    {2, 0, 4, 5, 6, x, c, y, c, qnnp_status_invalid_parameter},
    {2, 3, 0, 5, 6, x, c, y, c, qnnp_status_invalid_parameter},
    {2, 3, 4, 0, 6, x, c, y, c, qnnp_status_invalid_parameter},
    {2, 3, 4, 5, 0, x, c, y, c, qnnp_status_invalid_parameter},
    {2, 0, big, 5, 6, x, c, y, c, qnnp_status_invalid_parameter},      /* invalid before unsupported */
    {2, 3, 4, 5, 6, NULL, c, y, c, qnnp_status_invalid_parameter},
    {2, 3, 4, 5, 6, x, c, NULL, c, qnnp_status_invalid_parameter},
    {2, big, 4, 5, 6, NULL, c, y, c, qnnp_status_invalid_parameter},
    {2, 3, 4, 5, 6, x, c - 1, y, c, qnnp_status_invalid_parameter},
    {2, 3, 4, 5, 6, x, c, y, c - 1, qnnp_status_invalid_parameter},
    {2, 3, 4, 5, 6, x, 0, y, c, qnnp_status_invalid_parameter},
    {2, big, 4, 5, 6, x, c, y, c, qnnp_status_unsupported_parameter},
    {2, 3, big, 5, 6, x, c, y, c, qnnp_status_unsupported_parameter},
    {2, 3, 4, big, 6, x, c, y, c, qnnp_status_unsupported_parameter},
    {2, 3, 4, 5, big, x, c, y, c, qnnp_status_unsupported_parameter},
    {2, 3, 4, SIZE_MAX, SIZE_MAX, x, c, y, c, qnnp_status_unsupported_parameter},
    {(size_t) 1 << 31, 1, 1, 1, 1, x, c, y, c, qnnp_status_unsupported_parameter},
    {SIZE_MAX, big - 1, big - 1, 1, 1, x, c, y, c, qnnp_status_unsupported_parameter},
    {129, 1, 1, big - 1, 1, x, c, y, c, qnnp_status_unsupported_parameter},            /* 129 * (2^24 - 1) > 2^31 output pixels */
    {1, 1, 1, 32768, 65536, x, c, y, c, qnnp_status_unsupported_parameter},            /* 2^31 output pixels */
    {1, 65536, 32768, 1, 1, x, c, y, c, qnnp_status_unsupported_parameter},            /* 2^31 input pixels */
    /* overlaps: the same base, the output inside the input, the input inside the output, one shared byte */
    {2, 3, 4, 5, 6, x, c, (uint8_t*) x, c, qnnp_status_invalid_parameter},
    {2, 3, 4, 1, 1, x, c, (uint8_t*) x + 40, c, qnnp_status_invalid_parameter},
    {1, 1, 1, 5, 6, x + 40, c, (uint8_t*) x, c, qnnp_status_invalid_parameter},
    {2, 3, 4, 5, 6, x, c, (uint8_t*) x + 24 * c - 1, c, qnnp_status_invalid_parameter},
  };
  for (size_t i = 0; i < sizeof(refused) / sizeof(refused[0]); i++) {
    /* a refused setup leaves the last one runnable */
    CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, refused[i].n, refused[i].ih, refused[i].iw, refused[i].oh,
        refused[i].ow, refused[i].x, refused[i].sx, refused[i].y, refused[i].sy) == refused[i].want);
    memset(y, FILL, 4096);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(memcmp(y, keep, 4096) == 0);
  }
  /* the output directly behind the input is accepted */
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 2, 3, 4, 5, 6, x, c, x + 24 * c, c) == qnnp_status_success);
  CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
  check_resized(x, x + 24 * c, 2, 3, 4, 5, 6, c, c, c, 0);

  /* allocations and copies that fail, each on a geometry LARGER than any before: the table's allocation, the table's copy,
   * the input's staging buffer. out_of_memory each time, and the operator is not runnable until the next good setup */
  for (long nth = 0; nth < 3; nth++) {
    qnnp_stub_fail_nth(nth);
    CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 2, 6, 8, 10 + (size_t) nth * 8, 12, x, c, y, c) == qnnp_status_out_of_memory);
    qnnp_stub_fail_nth(-1);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_invalid_parameter);
    CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 2, 3, 4, 5, 6, x, c, y, c + 3) == qnnp_status_success);
    memset(y, FILL, 4096);
    CHECK(qnnp_run_operator(op, NULL) == qnnp_status_success);
    CHECK(memcmp(y, keep, 4096) == 0);
  }

  /* setups of other kinds */
  qnnp_operator_t add = NULL;
  CHECK(qnnp_create_add_nc_q8(c, 0, 1.0f, 0, 1.0f, 0, 1.0f, 0, 255, 0, &add) == qnnp_status_success);
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(add, 2, 3, 4, 5, 6, x, c, y, c) == qnnp_status_invalid_parameter);
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(NULL, 2, 3, 4, 5, 6, x, c, y, c) == qnnp_status_invalid_parameter);
  CHECK(qnnp_setup_add_nc_q8(op, 1, x, c, x, c, y, c) == qnnp_status_invalid_parameter);
  /* inside a graph capture create and setup refuse and allocate nothing */
  {
    qnnp_operator_t none = NULL;
    const size_t live = qnnp_stub_live_allocs();
    qnnp_stub_set_capturing(1);
    CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(c, 0, &none) == qnnp_status_invalid_parameter);
    CHECK(none == NULL);
    CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(op, 2, 3, 4, 5, 6, x, c, y, c) == qnnp_status_invalid_parameter);
    CHECK(qnnp_stub_live_allocs() == live);
    qnnp_stub_set_capturing(0);
  }
  float ms = -1.0f;
  CHECK(qnnp_gfx950_time_operator(op, 1, 2, &ms) == qnnp_status_invalid_parameter);   /* host pointers cannot be timed */
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
  CHECK(qnnp_delete_operator(add) == qnnp_status_success);
  free(keep);
  free(x);
  free(y);
}

int main(void)
{
  qnnp_operator_t op = NULL;
  /* before qnnp_initialize: uninitialized, whatever the arguments */
  CHECK(qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(0, 2, &op) == qnnp_status_uninitialized);
  CHECK(qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(NULL, 1, 0, 0, 0, 0, NULL, 0, NULL, 0) == qnnp_status_uninitialized);
  CHECK(op == NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  statuses();
  hand_values();
  {
    /* channels, extra stride bytes of the input and the output */
    const size_t shapes[5][3] = {{1, 0, 0}, {3, 0, 0}, {5, 3, 7}, {16, 16, 0}, {21, 0, 2}};
    for (int k = 0; k < 5; k++) {
      for (int align = 0; align < 2; align++) walk(shapes[k][0], shapes[k][1], shapes[k][2], align);
    }
  }
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("host-sanitizers-resize-ok\n");
  return 0;
}
