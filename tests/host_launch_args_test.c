/*
 * host_launch_args_test.c -- TEST INFRASTRUCTURE: records what every operator of the host tier hands to its kernel entry
 * point. The host code runs against tests/hip_stub.c (+ hip_stub_lut.c, hip_stub_mul.c) under AddressSanitizer +
 * UndefinedBehaviorSanitizer (Makefile target asan-launch-args; run by tests/test_launch_args_host.py); the stub's launch
 * log writes one line per *_run call -- every field of the argument block, pointers by name -- to the file named by
 * argv[1], and this program adds a heading per case and the status of every run. The list of operators is fixed and
 * the log has no addresses in it, so it is the same text from run to run: tests/golden/launch_args.txt, recorded from
 * the run path as it was before the operators got their own launch functions. Each case runs on host tensors (staged
 * through the device) and again on tensors the stub counts as device memory. Prints "launch-args-ok" on success.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>
#include <qnnpack_gfx950_perchannel.h>
#include <qnnpack_gfx950_test.h>

#include "hip/qnnp_hip.h"
#include "operator.h"   /* (qnnpack_amd/csrc: ran_dense) */

/* tests/hip_stub.c and tests/hip_stub_mul.c test controls */
void qnnp_stub_log_to(FILE* file);
void qnnp_stub_log_tensor(int slot, const char* name, const void* base, size_t bytes);
void qnnp_stub_name_pointer(const void* p, char* text, size_t size);
void qnnp_stub_set_device_pointers(int on);
void qnnp_stub_refuse_igemm_variant(int variant);
size_t qnnp_stub_live_allocs(void);
extern struct qnnp_hip_mul_args qnnp_stub_mul_last;
extern unsigned qnnp_stub_mul_launches;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

enum { IN, IN2, OUT, RESIDUAL };
static const char* const slot_names[4] = {"in", "in2", "out", "residual"};
static FILE* log_file;

static void fill(uint8_t* p, size_t n, unsigned salt)
{
  for (size_t i = 0; i < n; i++) p[i] = (uint8_t) (i * 37u + 11u + salt * 101u + (i >> 8));
}

static uint8_t* weights(size_t n, unsigned salt)
{
  uint8_t* p = (uint8_t*) malloc(n);
  CHECK(p != NULL);
  fill(p, n, salt);
  return p;
}

static int32_t* biases(size_t n)
{
  int32_t* p = (int32_t*) malloc(sizeof(int32_t) * n);
  CHECK(p != NULL);
  for (size_t i = 0; i < n; i++) p[i] = (int32_t) (i * 79u) - 1000;
  return p;
}

/* a tensor in host memory, or one the stub counts as device memory; registered with the log under the slot's name */
static uint8_t* tensor(int slot, size_t bytes, int device)
{
  uint8_t* p = (uint8_t*) (device ? qnnp_hip_alloc(bytes) : malloc(bytes));
  CHECK(p != NULL);
  fill(p, bytes, (unsigned) slot);
  qnnp_stub_log_tensor(slot, slot_names[slot], p, bytes);
  return p;
}

static void release(int slot, uint8_t* p, int device)
{
  qnnp_stub_log_tensor(slot, slot_names[slot], NULL, 0);
  if (device) qnnp_hip_free(p); else free(p);
}

static void heading(const char* name, int device)
{
  fprintf(log_file, "== %s [%s]\n", name, device ? "device" : "host");
  qnnp_stub_set_device_pointers(device);
}

static void run(qnnp_operator_t op)
{
  const enum qnnp_status status = qnnp_run_operator(op, NULL);
  const char* kernel = qnnp_gfx950_operator_kernel(op);
  fprintf(log_file, "   run: status=%d kernel=%s ran_dense=%u residual_folded=%d\n", (int) status,
      kernel != NULL ? kernel : "none", (unsigned) op->ran_dense, qnnp_gfx950_operator_residual_folded(op));
}

static void option(const char* key, int value)
{
  CHECK(qnnp_gfx950_test_force_kernel(key, value) == qnnp_status_success);
}

/* ---- convolutions ------------------------------------------------------------------------------------------------ */
struct conv {
  uint32_t pad, k, stride, groups;
  size_t gic, goc;
  uint8_t kzp;
  int per_channel;
};

static qnnp_operator_t create_conv(const struct conv* c)
{
  const size_t cout = c->groups * c->goc;
  uint8_t* kernel = weights(cout * c->k * c->k * c->gic, 5);
  if (c->gic == 1 && c->goc == 1) {
    for (size_t i = 0; i < cout * c->k * c->k; i++) kernel[i] = (uint8_t) (c->kzp - 50 + kernel[i] % 100);   /* w - kzp fits int8 */
  }
  int32_t* bias = biases(cout);
  float* scales = (float*) malloc(sizeof(float) * cout);
  CHECK(scales != NULL);
  for (size_t i = 0; i < cout; i++) scales[i] = 0.25f + 0.015625f * (float) (i % 16);
  qnnp_operator_t op = NULL;
  if (c->per_channel) {
    CHECK(qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(c->pad, c->pad, c->pad, c->pad, c->k, c->k, c->stride,
        c->stride, 1, 1, c->groups, c->gic, c->goc, 121, 0.5f, c->kzp, scales, kernel, bias, 130, 0.75f, 3, 250, 0, &op) ==
        qnnp_status_success);
  } else {
    CHECK(qnnp_create_convolution2d_nhwc_q8(c->pad, c->pad, c->pad, c->pad, c->k, c->k, c->stride, c->stride, 1, 1,
        c->groups, c->gic, c->goc, 121, 0.5f, c->kzp, 0.5f, kernel, bias, 130, 0.75f, 3, 250, 0, &op) == qnnp_status_success);
  }
  free(kernel);
  free(bias);
  free(scales);
  return op;
}

static qnnp_operator_t create_add(size_t channels)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_add_nc_q8(channels, 121, 0.75f, 127, 1.25f, 133, 0.96875f, 2, 251, 0, &op) == qnnp_status_success);
  return op;
}

/* setup under "gemm_kernel" / "dwconv_kernel" = `forced`, [attach a residual add,] run; on host tensors and on device
 * tensors (with a residual: device tensors only, attach takes no others) */
static void conv_case(const char* name, qnnp_operator_t op, const struct conv* c, size_t batch, size_t h, size_t w,
                      size_t in_extra, size_t out_extra, int forced, int with_residual)
{
  const size_t cin = c->groups * c->gic, cout = c->groups * c->goc;
  const size_t oh = (h + 2 * c->pad - c->k) / c->stride + 1, ow = (w + 2 * c->pad - c->k) / c->stride + 1;
  const size_t in_stride = cin + in_extra, out_stride = cout + out_extra, res_stride = cout + 3;
  for (int device = with_residual ? 1 : 0; device < 2; device++) {
    heading(name, device);
    uint8_t* in = tensor(IN, (batch * h * w - 1) * in_stride + cin, device);
    uint8_t* out = tensor(OUT, (batch * oh * ow - 1) * out_stride + cout, device);
    option("gemm_kernel", forced);
    CHECK(qnnp_setup_convolution2d_nhwc_q8(op, batch, h, w, in, in_stride, out, out_stride, NULL) == qnnp_status_success);
    option("gemm_kernel", 0);
    uint8_t* residual = NULL;
    if (with_residual) {
      qnnp_operator_t add = create_add(cout);
      residual = tensor(RESIDUAL, (batch * oh * ow - 1) * res_stride + cout, 1);
      CHECK(qnnp_gfx950_attach_residual_add(op, add, residual, res_stride) == qnnp_status_success);
      CHECK(qnnp_delete_operator(add) == qnnp_status_success);
    }
    run(op);
    run(op);   /* (depthwise: the second run finds the plan the first one left) */
    if (with_residual) release(RESIDUAL, residual, 1);
    release(IN, in, device);
    release(OUT, out, device);
  }
}

static void conv_once(const char* name, const struct conv* c, size_t batch, size_t h, size_t w, size_t in_extra,
                      size_t out_extra, int forced, int with_residual)
{
  qnnp_operator_t op = create_conv(c);
  conv_case(name, op, c, batch, h, w, in_extra, out_extra, forced, with_residual);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void fully_connected(void)
{
  uint8_t* kernel = weights(8 * 16, 6);
  int32_t* bias = biases(8);
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_fully_connected_nc_q8(16, 8, 121, 0.5f, 127, 0.5f, kernel, bias, 130, 0.75f, 3, 250, 0, &op) == qnnp_status_success);
  free(kernel);
  free(bias);
  for (int device = 0; device < 2; device++) {
    heading("fully connected 16 -> 8, batch 3", device);
    uint8_t* in = tensor(IN, 2 * 19 + 16, device);
    uint8_t* out = tensor(OUT, 2 * 9 + 8, device);
    CHECK(qnnp_setup_fully_connected_nc_q8(op, 3, in, 19, out, 9) == qnnp_status_success);
    run(op);
    release(IN, in, device);
    release(OUT, out, device);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

/* ---- deconvolutions ---------------------------------------------------------------------------------------------- */
static void deconv_case(const char* name, uint32_t k, uint32_t stride, uint32_t pad, uint32_t groups, size_t gic, size_t goc,
                        int forced, int refused_variant)
{
  const size_t h = 2, w = 3, cin = groups * gic, cout = groups * goc;
  const size_t oh = stride * (h - 1) + k - 2 * pad, ow = stride * (w - 1) + k - 2 * pad;
  uint8_t* kernel = weights(groups * gic * k * k * goc, 7);
  int32_t* bias = biases(cout);
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_deconvolution2d_nhwc_q8(pad, pad, pad, pad, 0, 0, k, k, stride, stride, 1, 1, groups, gic, goc,
      121, 0.5f, 127, 0.5f, kernel, bias, 130, 0.75f, 3, 250, 0, &op) == qnnp_status_success);
  free(kernel);
  free(bias);
  for (int device = 0; device < 2; device++) {
    heading(name, device);
    uint8_t* in = tensor(IN, (2 * h * w - 1) * (cin + 1) + cin, device);
    uint8_t* out = tensor(OUT, (2 * oh * ow - 1) * (cout + 2) + cout, device);
    option("gemm_kernel", forced);
    CHECK(qnnp_setup_deconvolution2d_nhwc_q8(op, 2, h, w, in, cin + 1, out, cout + 2, NULL) == qnnp_status_success);
    option("gemm_kernel", 0);
    qnnp_stub_refuse_igemm_variant(refused_variant);
    run(op);
    qnnp_stub_refuse_igemm_variant(-1);
    release(IN, in, device);
    release(OUT, out, device);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

/* ---- add, global average pooling, multiply ------------------------------------------------------------------------ */
static void add_case(const char* name, int device, int device_b)
{
  qnnp_operator_t op = create_add(8);
  heading(name, device);
  uint8_t* a = tensor(IN, 4 * 11 + 8, device);
  uint8_t* b = tensor(IN2, 4 * 9 + 8, device_b);
  uint8_t* sum = tensor(OUT, 4 * 10 + 8, device);
  CHECK(qnnp_setup_add_nc_q8(op, 5, a, 11, b, 9, sum, 10) == qnnp_status_success);
  run(op);
  release(IN, a, device);
  release(IN2, b, device_b);
  release(OUT, sum, device);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void global_average_pooling(void)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_create_global_average_pooling_nwc_q8(8, 121, 1.0f, 133, 1.0f, 3, 250, 0, &op) == qnnp_status_success);
  for (int device = 0; device < 2; device++) {
    heading("global average pooling, 2 x 4 pixels x 8 channels", device);
    uint8_t* in = tensor(IN, (2 * 4 - 1) * 9 + 8, device);
    uint8_t* out = tensor(OUT, 10 + 8, device);
    CHECK(qnnp_setup_global_average_pooling_nwc_q8(op, 2, 4, in, 9, out, 10) == qnnp_status_success);
    run(op);
    release(IN, in, device);
    release(OUT, out, device);
  }
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

static void multiply_case(const char* name, int device, int device_b)
{
  qnnp_operator_t op = NULL;
  CHECK(qnnp_gfx950_create_multiply_nc_q8(8, 128, 1.0f, 121, 0.5f, 128, 1.0f, 0, 255, 0, &op) == qnnp_status_success);
  heading(name, device);
  uint8_t* a = tensor(IN, 5 * 9 + 8, device);
  uint8_t* b = tensor(IN2, 1 * 10 + 8, device_b);
  uint8_t* product = tensor(OUT, 5 * 11 + 8, device);
  CHECK(qnnp_gfx950_setup_multiply_nc_q8(op, 2, 3, a, 9, b, 10, product, 11) == qnnp_status_success);
  const unsigned launches = qnnp_stub_mul_launches;
  run(op);
  const struct qnnp_hip_mul_args* m = &qnnp_stub_mul_last;
  char pa[48], pb[48], pp[48];
  qnnp_stub_name_pointer(m->a, pa, sizeof(pa));
  qnnp_stub_name_pointer(m->b, pb, sizeof(pb));
  qnnp_stub_name_pointer(m->product, pp, sizeof(pp));
  fprintf(log_file, "   qnnp_hip_mul_run x %u: a=%s b=%s product=%s b_rows=%u a_rows_per_b_row=%u channels=%u a_stride=%llu "
      "b_stride=%llu product_stride=%llu a_zero_point=%d b_zero_point=%d rq.multiplier=%d rq.shift=%u "
      "rq.accumulator_bits=%u streaming_mode=%u\n", qnnp_stub_mul_launches - launches, pa, pb, pp, m->b_rows,
      m->a_rows_per_b_row, m->channels, (unsigned long long) m->a_stride, (unsigned long long) m->b_stride,
      (unsigned long long) m->product_stride, m->a_zero_point, m->b_zero_point, m->rq.multiplier, m->rq.shift,
      m->rq.accumulator_bits, m->streaming_mode);
  release(IN, a, device);
  release(IN2, b, device_b);
  release(OUT, product, device);
  CHECK(qnnp_delete_operator(op) == qnnp_status_success);
}

/* ---- fused block: 8 -> 32 expand, 3x3 depthwise, 32 -> 8 project, + input ------------------------------------------- */
static void fused_blocks(void)
{
  const struct conv expand_c = {0, 1, 1, 1, 8, 32, 127, 0}, dw_c = {1, 3, 1, 32, 1, 1, 128, 0}, project_c = {0, 1, 1, 1, 32, 8, 127, 0};
  qnnp_operator_t expand = create_conv(&expand_c), dw = create_conv(&dw_c), project = create_conv(&project_c);
  qnnp_operator_t add = create_add(8), fused = NULL;
  CHECK(qnnp_gfx950_create_fused_block(expand, dw, project, add, &fused) == qnnp_status_success);
  for (int kernel = 0; kernel < 2; kernel++) {
    for (int device = 0; device < 2; device++) {
      heading(kernel == 0 ? "fused block, strip kernel" : "fused block, tile kernel (\"fused_kernel\" 1)", device);
      uint8_t* in = tensor(IN, (2 * 4 * 5 - 1) * 9 + 8, device);
      uint8_t* out = tensor(OUT, (2 * 4 * 5 - 1) * 10 + 8, device);
      option("fused_kernel", kernel);
      CHECK(qnnp_gfx950_setup_fused_block(fused, 2, 4, 5, in, 9, out, 10) == qnnp_status_success);
      option("fused_kernel", 0);
      run(fused);
      release(IN, in, device);
      release(OUT, out, device);
    }
  }
  qnnp_operator_t ops[] = {fused, expand, dw, project, add};
  for (size_t i = 0; i < sizeof(ops) / sizeof(ops[0]); i++) CHECK(qnnp_delete_operator(ops[i]) == qnnp_status_success);
}

/* ---- timing: two input / output sets, warmup 1, iters 3; the stub refuses graphs, so this is the plain loop -------- */
static void timed(const char* name, qnnp_operator_t op, uint8_t* in, size_t in_set, uint8_t* out, size_t out_set)
{
  const void* inputs[2] = {in, in + in_set};
  void* outputs[2] = {out, out + out_set};
  float ms = -1.0f;
  fprintf(log_file, "   %s:\n", name);
  const enum qnnp_status status = qnnp_gfx950_time_operator_rotating(op, 2, inputs, outputs, 1, 3, &ms);
  fprintf(log_file, "   timed: status=%d residual_folded=%d\n", (int) status, qnnp_gfx950_operator_residual_folded(op));
}

static void timing(void)
{
  const struct conv c = {1, 3, 1, 1, 8, 8, 121, 0};
  qnnp_operator_t conv = create_conv(&c), add = create_add(8);
  heading("timing, two rotating sets", 1);
  {
    const size_t set = 64 * 8;   /* 1 x 8 x 8 pixels of 8 channels */
    uint8_t* in = tensor(IN, 2 * set, 1);
    uint8_t* out = tensor(OUT, 2 * set, 1);
    uint8_t* residual = tensor(RESIDUAL, set, 1);
    CHECK(qnnp_setup_convolution2d_nhwc_q8(conv, 1, 8, 8, in, 8, out, 8, NULL) == qnnp_status_success);
    timed("convolution 3x3 8 -> 8", conv, in, set, out, set);
    CHECK(qnnp_gfx950_attach_residual_add(conv, add, residual, 8) == qnnp_status_success);
    timed("the same with a residual add attached", conv, in, set, out, set);
    release(IN, in, 1);
    release(OUT, out, 1);
    release(RESIDUAL, residual, 1);
  }
  {
    uint8_t* a = tensor(IN, 2 * 64, 1);
    uint8_t* b = tensor(IN2, 4 * 9 + 8, 1);
    uint8_t* sum = tensor(OUT, 2 * 64, 1);
    CHECK(qnnp_setup_add_nc_q8(add, 5, a, 11, b, 9, sum, 10) == qnnp_status_success);
    timed("add", add, a, 64, sum, 64);
    release(IN, a, 1);
    release(IN2, b, 1);
    release(OUT, sum, 1);
  }
  CHECK(qnnp_delete_operator(conv) == qnnp_status_success);
  CHECK(qnnp_delete_operator(add) == qnnp_status_success);
}

int main(int argc, char** argv)
{
  CHECK(argc == 2);
  log_file = fopen(argv[1], "w");
  CHECK(log_file != NULL);
  CHECK(qnnp_initialize() == qnnp_status_success);
  qnnp_stub_log_to(log_file);

  /*                        pad k  s  groups gic goc kzp  per-channel */
  const struct conv dw =     {1, 3, 1, 8,     1,  1,  121, 0}, dw_pc =   {1, 3, 1, 8, 1,  1, 121, 1};
  const struct conv c3x3 =   {1, 3, 1, 1,     8,  8,  121, 0}, first =   {1, 3, 2, 1, 3,  8, 127, 0};
  const struct conv grouped = {1, 3, 1, 2,    4,  4,  121, 0};
  const struct conv pw127 =  {0, 1, 1, 1,     64, 8,  127, 0}, pw128 =   {0, 1, 1, 1, 64, 8, 128, 0};
  const struct conv pw5 =    {0, 1, 1, 1,     64, 8,  5,   0}, pw_pc =   {0, 1, 1, 1, 64, 8, 127, 1};
  const struct conv g1x1 =   {0, 1, 1, 2,     8,  8,  121, 0}, wide =    {0, 1, 1, 2, 520, 8, 121, 0};

  /*        name                                                          batch h  w  strides  forced residual */
  conv_once("depthwise 3x3, 8 channels", &dw,                                1, 5, 5, 0, 0,    0, 0);
  conv_once("depthwise 3x3, 8 channels, per-channel scales", &dw_pc,         1, 5, 5, 0, 0,    0, 0);
  conv_once("convolution 3x3 8 -> 8, strided pixels", &c3x3,                 1, 5, 5, 3, 5,    0, 0);
  conv_once("convolution 3x3 stride 2, 3 -> 8, kernel zero point 127", &first, 1, 5, 5, 0, 0,  0, 0);
  conv_once("convolution 3x3, 2 groups of 4 -> 4", &grouped,                 1, 5, 5, 0, 0,    0, 0);
  conv_once("1x1 64 -> 8, kernel zero point 127 (own centred image)", &pw127, 1, 2, 2, 0, 0,   0, 0);
  conv_once("1x1 64 -> 8, kernel zero point 128 (the image is centred)", &pw128, 1, 2, 2, 0, 0, 0, 0);
  conv_once("1x1 64 -> 8, kernel zero point 5 (no centred image)", &pw5,     1, 2, 2, 0, 0,    0, 0);
  conv_once("1x1 64 -> 8, per-channel scales", &pw_pc,                       1, 2, 2, 0, 0,    0, 0);
  fully_connected();

  conv_once("grouped 1x1, 4 rows: the grouped image", &g1x1,                 1, 2, 2, 0, 0,    0, 0);
  conv_once("grouped 1x1, 65536 rows: the dense image", &g1x1,               1, 256, 256, 0, 0, 0, 0);
  conv_once("grouped 1x1, 65535 rows: the grouped image", &g1x1,             1, 255, 257, 0, 0, 0, 0);
  conv_once("grouped 1x1, \"gemm_kernel\" 31: the dense image", &g1x1,         1, 2, 2, 0, 0,    31, 0);
  conv_once("grouped 1x1 too wide for a dense image, \"gemm_kernel\" 31", &wide, 1, 2, 2, 0, 0,  31, 0);
  conv_once("grouped 1x1, 65536 rows, residual attached: the grouped image", &g1x1, 1, 256, 256, 0, 0, 0, 1);
  conv_once("grouped 1x1, \"gemm_kernel\" 31, residual attached", &g1x1,       1, 2, 2, 0, 0,    31, 1);

  conv_once("convolution 3x3 8 -> 8 with a residual add", &c3x3,             1, 5, 5, 3, 5,    0, 1);
  conv_once("1x1 64 -> 8 with a residual add", &pw128,                       1, 2, 2, 0, 0,    0, 1);
  conv_once("depthwise 3x3 with a residual add", &dw,                        1, 5, 5, 0, 0,    0, 1);

  /*          name                                                        k  s  pad groups gic goc forced refused */
  deconv_case("deconvolution 2x2 stride 2: depth-to-space GEMM",           2, 2, 0, 1, 16, 8,  0,  -1);
  deconv_case("deconvolution 2x2 stride 2, depth-to-space GEMM refused",   2, 2, 0, 1, 16, 8,  0,  5);
  deconv_case("deconvolution 3x3 stride 2",                                3, 2, 1, 1, 8,  8,  0,  -1);
  deconv_case("deconvolution 3x3 stride 2, \"gemm_kernel\" 13",              3, 2, 1, 1, 8,  8,  13, -1);
  deconv_case("deconvolution 3x3 stride 2, \"gemm_kernel\" 1",               3, 2, 1, 1, 8,  8,  1,  -1);
  deconv_case("deconvolution 3x3 stride 2, 2 groups, \"gemm_kernel\" 13",    3, 2, 1, 2, 8,  8,  13, -1);
  deconv_case("deconvolution 3x3 stride 2, 2 groups",                      3, 2, 1, 2, 8,  8,  0,  -1);
  deconv_case("deconvolution 3x3 stride 1: one table",                     3, 1, 1, 1, 8,  8,  0,  -1);
  deconv_case("deconvolution 3x3 stride 1, \"gemm_kernel\" 13",              3, 1, 1, 1, 8,  8,  13, -1);

  add_case("add, strided, host b", 0, 0);
  add_case("add, strided, host b", 1, 0);
  add_case("add, strided, device b", 1, 1);
  global_average_pooling();
  fused_blocks();
  timing();
  multiply_case("multiply, host b", 0, 0);
  multiply_case("multiply, host b", 1, 0);
  multiply_case("multiply, device b", 1, 1);

  qnnp_stub_log_to(NULL);
  CHECK(fclose(log_file) == 0);
  CHECK(qnnp_stub_live_allocs() == 0);
  CHECK(qnnp_deinitialize() == qnnp_status_success);
  printf("launch-args-ok\n");
  return 0;
}
