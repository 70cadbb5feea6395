/*
 * hip_stub.c -- TEST INFRASTRUCTURE: a host-memory stand-in for the HIP seam (qnnpack_amd/csrc/hip/qnnp_hip.h) so the
 * plain-C host code of the product (create / setup / run plumbing / delete, weight packers, offset tables) can be
 * exercised under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU (SURVEY.md section 5:
 * host-sanitizer cleanliness). "Device" memory is malloc, copies are memcpy, kernel launches validate their argument
 * block and touch the first and last byte of every tensor / table they were given (so ASan sees an undersized
 * allocation), nothing is computed. On request they also record the argument blocks they were handed, as text (the
 * launch log below). Never linked into the product.
 */
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hip/qnnp_hip.h"

static int g_bound = 0;
static int g_async = 0;
static void* g_stream = NULL;
static volatile uint8_t g_sink;

static void touch(const void* p, size_t bytes)
{
  if (p != NULL && bytes != 0) {
    g_sink ^= ((const volatile uint8_t*) p)[0];
    g_sink ^= ((const volatile uint8_t*) p)[bytes - 1];
  }
}

int qnnp_hip_init(int device) { (void) device; g_bound = 1; return QNNP_HIP_OK; }
int qnnp_hip_bind(int device) { return device == 0 && g_bound ? QNNP_HIP_OK : QNNP_HIP_ENODEV; }
int qnnp_hip_shutdown(void) { g_bound = 0; return QNNP_HIP_OK; }
int qnnp_hip_device_count(void) { return 1; }
int qnnp_hip_select(int device) { return device == 0 && g_bound ? QNNP_HIP_OK : QNNP_HIP_ENODEV; }
int qnnp_hip_device(void) { return g_bound ? 0 : -1; }
int qnnp_hip_enter(int device) { return device == 0 && g_bound ? 0 : -1; }
void qnnp_hip_leave(int token) { (void) token; }
int qnnp_hip_device_info(char* arch, size_t arch_len, int* cus, int* clock_khz, size_t* mem_bytes)
{
  if (arch != NULL && arch_len != 0) { strncpy(arch, "gfx950-stub", arch_len - 1); arch[arch_len - 1] = '\0'; }
  if (cus != NULL) *cus = 256;
  if (clock_khz != NULL) *clock_khz = 2400000;
  if (mem_bytes != NULL) *mem_bytes = (size_t) 1 << 30;
  return QNNP_HIP_OK;
}
int qnnp_hip_compute_units(void) { return 256; }
static int g_streaming = 1;
void qnnp_hip_set_streaming_stores(int on) { g_streaming = on != 0; }
int qnnp_hip_streaming_stores(void) { return g_streaming; }
void qnnp_hip_set_stream(void* stream) { g_stream = stream; }
void* qnnp_hip_get_stream(void) { return g_stream; }
void qnnp_hip_set_async(int async) { g_async = async != 0; }
int qnnp_hip_get_async(void) { return g_async; }
int qnnp_hip_stream_sync(void) { return QNNP_HIP_OK; }
const uint8_t* qnnp_hip_fill_table(void) { return NULL; }

/* ---- test controls (host_asan_test.c, host_asan_pool_test.c): failure injection, a pretend graph capture and a count
 * of live "device" allocations. qnnp_stub_fail_nth(n): the n-th qnnp_hip_alloc / qnnp_hip_h2d from now on (0 = the next
 * one) fails, once; n < 0 disarms. qnnp_stub_fail_pending(): 1 while that failure has not happened yet. */
static long g_fail_in = -1;
static int g_capturing = 0;
static size_t g_live = 0;
void qnnp_stub_fail_nth(long n) { g_fail_in = n; }
int qnnp_stub_fail_pending(void) { return g_fail_in >= 0; }
void qnnp_stub_set_capturing(int on) { g_capturing = on != 0; }
size_t qnnp_stub_live_allocs(void) { return g_live; }
static int injected_failure(void) { return g_fail_in >= 0 && g_fail_in-- == 0; }

/* every "device" allocation carries a tag in front so that is_device_pointer can tell it from caller memory */
#define STUB_MAGIC UINT64_C(0x51AB51AB51AB51AB)
void* qnnp_hip_alloc(size_t bytes)
{
  if (injected_failure()) return NULL;
  uint64_t* p = (uint64_t*) malloc(bytes + 16);
  if (p == NULL) return NULL;
  p[0] = STUB_MAGIC;
  p[1] = bytes;
  g_live++;
  return p + 2;
}
void qnnp_hip_free(void* p) { if (p != NULL) { free((uint64_t*) p - 2); g_live--; } }
int qnnp_hip_h2d(void* dst, const void* src, size_t bytes, int async)
{
  (void) async;
  if (injected_failure()) return QNNP_HIP_ELAUNCH;
  memcpy(dst, src, bytes);
  return QNNP_HIP_OK;
}
int qnnp_hip_d2h(void* dst, const void* src, size_t bytes, int async) { (void) async; memcpy(dst, src, bytes); return QNNP_HIP_OK; }
int qnnp_hip_memset(void* dst, int value, size_t bytes) { memset(dst, value, bytes); return QNNP_HIP_OK; }
/* whether `p` is what qnnp_hip_alloc returned, and of how many bytes; it reads the 16 bytes in front of ANY pointer, which
 * for caller memory is an allocator's header or red zone: mapped, but not the sanitizer's business */
__attribute__((noinline, no_sanitize("address")))
static int tagged(const void* p, uint64_t* bytes)
{
  if (p == NULL || (uintptr_t) p % 8 != 0) return 0;
  const volatile uint64_t* head = (const volatile uint64_t*) p - 2;
  if (head[0] != STUB_MAGIC) return 0;
  *bytes = head[1];
  return 1;
}
/* host tensors by default: every program keeps the staged path. qnnp_stub_set_device_pointers(1) (host_launch_args_test.c)
 * makes the stub's own allocations count as memory of the device, which opens the device-pointer run path and the timing
 * entry points */
static int g_device_pointers = 0;
void qnnp_stub_set_device_pointers(int on) { g_device_pointers = on != 0; }
static const void* registered_base(const void* p);
int qnnp_hip_is_device_pointer(const void* p)
{
  uint64_t bytes;
  if (!g_device_pointers) return 0;
  /* a pointer into a registered tensor (the launch log below) lives where that tensor does */
  const void* base = registered_base(p);
  return tagged(base != NULL ? base : p, &bytes);
}

int qnnp_hip_timer_create(void** timer) { *timer = malloc(1); return *timer != NULL ? QNNP_HIP_OK : QNNP_HIP_ENOMEM; }
int qnnp_hip_timer_start(void* timer) { (void) timer; return QNNP_HIP_OK; }
int qnnp_hip_timer_stop_ms(void* timer, float* ms) { (void) timer; *ms = 1.0f; return QNNP_HIP_OK; }
void qnnp_hip_timer_destroy(void* timer) { free(timer); }

int qnnp_hip_graph_capturing(void) { return g_capturing; }
int qnnp_hip_graph_begin(void) { return QNNP_HIP_EINVAL; }   /* no graphs in the stub: timing falls back to the plain loop */
int qnnp_hip_graph_end(void** graph) { (void) graph; return QNNP_HIP_EINVAL; }
int qnnp_hip_graph_device(void* graph) { (void) graph; return 0; }
int qnnp_hip_graph_launch(void* graph) { (void) graph; return QNNP_HIP_EINVAL; }
int qnnp_hip_graph_time(void* graph, int warmup, int iters, float* avg_ms) { (void) graph; (void) warmup; (void) iters; (void) avg_ms; return QNNP_HIP_EINVAL; }
int qnnp_hip_graph_time_median(void* graph, int warmup, int iters, int samples, float* avg_ms)
{ (void) graph; (void) warmup; (void) iters; (void) samples; (void) avg_ms; return QNNP_HIP_EINVAL; }
int qnnp_hip_graph_sync(void* graph) { (void) graph; return QNNP_HIP_EINVAL; }
void qnnp_hip_graph_destroy(void* graph) { (void) graph; }

/* ---- launch log (host_launch_args_test.c): while a file is set, every *_run below appends one line -- its name, every
 * field of its argument block in declaration order, the status it returned. Integers in decimal, nested blocks field by
 * field, pointers by what they point into and never as addresses, so that the log is the same from run to run:
 *   NULL | <tensor>+<offset> inside a tensor the test registered | dev(<bytes>) for a qnnp_hip_alloc block | other */
static FILE* g_log = NULL;
static struct { const char* name; const uint8_t* base; size_t bytes; } g_tensors[4];
static int g_refuse_variant = -1;
void qnnp_stub_log_to(FILE* file) { g_log = file; }
void qnnp_stub_log_tensor(int slot, const char* name, const void* base, size_t bytes)
{
  g_tensors[slot].name = name;
  g_tensors[slot].base = (const uint8_t*) base;
  g_tensors[slot].bytes = base != NULL ? bytes : 0;
}
/* the next qnnp_hip_igemm_run whose `variant` is this one answers QNNP_HIP_EINVAL, once; < 0 disarms */
void qnnp_stub_refuse_igemm_variant(int variant) { g_refuse_variant = variant; }

static int registered_slot(const void* p)
{
  for (int i = 0; i < 4; i++) {
    if (g_tensors[i].bytes != 0 && (const uint8_t*) p >= g_tensors[i].base && (const uint8_t*) p < g_tensors[i].base + g_tensors[i].bytes) {
      return i;
    }
  }
  return -1;
}
static const void* registered_base(const void* p)
{
  const int slot = registered_slot(p);
  return slot >= 0 ? g_tensors[slot].base : NULL;
}

void qnnp_stub_name_pointer(const void* p, char* text, size_t size)
{
  uint64_t bytes;
  if (p == NULL) {
    snprintf(text, size, "NULL");
    return;
  }
  const int slot = registered_slot(p);
  if (slot >= 0) {
    snprintf(text, size, "%s+%zu", g_tensors[slot].name, (size_t) ((const uint8_t*) p - g_tensors[slot].base));
    return;
  }
  if (tagged(p, &bytes)) {
    snprintf(text, size, "dev(%" PRIu64 ")", bytes);
  } else {
    snprintf(text, size, "other");
  }
}

static void log_p(const char* name, const void* p)
{
  char text[48];
  qnnp_stub_name_pointer(p, text, sizeof(text));
  fprintf(g_log, " %s=%s", name, text);
}
static void log_u(const char* name, uint64_t v) { fprintf(g_log, " %s=%" PRIu64, name, v); }
static void log_i(const char* name, int64_t v) { fprintf(g_log, " %s=%" PRId64, name, v); }
#define P(field) log_p(#field, a->field)
#define U(field) log_u(#field, a->field)
#define I(field) log_i(#field, a->field)

static void log_rq(const char* name, const struct qnnp_hip_requant* a)
{
  fprintf(g_log, " %s={", name);
  I(multiplier); I(remainder_mask); I(remainder_threshold); U(shift); I(output_min_less_zero_point);
  I(output_max_less_zero_point); I(output_zero_point); U(accumulator_bits);
  fprintf(g_log, " }");
}

static void log_add(const char* name, const struct qnnp_hip_add_params* a)
{
  if (a == NULL) {
    fprintf(g_log, " %s=NULL", name);
    return;
  }
  fprintf(g_log, " %s={", name);
  U(a_multiplier); U(b_multiplier); I(zero_point_product); U(shift); I(remainder_mask); I(remainder_threshold);
  I(y_zero_point); I(y_min); I(y_max);
  fprintf(g_log, " }");
}

static void log_avgpool(const char* name, const struct qnnp_hip_avgpool_params* a)
{
  fprintf(g_log, " %s={", name);
  I(bias); I(multiplier); I(rounding); U(right_shift); I(output_min_less_zero_point); I(output_max_less_zero_point);
  I(output_zero_point);
  fprintf(g_log, " }");
}

static void log_plan(const char* name, const struct qnnp_hip_dwconv_plan* a)
{
  if (a == NULL) {
    fprintf(g_log, " %s=NULL", name);
    return;
  }
  fprintf(g_log, " %s={", name);
  U(key); U(kernel); U(CS); U(TOH); U(IR); U(IC); U(PP); U(bands); U(slabs); U(store_mode); U(vec16);
  fprintf(g_log, " }");
}

static void log_igemm(const struct qnnp_hip_igemm_args* a)
{
  fprintf(g_log, "qnnp_hip_igemm_run");
  P(input); P(output); P(packed_w); P(packed_w_rows16); P(bias2_rows); P(bias2); P(offsets); U(rows); U(rows_per_image);
  U(image_stride); U(groups); U(n); U(n_pad); U(kc); U(kc_slot); U(input_bytes); U(ks); U(k_total); U(k_pad);
  U(input_stride); U(output_stride); I(row_coeff); U(input_zero_point); log_rq("rq", &a->rq); I(variant); P(out_rows);
  U(out_image_rows); P(phases); U(nphases); U(d2s_stride_h); U(d2s_stride_w); U(d2s_input_h); U(d2s_input_w);
  U(input_height); U(input_width); U(output_height); U(output_width); U(kernel_height); U(kernel_width);
  U(stride_height); U(stride_width); U(dilation_height); U(dilation_width); U(pad_top); U(pad_left); P(residual);
  U(residual_stride); log_add("residual_add", a->residual_add);
  if (a->residual_folded != NULL) log_u("*residual_folded", *a->residual_folded); else P(residual_folded);
  U(bias2_pair); P(packed_w_centred); P(bias2_centred); U(centre_flip); U(streaming_mode); P(rq_pc);
}

static void log_deconv_s2(const struct qnnp_hip_deconv_s2_args* a)
{
  fprintf(g_log, "qnnp_hip_deconv_s2_run");
  P(input); P(output);
  P(packed_w[0]); P(packed_w[1]); P(packed_w[2]); P(packed_w[3]);
  P(bias2[0]); P(bias2[1]); P(bias2[2]); P(bias2[3]);
  U(k_pad[0]); U(k_pad[1]); U(k_pad[2]); U(k_pad[3]);
  U(batch); U(input_height); U(input_width); U(output_height); U(output_width); U(kernel_height); U(kernel_width);
  U(pad_top); U(pad_left); U(channels); U(n); U(n_pad); U(input_stride); U(output_stride); I(row_coeff);
  U(input_zero_point); log_rq("rq", &a->rq); U(bias2_pair);
}

static void log_dwconv(const struct qnnp_hip_dwconv_args* a)
{
  fprintf(g_log, "qnnp_hip_dwconv_run");
  P(input); P(output); P(wadj); P(bias1); P(dwm_x); P(dwm_bias); U(dwm_parts); U(w_range); P(dot4); U(c_pad32); U(batch);
  U(input_height); U(input_width); U(output_height); U(output_width); U(channels); U(c_pad); U(kernel_height);
  U(kernel_width); U(stride_height); U(stride_width); U(dilation_height); U(dilation_width); U(pad_top); U(pad_left);
  U(input_stride); U(output_stride); U(input_zero_point); log_rq("rq", &a->rq); I(variant);
  log_plan("plan", a->plan); U(streaming_mode); P(rq_pc);
}

static void log_vadd(const struct qnnp_hip_vadd_args* a)
{
  fprintf(g_log, "qnnp_hip_vadd_run");
  P(a); P(b); P(sum); U(rows); U(channels); U(a_stride); U(b_stride); U(sum_stride); log_add("params", &a->params);
  U(streaming_mode);
}

static void log_gavgpool(const struct qnnp_hip_gavgpool_args* a)
{
  fprintf(g_log, "qnnp_hip_gavgpool_run");
  P(input); P(output); U(batch); U(width); U(channels); U(input_stride); U(output_stride);
  log_avgpool("params", &a->params);
}

static void log_fused_strip(const struct qnnp_hip_fused_strip_args* a)
{
  fprintf(g_log, "qnnp_hip_fused_strip_run");
  P(input); P(output); U(batch); U(input_height); U(input_width); U(output_height); U(output_width); U(input_channels);
  U(hidden_channels); U(output_channels); U(input_stride); U(output_stride); U(stride); U(has_expand); U(has_residual);
  P(expand_w); P(expand_bias); U(expand_flip); log_rq("expand_rq", &a->expand_rq);
  P(dw_w); P(dw_bias); U(dw_flip); U(dw_pad); log_rq("dw_rq", &a->dw_rq);
  P(project_w); P(project_bias); U(project_flip); log_rq("project_rq", &a->project_rq);
  U(hidden_pad); U(output_pad); log_add("add", &a->add); U(rows_per_strip); U(weights_in_lds);
}

static void log_fused(const struct qnnp_hip_fused_args* a)
{
  fprintf(g_log, "qnnp_hip_fused_block_run");
  P(input); P(output); U(batch); U(input_height); U(input_width); U(output_height); U(output_width); U(input_channels);
  U(hidden_channels); U(output_channels); U(input_stride); U(output_stride); U(stride); U(has_expand);
  P(expand_w); P(expand_bias2); U(expand_k_pad); U(expand_n_pad); I(expand_row_coeff); log_rq("expand_rq", &a->expand_rq);
  P(dw_wadj); P(dw_bias1); U(dw_c_pad); U(dw_input_zero_point); log_rq("dw_rq", &a->dw_rq);
  P(project_w); P(project_bias2); U(project_k_pad); U(project_n_pad); I(project_row_coeff);
  log_rq("project_rq", &a->project_rq); U(has_residual); log_add("add", &a->add);
}
#undef P
#undef U
#undef I

/* one public *_run: the block as it arrived, then the kernel stand-in, then its status */
#define LOGGED_RUN(name, type, log_args, impl) \
  int name(const type* a, const char** kernel_name) \
  { \
    if (g_log != NULL && a != NULL) log_args(a); \
    const int rc = impl(a, kernel_name); \
    if (g_log != NULL && a != NULL) fprintf(g_log, " -> %d\n", rc); \
    return rc; \
  }

/* ---- "kernels": check the argument block against the documented layout, touch every buffer end to end ---- */
static int deconv_s2_run(const struct qnnp_hip_deconv_s2_args* a, const char** kernel_name)
{
  (void) kernel_name;
  if (a == NULL || a->batch == 0) return QNNP_HIP_EINVAL;
  for (int ph = 0; ph < 4; ph++) {
    touch(a->packed_w[ph], (size_t) a->n_pad * a->k_pad[ph]);
    touch(a->bias2[ph], (size_t) a->n_pad * 4);
  }
  return QNNP_HIP_EINVAL;   /* "outside the streaming kernel's range": the host then takes the phase-table path */
}

LOGGED_RUN(qnnp_hip_deconv_s2_run, struct qnnp_hip_deconv_s2_args, log_deconv_s2, deconv_s2_run)

static int igemm_run(const struct qnnp_hip_igemm_args* a, const char** kernel_name)
{
  if (a != NULL && a->variant == g_refuse_variant) {
    g_refuse_variant = -1;
    return QNNP_HIP_EINVAL;
  }
  if (a == NULL || a->rows == 0 || a->n == 0 || a->n_pad % 32 != 0 || a->k_pad % 64 != 0 || a->n_pad < a->n) return QNNP_HIP_EINVAL;
  if (kernel_name != NULL) *kernel_name = "stub_igemm";
  if (a->phases == NULL) {
    touch(a->packed_w, (size_t) a->groups * a->n_pad * a->k_pad);
    touch(a->bias2, (size_t) a->groups * a->n_pad * 4);
    if (a->offsets != NULL) touch(a->offsets, (size_t) a->rows_per_image * a->ks * 4);
  } else {
    touch(a->phases, (size_t) a->nphases * sizeof(struct qnnp_hip_igemm_phase));
    for (uint32_t i = 0; i < a->nphases; i++) {
      const struct qnnp_hip_igemm_phase* ph = &a->phases[i];
      touch(ph->packed_w, (size_t) a->n_pad * ph->k_pad);
      touch(ph->bias2, (size_t) a->n_pad * 4);
      touch(ph->offsets, (size_t) ph->rows_per_image * ph->ks * 4);
      touch(ph->out_rows, (size_t) ph->rows_per_image * 4);
    }
  }
  touch(a->input, a->input_bytes);
  return QNNP_HIP_OK;
}

LOGGED_RUN(qnnp_hip_igemm_run, struct qnnp_hip_igemm_args, log_igemm, igemm_run)

static int dwconv_run(const struct qnnp_hip_dwconv_args* a, const char** kernel_name)
{
  if (a == NULL || a->batch == 0 || a->channels == 0 || a->c_pad < a->channels) return QNNP_HIP_EINVAL;
  if (kernel_name != NULL) *kernel_name = "stub_dwconv";
  const size_t taps = (size_t) a->kernel_height * a->kernel_width;
  touch(a->wadj, taps * a->c_pad * 2);
  touch(a->bias1, (size_t) a->c_pad * 4);
  if (a->dwm_x != NULL) touch(a->dwm_x, (size_t) a->dwm_parts * taps * a->c_pad32);
  if (a->dwm_bias != NULL) touch(a->dwm_bias, (size_t) a->c_pad32 * 4);
  touch(a->input, ((size_t) a->batch * a->input_height * a->input_width - 1) * a->input_stride + a->channels);
  touch(a->output, ((size_t) a->batch * a->output_height * a->output_width - 1) * a->output_stride + a->channels);
  if (a->plan != NULL) a->plan->key = 0x80000000u;
  return QNNP_HIP_OK;
}

LOGGED_RUN(qnnp_hip_dwconv_run, struct qnnp_hip_dwconv_args, log_dwconv, dwconv_run)

static int vadd_run(const struct qnnp_hip_vadd_args* a, const char** kernel_name)
{
  if (a == NULL || a->rows == 0 || a->channels == 0) return QNNP_HIP_EINVAL;
  if (kernel_name != NULL) *kernel_name = "stub_vadd";
  touch(a->a, (size_t) (a->rows - 1) * a->a_stride + a->channels);
  touch(a->b, (size_t) (a->rows - 1) * a->b_stride + a->channels);
  touch(a->sum, (size_t) (a->rows - 1) * a->sum_stride + a->channels);
  return QNNP_HIP_OK;
}

LOGGED_RUN(qnnp_hip_vadd_run, struct qnnp_hip_vadd_args, log_vadd, vadd_run)

static int gavgpool_run(const struct qnnp_hip_gavgpool_args* a, const char** kernel_name)
{
  if (a == NULL || a->batch == 0 || a->width == 0 || a->channels == 0) return QNNP_HIP_EINVAL;
  if (kernel_name != NULL) *kernel_name = "stub_gavgpool";
  touch(a->input, (size_t) (a->batch * a->width - 1) * a->input_stride + a->channels);
  touch(a->output, (size_t) (a->batch - 1) * a->output_stride + a->channels);
  return QNNP_HIP_OK;
}

LOGGED_RUN(qnnp_hip_gavgpool_run, struct qnnp_hip_gavgpool_args, log_gavgpool, gavgpool_run)

int qnnp_hip_fused_strip_bias_offset(const struct qnnp_hip_requant* rq) { return rq != NULL && rq->shift == 0; }
int qnnp_hip_fused_strip_supported(const struct qnnp_hip_fused_strip_args* a) { return a != NULL && a->hidden_channels % 32 == 0; }
static int fused_strip_run(const struct qnnp_hip_fused_strip_args* a, const char** kernel_name)
{
  if (!qnnp_hip_fused_strip_supported(a)) return QNNP_HIP_EINVAL;
  if (kernel_name != NULL) *kernel_name = "stub_fused_strip";
  return QNNP_HIP_OK;
}
LOGGED_RUN(qnnp_hip_fused_strip_run, struct qnnp_hip_fused_strip_args, log_fused_strip, fused_strip_run)
int qnnp_hip_fused_block_supported(const struct qnnp_hip_fused_args* a) { return a != NULL && a->hidden_channels % 16 == 0; }
static int fused_block_run(const struct qnnp_hip_fused_args* a, const char** kernel_name)
{
  if (!qnnp_hip_fused_block_supported(a)) return QNNP_HIP_EINVAL;
  if (kernel_name != NULL) *kernel_name = "stub_fused";
  touch(a->dw_wadj, (size_t) 9 * a->dw_c_pad * 2);
  touch(a->project_w, (size_t) a->project_n_pad * a->project_k_pad);
  if (a->has_expand) touch(a->expand_w, (size_t) a->expand_n_pad * a->expand_k_pad);
  return QNNP_HIP_OK;
}
LOGGED_RUN(qnnp_hip_fused_block_run, struct qnnp_hip_fused_args, log_fused, fused_block_run)
