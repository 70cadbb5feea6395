/*
 * qnnpack_gfx950.h -- MI355X-specific extensions that sit BESIDE the unchanged
 * qnnpack.h API. Nothing here is required by a drop-in caller; these entry
 * points exist for callers that own device memory and streams (frameworks,
 * bench.py, the parity tests).
 *
 * The reference has no counterpart for any of these: its only execution
 * resource is the pthreadpool argument of qnnp_run_operator
 * (include/qnnpack.h:327-329, src/operator-run.c:639), which this build ignores.
 *
 * All functions are plain C ABI: pointers and sizes only, no HIP types. A HIP
 * stream is passed as the opaque `void*` value of a hipStream_t.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "qnnpack.h"
#include "qnnpack_gfx950_squeeze_excite.h"   /* the fused squeeze-and-excite block, beside the fused block below */
#include "qnnpack_gfx950_output_table.h"     /* a byte table folded behind a convolution, beside the residual add below */

#ifdef __cplusplus
extern "C" {
#endif

/* Windowed pooling (reference include/qnnpack.h:162-218, prototypes unchanged; the rest of the reference's qnnpack.h
 * subset is in qnnpack.h). Semantics and status codes are the reference's (src/average-pooling.c, src/max-pooling.c):
 *   average pooling: sum (x - input_zero_point) over the taps inside the image, padding taps counting as zero but
 *     counting in the divisor (pooling_height * pooling_width), quantized as global average pooling is;
 *   max pooling: max over the window with every tap's coordinates clamped into the image (a window wholly in padding
 *     returns the nearest edge pixel), then clamped to [output_min, output_max].
 * Computed by HIP kernels (no indirection buffer); `threadpool` is ignored. Where the reference checks nothing and
 * would read out of range, setup answers invalid_parameter: NULL tensors, a pixel stride below the channel count, a
 * padded input smaller than the (dilated) window. Tensors beyond the kernels' index range (padded extent >= 2^31,
 * output width * channels >= 2^31, batch * output height >= 2^32) are unsupported_parameter. */
enum qnnp_status qnnp_create_average_pooling2d_nhwc_q8(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t pooling_height,
    uint32_t pooling_width,
    uint32_t stride_height,
    uint32_t stride_width,
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* average_pooling);

enum qnnp_status qnnp_setup_average_pooling2d_nhwc_q8(
    qnnp_operator_t average_pooling,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride,
    pthreadpool_t threadpool);

enum qnnp_status qnnp_create_max_pooling2d_nhwc_u8(
    uint32_t input_padding_top,
    uint32_t input_padding_right,
    uint32_t input_padding_bottom,
    uint32_t input_padding_left,
    uint32_t pooling_height,
    uint32_t pooling_width,
    uint32_t stride_height,
    uint32_t stride_width,
    uint32_t dilation_height,
    uint32_t dilation_width,
    size_t channels,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* max_pooling);

enum qnnp_status qnnp_setup_max_pooling2d_nhwc_u8(
    qnnp_operator_t max_pooling,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride,
    pthreadpool_t threadpool);

/* Channel shuffle and clamp (reference include/qnnpack.h:220-232, 257-270, prototypes unchanged). Semantics and status
 * codes are the reference's (src/channel-shuffle.c, src/clamp.c):
 *   channel shuffle: y[c * groups + g] = x[g * group_channels + c] for each pixel (groups >= 2, group_channels >= 1);
 *   clamp: y = min(max(x, output_min), output_max) for each byte (channels >= 1, output_min <= output_max).
 * Computed by HIP kernels. Clamp runs in place when input == output with equal strides. Where the reference checks
 * nothing and would go out of range, setup answers invalid_parameter: NULL tensors, a pixel stride below the channel
 * count (groups * group_channels), input and output byte spans that overlap (for clamp: other than exactly in place).
 * Sizes beyond the kernels' index range (channels >= 2^31, batch >= 2^31) are unsupported_parameter. */
enum qnnp_status qnnp_create_channel_shuffle_nc_x8(
    size_t groups,
    size_t group_channels,
    uint32_t flags,
    qnnp_operator_t* channel_shuffle);

enum qnnp_status qnnp_setup_channel_shuffle_nc_x8(
    qnnp_operator_t channel_shuffle,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride);

enum qnnp_status qnnp_create_clamp_nc_u8(
    size_t channels,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* clamp);

enum qnnp_status qnnp_setup_clamp_nc_u8(
    qnnp_operator_t clamp,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride);

/* Sigmoid and leaky ReLU (reference include/qnnpack.h:272-309, prototypes unchanged). Semantics and status codes are
 * the reference's (src/sigmoid.c, src/leaky-relu.c): create builds a 256-byte table on the host with the reference's
 * float arithmetic, run is y = table[x] for each byte.
 *   sigmoid: table[i] = lrintf(clamp(256 / (1 + expf(-input_scale * (i - input_zero_point))), output_min, output_max));
 *     the output scale must be 1/256 and the output zero point 0 (else unsupported_parameter);
 *   leaky ReLU: x = (input_scale / output_scale) * (i - input_zero_point), y = x < 0 ? x * negative_slope : x,
 *     table[i] = lrintf(clamp(y, output_min - output_zero_point, output_max - output_zero_point)) + output_zero_point;
 *     0 < negative_slope <= 1, and the scale ratio must lie in [2^-8, 2^8) (else unsupported_parameter).
 * Both need output_min < output_max (clamp allows equality). Computed by HIP kernels; they run in place when input ==
 * output with equal strides. Where the reference checks nothing and would go out of range, setup answers
 * invalid_parameter: NULL tensors, a pixel stride below the channel count, input and output byte spans that overlap
 * other than exactly in place. Sizes beyond the kernels' index range (channels >= 2^31, batch >= 2^31) are
 * unsupported_parameter. */
enum qnnp_status qnnp_create_sigmoid_nc_q8(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* sigmoid);

enum qnnp_status qnnp_setup_sigmoid_nc_q8(
    qnnp_operator_t sigmoid,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride);

enum qnnp_status qnnp_create_leaky_relu_nc_q8(
    size_t channels,
    float negative_slope,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* leaky_relu);

enum qnnp_status qnnp_setup_leaky_relu_nc_q8(
    qnnp_operator_t leaky_relu,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride);

/* Softargmax (reference include/qnnpack.h:311-324, prototypes unchanged; note: no input zero point). With it every operator
 * of the reference's qnnpack.h runs as a HIP kernel. Semantics and status codes are the reference's (src/softargmax.c,
 * src/operator-run.c:625-637, src/u8lut32norm/scalar.c): create builds a table of 256 uint32_t on the host with the
 * reference's double arithmetic,
 *   table[i] = lrint(fmin((2^32 - 1) / channels, 8388607) * exp((i - 255) * input_scale)),
 * the output scale must be 1/256 and the output zero point 0 (else unsupported_parameter), and run computes for each of
 * batch_size rows of `channels` bytes, all in uint32_t:
 *   m = max_c x[c];  t_c = table[x[c] + 255 - m];  vsum = sum_c t_c;  y[c] = min(((t_c << 8) + (vsum >> 1)) / vsum, 255).
 * The sum WRAPS modulo 2^32, as the reference's does (rows of more than 512 channels whose bytes all sit near the row's
 * maximum), and the division is exact. Where vsum is 0 modulo 2^32 -- a constant row of 1024, 4096 or 65536 channels,
 * say -- the reference divides by zero and dies; here that row's output is all 0: the sum can only be 0 modulo 2^32 by
 * being at least 2^32, and every t_c << 8 is below 2^31. Runs in place when input == output with equal strides. Setup
 * answers as the table activations' above: invalid_parameter for NULL tensors, a row stride below the channel count, and
 * input and output byte spans that overlap other than exactly in place; unsupported_parameter for sizes beyond the
 * kernels' index range (channels >= 2^31 at create, batch >= 2^31). */
enum qnnp_status qnnp_create_softargmax_nc_q8(
    size_t channels,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint32_t flags,
    qnnp_operator_t* softargmax);

enum qnnp_status qnnp_setup_softargmax_nc_q8(
    qnnp_operator_t softargmax,
    size_t batch_size,
    const uint8_t* input,
    size_t input_stride,
    uint8_t* output,
    size_t output_stride);

/* The table operator under sigmoid, leaky ReLU, hardswish and hardsigmoid, for any other uint8 -> uint8 function of one
 * byte (tanh, re-quantisation between two scales, ...). No reference counterpart: the reference keeps it internal. Setup and run behave as theirs;
 * create answers invalid_parameter for channels == 0 or a NULL table. */
/* y[c] = table[x[c]] for every byte of every pixel; the 256 bytes of `table` are copied at create */
enum qnnp_status qnnp_gfx950_create_lut_nc_x8(size_t channels, const uint8_t table[256], uint32_t flags, qnnp_operator_t* lut);
enum qnnp_status qnnp_gfx950_setup_lut_nc_x8(qnnp_operator_t lut, size_t batch_size,
    const uint8_t* input, size_t input_stride, uint8_t* output, size_t output_stride);

/* Hardswish and hardsigmoid, MobileNetV3's two activations, as table operators. No reference counterpart. Create builds
 * the 256-byte table on the host in float32, every operation rounded once (no fused multiply-add), lrintf rounding to
 * nearest even:
 *   x = input_scale * (float) (i - input_zero_point);   h = min(max(x + 3.0f, 0.0f), 6.0f);
 *   hardswish:   table[i] = lrintf(min(max((1.0f / output_scale) * ((x * h) / 6.0f) + (float) output_zero_point,
 *                                          (float) output_min), (float) output_max));
 *   hardsigmoid: table[i] = lrintf(min(max(256.0f * (h / 6.0f), (float) output_min), (float) output_max));
 *     the output scale must be 1/256 and the output zero point 0, as sigmoid's (else unsupported_parameter).
 * Status codes as qnnp_create_sigmoid_nc_q8, in its order: uninitialized; invalid_parameter for channels == 0, a scale
 * that is not a normal number above zero, output_min >= output_max; unsupported_parameter for channels >= 2^31.
 * Setup, run and delete are the table operator's: qnnp_gfx950_setup_lut_nc_x8 (in place when input == output with equal
 * strides), qnnp_run_operator, qnnp_delete_operator. */
enum qnnp_status qnnp_gfx950_create_hardswish_nc_q8(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* hardswish);

enum qnnp_status qnnp_gfx950_create_hardsigmoid_nc_q8(
    size_t channels,
    uint8_t input_zero_point,
    float input_scale,
    uint8_t output_zero_point,
    float output_scale,
    uint8_t output_min,
    uint8_t output_max,
    uint32_t flags,
    qnnp_operator_t* hardsigmoid);

/* Quantized multiply, element-wise or with the second operand broadcast over groups of rows. No reference counterpart.
 * `a` and `product` have b_rows * a_rows_per_b_row rows of `channels` bytes, `b` has b_rows rows; strides are bytes
 * between rows. Row r of `a` meets row r / a_rows_per_b_row of `b`: a_rows_per_b_row == 1 is the plain element-wise
 * product, a_rows_per_b_row == the pixels of an image is the scale x * s that ends a squeeze-and-excite block (s: one
 * row per image). For each byte, bit-exact:
 *   acc     = ((int32) a - a_zero_point) * ((int32) b - b_zero_point)                 |acc| <= 65025
 *   product = qnnp_q31_requantize(acc, ratio, product_zero_point, product_min, product_max)
 *   ratio   = a_scale * b_scale / product_scale      in float32, left to right: one rounding after *, one after /
 * with the reference's scalar qnnp_q31_requantize, the one the convolutions fuse. `flags` is accepted and ignored.
 * Create, in this order: uninitialized; invalid_parameter for channels == 0, for any of the three scales not a normal
 * number above zero, for product_min >= product_max; unsupported_parameter for channels >= 2^31 and for a ratio outside
 * [2^-32, 1), the domain of the Q31 down-convert -- with |acc| up to 65025, a ratio of 1 or more would saturate nearly
 * every output anyway.
 * Setup: b_rows == 0 or a_rows_per_b_row == 0 succeeds and run then does nothing. invalid_parameter: a NULL tensor; a
 * stride below `channels`; byte spans that overlap other than the permitted in-place forms -- product == a with equal
 * strides always, product == b with equal strides only when a_rows_per_b_row == 1; a and b are only read and may
 * overlap freely (a == b is the square); memory of another GPU. unsupported_parameter: b_rows * a_rows_per_b_row >=
 * 2^31. A setup refused by these checks leaves the previous valid setup runnable. Tensors are host or device memory;
 * the operator records into a hipGraph capture with device pointers, runs in async mode, and honours
 * qnnp_gfx950_operator_set_streaming_stores where the product is not in place (kernel q8_mul_x16). */
enum qnnp_status qnnp_gfx950_create_multiply_nc_q8(
    size_t channels,
    uint8_t a_zero_point,
    float a_scale,
    uint8_t b_zero_point,
    float b_scale,
    uint8_t product_zero_point,
    float product_scale,
    uint8_t product_min,
    uint8_t product_max,
    uint32_t flags,
    qnnp_operator_t* multiply);

enum qnnp_status qnnp_gfx950_setup_multiply_nc_q8(
    qnnp_operator_t multiply,
    size_t b_rows,
    size_t a_rows_per_b_row,
    const uint8_t* a,
    size_t a_stride,
    const uint8_t* b,
    size_t b_stride,
    uint8_t* product,
    size_t product_stride);

/* Bilinear resize of a uint8 NHWC tensor to another height and width: the upsampling that ends a segmentation head, the
 * resize of a decoded image in front of a network's first convolution. No reference counterpart. Quantization is
 * unchanged (the same scale and zero point in and out, as max pooling's), so there are no scale arguments. Pixels are
 * `channels` bytes, `*_pixel_stride` bytes apart; an image is height * width pixels, images follow each other.
 *
 * The definition is integers only, so the result is bit-exact by construction. For each axis take the input size n_in,
 * the output size n_out and the output index o; all arithmetic in uint64_t, divisions round down:
 *   default (half-pixel centres, PyTorch's align_corners=False):
 *     num = max((2 * o + 1) * n_in - n_out, 0)   [the signed value, clamped];   f = (4096 * num + 2 * n_out) / (4 * n_out)
 *   with QNNP_GFX950_RESIZE_ALIGN_CORNERS:
 *     f = 0 if n_out == 1, else (4096 * o * (n_in - 1) + (n_out - 1)) / (2 * (n_out - 1))
 *   f is the source coordinate in Q11, rounded to nearest. Then
 *     i0 = min(f >> 11, n_in - 1),   i1 = min(i0 + 1, n_in - 1),   w = (i0 == i1) ? 0 : (f & 2047)
 * With (y0, y1, wy) from the rows and (x0, x1, wx) from the columns, every channel c of output pixel (oy, ox) of every
 * image is, in uint32_t:
 *     top = x[y0][x0][c] * (2048 - wx) + x[y0][x1][c] * wx
 *     bot = x[y1][x0][c] * (2048 - wx) + x[y1][x1][c] * wx
 *     y   = (top * (2048 - wy) + bot * wy + 2^21) >> 22                        (<= 255 * 2^22 + 2^21 < 2^31)
 * Equal sizes give the identity; the result is within 0.63 of the real-valued bilinear value (0.5 from the last
 * rounding, 255 * 2 * 2^-12 from the two Q11 weights), hence within 1 of its rounding.
 *
 * Create, in this order: uninitialized; invalid_parameter for channels == 0 and for a flag bit other than
 * QNNP_GFX950_RESIZE_ALIGN_CORNERS (flags carry meaning here and are not ignored); unsupported_parameter for channels >=
 * 2^31.
 * Setup: batch_size == 0 succeeds and run then does nothing. Then, in this order: invalid_parameter for any of the four
 * sizes 0, a NULL tensor, a pixel stride below `channels`; unsupported_parameter for any of the four sizes >= 2^24 (which
 * keeps the table arithmetic inside 64 bits) and for batch_size * output_height * output_width >= 2^31 or batch_size *
 * input_height * input_width >= 2^31; invalid_parameter for input and output byte spans that share a byte -- there is
 * no in-place form: every output pixel reads up to four input pixels that other lanes' stores could hit -- and for memory
 * of another GPU; out_of_memory for the tables (setup builds one table per axis on the host and keeps both in one
 * grow-only device allocation of the operator). A setup refused by these checks leaves the previous valid setup runnable.
 * Inside a graph capture create and setup answer invalid_parameter. Tensors are host or device memory; the operator
 * records into a hipGraph capture with device pointers, runs in async mode, and honours
 * qnnp_gfx950_operator_set_streaming_stores on its 16-byte kernel (u8_resize_x16: channels, base addresses and pixel
 * strides multiples of 16; u8_resize_x4 serves every other tensor of 4 channels and more at any alignment, u8_resize_x1
 * fewer channels). Run and delete are qnnp_run_operator / qnnp_delete_operator. */
#define QNNP_GFX950_RESIZE_ALIGN_CORNERS 0x00000001u

enum qnnp_status qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(
    size_t channels,
    uint32_t flags,
    qnnp_operator_t* resize);

enum qnnp_status qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(
    qnnp_operator_t resize,
    size_t batch_size,
    size_t input_height,
    size_t input_width,
    size_t output_height,
    size_t output_width,
    const uint8_t* input,
    size_t input_pixel_stride,
    uint8_t* output,
    size_t output_pixel_stride);

/* Devices. The library keeps one context (launch stream, asynchrony flag) per gfx950 GPU of the node.
 *   BEFORE qnnp_initialize: names the PRIMARY device qnnp_initialize binds (default: env QNNP_GFX950_DEVICE,
 *     else the calling thread's current HIP device).
 *   AFTER qnnp_initialize: binds `device` on first use and makes it the CALLING THREAD's device: operators the
 *     thread creates from now on live there, and set_stream / set_async / synchronize / malloc / memcpy /
 *     graph_begin act on it. Threads that never call it use the primary device.
 * An operator remembers its device: setup / run / delete may be called from any thread, whatever that thread's
 * current HIP device is (it is restored on return). Tensors handed to setup must be host memory or memory of the
 * operator's device (another GPU's memory -> invalid_parameter). Batches shard across the GPUs of a node without
 * a collective -- every output pixel depends on one image (reference src/operator-run.c:675-679, 797-802,
 * 837-842) -- so both "one process per GPU" (bench.py) and "one process, one host thread per GPU" work.
 * invalid_parameter: negative ordinal, or not a usable gfx950 device. */
enum qnnp_status qnnp_gfx950_set_device(int device);
int qnnp_gfx950_get_device(void);      /* the calling thread's device, -1 before qnnp_initialize */
int qnnp_gfx950_device_count(void);    /* HIP devices visible to the process */

/* Threads: as in the reference (run contexts are stack-local, src/operator-run.c:783-795) DISTINCT operators may
 * be created, set up, run and deleted from different threads concurrently, on the same device or different ones.
 * One operator must not be used by two threads at once. set_option is configuration, read at setup time. */

/* Stream all subsequent qnnp_run_operator launches (and host-pointer staging
 * copies) on the calling thread's device are enqueued on. NULL = the device's default stream. */
enum qnnp_status qnnp_gfx950_set_stream(void* hip_stream);

/* async = 1: qnnp_run_operator only enqueues work and returns; the caller
 * synchronises (qnnp_gfx950_synchronize or its own stream sync). Requires device
 * pointers for input/output (host pointers force a synchronous staged run).
 * async = 0 (default): reference semantics, outputs complete on return.
 * A property of the calling thread's device context. */
enum qnnp_status qnnp_gfx950_set_async(int async);
enum qnnp_status qnnp_gfx950_synchronize(void);

/* Device memory helpers for C callers without HIP headers. */
void* qnnp_gfx950_malloc(size_t bytes);
void qnnp_gfx950_free(void* device_ptr);
enum qnnp_status qnnp_gfx950_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes);
enum qnnp_status qnnp_gfx950_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes);
enum qnnp_status qnnp_gfx950_memset(void* dst_device, int value, size_t bytes);

/* Time `iters` back-to-back qnnp_run_operator launches of one operator with hipEvents, after `warmup`
 * untimed launches; writes the AVERAGE milliseconds per launch. Device pointers only. By default the
 * launches are recorded into a hipGraph and its replay is timed (option "timing_graph"), so the figure is
 * kernel time -- what rocprofv3 reports per kernel -- not the host's per-launch dispatch gap. The replay is
 * timed five times, each with its own event pair, and the MEDIAN is reported. */
enum qnnp_status qnnp_gfx950_time_operator(
    qnnp_operator_t op, int warmup, int iters, float* avg_ms_out);

/* Same, but rotates through `nsets` (input, output) device buffer pairs between
 * launches so the working set exceeds the 256 MiB Infinity Cache when an HBM
 * bandwidth figure is claimed. inputs/outputs: arrays of nsets device pointers. */
enum qnnp_status qnnp_gfx950_time_operator_rotating(
    qnnp_operator_t op, size_t nsets, const void* const* inputs, void* const* outputs,
    int warmup, int iters, float* avg_ms_out);

/* hipGraph capture: between begin and end, qnnp_run_operator only RECORDS its launch (device pointers only; a
 * host-pointer operator returns invalid_parameter). The graph replays the whole sequence -- e.g. every layer of
 * a network -- as one submission: no per-launch dispatch gap, which on MI355X is as long as the small layers
 * themselves. Replays run on the stream given to qnnp_gfx950_set_stream at capture time (a private stream
 * stands in for the default stream, which cannot be captured): synchronous unless qnnp_gfx950_set_async(1),
 * then qnnp_gfx950_graph_synchronize. Operators and their buffers must outlive the graph.
 * The capture belongs to the calling THREAD (its launches are recorded, other threads keep running normally).
 * qnnp_gfx950_graph_time: milliseconds per replay, hipEvents on the replay stream -- five batches of `iters`
 * replays after `warmup` untimed ones, the median batch / iters. */
enum qnnp_status qnnp_gfx950_graph_begin(void);
enum qnnp_status qnnp_gfx950_graph_end(void** graph_out);
enum qnnp_status qnnp_gfx950_graph_launch(void* graph);
enum qnnp_status qnnp_gfx950_graph_synchronize(void* graph);
enum qnnp_status qnnp_gfx950_graph_time(void* graph, int warmup, int iters, float* avg_ms_out);
void qnnp_gfx950_graph_destroy(void* graph);

/* Fused inverted-residual block (no reference counterpart):
 *     [1x1 expand ->] 3x3 depthwise (padding 1, stride 1 | 2) -> 1x1 project [-> quantized add with the block input]
 * as ONE operator; the expanded tensors stay in LDS. Built FROM stand-alone operators created with qnnpack.h
 * (`expand` and `residual_add` may be NULL): it borrows their packed weights and quantization parameters, so the
 * result is bit-identical to running them in sequence, and they must outlive it. Run / delete with
 * qnnp_run_operator / qnnp_delete_operator. unsupported_parameter (from create or setup) = outside the fused
 * kernel's range (channel multiples, LDS) -- keep using the stand-alone operators for that block. */
enum qnnp_status qnnp_gfx950_create_fused_block(
    qnnp_operator_t expand, qnnp_operator_t depthwise, qnnp_operator_t project, qnnp_operator_t residual_add,
    qnnp_operator_t* fused);
enum qnnp_status qnnp_gfx950_setup_fused_block(
    qnnp_operator_t fused, size_t batch_size, size_t input_height, size_t input_width,
    const uint8_t* input, size_t input_stride, uint8_t* output, size_t output_stride);

/* (The other fused operator, a squeeze-and-excite block built from its five stand-alone operators --
 * qnnp_gfx950_create_squeeze_excite / qnnp_gfx950_setup_squeeze_excite -- is declared in
 * qnnpack_gfx950_squeeze_excite.h, included above.) */

/* Residual add folded into a convolution (no reference counterpart: there it is a convolution operator followed by
 * an add operator, src/add.c). After a successful qnnp_setup_convolution2d_nhwc_q8 / qnnp_setup_fully_connected_nc_q8
 * of `convolution` on DEVICE pointers, attach an add operator created with qnnp_create_add_nc_q8 whose channel count
 * is the convolution's output channel count: from then on qnnp_run_operator(convolution) writes
 *     output = add(a = residual pixel, b = convolution output pixel)
 * bit-identical to running `convolution` and then `add` set up with (a = residual, b = the convolution's output).
 * The add's parameters are copied (the add operator may be deleted); `residual` is caller-owned device memory,
 * residual_stride bytes between pixels, and may be the convolution's input tensor or any other tensor except its
 * output. The next setup of `convolution` detaches it. The add rides in the convolution kernel's epilogue where that
 * kernel carries it (pointwise layers: every MobileNetV2 project layer; needs residual_stride == output stride and
 * the output's alignment), otherwise the add kernel is launched in place behind the convolution.
 * qnnp_gfx950_operator_residual_folded: after a run, 1 = epilogue, 0 = separate launch, -1 = nothing attached.
 * NO OVERLAP: the residual range [residual, residual + (pixels - 1) * residual_stride + channels) must not intersect
 * the convolution's output range, not even exactly (residual == output): the kernels read the residual through
 * non-aliasing / streaming loads while other workgroups write the output. An in-place sum is what the stand-alone add
 * operator is for (qnnp_setup_add_nc_q8 accepts sum == a or sum == b).
 * Status: invalid_parameter (NULL / wrong operator kinds / channel mismatch / no valid setup / during capture /
 * residual overlapping the output), unsupported_parameter (host-memory endpoints -- answered before the overlap is
 * looked at, the addresses of a host-staged output mean nothing on the device). */
enum qnnp_status qnnp_gfx950_attach_residual_add(
    qnnp_operator_t convolution, qnnp_operator_t add, const uint8_t* residual, size_t residual_stride);
int qnnp_gfx950_operator_residual_folded(qnnp_operator_t op);

/* Process-wide options of the product. Keys:
 *   "timing_graph":  1 (default) = qnnp_gfx950_time_operator* time a hipGraph replay of the launches (kernel
 *                    time without per-launch dispatch gaps); 0 = a plain back-to-back launch loop
 *   "streaming_stores": 1 (default) = kernels whose waves write whole cache lines exactly once (pointwise / fully
 *                    connected outputs, the 4096^3-class GEMM, the element-wise add) mark those stores as streaming:
 *                    right for an operator that runs on its own (per-layer sweep +4-5 %, GEMM +2 %); 0 = plain stores,
 *                    for callers that chain operators -- a streamed tensor is not in the last-level cache when its
 *                    consumer starts (whole MobileNetV2: -1 % with the hint). Read at launch (or graph-capture) time.
 *                    This is the DEFAULT of every operator; qnnp_gfx950_operator_set_streaming_stores below sets it per
 *                    operator, which is what a caller with both kinds of operators in one process wants.
 * Unknown key -> invalid_parameter.
 * (Kernel-forcing codes -- which kernel an operator runs on, for A/B measurement and for the test tiers -- are NOT part of
 *  this interface: include/qnnpack_gfx950_test.h, qnnp_gfx950_test_force_kernel.) */
enum qnnp_status qnnp_gfx950_set_option(const char* key, int value);

/* The streaming-store hint ("streaming_stores" above) of ONE operator: value 1 / 0 = on / off for every later launch of
 * `op`, -1 = follow the process-wide option again (the default). An operator whose output the next operator reads at
 * once (a chained network) wants 0; an operator on its own, as the reference bench runs them, 1 -- both kinds can live
 * in one process, and no launch of another thread is affected.
 * Honoured by every kernel that has a streaming form: convolution / fully connected / depthwise operators, the
 * element-wise add, the multiply (16-byte pieces, product not in place), the bilinear resize (u8_resize_x16: the store
 * only, its loads are re-read by neighbouring output pixels), and deconvolutions that run as GEMMs (kernel ==
 * stride, and the per-phase GEMMs). Kernels WITHOUT a
 * streaming form write plain stores whatever the setting, and the call still answers success for them: the stride-2
 * 3x3 / 4x4 deconvolution stream kernel, global average pooling (its output is a few KB) and fused blocks (their output
 * feeds the next block). */
enum qnnp_status qnnp_gfx950_operator_set_streaming_stores(qnnp_operator_t op, int value);

/* Name of the HIP kernel the operator's last setup selected (static string), or
 * NULL. Lets tests assert that the intended kernel actually ran. */
const char* qnnp_gfx950_operator_kernel(qnnp_operator_t op);

/* Device properties as seen by the library: gcnArchName copied into `arch`
 * (NUL-terminated, truncated to arch_len), CU count, clock in kHz. */
enum qnnp_status qnnp_gfx950_device_info(
    char* arch, size_t arch_len, int* compute_units, int* clock_khz, size_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
