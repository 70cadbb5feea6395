/*
 * lut.h -- what sigmoid.c and leaky-relu.c share with lut.c: the operator behind all three is a 256-byte table.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>

/* The create of every table operator once its own checks have passed and `table` is built: `channels` beyond the
 * kernels' index range is unsupported_parameter; then the operator is allocated and the table uploaded on the calling
 * thread's device (out_of_memory). `what` names the operator in the log. Call with the library initialized. */
enum qnnp_status qnnp_create_lut_operator(const char* what, size_t channels, const uint8_t table[256],
                                          qnnp_operator_t* lut_out);

/* The setup of every table operator (`what` names the entry point in the log). */
enum qnnp_status qnnp_setup_lut_operator(const char* what, qnnp_operator_t lut, size_t batch_size, const uint8_t* input,
                                         size_t input_stride, uint8_t* output, size_t output_stride);
