/*
 * output-table.c -- qnnp_gfx950_attach_output_table (qnnpack_gfx950_output_table.h): a convolution that also performs
 * the byte table behind it. No reference counterpart: in the reference an activation that is not a clamp is a table
 * operator behind the convolution (src/sigmoid.c, src/leaky-relu.c + x8lut), i.e. one more launch and one more pass over
 * the tensor. Here the lookup rides in the epilogue of the convolution's kernel where that kernel has a table flavour
 * (the pointwise streaming kernels, q8pwconv.hip and its kernel units, and the depthwise column walks, q8dwcol.hip / q8dwcol5.hip), and runs
 * as an in-place launch of the table kernel behind the convolution otherwise (convolution.c finish_output_table); either
 * way the bytes are those of convolution -> qnnp_gfx950_setup_lut_nc_x8 in place on its output.
 *
 * Unlike the residual add (residual.c) the table names no tensor, so it is independent of the setup: it may be attached
 * before the first one and stays across later ones. The 256 bytes are the table operator's own device table, copied at
 * attach time into a table this operator owns: the table operator may be deleted afterwards.
 */
#include <stddef.h>
#include <stdint.h>

#include <qnnpack.h>
#include <qnnpack_gfx950.h>

#include "hip/qnnp_hip.h"
#include "lifecycle.h"
#include "log.h"
#include "operator.h"
#include "upload.h"

enum qnnp_status qnnp_gfx950_attach_output_table(qnnp_operator_t convolution, qnnp_operator_t table)
{
  /* Like a setup that validates first: every check that needs no device comes before the device is entered. */
  enum qnnp_status status = qnnp_check_initialized("qnnp_gfx950_attach_output_table");
  if (status != qnnp_status_success) {
    return status;
  }
  if (convolution == NULL) {
    return qnnp_status_invalid_parameter;
  }
  const int is_conv = convolution->ukernel_type == qnnp_ukernel_type_conv ||
      convolution->ukernel_type == qnnp_ukernel_type_gemm || convolution->ukernel_type == qnnp_ukernel_type_dwconv;
  if (!is_conv || convolution->transposed || (table != NULL && table->ukernel_type != qnnp_ukernel_type_lut)) {
    qnnp_log_error("failed to attach output table: needs a convolution / fully connected operator and a table operator");
    return qnnp_status_invalid_parameter;
  }
  if (table != NULL) {
    const size_t channels = (size_t) convolution->groups * convolution->group_output_channels;
    if (table->channels != channels) {
      qnnp_log_error("failed to attach output table: table operator of %zu channels on a convolution with %zu output channels",
          table->channels, channels);
      return qnnp_status_invalid_parameter;
    }
    if (convolution->device != table->device) {
      qnnp_log_error("failed to attach output table: the operators belong to different devices");
      return qnnp_status_invalid_parameter;
    }
  }
  /* the device table is replaced or freed: not inside a graph capture, which may have recorded launches that read it */
  int token;
  status = qnnp_enter_for_update(convolution->device, qnnp_status_invalid_parameter, &token);
  if (status != qnnp_status_success) {
    return status;
  }
  if (table == NULL) {
    qnnp_hip_free(convolution->d_output_table);
    convolution->d_output_table = NULL;
    convolution->table_folded = 0;
  } else if (convolution->residual != NULL) {
    /* add then table, or table then add: neither chain is this operator's definition */
    qnnp_log_error("failed to attach output table: the convolution has a residual add attached");
    status = qnnp_status_unsupported_parameter;
  } else {
    /* the new table first, so that a failure leaves the previous one in force */
    uint8_t bytes[256];
    void* d_table = NULL;
    if (qnnp_hip_d2h(bytes, table->d_weights, sizeof(bytes), 0) == QNNP_HIP_OK) {
      d_table = qnnp_upload(bytes, sizeof(bytes));
    }
    if (d_table == NULL) {
      qnnp_log_error("failed to attach output table: no room for the 256-byte table on the device");
      status = qnnp_status_out_of_memory;
    } else {
      qnnp_hip_free(convolution->d_output_table);
      convolution->d_output_table = d_table;
      convolution->table_folded = 0;
    }
  }
  qnnp_hip_leave(token);
  return status;
}

int qnnp_gfx950_operator_table_folded(qnnp_operator_t op)
{
  if (op == NULL || op->d_output_table == NULL) {
    return -1;
  }
  return (int) op->table_folded;
}
