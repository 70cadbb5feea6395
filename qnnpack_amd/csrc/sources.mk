# The product's core sources: plain-C host code and gfx950 HIP units, paths relative to qnnpack_amd/csrc. ONE list,
# included by qnnpack_amd/csrc/Makefile (libqnnpack_gfx950.so, and what the sanitizer programs link against
# tests/hip_stub.c) and by oracle/Makefile (the product half of the seam library, which links with --no-undefined: a
# unit missing there breaks the build).
C_SRCS   := init.c convolution.c deconvolution.c fully-connected.c add.c global-average-pooling.c fused-block.c residual.c output-table.c operator-run.c operator-delete.c indirection.c
HIP_SRCS := hip/runtime.hip hip/q8igemm.hip hip/q8gemm256.hip hip/q8gemm256c.hip hip/q8gemm256x.hip hip/q8gemm128x.hip hip/q8gemm128u.hip hip/q8pwconv.hip hip/q8pwstream.hip hip/q8pwstaged.hip hip/q8pwlongk.hip hip/q8pwgw.hip hip/q8convlds.hip hip/q8convwave.hip hip/q8convws16s.hip hip/q8convpatch.hip hip/q8convc3.hip hip/q8convc3s.hip hip/q8deconv.hip hip/q8dwconv.hip hip/q8dwlds.hip hip/q8dwrow.hip hip/q8dwcol.hip hip/q8dwcol5.hip hip/q8dwmfma.hip hip/q8dwmfma16.hip hip/q8pointwise.hip hip/q8fused.hip hip/q8fusedstrip.hip
