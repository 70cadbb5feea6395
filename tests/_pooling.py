"""Cases, a numpy model and drivers for the windowed pooling operators (max pooling, average pooling).

Case lists restate the reference's operator tests with the parameters of its x86 build (the SSE2 microkernels:
u8maxpool kr = 16, mr = 9, qr = 8; q8avgpool kr = 8, mr = 9, qr = 8; reference src/init.c:213-224):
test/max-pooling.cc (51 tests) and test/average-pooling.cc (57 tests), loop for loop, with the defaults of
test/max-pooling-operator-tester.h:618-639 and test/average-pooling-operator-tester.h:623-646 (input scale 1, output
scale 1, input zero point 121, output zero point 133, qmin 0, qmax 255, pixel strides = channels). A case with `next_*`
fields is one of the setup_* tests: set up and run, then set up again with the next sizes on the same buffers and run.
The reference testers compare against a float model with a tolerance; here the expectation is bit-exact (the numpy model
below, pinned to the compiled reference by tests/golden/reference_pooling_outputs.npz).

Beyond those lists: dilation for max pooling, windows wholly in padding, one-sided padding, the channel counts of the
vector / dword / byte kernel paths, pixel strides that are not multiples of 4, device base pointers offset by 1-3
bytes, host-pointer tensors, and the reference's bench lists (bench/max-pooling.cc:93-138,
bench/average-pooling.cc:94-145) at batch 1 and 128.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace
from typing import List, Optional

import numpy as np

FILL = 0xA5


def _seed(name: str) -> int:
    return 0x9001 ^ (zlib.crc32(name.encode()) & 0x7FFFFFFF)


@dataclass(frozen=True)
class PoolCase:
    kind: str                 # "max" | "avg"
    name: str
    batch: int
    input_height: int
    input_width: int
    channels: int
    pooling_height: int
    pooling_width: int
    pad_top: int = 0
    pad_right: int = 0
    pad_bottom: int = 0
    pad_left: int = 0
    stride_height: int = 1
    stride_width: int = 1
    dilation_height: int = 1  # max pooling only
    dilation_width: int = 1
    in_stride: int = 0        # 0: channels
    out_stride: int = 0
    qmin: int = 0
    qmax: int = 255
    in_scale: float = 1.0     # average pooling only
    out_scale: float = 1.0
    in_zp: int = 121
    out_zp: int = 133
    next_batch: int = 0       # setup_* tests: 0 = unchanged
    next_height: int = 0
    next_width: int = 0
    misalign_in: int = 0      # GPU tier: device base pointer offsets (bytes)
    misalign_out: int = 0
    host: bool = False        # GPU tier: host pointers (the staged path)

    @property
    def strides(self):
        return (self.in_stride or self.channels, self.out_stride or self.channels)

    @property
    def resetup(self) -> bool:
        return bool(self.next_batch or self.next_height or self.next_width)

    def geometries(self):
        """(batch, input height, input width) of each setup the case runs"""
        first = (self.batch, self.input_height, self.input_width)
        if not self.resetup:
            return [first]
        return [first, (self.next_batch or self.batch, self.next_height or self.input_height,
                        self.next_width or self.input_width)]

    def output_size(self, height: int, width: int):
        dh, dw = (self.dilation_height, self.dilation_width) if self.kind == "max" else (1, 1)
        eh = (self.pooling_height - 1) * dh + 1
        ew = (self.pooling_width - 1) * dw + 1
        return ((self.pad_top + height + self.pad_bottom - eh) // self.stride_height + 1,
                (self.pad_left + width + self.pad_right - ew) // self.stride_width + 1)


_TESTER_KEYS = {
    "batchSize": "batch", "inputHeight": "input_height", "inputWidth": "input_width", "channels": "channels",
    "poolingHeight": "pooling_height", "poolingWidth": "pooling_width", "paddingTop": "pad_top",
    "paddingRight": "pad_right", "paddingBottom": "pad_bottom", "paddingLeft": "pad_left",
    "strideHeight": "stride_height", "strideWidth": "stride_width", "dilationHeight": "dilation_height",
    "dilationWidth": "dilation_width", "inputPixelStride": "in_stride", "outputPixelStride": "out_stride",
    "qmin": "qmin", "qmax": "qmax", "inputScale": "in_scale", "outputScale": "out_scale",
    "inputZeroPoint": "in_zp", "outputZeroPoint": "out_zp", "nextBatchSize": "next_batch",
    "nextInputHeight": "next_height", "nextInputWidth": "next_width",
}


def _fgeom(start: float, stop: float, factor: float):
    """for (float v = start; v < stop; v *= factor) in float32 arithmetic"""
    v = np.float32(start)
    while v < np.float32(stop):
        yield float(v)
        v = np.float32(v * np.float32(factor))


# ---- the reference's test lists (test/max-pooling.cc, test/average-pooling.cc), loop for loop ----------------------
# (16 / 9 / 8 are kr / mr / qr of the SSE2 kernels; each `add` is one operator-tester run)

def _reference_max_pooling_tests(add):
    name = 'zero_batch'
    add(name, 'testU8', batchSize=0, inputHeight=2, inputWidth=6, poolingHeight=1, poolingWidth=8, channels=8)
    name = 'unit_batch_many_channels_small_1xM_pool'
    for channels in range(16, (3 * 16) + 1, 1):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_small_1xM_pool_with_padding'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(3, (9) + 1, 1):
            for paddingLeft in range(0, (1) + 1, 1):
                for paddingRight in range(0, (1) + 1, 1):
                    add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, paddingLeft=paddingLeft, paddingRight=paddingRight, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_small_1xM_pool_with_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 4, poolingHeight=1, poolingWidth=poolSize, strideWidth=2, channels=channels)
    name = 'unit_batch_many_channels_small_1xM_pool_with_dilation'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=2 * poolSize + 1, poolingHeight=1, poolingWidth=poolSize, dilationWidth=2, channels=channels)
    name = 'unit_batch_many_channels_small_Mx1_pool'
    for channels in range(16, (3 * 16) + 1, 1):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_small_Mx1_pool_with_padding'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            for paddingTop in range(0, (1) + 1, 1):
                for paddingBottom in range(0, (1) + 1, 1):
                    add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, paddingTop=paddingTop, paddingBottom=paddingBottom, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_small_Mx1_pool_with_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 3, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, strideHeight=2, channels=channels)
    name = 'unit_batch_many_channels_small_Mx1_pool_with_dilation'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2 * poolSize, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, dilationHeight=2, channels=channels)
    name = 'unit_batch_many_channels_small_pool_with_input_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 16)
    name = 'unit_batch_many_channels_small_pool_with_output_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 16)
    name = 'unit_batch_many_channels_small_pool_with_qmin'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmin=192)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmin=192)
    name = 'unit_batch_many_channels_small_pool_with_qmax'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmax=192)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmax=192)
    name = 'unit_batch_many_channels_large_1xM_pool'
    for channels in range(16, (3 * 16) + 1, 1):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_large_1xM_pool_with_padding'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(3, (9) + 1, 1):
            for paddingLeft in range(0, (1) + 1, 1):
                for paddingRight in range(0, (1) + 1, 1):
                    add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, paddingLeft=paddingLeft, paddingRight=paddingRight, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_large_1xM_pool_with_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 4, poolingHeight=1, poolingWidth=poolSize, strideWidth=2, channels=channels)
    name = 'unit_batch_many_channels_large_1xM_pool_with_dilation'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=2 * poolSize + 1, poolingHeight=1, poolingWidth=poolSize, dilationWidth=2, channels=channels)
    name = 'unit_batch_many_channels_large_Mx1_pool'
    for channels in range(16, (3 * 16) + 1, 1):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_large_Mx1_pool_with_padding'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            for paddingTop in range(0, (1) + 1, 1):
                for paddingBottom in range(0, (1) + 1, 1):
                    add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, paddingTop=paddingTop, paddingBottom=paddingBottom, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_large_Mx1_pool_with_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 3, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, strideHeight=2, channels=channels)
    name = 'unit_batch_many_channels_large_Mx1_pool_with_dilation'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2 * poolSize, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, dilationHeight=2, channels=channels)
    name = 'unit_batch_many_channels_large_pool_with_input_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 16)
    name = 'unit_batch_many_channels_large_pool_with_output_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 16)
    name = 'unit_batch_many_channels_large_pool_with_qmin'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmin=192)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmin=192)
    name = 'unit_batch_many_channels_large_pool_with_qmax'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(9, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmax=192)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmax=192)
    name = 'unit_batch_few_channels_1xM_pool'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_few_channels_1xM_pool_with_padding'
    for channels in range(1, (16), 1):
        for poolSize in range(3, (9) + 1, 1):
            for paddingLeft in range(0, (1) + 1, 1):
                for paddingRight in range(0, (1) + 1, 1):
                    add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, paddingLeft=paddingLeft, paddingRight=paddingRight, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_few_channels_1xM_pool_with_stride'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 4, poolingHeight=1, poolingWidth=poolSize, strideWidth=2, channels=channels)
    name = 'unit_batch_few_channels_1xM_pool_with_dilation'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=2 * poolSize + 1, poolingHeight=1, poolingWidth=poolSize, dilationWidth=2, channels=channels)
    name = 'unit_batch_few_channels_Mx1_pool'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_few_channels_Mx1_pool_with_padding'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            for paddingTop in range(0, (1) + 1, 1):
                for paddingBottom in range(0, (1) + 1, 1):
                    add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, paddingTop=paddingTop, paddingBottom=paddingBottom, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_few_channels_Mx1_pool_with_stride'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 3, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, strideHeight=2, channels=channels)
    name = 'unit_batch_few_channels_Mx1_pool_with_dilation'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=2 * poolSize, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, dilationHeight=2, channels=channels)
    name = 'unit_batch_few_channels_with_input_stride'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 16)
    name = 'unit_batch_few_channels_with_output_stride'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 16)
    name = 'unit_batch_few_channels_with_qmin'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmin=192)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmin=192)
    name = 'unit_batch_few_channels_with_qmax'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmax=192)
            add(name, 'testU8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmax=192)
    name = 'small_batch_many_channels_small_pool'
    for channels in range(16, (3 * 16) + 1, 1):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'small_batch_many_channels_small_pool_with_input_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 16)
    name = 'small_batch_many_channels_small_pool_with_output_stride'
    for channels in range(16, (3 * 16) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 16)
    name = 'small_batch_many_channels_large_pool'
    for channels in range(16, (3 * 16) + 1, 1):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'small_batch_many_channels_large_pool_with_input_stride'
    for channels in range(16, (3 * 16) + 1, 5):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 16)
    name = 'small_batch_many_channels_large_pool_with_output_stride'
    for channels in range(16, (3 * 16) + 1, 5):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 16)
    name = 'small_batch_few_channels'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 1):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'small_batch_few_channels_with_input_stride'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 3):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 16)
    name = 'small_batch_few_channels_with_output_stride'
    for channels in range(1, (16), 1):
        for poolSize in range(2, (2 * 16) + 1, 3):
            add(name, 'testU8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 16)
            add(name, 'testU8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 16)
    name = 'setup_increasing_batch'
    add(name, 'testSetupU8', batchSize=3, nextBatchSize=5, inputHeight=8, inputWidth=8, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_decreasing_batch'
    add(name, 'testSetupU8', batchSize=5, nextBatchSize=3, inputHeight=8, inputWidth=8, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_changing_height'
    add(name, 'testSetupU8', batchSize=3, inputHeight=8, inputWidth=8, nextInputHeight=9, poolingHeight=5, poolingWidth=3, channels=24)
    add(name, 'testSetupU8', batchSize=3, inputHeight=8, inputWidth=8, nextInputHeight=7, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_changing_width'
    add(name, 'testSetupU8', batchSize=3, inputHeight=8, inputWidth=8, nextInputWidth=9, poolingHeight=5, poolingWidth=3, channels=24)
    add(name, 'testSetupU8', batchSize=3, inputHeight=8, inputWidth=8, nextInputWidth=7, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_swap_height_and_width'
    add(name, 'testSetupU8', batchSize=3, inputHeight=9, inputWidth=8, nextInputHeight=8, nextInputWidth=9, poolingHeight=5, poolingWidth=3, channels=24)


def _reference_average_pooling_tests(add):
    name = 'zero_batch'
    add(name, 'testQ8', batchSize=0, inputHeight=2, inputWidth=4, poolingHeight=1, poolingWidth=2, channels=4)
    name = 'unit_batch_many_channels_small_1xM_pool'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_small_1xM_pool_with_padding'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(3, (9) + 1, 1):
            for paddingLeft in range(0, (1) + 1, 1):
                for paddingRight in range(0, (1) + 1, 1):
                    add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, paddingLeft=paddingLeft, paddingRight=paddingRight, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_small_1xM_pool_with_stride'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 4, poolingHeight=1, poolingWidth=poolSize, strideWidth=2, channels=channels)
    name = 'unit_batch_many_channels_small_Mx1_pool'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_small_Mx1_pool_with_padding'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            for paddingTop in range(0, (1) + 1, 1):
                for paddingBottom in range(0, (1) + 1, 1):
                    add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, paddingTop=paddingTop, paddingBottom=paddingBottom, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_small_Mx1_pool_with_stride'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 3, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, strideHeight=2, channels=channels)
    name = 'unit_batch_many_channels_small_pool_with_input_stride'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 8)
    name = 'unit_batch_many_channels_small_pool_with_output_stride'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 8)
    name = 'unit_batch_many_channels_small_pool_with_input_scale'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            for inputScale in _fgeom(0.01, 100.0, 3.14159265):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputScale=inputScale)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputScale=inputScale)
    name = 'unit_batch_many_channels_small_pool_with_input_zero_point'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            for inputZeroPoint in range(0, (255) + 1, 51):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputZeroPoint=inputZeroPoint)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputZeroPoint=inputZeroPoint)
    name = 'unit_batch_many_channels_small_pool_with_output_scale'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            for outputScale in _fgeom(0.01, 100.0, 3.14159265):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputScale=outputScale)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputScale=outputScale)
    name = 'unit_batch_many_channels_small_pool_with_output_zero_point'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            for outputZeroPoint in range(0, (255) + 1, 51):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputZeroPoint=outputZeroPoint)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputZeroPoint=outputZeroPoint)
    name = 'unit_batch_many_channels_small_pool_with_qmin'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmin=128)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmin=128)
    name = 'unit_batch_many_channels_small_pool_with_qmax'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmax=128)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmax=128)
    name = 'unit_batch_many_channels_large_1xM_pool'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_large_1xM_pool_with_padding'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(3, (9) + 1, 1):
            for paddingLeft in range(0, (1) + 1, 1):
                for paddingRight in range(0, (1) + 1, 1):
                    add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, paddingLeft=paddingLeft, paddingRight=paddingRight, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_many_channels_large_1xM_pool_with_stride'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 4, poolingHeight=1, poolingWidth=poolSize, strideWidth=2, channels=channels)
    name = 'unit_batch_many_channels_large_Mx1_pool'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_large_Mx1_pool_with_padding'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            for paddingTop in range(0, (1) + 1, 1):
                for paddingBottom in range(0, (1) + 1, 1):
                    add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, paddingTop=paddingTop, paddingBottom=paddingBottom, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_large_Mx1_pool_with_stride'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            for paddingTop in range(0, (1) + 1, 1):
                for paddingBottom in range(0, (1) + 1, 1):
                    add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, paddingTop=paddingTop, paddingBottom=paddingBottom, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_many_channels_large_pool_with_input_stride'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 8)
    name = 'unit_batch_many_channels_large_pool_with_input_scale'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            for inputScale in _fgeom(0.01, 100.0, 3.14159265):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputScale=inputScale)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputScale=inputScale)
    name = 'unit_batch_many_channels_large_pool_with_input_zero_point'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            for inputZeroPoint in range(0, (255) + 1, 51):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputZeroPoint=inputZeroPoint)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputZeroPoint=inputZeroPoint)
    name = 'unit_batch_many_channels_large_pool_with_output_stride'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 8)
    name = 'unit_batch_many_channels_large_pool_with_output_scale'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            for outputScale in _fgeom(0.01, 100.0, 3.14159265):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputScale=outputScale)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputScale=outputScale)
    name = 'unit_batch_many_channels_large_pool_with_output_zero_point'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            for outputZeroPoint in range(0, (255) + 1, 51):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputZeroPoint=outputZeroPoint)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputZeroPoint=outputZeroPoint)
    name = 'unit_batch_many_channels_large_pool_with_qmin'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmin=128)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmin=128)
    name = 'unit_batch_many_channels_large_pool_with_qmax'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmax=128)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmax=128)
    name = 'unit_batch_few_channels_1xM_pool'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_few_channels_1xM_pool_with_padding'
    for channels in range(1, (8), 1):
        for poolSize in range(3, (9) + 1, 1):
            for paddingLeft in range(0, (1) + 1, 1):
                for paddingRight in range(0, (1) + 1, 1):
                    add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, paddingLeft=paddingLeft, paddingRight=paddingRight, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'unit_batch_few_channels_1xM_pool_with_stride'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 4, poolingHeight=1, poolingWidth=poolSize, strideWidth=2, channels=channels)
    name = 'unit_batch_few_channels_Mx1_pool'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_few_channels_Mx1_pool_with_padding'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            for paddingTop in range(0, (1) + 1, 1):
                for paddingBottom in range(0, (1) + 1, 1):
                    add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, paddingTop=paddingTop, paddingBottom=paddingBottom, poolingHeight=poolSize, poolingWidth=1, channels=channels)
    name = 'unit_batch_few_channels_Mx1_pool_with_stride'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 3, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, strideHeight=2, channels=channels)
    name = 'unit_batch_few_channels_with_input_stride'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 8)
    name = 'unit_batch_few_channels_with_input_scale'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            for inputScale in _fgeom(0.01, 100.0, 3.14159265):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputScale=inputScale)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputScale=inputScale)
    name = 'unit_batch_few_channels_with_input_zero_point'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            for inputZeroPoint in range(0, (255) + 1, 51):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputZeroPoint=inputZeroPoint)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputZeroPoint=inputZeroPoint)
    name = 'unit_batch_few_channels_with_output_stride'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 8)
    name = 'unit_batch_few_channels_with_output_scale'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            for outputScale in _fgeom(0.01, 100.0, 3.14159265):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputScale=outputScale)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputScale=outputScale)
    name = 'unit_batch_few_channels_with_output_zero_point'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            for outputZeroPoint in range(0, (255) + 1, 51):
                add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputZeroPoint=outputZeroPoint)
                add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputZeroPoint=outputZeroPoint)
    name = 'unit_batch_few_channels_with_qmin'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmin=128)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 1, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmin=128)
    name = 'unit_batch_few_channels_with_qmax'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=1, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, qmax=128)
            add(name, 'testQ8', batchSize=1, inputHeight=2, inputWidth=poolSize + 1, poolingHeight=1, poolingWidth=poolSize, channels=channels, qmax=128)
    name = 'small_batch_many_channels_small_pool'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'small_batch_many_channels_small_pool_with_input_stride'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 1, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 8)
    name = 'small_batch_many_channels_small_pool_with_output_stride'
    for channels in range(8, (3 * 8) + 1, 3):
        for poolSize in range(2, (9) + 1, 1):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 1, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 8)
    name = 'small_batch_many_channels_large_pool'
    for channels in range(8, (3 * 8) + 1, 1):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'small_batch_many_channels_large_pool_with_input_stride'
    for channels in range(8, (3 * 8) + 1, 5):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 1, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 8)
    name = 'small_batch_many_channels_large_pool_with_output_stride'
    for channels in range(8, (3 * 8) + 1, 5):
        for poolSize in range(9 + 1, (9 + 8) + 1, 1):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 1, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 8)
    name = 'small_batch_few_channels'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 1):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels)
    name = 'small_batch_few_channels_with_input_stride'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 3):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, inputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, inputPixelStride=5 * 8)
    name = 'small_batch_few_channels_with_output_stride'
    for channels in range(1, (8), 1):
        for poolSize in range(2, (2 * 8) + 1, 3):
            add(name, 'testQ8', batchSize=3, inputHeight=poolSize + 1, inputWidth=3, poolingHeight=poolSize, poolingWidth=1, channels=channels, outputPixelStride=5 * 8)
            add(name, 'testQ8', batchSize=3, inputHeight=2, inputWidth=poolSize + 2, poolingHeight=1, poolingWidth=poolSize, channels=channels, outputPixelStride=5 * 8)
    name = 'setup_increasing_batch'
    add(name, 'testSetupQ8', batchSize=3, nextBatchSize=5, inputHeight=8, inputWidth=8, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_decreasing_batch'
    add(name, 'testSetupQ8', batchSize=5, nextBatchSize=3, inputHeight=8, inputWidth=8, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_changing_height'
    add(name, 'testSetupQ8', batchSize=3, inputHeight=8, inputWidth=8, nextInputHeight=9, poolingHeight=5, poolingWidth=3, channels=24)
    add(name, 'testSetupQ8', batchSize=3, inputHeight=8, inputWidth=8, nextInputHeight=7, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_changing_width'
    add(name, 'testSetupQ8', batchSize=3, inputHeight=8, inputWidth=8, nextInputWidth=9, poolingHeight=5, poolingWidth=3, channels=24)
    add(name, 'testSetupQ8', batchSize=3, inputHeight=8, inputWidth=8, nextInputWidth=7, poolingHeight=5, poolingWidth=3, channels=24)
    name = 'setup_swap_height_and_width'
    add(name, 'testSetupQ8', batchSize=3, inputHeight=9, inputWidth=8, nextInputHeight=8, nextInputWidth=9, poolingHeight=5, poolingWidth=3, channels=24)


def _collect(kind: str, fn) -> List[PoolCase]:
    out: List[PoolCase] = []
    counts = {}

    def add(test, _method, **kw):
        k = counts.get(test, 0)
        counts[test] = k + 1
        fields = {_TESTER_KEYS[key]: value for key, value in kw.items()}
        fields.setdefault("batch", 1)
        fields.setdefault("input_height", 1)
        fields.setdefault("input_width", 1)
        fields.setdefault("channels", 1)
        fields.setdefault("pooling_height", 1)
        fields.setdefault("pooling_width", 1)
        out.append(PoolCase(kind, f"{kind}/{test}/{k}", **fields))
    fn(add)
    return out


def reference_max_cases() -> List[PoolCase]:
    return _collect("max", _reference_max_pooling_tests)


def reference_avg_cases() -> List[PoolCase]:
    return _collect("avg", _reference_average_pooling_tests)


# ---- the reference's bench lists (bench/max-pooling.cc:93-138, bench/average-pooling.cc:94-145): N H W K P S C -----
MAX_BENCH = [
    ("ShuffleNet", 112, 112, 3, 1, 2, 24),
    ("SqueezeNetV10_pool1", 111, 111, 3, 0, 2, 96), ("SqueezeNetV10_pool4", 27, 27, 3, 0, 2, 256),
    ("SqueezeNetV10_pool8", 13, 13, 3, 0, 2, 512),
    ("SqueezeNetV11_pool1", 111, 111, 3, 0, 2, 64), ("SqueezeNetV11_pool3", 55, 55, 3, 0, 2, 128),
    ("SqueezeNetV11_pool5", 13, 13, 3, 0, 2, 256),
    ("VGG_1", 224, 224, 2, 1, 2, 64), ("VGG_2", 112, 112, 2, 1, 2, 128), ("VGG_3", 56, 56, 2, 1, 2, 256),
    ("VGG_4", 28, 28, 2, 1, 2, 512), ("VGG_5", 14, 14, 2, 1, 2, 512),
]
AVG_BENCH = []
for _g, _cs in ((1, (24, 144, 288, 576)), (2, (24, 200, 400, 800)), (3, (24, 240, 480, 960)), (4, (24, 272, 576, 1088)),
                (8, (24, 384, 768, 1536))):
    for _hw, _c in zip((56, 28, 14, 7), _cs):
        AVG_BENCH.append((f"ShuffleNetV1G{_g}_{_hw}x{_hw}x{_c}", _hw, _hw, 3, 1, 2, _c))


def bench_case(kind: str, row, batch: int) -> PoolCase:
    name, h, w, k, p, s, c = row
    extra = dict(in_zp=127, in_scale=0.75, out_zp=127, out_scale=1.25) if kind == "avg" else {}
    return PoolCase(kind, f"{kind}/bench/{name}/b{batch}", batch, h, w, c, k, k, p, p, p, p, s, s, **extra)


def bench_cases(batch: int) -> List[PoolCase]:
    return [bench_case("max", r, batch) for r in MAX_BENCH] + [bench_case("avg", r, batch) for r in AVG_BENCH]


def extra_cases() -> List[PoolCase]:
    out: List[PoolCase] = []
    for kind in ("max", "avg"):
        x = f"{kind}/x"
        out += [
            PoolCase(kind, f"{x}/resnet_stem_3x3s2p1", 2, 112, 112, 64, 3, 3, 1, 1, 1, 1, 2, 2),
            PoolCase(kind, f"{x}/window_wholly_in_padding", 2, 3, 4, 16, 3, 3, 4, 4, 4, 4, 1, 1),
            PoolCase(kind, f"{x}/window_wholly_in_padding_odd", 1, 2, 3, 5, 2, 2, 3, 0, 0, 3, 2, 2),
            PoolCase(kind, f"{x}/pad_top_only", 2, 9, 8, 32, 3, 3, 2, 0, 0, 0, 2, 2),
            PoolCase(kind, f"{x}/pad_left_only", 2, 8, 9, 32, 3, 3, 0, 0, 0, 2, 2, 2),
            PoolCase(kind, f"{x}/pad_bottom_right_only", 2, 9, 9, 32, 3, 3, 0, 2, 2, 0, 2, 2),
            PoolCase(kind, f"{x}/large_window_7x7", 2, 14, 14, 48, 7, 7, 3, 3, 3, 3, 2, 2),
            PoolCase(kind, f"{x}/window_over_257_taps", 1, 20, 20, 32, 17, 17, 1, 1, 1, 1, 3, 3),
            PoolCase(kind, f"{x}/qmin_qmax", 2, 10, 10, 32, 3, 3, 1, 1, 1, 1, 2, 2, qmin=40, qmax=200),
            PoolCase(kind, f"{x}/qmin_above_qmax", 1, 6, 6, 16, 2, 2, 0, 0, 0, 0, 2, 2, qmin=200, qmax=40),
        ]
        for c in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 200, 1088):
            out.append(PoolCase(kind, f"{x}/channels{c}", 2, 11, 10, c, 3, 3, 1, 1, 1, 1, 2, 2))
        for si, so in ((19, 23), (66, 70), (130, 129), (100, 96)):
            out.append(PoolCase(kind, f"{x}/strides_{si}_{so}", 2, 9, 9, 64 if si >= 64 and so >= 64 else 16,
                                3, 3, 1, 1, 1, 1, 2, 2, in_stride=si, out_stride=so))
        for mi, mo in ((1, 0), (0, 2), (3, 3), (4, 0), (0, 4), (8, 8)):
            out.append(PoolCase(kind, f"{x}/misaligned_{mi}_{mo}", 2, 9, 9, 64, 3, 3, 1, 1, 1, 1, 2, 2,
                                misalign_in=mi, misalign_out=mo))
        out.append(PoolCase(kind, f"{x}/host_pointers", 2, 12, 12, 64, 3, 3, 1, 1, 1, 1, 2, 2, host=True))
        out.append(PoolCase(kind, f"{x}/host_pointers_strided", 2, 12, 12, 20, 3, 3, 1, 1, 1, 1, 2, 2, in_stride=24,
                            out_stride=22, host=True))
        out.append(PoolCase(kind, f"{x}/resetup_larger", 2, 9, 9, 32, 3, 3, 1, 1, 1, 1, 2, 2, next_batch=3,
                            next_height=13, next_width=11))
    out += [
        PoolCase("max", "max/x/dilation_2x3", 2, 13, 14, 32, 3, 3, 1, 2, 1, 2, 1, 2, dilation_height=2, dilation_width=3),
        PoolCase("max", "max/x/dilation_wider_than_image", 1, 3, 3, 16, 2, 2, 2, 2, 2, 2, 1, 1, dilation_height=5,
                 dilation_width=5),
        PoolCase("max", "max/x/dilation_odd_channels", 2, 12, 12, 7, 2, 3, 0, 1, 0, 1, 2, 1, dilation_height=3,
                 dilation_width=2),
        PoolCase("avg", "avg/x/scale_ratio_low", 2, 9, 9, 16, 3, 3, 1, 1, 1, 1, 2, 2, in_scale=0.004, out_scale=1.0),
        PoolCase("avg", "avg/x/scale_ratio_high", 2, 9, 9, 16, 3, 3, 1, 1, 1, 1, 2, 2, in_scale=200.0, out_scale=1.0),
        PoolCase("avg", "avg/x/zero_points", 2, 9, 9, 16, 2, 2, 1, 0, 0, 1, 1, 1, in_zp=0, out_zp=255),
    ]
    return out


def all_cases() -> List[PoolCase]:
    return reference_max_cases() + reference_avg_cases() + extra_cases() + bench_cases(1)


def thin(cases: List[PoolCase], every: int) -> List[PoolCase]:
    """every `every`-th case of each reference test, plus its first and last"""
    groups = {}
    for c in cases:
        groups.setdefault(c.name.rsplit("/", 1)[0], []).append(c)
    out = []
    for g in groups.values():
        picked = g[::every]
        if g[-1] is not picked[-1]:
            picked.append(g[-1])
        out += picked
    return out


# ---- tensors ----------------------------------------------------------------------------------------------------
def _input_size(case: PoolCase) -> int:
    si, _ = case.strides
    return max(((n * h * w - 1) * si + case.channels) if n else 0 for n, h, w in case.geometries())


def _output_size(case: PoolCase) -> int:
    _, so = case.strides
    sizes = []
    for n, h, w in case.geometries():
        oh, ow = case.output_size(h, w)
        sizes.append(((n * oh * ow - 1) * so + case.channels) if n else 0)
    return max(sizes)


def input_tensor(case: PoolCase) -> np.ndarray:
    rng = np.random.default_rng(_seed(case.name))
    return rng.integers(0, 256, size=_input_size(case), dtype=np.uint8)


def output_tensor(case: PoolCase) -> np.ndarray:
    return np.full(_output_size(case), FILL, dtype=np.uint8)


# ---- numpy model ------------------------------------------------------------------------------------------------
def _pixels(case: PoolCase, x: np.ndarray, n: int, h: int, w: int) -> np.ndarray:
    si, _ = case.strides
    rows = np.arange(n * h * w, dtype=np.int64)[:, None] * si + np.arange(case.channels)[None, :]
    return x[rows].reshape(n, h, w, case.channels)


def _scatter(case: PoolCase, out: np.ndarray, y: np.ndarray) -> None:
    _, so = case.strides
    n, oh, ow, c = y.shape
    rows = np.arange(n * oh * ow, dtype=np.int64)[:, None] * so + np.arange(c)[None, :]
    out[rows] = y.reshape(n * oh * ow, c)


def avgpool_params(case: PoolCase):
    """qnnp_compute_avgpool_quantization_params, scalar members (reference src/qnnpack/requantization.h:200-265)"""
    scale = np.float32(case.in_scale) / (np.float32(case.out_scale) * np.float32(case.pooling_height * case.pooling_width))
    bits = int(np.array([scale], dtype=np.float32).view(np.uint32)[0])
    multiplier = (bits & 0x007FFFFF) | 0x00800000
    shift = 127 + 23 - (bits >> 23)
    return multiplier, shift


def max_pool(case: PoolCase, x: np.ndarray, n: int, h: int, w: int) -> np.ndarray:
    """reference src/indirection.c:192-230 (clamped taps) + u8maxpool: max(min(max over taps, qmax), qmin)"""
    img = _pixels(case, x, n, h, w)
    oh, ow = case.output_size(h, w)
    y = np.zeros((n, oh, ow, case.channels), np.uint8)
    for ky in range(case.pooling_height):
        iy = np.clip(np.arange(oh) * case.stride_height + ky * case.dilation_height - case.pad_top, 0, h - 1)
        for kx in range(case.pooling_width):
            ix = np.clip(np.arange(ow) * case.stride_width + kx * case.dilation_width - case.pad_left, 0, w - 1)
            y = np.maximum(y, img[:, iy][:, :, ix])
    return np.maximum(np.minimum(y, np.uint8(case.qmax)), np.uint8(case.qmin))


def avg_pool(case: PoolCase, x: np.ndarray, n: int, h: int, w: int) -> np.ndarray:
    """sum (x - izp) over in-image taps (padding reads the zero point: src/average-pooling.c:139-179), then
    qnnp_avgpool_quantize (src/qnnpack/requantization.h:482-498); the SSE2 kernels clamp with min(., qmax) first,
    max(., qmin) last (src/q8avgpool/up8x9-sse2.c:141-142)"""
    img = _pixels(case, x, n, h, w).astype(np.int64) - case.in_zp
    oh, ow = case.output_size(h, w)
    acc = np.zeros((n, oh, ow, case.channels), np.int64)
    for ky in range(case.pooling_height):
        iy = np.arange(oh) * case.stride_height + ky - case.pad_top
        vy = (iy >= 0) & (iy < h)
        for kx in range(case.pooling_width):
            ix = np.arange(ow) * case.stride_width + kx - case.pad_left
            vx = (ix >= 0) & (ix < w)
            tap = img[:, np.clip(iy, 0, h - 1)][:, :, np.clip(ix, 0, w - 1)]
            acc += np.where((vy[:, None] & vx[None, :])[None, :, :, None], tap, 0)
    acc = acc.astype(np.int32).astype(np.int64)       # the reference's int32 accumulator
    multiplier, shift = avgpool_params(case)
    q = (acc * multiplier - (acc < 0) + (1 << (shift - 1))) >> shift
    v = np.clip(q + case.out_zp, 0, 255)
    return np.maximum(np.minimum(v, case.qmax), case.qmin).astype(np.uint8)


def expected(case: PoolCase, x: np.ndarray) -> List[np.ndarray]:
    """the output buffer after each setup + run of the case (FILL where nothing is written)"""
    outs = []
    out = output_tensor(case)
    for n, h, w in case.geometries():
        if n:
            y = max_pool(case, x, n, h, w) if case.kind == "max" else avg_pool(case, x, n, h, w)
            _scatter(case, out, y)
        outs.append(out.copy())
    return outs


# ---- average pooling over its whole range of scale ratios, held to real arithmetic ---------------------------------
# The numpy model above restates the integer algorithm, so it cannot notice a defect of the algorithm itself. These
# cases sit at the edges of the accepted input-to-output scale ratios, [2^-8, 2^8), and at the zero-point corners, and
# avg_real() is the operator in float64. A list of its own: all_cases() also runs against the compiled reference.
# tests/test_pointwise_range_host.py checks the model against avg_real(), tests/test_pointwise_range_gpu.py the kernels
# against the model.
def _f32_below(x: float) -> float:
    return float(np.nextafter(np.float32(x), np.float32(0.0)))


RANGE_RATIOS = [float(np.float32(v)) for v in (2.0 ** -8, 1.37 * 2.0 ** -8, 1.0, 1.11 * 2.0 ** 7, _f32_below(2.0 ** 8))]
RANGE_ZERO_POINTS = [(0, 0), (255, 255), (0, 255), (255, 0), (121, 133)]      # (input, output)
RANGE_CLAMPS = [(0, 255), (100, 101)]
# (tag, image side, window, padding, stride)
RANGE_GEOMETRIES = [("2x2s2", 6, 2, 0, 2), ("3x3s1p1", 5, 3, 1, 1), ("7x7_whole_image", 7, 7, 0, 1)]

# |y - clip(real)| <= RANGE_TOL, derived (not measured). With N taps in the window (the divisor, padded taps included)
# and n = the sum of (x - in_zp) over the taps inside the image (|n| <= 255 * N), the kernel rounds n * s to the nearest
# integer exactly: 0.5. s = fl(in_scale / fl(out_scale * N)) is the float32 that create forms: two roundings, so n * s
# is within 255 * ratio * (2^-23 + 2^-48) < 255 * 2^8 * 2^-23 of the real value for every float32 ratio below 2^8. The
# list has out_scale = 1, so the ratio itself is exact.
RANGE_TOL = 0.5 + 255 * 2.0 ** 8 * 2.0 ** -23


def range_cases() -> List[PoolCase]:
    """batch 2 (the two images of range_input): geometries x {16, 19} channels x ratios x zero-point corners x clamps"""
    out = []
    for tag, side, window, pad, stride in RANGE_GEOMETRIES:
        for channels in (16, 19):
            for k, ratio in enumerate(RANGE_RATIOS):
                for in_zp, out_zp in RANGE_ZERO_POINTS:
                    for qmin, qmax in RANGE_CLAMPS:
                        out.append(PoolCase("avg", f"avg/range/{tag}_c{channels}_r{k}_zp{in_zp}_{out_zp}_q{qmin}_{qmax}", 2, side,
                                            side, channels, window, window, pad, pad, pad, pad, stride, stride, qmin=qmin,
                                            qmax=qmax, in_scale=ratio, out_scale=1.0, in_zp=in_zp, out_zp=out_zp))
    return out


def range_input(case: PoolCase) -> np.ndarray:
    """image 0: channel c holds one byte at every pixel, 0 in the first channel and 255 in the last; image 1: random.
    Laid out with the case's input stride (the bytes between pixels are 0x5A)."""
    n, h, w = case.batch, case.input_height, case.input_width
    assert n == 2
    rng = np.random.default_rng(_seed(f"range/{h}x{w}x{case.channels}"))
    img = np.empty((2, h, w, case.channels), np.uint8)
    img[0] = (np.arange(case.channels) * 255 // (case.channels - 1)).astype(np.uint8)[None, None, :]
    img[1] = rng.integers(0, 256, size=(h, w, case.channels), dtype=np.uint8)
    si, _ = case.strides
    rows = n * h * w
    flat = np.full((rows - 1) * si + case.channels, 0x5A, dtype=np.uint8)
    idx = np.arange(rows, dtype=np.int64)[:, None] * si + np.arange(case.channels)[None, :]
    flat[idx] = img.reshape(rows, case.channels)
    return flat


def avg_real(case: PoolCase, x: np.ndarray) -> np.ndarray:
    """[n][oh][ow][c] in real arithmetic (float64), unclamped: (mean - in_zp) * ratio + out_zp, where a padded tap of
    the window counts as in_zp and the divisor is the whole window"""
    n, h, w = case.batch, case.input_height, case.input_width
    img = _pixels(case, x, n, h, w).astype(np.float64) - case.in_zp
    padded = np.zeros((n, h + case.pad_top + case.pad_bottom, w + case.pad_left + case.pad_right, case.channels))
    padded[:, case.pad_top:case.pad_top + h, case.pad_left:case.pad_left + w] = img
    oh, ow = case.output_size(h, w)
    total = np.zeros((n, oh, ow, case.channels))
    for ky in range(case.pooling_height):
        for kx in range(case.pooling_width):
            total += padded[:, ky:ky + (oh - 1) * case.stride_height + 1:case.stride_height,
                            kx:kx + (ow - 1) * case.stride_width + 1:case.stride_width]
    ratio = float(np.float32(case.in_scale) / np.float32(case.out_scale))
    return total / float(case.pooling_height * case.pooling_width) * ratio + case.out_zp


# ---- drivers ----------------------------------------------------------------------------------------------------
def create(lib, case: PoolCase):
    if case.kind == "max":
        return lib.create_max_pooling2d_nhwc_u8_status(
            case.pad_top, case.pad_right, case.pad_bottom, case.pad_left, case.pooling_height, case.pooling_width,
            case.stride_height, case.stride_width, case.dilation_height, case.dilation_width, case.channels,
            case.qmin, case.qmax, 0)
    return lib.create_average_pooling2d_nhwc_q8_status(
        case.pad_top, case.pad_right, case.pad_bottom, case.pad_left, case.pooling_height, case.pooling_width,
        case.stride_height, case.stride_width, case.channels, case.in_zp, case.in_scale, case.out_zp, case.out_scale,
        case.qmin, case.qmax, 0)


def setup_status(lib, case: PoolCase, op, n, h, w, x, y):
    si, so = case.strides
    fn = lib.setup_max_pooling2d_nhwc_u8_status if case.kind == "max" else lib.setup_average_pooling2d_nhwc_q8_status
    return fn(op, n, h, w, x, si, y, so)


def run(lib, case: PoolCase, x: np.ndarray, to_device=None, from_device=None, async_check=None):
    """Run every setup of the case; returns (the output buffer after each run, kernel name of the last run).
    With to_device / from_device (GPU tier) the tensors are device buffers offset by the case's misalignment."""
    st, op = create(lib, case)
    if st != 0:
        raise RuntimeError(f"{case.name}: create -> {st!r}")
    outs, kname = [], None
    out = output_tensor(case)
    one = np.zeros(1, np.uint8)
    try:
        if to_device is not None and not case.host:
            d_x = to_device(x if x.size else one, case.misalign_in)
            d_y = to_device(out if out.size else one, case.misalign_out)
        else:
            d_x, d_y = (x if x.size else one), (out if out.size else one)
        for n, h, w in case.geometries():
            st = setup_status(lib, case, op, n, h, w, d_x, d_y)
            if st != 0:
                raise RuntimeError(f"{case.name}: setup {n}x{h}x{w} -> {st!r}")
            lib.run_operator(op)
            if to_device is not None and not case.host:
                outs.append(from_device(d_y)[:out.size].copy())
            else:
                outs.append(out.copy())
        kname = lib.operator_kernel(op) if hasattr(lib, "operator_kernel") else None
    finally:
        lib.delete_operator(op)
    return outs, kname
