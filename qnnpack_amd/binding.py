"""ctypes binding of the QNNPACK q8 conv/GEMM C API (include/qnnpack.h).

One class binds any shared library that exports the reference's C ABI for the
hot path: the product (``libqnnpack_gfx950.so``) and, in the test
infrastructure, the compiled reference (``oracle/_ref/libqnnpack_ref.so``).
That both load through the same signatures IS the drop-in claim.

Reference interface mirrored: include/qnnpack.h:24-76, 118-140, 327-332.
Pointers are passed as raw addresses (``int``), numpy arrays (host memory) or
anything with a ``data_ptr()`` method (e.g. a torch tensor on the bound GPU).

Every C function is described once, in the tables below; ``argtypes`` / ``restype`` and the operators' methods are
made from them, and tests/test_binding_signatures.py holds the tables to the prototypes of the public headers.
"""
from __future__ import annotations

import ast
import ctypes
import inspect
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_uint8, c_uint32, c_void_p
from enum import IntEnum
from typing import NamedTuple, Optional

import numpy as np


class Status(IntEnum):
    """enum qnnp_status, include/qnnpack.h:24-32"""

    success = 0
    uninitialized = 1
    invalid_parameter = 2
    unsupported_parameter = 3
    unsupported_hardware = 4
    out_of_memory = 5


class QnnpackError(RuntimeError):
    def __init__(self, call: str, status: int):
        self.status = Status(status)
        super().__init__(f"{call} -> qnnp_status_{self.status.name}")


def address_of(buf) -> Optional[int]:
    """Raw address of a buffer argument (None -> NULL)."""
    if buf is None:
        return None
    if isinstance(buf, int):
        return buf
    if isinstance(buf, np.ndarray):
        return buf.ctypes.data
    if hasattr(buf, "data_ptr"):
        return int(buf.data_ptr())
    raise TypeError(f"cannot take the address of {type(buf)!r}")


# ---- the description of the C API ----
# A parameter is "<kind> <name>" or "<kind> <name>=<default>"; the kind gives its ctype and what a generated method does
# with the caller's value.
_CTYPES = {
    "size_t": c_size_t, "u32": c_uint32, "u8": c_uint8, "f32": c_float, "int": c_int, "str": c_char_p,
    "ptr": c_void_p,        # passed as it is: an operator handle (named `op` where it is the function's own), stream, graph
    "tensor": c_void_p,     # through address_of
    "u8[]": c_void_p, "i32[]": c_void_p, "f32[]": c_void_p, "u8[256]": c_void_p,   # host array of that dtype (and size), None -> NULL
    "out": POINTER(c_void_p),   # a create's trailing handle: not a Python parameter, returned
    "null": c_void_p,           # the setups' threadpool: not a Python parameter, always NULL
    "ptr*": POINTER(c_void_p), "f32*": POINTER(c_float), "int*": POINTER(c_int), "size_t*": POINTER(c_size_t),
}
_HOST_ARRAYS = {"u8[]": (np.uint8, None), "i32[]": (np.int32, None), "f32[]": (np.float32, None), "u8[256]": (np.uint8, 256)}

# When a symbol is bound at load. QNNP_GFX950_LIBRARY may name an OLDER build for a same-box A/B: entry points younger
# than it are then simply not bound; the product library must have them all (tests/test_abi.py).
ALWAYS = "always"               # a missing symbol is an AttributeError at load
UNLESS_OLDER = "unless_older"   # the same, unless QNNP_GFX950_LIBRARY is set and the symbol is missing
IF_PRESENT = "if_present"       # the product's own operators, which the compiled reference does not have


class Param(NamedTuple):
    kind: str
    name: str
    default: object = inspect.Parameter.empty


class Function(NamedTuple):
    symbol: str
    params: tuple
    bound: str
    restype: object
    methods: bool       # whether <name>_status and <name> are generated, <name> the symbol without qnnp_ / gfx950_
    doc: Optional[str]

    @property
    def argtypes(self) -> list:
        return [_CTYPES[p.kind] for p in self.params]


def _fn(symbol, spec="", bound=ALWAYS, restype=c_int, methods=False, doc=None) -> Function:
    params = []
    for item in filter(None, (s.strip() for s in spec.split(","))):
        kind, _, name = item.partition(" ")
        name, has_default, default = name.partition("=")
        params.append(Param(kind, name, ast.literal_eval(default) if has_default else inspect.Parameter.empty))
    return Function(symbol, tuple(params), bound, restype, methods, doc)


def _op(symbol, spec="", bound=ALWAYS, doc=None) -> Function:
    return _fn(symbol, spec, bound, methods=True, doc=doc)


# parameter runs that several prototypes share (the headers call the four paddings input_padding_*)
_PADDING = "u32 pad_top, u32 pad_right, u32 pad_bottom, u32 pad_left, "
_IN_Q = "u8 input_zero_point, f32 input_scale, "
_OUT_Q = "u8 output_zero_point, f32 output_scale, u8 output_min, u8 output_max, u32 flags=0, out "
_WEIGHTS_Q = _IN_Q + "u8 kernel_zero_point, f32 kernel_scale, u8[] kernel, i32[] bias, " + _OUT_Q
_GROUPS = "u32 groups, size_t group_input_channels, size_t group_output_channels, "
_POOLING = "u32 pooling_height, u32 pooling_width, u32 stride_height, u32 stride_width, "
_BINARY_Q = ("size_t channels, u8 a_zero_point, f32 a_scale, u8 b_zero_point, f32 b_scale, "
             "u8 {0}_zero_point, f32 {0}_scale, u8 {0}_min, u8 {0}_max, u32 flags=0, out ")
_SETUP_NHWC = ("ptr op, size_t batch_size, size_t input_height, size_t input_width, "
               "tensor input, size_t input_stride, tensor output, size_t output_stride")
_SETUP_NC = "ptr op, size_t batch_size, tensor input, size_t input_stride, tensor output, size_t output_stride"
_LUT_DOC = "a table operator: set it up with setup_lut_nc_x8"

# include/qnnpack.h, then the operators that the product declares in include/qnnpack_gfx950.h
QNNPACK_API = (
    _op("qnnp_initialize"),
    _fn("qnnp_deinitialize"),
    _op("qnnp_create_convolution2d_nhwc_q8",
        _PADDING + "u32 kernel_height, u32 kernel_width, u32 subsampling_height, u32 subsampling_width, "
        "u32 dilation_height, u32 dilation_width, " + _GROUPS + _WEIGHTS_Q + "convolution"),
    _op("qnnp_setup_convolution2d_nhwc_q8", _SETUP_NHWC + ", null threadpool"),
    _op("qnnp_create_deconvolution2d_nhwc_q8",
        _PADDING + "u32 adjustment_height, u32 adjustment_width, u32 kernel_height, u32 kernel_width, "
        "u32 stride_height, u32 stride_width, u32 dilation_height, u32 dilation_width, "
        + _GROUPS + _WEIGHTS_Q + "deconvolution",
        doc="kernel: [groups][group_input_channels][kh][kw][group_output_channels] (reference include/qnnpack.h:78-105)."),
    _op("qnnp_setup_deconvolution2d_nhwc_q8", _SETUP_NHWC + ", null threadpool"),
    _op("qnnp_create_fully_connected_nc_q8", "size_t input_channels, size_t output_channels, " + _WEIGHTS_Q + "fully_connected"),
    _op("qnnp_setup_fully_connected_nc_q8", _SETUP_NC),
    _op("qnnp_create_global_average_pooling_nwc_q8", "size_t channels, " + _IN_Q + _OUT_Q + "global_average_pooling"),
    _op("qnnp_setup_global_average_pooling_nwc_q8",
        "ptr op, size_t batch_size, size_t width, tensor input, size_t input_stride, tensor output, size_t output_stride"),
    _op("qnnp_create_add_nc_q8", _BINARY_Q.format("sum") + "add"),
    _op("qnnp_setup_add_nc_q8",
        "ptr op, size_t batch_size, tensor a, size_t a_stride, tensor b, size_t b_stride, tensor sum, size_t sum_stride"),
    _op("qnnp_run_operator", "ptr op, ptr threadpool=None"),
    _op("qnnp_delete_operator", "ptr op"),
    # the rest of the reference's include/qnnpack.h (162-232, 257-324)
    _op("qnnp_create_average_pooling2d_nhwc_q8",
        _PADDING + _POOLING + "size_t channels, " + _IN_Q + _OUT_Q + "average_pooling", UNLESS_OLDER),
    _op("qnnp_setup_average_pooling2d_nhwc_q8", _SETUP_NHWC + ", null threadpool", UNLESS_OLDER),
    _op("qnnp_create_max_pooling2d_nhwc_u8",
        _PADDING + _POOLING + "u32 dilation_height, u32 dilation_width, size_t channels, "
        "u8 output_min, u8 output_max, u32 flags=0, out max_pooling", UNLESS_OLDER),
    _op("qnnp_setup_max_pooling2d_nhwc_u8", _SETUP_NHWC + ", null threadpool", UNLESS_OLDER),
    _op("qnnp_create_channel_shuffle_nc_x8", "size_t groups, size_t group_channels, u32 flags=0, out channel_shuffle", UNLESS_OLDER),
    _op("qnnp_setup_channel_shuffle_nc_x8", _SETUP_NC, UNLESS_OLDER),
    _op("qnnp_create_clamp_nc_u8", "size_t channels, u8 output_min, u8 output_max, u32 flags=0, out clamp", UNLESS_OLDER),
    _op("qnnp_setup_clamp_nc_u8", _SETUP_NC, UNLESS_OLDER),
    _op("qnnp_create_sigmoid_nc_q8", "size_t channels, " + _IN_Q + _OUT_Q + "sigmoid", UNLESS_OLDER),
    _op("qnnp_setup_sigmoid_nc_q8", _SETUP_NC, UNLESS_OLDER),
    _op("qnnp_create_leaky_relu_nc_q8", "size_t channels, f32 negative_slope, " + _IN_Q + _OUT_Q + "leaky_relu", UNLESS_OLDER),
    _op("qnnp_setup_leaky_relu_nc_q8", _SETUP_NC, UNLESS_OLDER),
    _op("qnnp_create_softargmax_nc_q8",
        "size_t channels, f32 input_scale, u8 output_zero_point, f32 output_scale, u32 flags=0, out softargmax", UNLESS_OLDER),
    _op("qnnp_setup_softargmax_nc_q8", _SETUP_NC, UNLESS_OLDER),
    # operators of the product only
    _op("qnnp_gfx950_create_lut_nc_x8", "size_t channels, u8[256] table, u32 flags=0, out lut", IF_PRESENT,
        doc="the product's table operator (qnnp_gfx950_create_lut_nc_x8); `table`: 256 uint8, or None"),
    _op("qnnp_gfx950_setup_lut_nc_x8", _SETUP_NC, IF_PRESENT),
    _op("qnnp_gfx950_create_hardswish_nc_q8", "size_t channels, " + _IN_Q + _OUT_Q + "hardswish", IF_PRESENT, doc=_LUT_DOC),
    _op("qnnp_gfx950_create_hardsigmoid_nc_q8", "size_t channels, " + _IN_Q + _OUT_Q + "hardsigmoid", IF_PRESENT, doc=_LUT_DOC),
    _op("qnnp_gfx950_create_multiply_nc_q8", _BINARY_Q.format("product") + "multiply", IF_PRESENT,
        doc="the product's multiply operator (qnnp_gfx950_create_multiply_nc_q8)"),
    _op("qnnp_gfx950_setup_multiply_nc_q8",
        "ptr op, size_t b_rows, size_t a_rows_per_b_row, tensor a, size_t a_stride, tensor b, size_t b_stride, "
        "tensor product, size_t product_stride", IF_PRESENT),
    _op("qnnp_gfx950_create_resize_bilinear2d_nhwc_u8", "size_t channels, u32 flags=0, out resize", IF_PRESENT,
        doc="the product's bilinear resize operator (qnnp_gfx950_create_resize_bilinear2d_nhwc_u8); flags: RESIZE_ALIGN_CORNERS"),
    _op("qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8",
        "ptr op, size_t batch_size, size_t input_height, size_t input_width, size_t output_height, size_t output_width, "
        "tensor input, size_t input_pixel_stride, tensor output, size_t output_pixel_stride", IF_PRESENT),
)

# the rest of include/qnnpack_gfx950.h and include/qnnpack_gfx950_test.h: Gfx950Library's own methods call these
GFX950_API = (
    _fn("qnnp_gfx950_set_device", "int device"),
    _fn("qnnp_gfx950_get_device"),
    _fn("qnnp_gfx950_device_count"),
    _fn("qnnp_gfx950_set_stream", "ptr hip_stream"),
    _fn("qnnp_gfx950_set_async", "int async"),
    _fn("qnnp_gfx950_synchronize"),
    _fn("qnnp_gfx950_malloc", "size_t bytes", restype=c_void_p),
    _fn("qnnp_gfx950_free", "ptr device_ptr", restype=None),
    _fn("qnnp_gfx950_memcpy_h2d", "ptr dst_device, ptr src_host, size_t bytes"),
    _fn("qnnp_gfx950_memcpy_d2h", "ptr dst_host, ptr src_device, size_t bytes"),
    _fn("qnnp_gfx950_memset", "ptr dst_device, int value, size_t bytes"),
    _fn("qnnp_gfx950_time_operator", "ptr op, int warmup, int iters, f32* avg_ms_out"),
    _fn("qnnp_gfx950_time_operator_rotating",
        "ptr op, size_t nsets, ptr* inputs, ptr* outputs, int warmup, int iters, f32* avg_ms_out"),
    _fn("qnnp_gfx950_graph_begin"),
    _fn("qnnp_gfx950_graph_end", "ptr* graph_out"),
    _fn("qnnp_gfx950_graph_launch", "ptr graph"),
    _fn("qnnp_gfx950_graph_synchronize", "ptr graph"),
    _fn("qnnp_gfx950_graph_time", "ptr graph, int warmup, int iters, f32* avg_ms_out"),
    _fn("qnnp_gfx950_graph_destroy", "ptr graph", restype=None),
    _op("qnnp_gfx950_create_fused_block", "ptr expand, ptr depthwise, ptr project, ptr residual_add=None, out fused"),
    _op("qnnp_gfx950_setup_fused_block", _SETUP_NHWC),
    _op("qnnp_gfx950_attach_residual_add", "ptr convolution, ptr add, tensor residual, size_t residual_stride", UNLESS_OLDER),
    _fn("qnnp_gfx950_operator_residual_folded", "ptr op", UNLESS_OLDER),
    _fn("qnnp_gfx950_set_option", "str key, int value"),
    _fn("qnnp_gfx950_test_force_kernel", "str family, int code"),
    _fn("qnnp_gfx950_test_operator_ran_dense", "ptr op"),
    _fn("qnnp_gfx950_operator_set_streaming_stores", "ptr op, int value"),
    _fn("qnnp_gfx950_operator_kernel", "ptr op", restype=c_char_p),
    _fn("qnnp_gfx950_device_info", "str arch, size_t arch_len, int* compute_units, int* clock_khz, size_t* hbm_bytes"),
)

API = {f.symbol: f for f in QNNPACK_API + GFX950_API}

# include/qnnpack_gfx950_float.h: float32 <-> uint8 at the two ends of a network. A table of its own, bound and installed
# on Gfx950Library only: API above stays the image of the three headers it is checked against. Float strides count
# elements, byte strides bytes.
FLOAT_API = (
    _op("qnnp_gfx950_create_quantize_nc_f32_q8",
        "size_t channels, u8 output_zero_point, f32 output_scale, u8 output_min, u8 output_max, u32 flags=0, out quantize",
        IF_PRESENT, doc="the product's quantize operator: set it up with setup_quantize_nc_f32_q8 (rows) or "
                        "setup_quantize_nchw_f32_nhwc_q8 (planar float in, NHWC uint8 out)"),
    _op("qnnp_gfx950_setup_quantize_nc_f32_q8", _SETUP_NC, IF_PRESENT),
    _op("qnnp_gfx950_setup_quantize_nchw_f32_nhwc_q8",
        "ptr op, size_t batch_size, size_t pixels, tensor input, tensor output, size_t output_pixel_stride", IF_PRESENT),
    _op("qnnp_gfx950_create_dequantize_nc_q8_f32",
        "size_t channels, u8 input_zero_point, f32 input_scale, u32 flags=0, out dequantize",
        IF_PRESENT, doc="the product's dequantize operator: set it up with setup_dequantize_nc_q8_f32 (rows) or "
                        "setup_dequantize_nhwc_q8_nchw_f32 (NHWC uint8 in, planar float out)"),
    _op("qnnp_gfx950_setup_dequantize_nc_q8_f32", _SETUP_NC, IF_PRESENT),
    _op("qnnp_gfx950_setup_dequantize_nhwc_q8_nchw_f32",
        "ptr op, size_t batch_size, size_t pixels, tensor input, size_t input_pixel_stride, tensor output", IF_PRESENT),
)


# include/qnnpack_gfx950_perchannel.h: convolution and fully connected with one weight scale per output channel. A table
# of its own like FLOAT_API, for the same reason. `kernel_scales`: groups * group_output_channels (output_channels) floats;
# setup, run and delete are the per-tensor operators' (setup_convolution2d_nhwc_q8, setup_fully_connected_nc_q8, ...).
_WEIGHTS_Q_PER_CHANNEL = _IN_Q + "u8 kernel_zero_point, f32[] kernel_scales, u8[] kernel, i32[] bias, " + _OUT_Q
PERCHANNEL_API = (
    _op("qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel",
        _PADDING + "u32 kernel_height, u32 kernel_width, u32 subsampling_height, u32 subsampling_width, "
        "u32 dilation_height, u32 dilation_width, " + _GROUPS + _WEIGHTS_Q_PER_CHANNEL + "convolution", IF_PRESENT,
        doc="qnnp_create_convolution2d_nhwc_q8 with one kernel scale per output channel (all groups); set it up with "
            "setup_convolution2d_nhwc_q8"),
    _op("qnnp_gfx950_create_fully_connected_nc_q8_per_channel",
        "size_t input_channels, size_t output_channels, " + _WEIGHTS_Q_PER_CHANNEL + "fully_connected", IF_PRESENT,
        doc="qnnp_create_fully_connected_nc_q8 with one kernel scale per output channel; set it up with "
            "setup_fully_connected_nc_q8"),
)


# include/qnnpack_gfx950_squeeze_excite.h (which qnnpack_gfx950.h includes): the fused squeeze-and-excite block, built from
# five stand-alone operators as the fused block is from three. A table of its own like FLOAT_API, for the same reason.
SQUEEZE_EXCITE_API = (
    _op("qnnp_gfx950_create_squeeze_excite", "ptr pool, ptr fc1, ptr fc2, ptr gate, ptr multiply, out squeeze_excite",
        IF_PRESENT, doc="the fused squeeze-and-excite block over its five members, which it borrows and which must "
                        "outlive it; set it up with setup_squeeze_excite"),
    _op("qnnp_gfx950_setup_squeeze_excite",
        "ptr op, size_t batch_size, size_t pixels, tensor input, size_t input_pixel_stride, tensor output, "
        "size_t output_pixel_stride", IF_PRESENT),
)


# include/qnnpack_gfx950_output_table.h (which qnnpack_gfx950.h includes): a byte table folded behind a convolution. A table
# of its own like FLOAT_API, for the same reason. `table`: a table operator, or None to detach.
OUTPUT_TABLE_API = (
    _op("qnnp_gfx950_attach_output_table", "ptr convolution, ptr table", IF_PRESENT,
        doc="from now on `convolution` writes table[b] for every output byte b; the table operator's 256 bytes are copied "
            "(it may be deleted); table=None detaches"),
    _fn("qnnp_gfx950_operator_table_folded", "ptr op", IF_PRESENT),
)


def _bind(lib, table) -> None:
    """Set argtypes / restype of the table's symbols on a loaded library."""
    older = bool(os.environ.get("QNNP_GFX950_LIBRARY"))
    for f in table:
        if (f.bound == IF_PRESENT or (f.bound == UNLESS_OLDER and older)) and not hasattr(lib, f.symbol):
            continue
        c_function = getattr(lib, f.symbol)
        c_function.restype = f.restype
        c_function.argtypes = f.argtypes


def _method_pair(f: Function):
    """<name>_status, which returns the Status (and the new handle, where the function creates one), and <name>, which
    raises QnnpackError for any status but success."""
    name = f.symbol.replace("qnnp_", "", 1).replace("gfx950_", "", 1)
    creates = bool(f.params) and f.params[-1].kind == "out"
    signature = inspect.Signature(
        [inspect.Parameter("self", inspect.Parameter.POSITIONAL_OR_KEYWORD)]
        + [inspect.Parameter(p.name, inspect.Parameter.POSITIONAL_OR_KEYWORD, default=p.default)
           for p in f.params if p.kind not in ("out", "null")])

    def status(self, *args, **kwargs):
        given = signature.bind(self, *args, **kwargs)
        given.apply_defaults()
        handle = c_void_p(None)
        host_arrays = []        # alive until the call has returned
        c_args = []
        for p in f.params:
            if p.kind == "out":
                c_args.append(ctypes.byref(handle))
                continue
            value = None if p.kind == "null" else given.arguments[p.name]
            if p.kind in _HOST_ARRAYS and value is not None:
                dtype, size = _HOST_ARRAYS[p.kind]
                value = np.ascontiguousarray(value, dtype=dtype)
                assert size is None or value.size == size, value.size
                host_arrays.append(value)
            c_args.append(address_of(value) if p.kind == "tensor" or p.kind in _HOST_ARRAYS else value)
        st = Status(getattr(self.lib, f.symbol)(*c_args))
        return (st, handle.value) if creates else st

    def checked(self, *args, **kwargs):
        result = getattr(self, status.__name__)(*args, **kwargs)
        st, handle = result if creates else (result, None)
        if st != Status.success:
            raise QnnpackError(f.symbol, st)
        return handle

    status.__name__, checked.__name__ = name + "_status", name
    status.__signature__ = checked.__signature__ = signature
    status.__doc__ = checked.__doc__ = f.doc
    return status, checked


def _with_methods_of(table):
    """Class decorator: the generated methods of the table's operator functions become attributes of the class."""
    def install(cls):
        for f in table:
            if f.methods:
                for method in _method_pair(f):
                    method.__qualname__ = f"{cls.__qualname__}.{method.__name__}"
                    method.__module__ = cls.__module__
                    setattr(cls, method.__name__, method)
        return cls
    return install


@_with_methods_of(QNNPACK_API)
class QnnpackLibrary:
    """The C API of include/qnnpack.h bound over ``path``.

    Every operator function of QNNPACK_API is two methods, e.g. create_add_nc_q8_status(...) -> (Status, handle or None)
    and create_add_nc_q8(...) -> handle, setup_add_nc_q8_status(op, ...) -> Status and setup_add_nc_q8(op, ...) -> None;
    tests of error behaviour use the _status forms, the others raise QnnpackError.
    """

    RESIZE_ALIGN_CORNERS = 0x00000001   # QNNP_GFX950_RESIZE_ALIGN_CORNERS (include/qnnpack_gfx950.h)

    def __init__(self, path: str):
        self.path = path
        self.lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        _bind(self.lib, QNNPACK_API)

    def deinitialize(self) -> Status:
        return Status(self.lib.qnnp_deinitialize())


@_with_methods_of(GFX950_API + FLOAT_API + PERCHANNEL_API + SQUEEZE_EXCITE_API + OUTPUT_TABLE_API)
class Gfx950Library(QnnpackLibrary):
    """Product library: qnnpack.h plus the extensions of include/qnnpack_gfx950.h (GFX950_API), the float32 <-> uint8
    operators of include/qnnpack_gfx950_float.h (FLOAT_API) and the per-channel creates of
    include/qnnpack_gfx950_perchannel.h (PERCHANNEL_API), and the fused squeeze-and-excite block of
    include/qnnpack_gfx950_squeeze_excite.h (SQUEEZE_EXCITE_API), and the output table of
    include/qnnpack_gfx950_output_table.h (OUTPUT_TABLE_API).

    Generated as above: the fused inverted-residual block ([create|setup]_fused_block[_status]), the residual add
    folded into a convolution (attach_residual_add[_status]), quantize / dequantize with their two setups each, and
    create_convolution2d_nhwc_q8_per_channel / create_fully_connected_nc_q8_per_channel, and
    [create|setup]_squeeze_excite[_status], and attach_output_table[_status].
    """

    def __init__(self, path: str):
        super().__init__(path)
        _bind(self.lib, GFX950_API)
        _bind(self.lib, FLOAT_API)
        _bind(self.lib, PERCHANNEL_API)
        _bind(self.lib, SQUEEZE_EXCITE_API)
        _bind(self.lib, OUTPUT_TABLE_API)

    def _check(self, call: str, st: int) -> None:
        if st != 0:
            raise QnnpackError(call, st)

    def set_device(self, device: int) -> None:
        self._check("qnnp_gfx950_set_device", self.lib.qnnp_gfx950_set_device(device))

    def get_device(self) -> int:
        return self.lib.qnnp_gfx950_get_device()

    def device_count(self) -> int:
        return self.lib.qnnp_gfx950_device_count()

    def set_stream(self, stream: Optional[int]) -> None:
        self._check("qnnp_gfx950_set_stream", self.lib.qnnp_gfx950_set_stream(stream))

    def set_async(self, enabled: bool) -> None:
        self._check("qnnp_gfx950_set_async", self.lib.qnnp_gfx950_set_async(1 if enabled else 0))

    def synchronize(self) -> None:
        self._check("qnnp_gfx950_synchronize", self.lib.qnnp_gfx950_synchronize())

    def malloc(self, nbytes: int) -> int:
        p = self.lib.qnnp_gfx950_malloc(nbytes)
        if not p:
            raise MemoryError(f"qnnp_gfx950_malloc({nbytes})")
        return p

    def free(self, ptr: int) -> None:
        self.lib.qnnp_gfx950_free(ptr)

    def memcpy_h2d(self, dst: int, src: np.ndarray) -> None:
        src = np.ascontiguousarray(src)
        self._check("qnnp_gfx950_memcpy_h2d", self.lib.qnnp_gfx950_memcpy_h2d(dst, src.ctypes.data, src.nbytes))

    def memcpy_d2h(self, dst: np.ndarray, src: int) -> None:
        assert dst.flags["C_CONTIGUOUS"]
        self._check("qnnp_gfx950_memcpy_d2h", self.lib.qnnp_gfx950_memcpy_d2h(dst.ctypes.data, src, dst.nbytes))

    def memset(self, dst: int, value: int, nbytes: int) -> None:
        self._check("qnnp_gfx950_memset", self.lib.qnnp_gfx950_memset(dst, value, nbytes))

    def time_operator(self, op, warmup: int, iters: int) -> float:
        ms = c_float(0.0)
        self._check("qnnp_gfx950_time_operator",
                    self.lib.qnnp_gfx950_time_operator(op, warmup, iters, ctypes.byref(ms)))
        return float(ms.value)

    def time_operator_rotating(self, op, inputs, outputs, warmup: int, iters: int) -> float:
        n = len(inputs)
        assert n == len(outputs) and n > 0
        ins = (c_void_p * n)(*[address_of(x) for x in inputs])
        outs = (c_void_p * n)(*[address_of(x) for x in outputs])
        ms = c_float(0.0)
        self._check("qnnp_gfx950_time_operator_rotating",
                    self.lib.qnnp_gfx950_time_operator_rotating(op, n, ins, outs, warmup, iters, ctypes.byref(ms)))
        return float(ms.value)

    def operator_residual_folded(self, op) -> int:
        """After a run: 1 = the add rode in the convolution kernel's epilogue, 0 = separate launch, -1 = none attached."""
        return int(self.lib.qnnp_gfx950_operator_residual_folded(op))

    def operator_table_folded(self, op) -> int:
        """After a run: 1 = the table rode in the convolution kernel's epilogue, 0 = separate launch, -1 = none attached."""
        return int(self.lib.qnnp_gfx950_operator_table_folded(op))

    # ---- hipGraph capture of operator launches (qnnpack_gfx950.h) ----
    def graph_begin(self) -> None:
        self._check("qnnp_gfx950_graph_begin", self.lib.qnnp_gfx950_graph_begin())

    def graph_end(self) -> int:
        g = c_void_p()
        self._check("qnnp_gfx950_graph_end", self.lib.qnnp_gfx950_graph_end(ctypes.byref(g)))
        return g.value

    def graph_launch(self, graph: int) -> None:
        self._check("qnnp_gfx950_graph_launch", self.lib.qnnp_gfx950_graph_launch(graph))

    def graph_synchronize(self, graph: int) -> None:
        self._check("qnnp_gfx950_graph_synchronize", self.lib.qnnp_gfx950_graph_synchronize(graph))

    def graph_time(self, graph: int, warmup: int, iters: int) -> float:
        ms = c_float(0.0)
        self._check("qnnp_gfx950_graph_time", self.lib.qnnp_gfx950_graph_time(graph, warmup, iters, ctypes.byref(ms)))
        return float(ms.value)

    def graph_destroy(self, graph: int) -> None:
        self.lib.qnnp_gfx950_graph_destroy(graph)

    def set_option(self, key: str, value: int) -> None:
        if key in ("gemm_kernel", "dwconv_kernel", "fused_kernel", "fused_rows", "fused_weights", "se_kernel"):
            # kernel-forcing codes are test / measurement hooks (include/qnnpack_gfx950_test.h), not product options
            self._check("qnnp_gfx950_test_force_kernel", self.lib.qnnp_gfx950_test_force_kernel(key.encode(), value))
            return
        self._check("qnnp_gfx950_set_option", self.lib.qnnp_gfx950_set_option(key.encode(), value))

    def operator_set_streaming_stores(self, op, value: int) -> None:
        """1 / 0: the streaming-store hint of this operator's launches; -1: follow the process-wide option again."""
        self._check("qnnp_gfx950_operator_set_streaming_stores", self.lib.qnnp_gfx950_operator_set_streaming_stores(op, value))

    def operator_ran_dense(self, op) -> bool:
        """include/qnnpack_gfx950_test.h: the operator's last run took the dense image of a grouped 1x1 convolution"""
        return bool(self.lib.qnnp_gfx950_test_operator_ran_dense(op))

    def operator_kernel(self, op) -> Optional[str]:
        name = self.lib.qnnp_gfx950_operator_kernel(op)
        return name.decode() if name else None

    def device_info(self) -> dict:
        arch = ctypes.create_string_buffer(64)
        cus, clk, mem = c_int(0), c_int(0), c_size_t(0)
        self._check("qnnp_gfx950_device_info",
                    self.lib.qnnp_gfx950_device_info(arch, 64, ctypes.byref(cus), ctypes.byref(clk), ctypes.byref(mem)))
        return {"arch": arch.value.decode(), "compute_units": cus.value, "clock_khz": clk.value,
                "hbm_bytes": mem.value}
