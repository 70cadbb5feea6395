"""CPU tier, no built library: the binding's tables (qnnpack_amd/binding.py) say what the public headers say, and the
methods generated from them forward their arguments to the C function in the header's order."""
import ctypes
import inspect
from ctypes import c_char_p, c_float, c_int, c_size_t, c_uint8, c_uint32, c_void_p

import numpy as np
import pytest

from qnnpack_amd import binding
from qnnpack_amd.binding import API, Gfx950Library, QnnpackError, QnnpackLibrary, Status

from _headers import HEADERS, declared_functions, prototypes

PROTOTYPES = {name: proto for header in HEADERS for name, proto in prototypes(header).items()}
SCALARS = {"size_t": c_size_t, "uint32_t": c_uint32, "uint8_t": c_uint8, "float": c_float, "int": c_int,
           "enum qnnp_status": c_int}
# the only parameters whose Python name is not the header's, besides `op` for the function's own operator handle
PYTHON_NAMES = {"input_padding_top": "pad_top", "input_padding_right": "pad_right",
                "input_padding_bottom": "pad_bottom", "input_padding_left": "pad_left"}
GENERATED = [f for f in API.values() if f.methods]
HANDLE = 0x7E57AB1E


def is_pointer(ctype):
    return ctype in (c_void_p, c_char_p) or (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))


def is_c_pointer(c_type):
    return "*" in c_type or c_type.endswith("[]") or c_type in ("qnnp_operator_t", "pthreadpool_t")


def python_name(f, c_type, header_name):
    name = PYTHON_NAMES.get(header_name, header_name)
    if c_type == "qnnp_operator_t" and name not in [p.name for p in f.params]:
        return "op"
    return name


# ---- the headers against the tables ----
def test_the_parser_finds_every_declared_function_and_the_tables_hold_exactly_those():
    declared = {name for header in HEADERS for name in declared_functions(header)}
    assert set(PROTOTYPES) == declared
    assert len(declared) == 65, len(declared)
    assert set(API) == declared
    assert len(binding.QNNPACK_API) + len(binding.GFX950_API) == len(API), "a symbol is in the tables twice"


@pytest.mark.parametrize("symbol", sorted(PROTOTYPES))
def test_table_entry_is_the_image_of_the_prototype(symbol):
    ret, params = PROTOTYPES[symbol]
    f = API[symbol]
    if ret == "void":
        assert f.restype is None
    elif ret == "char*":
        assert f.restype is c_char_p
    elif is_c_pointer(ret):
        assert is_pointer(f.restype), (ret, f.restype)
    else:
        assert f.restype is SCALARS[ret], (ret, f.restype)
    assert len(f.params) == len(params)
    for (c_type, header_name), p, ctype in zip(params, f.params, f.argtypes):
        if is_c_pointer(c_type):
            assert is_pointer(ctype), (header_name, c_type, ctype)
        else:
            assert ctype is SCALARS[c_type], (header_name, c_type, ctype)
        assert p.name == python_name(f, c_type, header_name), (p.name, header_name)


# ---- forwarding ----
class FakeFunction:
    def __init__(self, lib, name):
        self.lib, self.name = lib, name

    def __call__(self, *args):
        self.lib.calls.append((self.name, args))
        if self.lib.status == 0 and args and isinstance(getattr(args[-1], "_obj", None), c_void_p):
            args[-1]._obj.value = HANDLE       # a create writes the handle only on success
        return self.lib.status


class FakeLibrary:
    """Stands in for ctypes.CDLL: every qnnp_ symbol but `missing` is there, records its calls and answers `status`."""

    def __init__(self, missing=()):
        self.missing, self.calls, self.status = missing, [], 0

    def __getattr__(self, name):
        if not name.startswith("qnnp_") or name in self.missing:
            raise AttributeError(f"undefined symbol: {name}")
        function = FakeFunction(self, name)
        setattr(self, name, function)
        return function


class FakeTensor:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def load(monkeypatch, cls=Gfx950Library, missing=(), older=False):
    fake = FakeLibrary(missing)
    monkeypatch.setattr(ctypes, "CDLL", lambda path, mode=0: fake)
    if older:
        monkeypatch.setenv("QNNP_GFX950_LIBRARY", "/somewhere/libqnnpack_gfx950_older.so")
    else:
        monkeypatch.delenv("QNNP_GFX950_LIBRARY", raising=False)
    return cls("libfake.so"), fake


def method_name(f):
    return f.symbol.replace("qnnp_", "", 1).replace("gfx950_", "", 1)


def distinct_arguments(f):
    """{Python name: value}, and what the C function must receive for it, for every parameter the method takes."""
    given, received = {}, {}
    for i, p in enumerate(f.params):
        if p.kind in ("out", "null"):
            continue
        if p.kind == "tensor":
            given[p.name], received[p.name] = FakeTensor(0x2000 + 16 * i), 0x2000 + 16 * i
        elif p.kind in binding._HOST_ARRAYS:
            dtype, size = binding._HOST_ARRAYS[p.kind]
            given[p.name] = np.arange(size or 8 + i).astype(dtype)
            received[p.name] = given[p.name].ctypes.data
        else:
            given[p.name] = received[p.name] = (i + 0.5) if p.kind == "f32" else 0x100 + i
    return given, received


def c_arguments_in_header_order(f, received):
    expected = []
    for c_type, header_name in PROTOTYPES[f.symbol][1]:
        name = python_name(f, c_type, header_name)
        expected.append(received.get(name, "handle by reference" if c_type == "qnnp_operator_t*" else None))
    return expected


def seen(args):
    return ["handle by reference" if isinstance(getattr(a, "_obj", None), c_void_p) else a for a in args]


def test_load_sets_argtypes_and_restype_from_the_tables(monkeypatch):
    _, fake = load(monkeypatch)
    for f in API.values():
        assert getattr(fake, f.symbol).argtypes == f.argtypes, f.symbol
        assert getattr(fake, f.symbol).restype is f.restype, f.symbol
    for symbol in ("qnnp_gfx950_get_device", "qnnp_gfx950_synchronize"):
        assert getattr(fake, symbol).argtypes == []
    _, fake = load(monkeypatch, QnnpackLibrary)
    assert {name for name in vars(fake) if name.startswith("qnnp_")} == {f.symbol for f in binding.QNNPACK_API}


@pytest.mark.parametrize("f", GENERATED, ids=lambda f: f.symbol)
def test_generated_methods_forward_in_header_order(monkeypatch, f):
    lib, fake = load(monkeypatch)
    name = method_name(f)
    given, received = distinct_arguments(f)
    expected = c_arguments_in_header_order(f, received)
    creates = bool(f.params) and f.params[-1].kind == "out"
    for cls in (QnnpackLibrary, Gfx950Library):         # real attributes of the class that has the function's table
        assert (name in vars(cls)) == (f in getattr(binding, "QNNPACK_API" if cls is QnnpackLibrary else "GFX950_API"))
    for method_name_ in (name + "_status", name):
        method = getattr(lib, method_name_)
        assert method.__name__ == method_name_ and method.__self__ is lib
        assert list(inspect.signature(method).parameters) == list(given)
        for call in (lambda: method(**given), lambda: method(*given.values())):     # by keyword, by position
            fake.calls.clear()
            result = call()
            assert [(symbol, seen(args)) for symbol, args in fake.calls] == [(f.symbol, expected)]
            if method.__name__.endswith("_status"):
                assert result == ((Status.success, HANDLE) if creates else Status.success)
                assert isinstance(result[0] if creates else result, Status)
            else:
                assert result == (HANDLE if creates else None)
    fake.status = int(Status.invalid_parameter)
    assert getattr(lib, name + "_status")(**given) == ((Status.invalid_parameter, None) if creates else Status.invalid_parameter)
    with pytest.raises(QnnpackError) as raised:
        getattr(lib, name)(**given)
    assert str(raised.value) == f"{f.symbol} -> qnnp_status_invalid_parameter"
    assert raised.value.status == Status.invalid_parameter


def test_defaults_null_arrays_and_array_coercion(monkeypatch):
    lib, fake = load(monkeypatch)
    # flags, residual_add and threadpool may be left out; None is NULL
    assert lib.create_clamp_nc_u8(8, 1, 2) == HANDLE
    assert seen(fake.calls[-1][1]) == [8, 1, 2, 0, "handle by reference"]
    lib.create_fused_block(11, 12, 13)
    assert seen(fake.calls[-1][1]) == [11, 12, 13, None, "handle by reference"]
    lib.run_operator(21)
    assert fake.calls[-1] == ("qnnp_run_operator", (21, None))
    lib.setup_clamp_nc_u8(21, 1, None, 8, None, 8)
    assert fake.calls[-1][1] == (21, 1, None, 8, None, 8)
    lib.create_fully_connected_nc_q8(4, 4, 0, 1.0, 0, 1.0, None, None, 0, 1.0, 0, 255)
    assert fake.calls[-1][1][6:8] == (None, None)
    # anything array-like is made a contiguous array of the C element type first
    lib.create_fully_connected_nc_q8(2, 2, 0, 1.0, 0, 1.0, [[1, 2], [3, 4]], np.arange(4.0)[::2], 0, 1.0, 0, 255)
    assert all(isinstance(a, int) and a for a in fake.calls[-1][1][6:8])
    with pytest.raises(AssertionError):
        lib.create_lut_nc_x8(8, np.zeros(255, np.uint8))
    # a misspelt method fails at lookup, and hardswish / hardsigmoid are set up as table operators
    with pytest.raises(AttributeError):
        lib.create_clamp_nc_q8
    assert not hasattr(lib, "setup_hardswish_nc_q8") and not hasattr(lib, "setup_hardsigmoid_nc_q8")
    for name in ("create_deconvolution2d_nhwc_q8", "create_lut_nc_x8", "create_multiply_nc_q8",
                 "create_resize_bilinear2d_nhwc_u8", "create_hardswish_nc_q8", "create_hardsigmoid_nc_q8"):
        assert getattr(QnnpackLibrary, name + "_status").__doc__, name


@pytest.mark.parametrize("older", [False, True], ids=["product", "QNNP_GFX950_LIBRARY"])
@pytest.mark.parametrize("f", API.values(), ids=lambda f: f.symbol)
def test_a_missing_symbol_by_binding_class(monkeypatch, f, older):
    if f.bound == binding.ALWAYS or (f.bound == binding.UNLESS_OLDER and not older):
        with pytest.raises(AttributeError, match=f.symbol):
            load(monkeypatch, missing=(f.symbol,), older=older)
        return
    assert f.bound in (binding.UNLESS_OLDER, binding.IF_PRESENT)
    lib, fake = load(monkeypatch, missing=(f.symbol,), older=older)
    assert f.symbol not in vars(fake)
    present = next(g for g in API.values() if g.bound == f.bound and g is not f)
    assert getattr(fake, present.symbol).argtypes == present.argtypes       # the others of its class are bound
    if f.methods:
        given, _ = distinct_arguments(f)
        for name in (method_name(f) + "_status", method_name(f)):
            with pytest.raises(AttributeError, match=f.symbol):
                getattr(lib, name)(**given)


def test_each_binding_class_has_the_symbols_it_had():
    by_class = {bound: {f.symbol for f in API.values() if f.bound == bound}
                for bound in (binding.UNLESS_OLDER, binding.IF_PRESENT)}
    assert by_class[binding.IF_PRESENT] == {
        "qnnp_gfx950_create_lut_nc_x8", "qnnp_gfx950_setup_lut_nc_x8", "qnnp_gfx950_create_multiply_nc_q8",
        "qnnp_gfx950_setup_multiply_nc_q8", "qnnp_gfx950_create_hardswish_nc_q8", "qnnp_gfx950_create_hardsigmoid_nc_q8",
        "qnnp_gfx950_create_resize_bilinear2d_nhwc_u8", "qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8"}
    assert by_class[binding.UNLESS_OLDER] == {
        side + operator for side in ("qnnp_create_", "qnnp_setup_")
        for operator in ("average_pooling2d_nhwc_q8", "max_pooling2d_nhwc_u8", "channel_shuffle_nc_x8", "clamp_nc_u8",
                         "sigmoid_nc_q8", "leaky_relu_nc_q8", "softargmax_nc_q8")
    } | {"qnnp_gfx950_attach_residual_add", "qnnp_gfx950_operator_residual_folded"}
