"""CPU tier of the per-channel convolution and fully connected operators (include/qnnpack_gfx950_perchannel.h;
convolution.c, fully-connected.c, per-channel.h, hip/requant_pc.h):

 * the requantization form both kernel families share, exported as qnnp_debug_requant_pc, against the oracle for every
   shift 0 ... 31 -- bit-exact, no tolerance;
 * the creates' statuses, case by case and in the documented order, and the table as the device received it, through the
   product's host code linked against the HIP stub (Makefile target stub-perchannel);
 * the header and the binding's PERCHANNEL_API are each other's image, and API stays the 65 functions of the three older
   headers;
 * the host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-perchannel), and the new
   kernels' resources: no scratch in hip/q8dwconv_pc.hip.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _perchannel as pc
from _headers import HEADERS, prototypes
from oracle import o1
from qnnpack_amd import Status, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qnnpack_amd", "csrc")
HEADER = "qnnpack_gfx950_perchannel.h"
FUNCTIONS = ["qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel", "qnnp_gfx950_create_fully_connected_nc_q8_per_channel"]
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the requantization form ------------------------------------------------------------------------------------------
def accumulators(seed):
    edge = [0, 1, -1, INT32_MIN, INT32_MAX]
    for k in range(31):
        for base in (2 ** k, -2 ** k):
            edge += [base, base + 1, base - 1]
    edge = [a for a in edge if INT32_MIN <= a <= INT32_MAX]
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array(edge, np.int64), rng.integers(INT32_MIN, INT32_MAX + 1, 2 ** 16)]).astype(np.int32)


def scales_of_shift(shift, rng):
    """the smallest, the largest and one random mantissa of the binade whose shift is `shift`"""
    low = np.float32(2.0 ** -(shift + 1))
    bits = low.view(np.uint32)
    return [low, np.uint32(bits | 0x7FFFFF).view(np.float32), np.uint32(bits | rng.integers(1, 0x7FFFFF)).view(np.float32)]


@pytest.mark.parametrize("shift", range(32))
def test_requantization_form_equals_the_oracle_at_every_shift(debug_hooks, shift):
    """0, +-1, +-2^k, +-(2^k +- 1), INT32_MIN, INT32_MAX and 2^16 random accumulators, at the smallest, the largest and one
    random mantissa, for zero points 0 / 128 / 255 and clamps [0, 255], [1, 254], [128, 128]"""
    fn = debug_hooks.lib.qnnp_debug_requant_pc
    fn.restype = None
    fn.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p]
    rq = debug_hooks.lib.qnnp_debug_compute_requant
    rq.restype = None
    rq.argtypes = [ctypes.c_float, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p]
    rng = np.random.default_rng(1000 + shift)
    acc = accumulators(shift)
    for scale in scales_of_shift(shift, rng):
        block = (ctypes.c_int32 * 8)()
        rq(scale, 0, 0, 255, block)
        assert block[3] == shift, (float(scale), block[3])          # struct qnnp_hip_requant: multiplier, mask, threshold, shift
        for zp in (0, 128, 255):
            for qmin, qmax in ((0, 255), (1, 254), (128, 128)):
                got = np.empty(acc.size, np.uint8)
                fn(acc.size, acc.ctypes.data, scale, zp, qmin, qmax, got.ctypes.data)
                want = o1.q31_requantize(acc, scale, zp, qmin, qmax)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (float(scale), zp, qmin, qmax, bad.size, int(acc[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))


# ---- the host code over the HIP stub ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stub():
    """the product's host C code + tests/hip_stub.c as one shared library: "device" memory is host memory"""
    build = subprocess.run(["make", "-C", CSRC, "stub-perchannel"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    lib = ctypes.CDLL(os.path.join(CSRC, "build", "stub", "libqnnpack_perchannel_stub.so"), mode=ctypes.RTLD_LOCAL)
    for f in binding.PERCHANNEL_API + tuple(binding.API[s] for s in ("qnnp_initialize", "qnnp_delete_operator")):
        getattr(lib, f.symbol).restype, getattr(lib, f.symbol).argtypes = f.restype, f.argtypes
    lib.qnnp_stub_per_channel_info.restype = ctypes.c_int
    lib.qnnp_stub_per_channel_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                               ctypes.c_void_p, ctypes.c_size_t]
    lib.qnnp_stub_operator_clamp.restype = None
    lib.qnnp_stub_operator_clamp.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int32)] * 3
    lib.qnnp_stub_live_allocs.restype = ctypes.c_size_t
    assert lib.qnnp_initialize() == Status.success
    return lib


def conv_create(stub, ks, groups=1, gic=8, goc=33, kernel=(3, 3), input_scale=0.75, output_scale=1.5, kernel_ptr=True,
                bias_ptr=True, stride=(1, 1), dilation=(1, 1), kzp=128, ozp=9, omin=1, omax=250):
    n = groups * goc
    w = np.arange(n * kernel[0] * kernel[1] * gic, dtype=np.uint32).astype(np.uint8)
    b = np.arange(n, dtype=np.int32) * 7 - 100
    scales = None if ks is None else np.ascontiguousarray(ks, np.float32)
    handle = ctypes.c_void_p(None)
    st = stub.qnnp_gfx950_create_convolution2d_nhwc_q8_per_channel(
        1, 1, 1, 1, kernel[0], kernel[1], stride[0], stride[1], dilation[0], dilation[1], groups, gic, goc, 127, input_scale, kzp,
        None if scales is None else scales.ctypes.data, w.ctypes.data if kernel_ptr else None,
        b.ctypes.data if bias_ptr else None, ozp, output_scale, omin, omax, 0, ctypes.byref(handle))
    return Status(st), handle.value


def fc_create(stub, ks, k=8, n=33, input_scale=0.75, output_scale=1.5, kernel_ptr=True, bias_ptr=True):
    w = np.arange(n * k, dtype=np.uint32).astype(np.uint8)
    b = np.arange(n, dtype=np.int32)
    scales = None if ks is None else np.ascontiguousarray(ks, np.float32)
    handle = ctypes.c_void_p(None)
    st = stub.qnnp_gfx950_create_fully_connected_nc_q8_per_channel(
        k, n, 127, input_scale, 128, None if scales is None else scales.ctypes.data, w.ctypes.data if kernel_ptr else None,
        b.ctypes.data if bias_ptr else None, 9, output_scale, 1, 250, 0, ctypes.byref(handle))
    return Status(st), handle.value


GOOD = pc.channel_scales(33)
NAN, INF = float("nan"), float("inf")


def with_scale(at, value):
    ks = GOOD.copy()
    ks[at] = value
    return ks


STATUS_CASES = [
    # invalid_parameter, in the order of the per-tensor create
    ("zero window", dict(kernel=(0, 3)), Status.invalid_parameter),
    ("zero subsampling", dict(stride=(1, 0)), Status.invalid_parameter),
    ("zero dilation", dict(dilation=(0, 1)), Status.invalid_parameter),
    ("input scale 0", dict(input_scale=0.0), Status.invalid_parameter),
    ("input scale inf", dict(input_scale=INF), Status.invalid_parameter),
    ("kernel_scales NULL", dict(ks=None), Status.invalid_parameter),
    ("output scale negative", dict(output_scale=-1.0), Status.invalid_parameter),
    ("output scale NaN", dict(output_scale=NAN), Status.invalid_parameter),
    ("no groups", dict(groups=0), Status.invalid_parameter),
    ("no input channels", dict(gic=0), Status.invalid_parameter),
    ("kernel NULL", dict(kernel_ptr=False), Status.invalid_parameter),
    ("bias NULL", dict(bias_ptr=False), Status.invalid_parameter),
] + [(f"kernel scale {value} at {at}", dict(ks=with_scale(at, value)), Status.invalid_parameter)
     for value in (0.0, -0.5, NAN, INF, -INF, 1.0e-40) for at in (0, 17, 32)] + [
    # ... before any unsupported_parameter
    ("invalid scale before the range", dict(ks=with_scale(32, 0.0), output_scale=1.0e-9), Status.invalid_parameter),
    ("NULL scales before the range", dict(ks=None, output_scale=1.0e-9), Status.invalid_parameter),
    # unsupported_parameter: scale_c = 0.75 * ks[c] / 1.5 outside [2^-32, 1)
] + [(f"scale_c {what} at {at}", dict(ks=with_scale(at, value)), Status.unsupported_parameter)
     for what, value in (("1", 2.0), ("above 1", 300.0), ("2^-33", 2.0 ** -32), ("tiny", 1.0e-30)) for at in (0, 17, 32)] + [
    ("every scale_c above 1", dict(output_scale=1.0e-9), Status.unsupported_parameter),
    # and the edges of the range are inside it
    ("scale_c 2^-32", dict(ks=with_scale(5, 2.0 ** -31)), Status.success),
    ("scale_c 1 - 2^-24", dict(ks=with_scale(5, 2.0 * (1.0 - 2.0 ** -24))), Status.success),
    ("flavours: depthwise", dict(groups=33, gic=1, goc=1), Status.success),
    ("flavours: grouped", dict(groups=3, gic=4, goc=11), Status.success),
]


@pytest.mark.parametrize("what,how,want", STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_create_statuses_in_order(stub, what, how, want):
    live = stub.qnnp_stub_live_allocs()
    for create in (conv_create, fc_create):
        args = dict(how)
        if create is fc_create:
            if {"kernel", "stride", "dilation", "groups"} & set(args):
                continue                                  # the fully connected create has no such parameter
            if "gic" in args:
                args["k"] = args.pop("gic")
        args.setdefault("ks", GOOD)
        st, handle = create(stub, **args)
        assert st == want, (create.__name__, what, st)
        if want == Status.success:
            assert handle and stub.qnnp_delete_operator(handle) == Status.success
        else:
            assert not handle, "a refused create writes no handle"
    assert stub.qnnp_stub_live_allocs() == live


def uploaded_table(stub, handle):
    runs, pad = ctypes.c_uint32(0), ctypes.c_uint32(0)
    table = np.zeros(2 * 4096, np.int32)
    assert stub.qnnp_stub_per_channel_info(handle, ctypes.byref(runs), ctypes.byref(pad), table.ctypes.data, 4096) == 1
    return runs.value, pad.value, table[:2 * runs.value * pad.value].reshape(runs.value, pad.value, 2)


@pytest.mark.parametrize("flavour,groups,gic,goc,pad", [
    ("dense", 1, 8, 33, 64), ("dense_1", 1, 8, 1, 32), ("dense_32", 1, 3, 32, 32), ("grouped", 3, 4, 11, 32),
    ("grouped_5", 2, 5, 5, 32), ("depthwise", 33, 1, 1, 48), ("depthwise_3", 3, 1, 1, 16), ("depthwise_16", 16, 1, 1, 16)])
def test_uploaded_table_is_compute_requant_per_channel_with_valid_pads(stub, debug_hooks, flavour, groups, gic, goc, pad):
    """entry g * pad + oc is (multiplier, shift) of channel g * goc + oc as qnnp_compute_requant derives them from
    scale_c; the entries up to the kernels' channel pad are (2^30, 0); zero point and clamp stay in the operator"""
    rq = debug_hooks.lib.qnnp_debug_compute_requant
    rq.restype = None
    rq.argtypes = [ctypes.c_float, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p]
    n = groups * goc
    ks = pc.channel_scales(n)
    st, handle = conv_create(stub, ks, groups, gic, goc)
    assert st == Status.success
    try:
        runs, got_pad, table = uploaded_table(stub, handle)
        depthwise = gic == 1 and goc == 1 and groups > 1
        assert (runs, got_pad) == ((1, pad) if depthwise else (groups, pad))
        per_run = n if depthwise else goc
        for g in range(runs):
            for c in range(got_pad):
                if c < per_run:
                    block = (ctypes.c_int32 * 8)()
                    rq(pc.requant_scale(0.75, ks[g * per_run + c], 1.5), 0, 0, 255, block)
                    assert tuple(table[g, c]) == (block[0], block[3]), (g, c)
                    assert 2 ** 30 <= table[g, c, 0] < 2 ** 31 and 0 <= table[g, c, 1] <= 31
                else:
                    assert tuple(table[g, c]) == (2 ** 30, 0), (g, c)
        zp, lo, hi = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        stub.qnnp_stub_operator_clamp(handle, ctypes.byref(zp), ctypes.byref(lo), ctypes.byref(hi))
        assert (zp.value, lo.value, hi.value) == (9, 1 - 9, 250 - 9)
    finally:
        assert stub.qnnp_delete_operator(handle) == Status.success
    assert stub.qnnp_stub_live_allocs() == 0


def test_debug_table_is_the_uploaded_table(stub, debug_hooks):
    fill = debug_hooks.lib.qnnp_debug_per_channel_table
    fill.restype = None
    fill.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    ks = pc.channel_scales(33)
    st, handle = fc_create(stub, ks)
    assert st == Status.success
    try:
        runs, pad, table = uploaded_table(stub, handle)
        assert (runs, pad) == (1, 64)
        mine = np.zeros((1, 64, 2), np.int32)
        fill(1, 33, 64, 0.75, ks.ctypes.data, 1.5, mine.ctypes.data)
        assert np.array_equal(mine, table)
    finally:
        assert stub.qnnp_delete_operator(handle) == Status.success


# ---- interface --------------------------------------------------------------------------------------------------------
def test_header_and_table_are_each_others_image_and_api_is_untouched():
    from test_binding_signatures import SCALARS, is_c_pointer, is_pointer, python_name
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "qnnpack_gfx950.h"' in raw
    declared = prototypes(HEADER)
    assert sorted(declared) == sorted(FUNCTIONS)
    assert "Per-channel kernel zero points are out of scope" in re.sub(r"\s+\*?\s*", " ", raw)
    for header in HEADERS:
        assert not set(prototypes(header)) & set(FUNCTIONS), header
    assert [f.symbol for f in binding.PERCHANNEL_API] == FUNCTIONS
    for f, per_tensor in zip(binding.PERCHANNEL_API, ("qnnp_create_convolution2d_nhwc_q8", "qnnp_create_fully_connected_nc_q8")):
        ret, params = declared[f.symbol]
        assert ret == "enum qnnp_status" and f.restype is SCALARS[ret]
        assert f.bound == binding.IF_PRESENT and f.methods
        assert len(f.params) == len(params), f.symbol
        for (c_type, header_name), p, ctype in zip(params, f.params, f.argtypes):
            if is_c_pointer(c_type):
                assert is_pointer(ctype), (f.symbol, header_name, c_type, ctype)
            else:
                assert ctype is SCALARS[c_type], (f.symbol, header_name, c_type, ctype)
            assert p.name == python_name(f, c_type, header_name), (f.symbol, p.name, header_name)
        # the per-tensor create's parameters in its order, `float kernel_scale` replaced by `const float* kernel_scales`
        theirs = prototypes("qnnpack.h")[per_tensor][1]
        assert [("float*", "kernel_scales") if pair == ("float", "kernel_scale") else pair for pair in theirs] == params
        kinds = {p.name: p.kind for p in f.params}
        assert kinds["kernel_scales"] == "f32[]" and kinds["kernel"] == "u8[]" and kinds["bias"] == "i32[]"
    assert binding._HOST_ARRAYS["f32[]"] == (np.float32, None) and binding._CTYPES["f32[]"] is ctypes.c_void_p
    assert len(binding.API) == 65 and len(binding.QNNPACK_API) + len(binding.GFX950_API) == 65
    assert not set(FUNCTIONS) & set(binding.API)
    for name in ("create_convolution2d_nhwc_q8_per_channel", "create_fully_connected_nc_q8_per_channel"):
        for method in (name, name + "_status"):
            assert method in vars(binding.Gfx950Library) and not hasattr(binding.QnnpackLibrary, method), method


def test_library_exports_the_entry_points(product):
    for f in binding.PERCHANNEL_API:
        assert hasattr(product.lib, f.symbol), f.symbol
        assert getattr(product.lib, f.symbol).argtypes == f.argtypes


def test_generated_method_passes_a_float_array(monkeypatch):
    from test_binding_signatures import load, seen
    lib, fake = load(monkeypatch)
    lib.create_fully_connected_nc_q8_per_channel(2, 3, 0, 1.0, 128, [0.5, 0.25, 0.125], np.zeros((3, 2), np.uint8), [1, 2, 3], 0, 1.0, 0, 255)
    symbol, args = fake.calls[-1]
    assert symbol == "qnnp_gfx950_create_fully_connected_nc_q8_per_channel" and len(args) == 14
    scales = np.ctypeslib.as_array(ctypes.cast(args[5], ctypes.POINTER(ctypes.c_float)), (3,))
    assert args[:5] == (2, 3, 0, 1.0, 128) and isinstance(args[5], int)
    assert seen(args)[-1] == "handle by reference"
    del scales
    lib, fake = load(monkeypatch, missing=tuple(FUNCTIONS))          # an older library: bound if present
    with pytest.raises(AttributeError):
        lib.create_fully_connected_nc_q8_per_channel(2, 3, 0, 1.0, 128, [0.5] * 3, None, None, 0, 1.0, 0, 255)


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="CPU-only behaviour")
def test_without_a_gpu_create_is_uninitialized(product):
    assert product.initialize_status() == Status.unsupported_hardware
    ks = pc.channel_scales(4)
    st, handle = product.create_fully_connected_nc_q8_per_channel_status(4, 4, 0, 1.0, 128, ks, np.zeros(16, np.uint8),
                                                                         np.zeros(4, np.int32), 0, 1.0, 0, 255)
    assert st == Status.uninitialized and not handle
    st, handle = product.create_convolution2d_nhwc_q8_per_channel_status(
        0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 4, 4, 0, 1.0, 128, ks, np.zeros(16, np.uint8), np.zeros(4, np.int32), 0, 1.0, 0, 255)
    assert st == Status.uninitialized and not handle


# ---- host code and kernels --------------------------------------------------------------------------------------------
def test_per_channel_host_code_is_clean_under_asan_and_ubsan():
    build = subprocess.run(["make", "-C", CSRC, "asan-perchannel"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(CSRC, "build", "asan", "host_asan_perchannel_test")
    # the ASan runtime is linked statically (Makefile asan-perchannel), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-perchannel-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_per_channel_kernels_are_there_and_the_depthwise_ones_use_no_scratch(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/q8dwconv_pc.hip, and the per-channel instantiations of the
    generic GEMM kernel beside the per-tensor ones (last template argument)"""
    from test_kernel_resources import READELF, _code_objects
    lib = os.path.join(ROOT, "qnnpack_amd", "libqnnpack_gfx950.so")
    if not os.path.exists(lib) or not os.path.exists(READELF):
        pytest.skip("library or llvm-readelf not available")
    dw, gemm = {}, []
    for k, elf in enumerate(_code_objects(open(lib, "rb").read())):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(elf)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for entry in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            if "q8_dwconv_pc_kernel" in name:
                dw[name] = tuple(int(re.search(rf"\.{field}:\s+(\d+)", entry).group(1)) for field in (
                    "vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                    "max_flat_workgroup_size", "group_segment_fixed_size"))
            elif "q8_igemm_mfma_kernel" in name:
                gemm.append(name)
    assert len(dw) == 5, sorted(dw)                     # <3, 1> <3, 2> <5, 1> <5, 2> and <0, 0>
    for name, (vgpr, scratch, vspill, sspill, wg, lds) in dw.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        assert wg == 256 and vgpr <= 128 and lds == 0, (name, vgpr, wg, lds)
        assert "col3x3" not in name
    # 27 per-tensor instantiations (4 load widths x 3 tiles x {GEMM, convolution} + 3 in slot mode) and their per-channel twins
    per_channel = [n for n in gemm if "Lb1EEEvN4qnnp11IgemmParamsE" in n]
    per_tensor = [n for n in gemm if "Lb0EEEvN4qnnp11IgemmParamsE" in n]
    assert len(per_channel) == 27 and len(per_tensor) == 27 and len(gemm) == 54, (len(per_channel), len(per_tensor), len(gemm))
