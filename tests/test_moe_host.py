"""CPU tier of the top-k router and the weighted combine (include/qnnpack_gfx950_moe.h, moe.c, hip/f32topk.hip,
hip/f32combine.hip): the header and the binding's MOE_API agree and the pinned headers are untouched; the numpy restatement
(tests/_moe.py), which the GPU tier takes as its expectation, at its fixed points and against float64; the host code under
AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-moe); the kernels' resources."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _moe as moe
from _headers import HEADERS, prototypes
from qnnpack_amd import binding
from test_kernel_resources import kernels     # noqa: F401  (the fixture: the gfx950 code objects' metadata)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_moe_api_is_the_image_of_the_header_and_api_is_untouched():
    declared = prototypes("qnnpack_gfx950_moe.h")
    assert [f.symbol for f in binding.MOE_API] == list(declared) and len(declared) == 4
    for f in binding.MOE_API:
        ret, params = declared[f.symbol]
        assert ret == "enum qnnp_status" and f.bound == binding.IF_PRESENT and f.methods and len(f.params) == len(params)
        for (c_type, _), p in zip(params, f.params):
            assert (p.kind == "tensor") == (c_type in ("float*", "int32_t*")), (f.symbol, p.name, c_type)
    assert len(binding.API) == 65 and not {f.symbol for f in binding.MOE_API} & set(binding.API)
    for header in HEADERS:
        assert not set(prototypes(header)) & set(declared), header
    assert '#include "qnnpack_gfx950.h"' not in open(os.path.join(ROOT, "include", "qnnpack_gfx950_moe.h")).read()


def test_restatement_fixed_points_and_float64():
    assert moe.exp_of(np.zeros(1, F32))[0] == 1 and moe.exp_of(np.array([-0.0, -2.0 ** -100], F32)).tolist() == [1, 1]
    x = np.random.default_rng(3).normal(0, 4, (64, 48)).astype(F32)
    ids, w = moe.router(x, 6, first_group=2)
    order = np.argsort(-x.astype(np.float64), axis=1, kind="stable")[:, :6]
    assert np.array_equal(ids + 2, order) and (w[:, 0] >= w[:, 5]).all()
    top = np.take_along_axis(x.astype(np.float64), order, axis=1)
    want = np.exp(top - top[:, :1]) / np.exp(top - top[:, :1]).sum(axis=1, keepdims=True)
    # the exp lines' 4.46 * 2^-24 (qnnpack_gfx950_dynamic.h), the sum's and the division's roundings on top: 2^-21 covers them
    assert np.all(np.abs(w - want) <= 2.0 ** -21 * want)
    # -0 ranks below +0, equal keys by index, NaN at the bottom
    assert moe.router(np.array([[-0.0, 0.0, np.nan, 0.0]], F32), 4)[0].tolist() == [[1, 3, 0, 2]]
    rows = np.array([[1.0, 2.0 ** -100], [3.0, -4.0], [np.nan, np.nan], [4.0, 2.0 ** -26]], F32)
    got = moe.combine(rows, np.array([0.5, 1, 1, 2.0 ** -100], F32), np.array([0, 1, 2, 0], np.int32), 2, 2)
    assert got.view(np.uint32).tolist() == np.array([[3.5, -4.0], [2.0 ** -98, 0.0]], F32).view(np.uint32).tolist()


def test_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-moe"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(csrc, "build", "asan", "host_asan_moe_test")], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-moe-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_the_kernels_use_no_scratch_memory(kernels):
    found = {name: k for name, k in kernels.items() if "f32_topk_kernel" in name or "f32_combine_kernel" in name}
    assert len(found) == 12 + 4, sorted(found)        # six (L, V) pairs and two workgroup sizes, each with its _x4 flavour
    for name, k in found.items():
        assert k["scratch"] == 0 and k["spill"] == 0, (name, k)


@pytest.mark.parametrize("run,fields,change,want", [
    ("qnnp_hip_topk_router_run", "PPPQIIII", {}, 0), ("qnnp_hip_topk_router_run", "PPPQIIII", {5: 1025}, -4),
    ("qnnp_hip_topk_router_run", "PPPQIIII", {6: 9}, -4), ("qnnp_hip_topk_router_run", "PPPQIIII", {3: 31}, -4),
    ("qnnp_hip_topk_router_run", "PPPQIIII", {1: 0x2002}, -4), ("qnnp_hip_topk_router_run", "PPPQIIII", {4: 2 ** 18}, -4),
    ("qnnp_hip_weighted_combine_run", "PPPPQQIIII", {}, 0), ("qnnp_hip_weighted_combine_run", "PPPPQQIIII", {9: 2 ** 24}, -4),
    ("qnnp_hip_weighted_combine_run", "PPPPQQIIII", {5: 31}, -4), ("qnnp_hip_weighted_combine_run", "PPPPQQIIII", {2: 0}, -4),
], ids=lambda v: str(v) if isinstance(v, dict) else None)
def test_the_launches_validate_before_they_touch_a_device(product, run, fields, change, want):
    """tokens = 0 launches nothing: the answer comes from the argument block alone"""
    types = {"P": ctypes.c_void_p, "Q": ctypes.c_uint64, "I": ctypes.c_uint32}
    router = [0x1000, 0x2000, 0x3000, 32, 0, 32, 4, 0]               # logits, ids, weights, stride, tokens, groups, A, first
    combine = [0x1000, 0x2000, 0x3000, 0x4000, 32, 32, 0, 4, 8, 32]  # input, weights, ids, output, strides, tokens, A, groups, N
    values = router if "router" in run else combine
    for at, value in change.items():
        values[at] = value

    class Args(ctypes.Structure):
        _fields_ = [(f"f{i}", types[t]) for i, t in enumerate(fields)]
    function = getattr(product.lib, run)
    function.argtypes, function.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    assert function(ctypes.byref(Args(*values)), None) == want
