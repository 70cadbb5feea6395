"""GPU tier of the windowed pooling operators (hip/q8pool.hip behind max-pooling.c / average-pooling.c).

Every case of tests/_pooling.py -- the restated reference test lists (test/max-pooling.cc, test/average-pooling.cc), the
extra cases and the reference's bench lists -- runs on the MI355X on device buffers (host buffers where the case says
so) and must give the bytes of the COMPILED REFERENCE (oracle/_ref/libqnnpack_ref.so, on the host) and of the numpy
model, including the FILL bytes between strided pixels. Then: the vector width the kernel name reports, the status codes
of the invalid / unsupported parameter paths against the reference's, a ResNet-style stem (7x7 stride-2 convolution ->
3x3 stride-2 max pool) captured in a hipGraph and replayed, async mode, and re-setup.
"""
import numpy as np
import pytest

import _pooling as pl
from _cases import ConvCase
from _gpu import from_device, to_device
from _runner import conv_expected, conv_run, conv_tensors
from oracle import ref
from qnnpack_amd import Status

pytestmark = pytest.mark.gpu

_REF_GROUPS = {}
for _c in pl.reference_max_cases() + pl.reference_avg_cases():
    _REF_GROUPS.setdefault(_c.name.rsplit("/", 1)[0], []).append(_c)


@pytest.fixture(scope="module")
def reference():
    if not ref.available():
        pytest.fail("oracle/_ref/libqnnpack_ref.so was not built (build() makes it where the reference tree exists)")
    return ref.lib()


def _check(qnnp, reference, case):
    x = pl.input_tensor(case)
    want = pl.expected(case, x)
    got, kname = pl.run(qnnp, case, x, to_device=to_device, from_device=from_device)
    ref_out, _ = pl.run(reference, case, x)         # (host buffers: misalignment and staging are device-side matters)
    for r, w in zip(ref_out, want):
        assert np.array_equal(r, w), f"{case.name}: numpy model vs compiled reference"
    for i, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{case.name} (setup {i}, {kname}): {bad.size} bytes differ, first at {bad[:4]}: "
                                 f"got {g[bad[:4]]}, want {w[bad[:4]]}")
    return kname


@pytest.mark.parametrize("test", sorted(_REF_GROUPS))
def test_reference_test_lists(qnnp, reference, test):
    for case in _REF_GROUPS[test]:
        _check(qnnp, reference, case)


@pytest.mark.parametrize("case", pl.extra_cases(), ids=lambda c: c.name)
def test_extra_cases(qnnp, reference, case):
    _check(qnnp, reference, case)


@pytest.mark.parametrize("case", pl.bench_cases(1), ids=lambda c: c.name)
def test_bench_lists_batch_1(qnnp, reference, case):
    _check(qnnp, reference, case)


LARGEST = ["max/bench/VGG_1/b128", "max/bench/SqueezeNetV10_pool1/b128", "max/bench/ShuffleNet/b128",
           "avg/bench/ShuffleNetV1G1_56x56x24/b128", "avg/bench/ShuffleNetV1G8_28x28x384/b128"]


@pytest.mark.parametrize("name", LARGEST)
def test_bench_lists_batch_128_largest_rows(qnnp, reference, name):
    case = {c.name: c for c in pl.bench_cases(128)}[name]
    _check(qnnp, reference, case)


@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("channels,stride,misalign,vec", [
    (64, 0, 0, 16), (1088, 0, 0, 16), (64, 68, 0, 4), (24, 0, 0, 4), (200, 0, 0, 4), (7, 0, 0, 1), (3, 0, 0, 1),
    (64, 0, 4, 4), (64, 0, 1, 1), (64, 0, 2, 1), (64, 0, 3, 1), (16, 19, 0, 1)])
def test_kernel_path_follows_alignment(qnnp, reference, kind, channels, stride, misalign, vec):
    case = pl.PoolCase(kind, f"{kind}/path/c{channels}_s{stride}_m{misalign}", 2, 9, 9, channels, 3, 3, 1, 1, 1, 1, 2, 2,
                       in_stride=stride, misalign_in=misalign)
    kname = _check(qnnp, reference, case)
    assert kname == f"q8_{kind}pool_x{vec}", kname


# (create arguments) -> both libraries must answer the same status (reference src/max-pooling.c:61-103,
# src/average-pooling.c:61-129)
MAX_CREATE = [
    (0, 0, 0, 0, 0, 3, 1, 1, 1, 1, 8, 0, 255), (0, 0, 0, 0, 3, 0, 1, 1, 1, 1, 8, 0, 255),
    (0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 8, 0, 255), (0, 0, 0, 0, 65536, 65536, 1, 1, 1, 1, 8, 0, 255),
    (0, 0, 0, 0, 2, 2, 0, 1, 1, 1, 8, 0, 255), (0, 0, 0, 0, 2, 2, 1, 0, 1, 1, 8, 0, 255),
    (0, 0, 0, 0, 2, 2, 1, 1, 0, 1, 8, 0, 255), (0, 0, 0, 0, 2, 2, 1, 1, 1, 0, 8, 0, 255),
    (0, 0, 0, 0, 2, 2, 1, 1, 1, 1, 0, 0, 255), (1, 1, 1, 1, 3, 3, 2, 2, 1, 1, 8, 0, 255),
    (0, 0, 0, 0, 1, 2, 1, 1, 1, 1, 1, 200, 40),
]
AVG_CREATE = [
    (0, 0, 0, 0, 0, 3, 1, 1, 8, 0, 1.0, 0, 1.0, 0, 255), (0, 0, 0, 0, 1, 1, 1, 1, 8, 0, 1.0, 0, 1.0, 0, 255),
    (0, 0, 0, 0, 2, 2, 0, 1, 8, 0, 1.0, 0, 1.0, 0, 255), (0, 0, 0, 0, 2, 2, 1, 1, 0, 0, 1.0, 0, 1.0, 0, 255),
    (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 0.0, 0, 1.0, 0, 255), (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, -1.0, 0, 1.0, 0, 255),
    (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, float("nan"), 0, 1.0, 0, 255), (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, float("inf"), 0, 1.0, 0, 255),
    (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0e-40, 0, 1.0, 0, 255), (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0, 0, 0.0, 0, 255),
    (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0, 0, 512.0, 0, 255), (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 256.0, 0, 1.0, 0, 255),
    (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 255.0, 0, 1.0, 0, 255), (0, 0, 0, 0, 2, 2, 1, 1, 8, 0, 1.0, 0, 256.0, 0, 255),
    (0, 0, 0, 0, 4096, 4096, 1, 1, 8, 0, 1.0, 0, 1.0, 0, 255), (0, 0, 0, 0, 4096, 4095, 1, 1, 8, 0, 1.0, 0, 1.0, 0, 255),
    (1, 1, 1, 1, 3, 3, 2, 2, 8, 121, 0.5, 133, 0.75, 0, 255),
]


@pytest.mark.parametrize("args", MAX_CREATE)
def test_max_pooling_create_statuses_match_the_reference(qnnp, reference, args):
    got = [lib.create_max_pooling2d_nhwc_u8_status(*args) for lib in (qnnp, reference)]
    for lib, (st, op) in zip((qnnp, reference), got):
        if op:
            lib.delete_operator(op)
    assert got[0][0] == got[1][0], (args, got[0][0], got[1][0])


@pytest.mark.parametrize("args", AVG_CREATE)
def test_average_pooling_create_statuses_match_the_reference(qnnp, reference, args):
    got = [lib.create_average_pooling2d_nhwc_q8_status(*args) for lib in (qnnp, reference)]
    for lib, (st, op) in zip((qnnp, reference), got):
        if op:
            lib.delete_operator(op)
    assert got[0][0] == got[1][0], (args, got[0][0], got[1][0])


@pytest.mark.parametrize("kind", ["max", "avg"])
def test_setup_statuses(qnnp, reference, kind):
    case = pl.PoolCase(kind, f"{kind}/setup_statuses", 1, 6, 6, 8, 3, 3, 1, 1, 1, 1, 2, 2)
    x = np.zeros(4096, np.uint8)
    y = np.zeros(4096, np.uint8)
    for n, h, w, expect in ((0, 6, 6, Status.success), (0, 0, 0, Status.success), (1, 0, 6, Status.invalid_parameter),
                            (1, 6, 0, Status.invalid_parameter), (2, 6, 6, Status.success)):
        for lib in (qnnp, reference):         # reference src/*-pooling.c: batch 0 first, then zero dimensions
            st, op = pl.create(lib, case)
            assert st == 0
            assert pl.setup_status(lib, case, op, n, h, w, x, y) == expect, (lib, n, h, w)
            if expect == Status.success:
                assert lib.run_operator_status(op) == Status.success
            lib.delete_operator(op)
    # where the reference checks nothing and would read out of range, the product refuses (include/qnnpack_gfx950.h)
    case = pl.PoolCase(kind, f"{kind}/setup_statuses_unpadded", 1, 6, 6, 8, 3, 3, stride_height=2, stride_width=2)
    st, op = pl.create(qnnp, case)
    try:
        assert pl.setup_status(qnnp, case, op, 1, 2, 6, x, y) == Status.invalid_parameter        # 2 rows < 3-row window
        assert pl.setup_status(qnnp, case, op, 1, 6, 2, x, y) == Status.invalid_parameter
        assert pl.setup_status(qnnp, case, op, 1, 6, 6, None, y) == Status.invalid_parameter
        assert pl.setup_status(qnnp, replace_strides(case, 7, 8), op, 1, 6, 6, x, y) == Status.invalid_parameter
        assert pl.setup_status(qnnp, replace_strides(case, 8, 7), op, 1, 6, 6, x, y) == Status.invalid_parameter
        assert qnnp.run_operator_status(op) == Status.invalid_parameter      # never set up successfully
    finally:
        qnnp.delete_operator(op)


def replace_strides(case, si, so):
    from dataclasses import replace
    return replace(case, in_stride=si, out_stride=so)


def test_resnet_stem_in_a_hipgraph(qnnp, reference):
    """7x7 stride-2 convolution (3 -> 64) -> 3x3 stride-2 max pool, both on device buffers, captured and replayed"""
    conv = ConvCase("stem_conv7x7s2", (112, 112), (7, 7), (3, 3, 3, 3), (2, 2), gic=3, goc=64, batch=2)
    inp, kernel, bias = conv_tensors(conv)
    _, quant, (oh, ow) = conv_expected(conv, inp, kernel, bias)
    mid_ref, _ = conv_run(reference, conv, quant, (oh, ow), inp, kernel, bias)
    pool = pl.PoolCase("max", "stem_pool3x3s2", conv.batch, oh, ow, 64, 3, 3, 1, 1, 1, 1, 2, 2)
    want = pl.run(reference, pool, mid_ref)[0][0]
    assert np.array_equal(want, pl.expected(pool, mid_ref)[0])

    oscale, ozp = quant
    cop = qnnp.create_convolution2d_nhwc_q8(3, 3, 3, 3, 7, 7, 2, 2, 1, 1, 1, 3, 64, conv.izp, 1.0, conv.kzp, 1.0,
                                             kernel, bias, ozp, float(oscale), 0, 255, 0)
    st, pop = pl.create(qnnp, pool)
    assert st == 0
    d_in = to_device(inp)
    d_mid = to_device(np.zeros(mid_ref.size, np.uint8))
    d_out = to_device(pl.output_tensor(pool))
    graph = None
    try:
        qnnp.setup_convolution2d_nhwc_q8(cop, conv.batch, 112, 112, d_in, 3, d_mid, 64)
        assert pl.setup_status(qnnp, pool, pop, pool.batch, oh, ow, d_mid, d_out) == 0
        qnnp.graph_begin()
        qnnp.run_operator(cop)
        qnnp.run_operator(pop)
        graph = qnnp.graph_end()
        for _ in range(2):
            d_out.fill_(pl.FILL)
            qnnp.graph_launch(graph)
            qnnp.graph_synchronize(graph)
            assert np.array_equal(from_device(d_out), want), "stem replayed from the graph"
        assert qnnp.operator_kernel(pop) == "q8_maxpool_x16"
    finally:
        if graph:
            qnnp.graph_destroy(graph)
        qnnp.delete_operator(cop)
        qnnp.delete_operator(pop)


@pytest.mark.parametrize("kind", ["max", "avg"])
def test_async_mode_and_resetup(qnnp, kind):
    import torch
    case = pl.PoolCase(kind, f"{kind}/async", 4, 30, 28, 96, 3, 3, 1, 1, 1, 1, 2, 2)
    x = pl.input_tensor(case)
    want = pl.expected(case, x)[0]
    st, op = pl.create(qnnp, case)
    assert st == 0
    d_x, d_y = to_device(x), to_device(pl.output_tensor(case))
    try:
        qnnp.set_async(True)
        assert pl.setup_status(qnnp, case, op, 4, 30, 28, d_x, d_y) == 0
        for _ in range(3):
            qnnp.run_operator(op)
        qnnp.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(from_device(d_y), want), "async runs"
        qnnp.set_async(False)
        # a second geometry on the same buffers, then back: each run gives that geometry's bytes
        small = pl.PoolCase(kind, case.name, 2, 17, 19, 96, 3, 3, 1, 1, 1, 1, 2, 2)
        d_y.fill_(pl.FILL)
        assert pl.setup_status(qnnp, case, op, 2, 17, 19, d_x, d_y) == 0
        qnnp.run_operator(op)
        got = from_device(d_y)
        want_small = pl.expected(small, x)[0]
        assert np.array_equal(got[:want_small.size], want_small) and np.all(got[want_small.size:] == pl.FILL)
        assert pl.setup_status(qnnp, case, op, 4, 30, 28, d_x, d_y) == 0
        qnnp.run_operator(op)
        assert np.array_equal(from_device(d_y), want), "second run after re-setup"
    finally:
        qnnp.set_async(False)
        qnnp.delete_operator(op)
