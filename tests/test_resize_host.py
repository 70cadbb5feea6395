"""CPU tier of the bilinear resize operator (qnnp_gfx950_*_resize_bilinear2d_nhwc_u8):

 * interface: the two prototypes in include/qnnpack_gfx950.h are the specified ones, the library exports both, and
   without a GPU create and setup answer uninitialized (no CPU fallback);
 * the C builder of the axis tables (resize-table.h through qnnp_debug_resize_axis_table) equals the definition of
   tests/_resize.py entry for entry;
 * the definition's properties: identity, hand values, the listed tables, < 0.63 from the float64 ideal and <= 1 from
   its rounding, constants stay constant, every byte between the min and max of its taps;
 * host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-resize), and the kernels of
   hip/u8resize.hip: four instantiations, no scratch, no spills, 256-thread workgroups, no LDS, at most 64 VGPRs.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _resize as rs
from qnnpack_amd import Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["qnnp_gfx950_create_resize_bilinear2d_nhwc_u8", "qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ---- 1. interface ----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_uninitialized_without_a_gpu(product):
    raw = open(os.path.join(ROOT, "include", "qnnpack_gfx950.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    text = re.sub(r"\s+", " ", text).replace("( ", "(")
    assert "#define QNNP_GFX950_RESIZE_ALIGN_CORNERS 0x00000001u" in text
    assert ("enum qnnp_status qnnp_gfx950_create_resize_bilinear2d_nhwc_u8(size_t channels, uint32_t flags, "
            "qnnp_operator_t* resize);") in text
    assert ("enum qnnp_status qnnp_gfx950_setup_resize_bilinear2d_nhwc_u8(qnnp_operator_t resize, size_t batch_size, "
            "size_t input_height, size_t input_width, size_t output_height, size_t output_width, const uint8_t* input, "
            "size_t input_pixel_stride, uint8_t* output, size_t output_pixel_stride);") in text
    # the header comment carries the definition
    for piece in ("(4096 * num + 2 * n_out) / (4 * n_out)", "(4096 * o * (n_in - 1) + (n_out - 1)) / (2 * (n_out - 1))",
                  "(top * (2048 - wy) + bot * wy + 2^21) >> 22"):
        assert piece in re.sub(r"\s+", " ", raw.replace("\n *", " ")), piece
    for name in FUNCTIONS:
        assert hasattr(product.lib, name), name
    assert product.RESIZE_ALIGN_CORNERS == rs.ALIGN_CORNERS == 1
    if not _has_gpu():
        assert product.initialize_status() == Status.unsupported_hardware
        st, handle = product.create_resize_bilinear2d_nhwc_u8_status(8)
        assert st == Status.uninitialized and not handle
        x = np.zeros(64, np.uint8)
        assert product.setup_resize_bilinear2d_nhwc_u8_status(None, 1, 2, 2, 2, 2, x, 8, x, 8) == Status.uninitialized


# ---- 2. the C table builder ------------------------------------------------------------------------------------------
def _c_axis(debug_hooks, n_in, n_out, align):
    fn = debug_hooks.lib.qnnp_debug_resize_axis_table
    fn.restype = None
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    out = [np.full(n_out, 0xFFFFFFFF, np.uint32) for _ in range(3)]
    fn(n_in, n_out, int(align), *(o.ctypes.data for o in out))
    return out


def test_c_axis_tables_equal_the_definition(debug_hooks):
    for align in (False, True):
        for n_in in rs.TABLE_IN:
            for n_out in rs.TABLE_OUT:
                got = _c_axis(debug_hooks, n_in, n_out, align)
                want = rs.axis(n_in, n_out, align)
                for g, w, what in zip(got, want, ("i0", "i1", "w")):
                    assert np.array_equal(g.astype(np.int64), w), (n_in, n_out, align, what)
                # the vectorised restatement against plain Python integers
                for o in {0, n_out // 2, n_out - 1}:
                    assert tuple(int(w[o]) for w in want) == rs.axis_entry(n_in, n_out, align, o), (n_in, n_out, align, o)
        for n_in, n_out in rs.TABLE_EDGES:
            got = _c_axis(debug_hooks, n_in, n_out, align)
            for o in (0, n_out // 2, n_out - 1):
                assert tuple(int(g[o]) for g in got) == rs.axis_entry(n_in, n_out, align, o), (n_in, n_out, align, o)
    # the entries stay inside the input and the weight inside Q11, at the largest sizes too
    i0, i1, w = _c_axis(debug_hooks, rs.SIZE_LIMIT - 1, rs.SIZE_LIMIT - 1, False)
    assert np.array_equal(i0, np.arange(rs.SIZE_LIMIT - 1, dtype=np.uint32)) and not w.any()
    assert int(i1.max()) == rs.SIZE_LIMIT - 2


# ---- 3. properties of the definition ---------------------------------------------------------------------------------
def test_listed_tables_and_hand_values():
    def table(n_in, n_out, align):
        return [rs.axis_entry(n_in, n_out, align, o) for o in range(n_out)]
    assert table(2, 4, False) == [(0, 1, 0), (0, 1, 512), (0, 1, 1536), (1, 1, 0)]
    assert [w for _, _, w in table(2, 4, True)] == [0, 683, 1365, 0]
    assert table(5, 2, False) == [(0, 1, 1536), (3, 4, 512)]
    x = np.array([[0, 60], [120, 180]], np.uint8).reshape(1, 2, 2, 1)
    assert rs.resize(x, 4, 4, False).reshape(4, 4).tolist() == [
        [0, 15, 45, 60], [30, 45, 75, 90], [90, 105, 135, 150], [120, 135, 165, 180]]
    assert rs.resize(x, 3, 3, True).reshape(3, 3).tolist() == [[0, 30, 60], [60, 90, 120], [120, 150, 180]]


def test_definition_is_identity_bounded_and_close_to_the_ideal():
    rng = np.random.default_rng(rs._seed("properties"))
    worst, differ, total = 0.0, 0, 0
    for align in (False, True):
        for n_in in rs.PROPERTY_IN:
            # height and width take the size lists in turn, the other axis a fixed 3 -> 4 or equal sizes
            x = rng.integers(0, 256, size=(2, n_in, n_in, 3), dtype=np.uint8)
            x[..., 1] = rng.integers(0, 2, size=x.shape[:3], dtype=np.uint8) * 255
            assert np.array_equal(rs.resize(x, n_in, n_in, align), x), ("identity", n_in, align)
            for n_out in rs.PROPERTY_OUT:
                for out_h, out_w in ((n_out, n_out), (n_out, n_in), (n_in, n_out)):
                    y = rs.resize(x, out_h, out_w, align)
                    real = rs.ideal(x, out_h, out_w, align)
                    err = float(np.abs(y.astype(np.float64) - real).max())
                    worst = max(worst, err)
                    # 0.5 from the last rounding, 255 * 2 * 2^-12 from the two Q11 weights
                    assert err < 0.63, (n_in, out_h, out_w, align, err)
                    rounded = np.floor(real + 0.5)
                    assert np.abs(y.astype(np.int64) - rounded.astype(np.int64)).max() <= 1, (n_in, out_h, out_w, align)
                    differ += int((y != rounded).sum())
                    total += y.size
                    t = np.stack(rs.taps(x, out_h, out_w, align))
                    assert np.all(y >= t.min(axis=0)) and np.all(y <= t.max(axis=0)), (n_in, out_h, out_w, align)
                for value in (0, 1, 127, 254, 255):
                    const = np.full((1, n_in, n_in, 2), value, np.uint8)
                    assert np.all(rs.resize(const, n_out, n_out, align) == value), (n_in, n_out, value, align)
    assert worst > 0.5 and differ / total < 0.05, (worst, differ, total)


def test_expected_keeps_the_fill_and_kernel_rule():
    c = rs.Case(2, 2, 3, 3, 2, 5, in_stride=8, out_stride=12)
    x, y = rs.tensors("example", c)
    out = rs.expected(c, x, y)
    assert out.size == 11 * 12 + 5
    between = np.lib.stride_tricks.as_strided(out[5:], shape=(11, 7), strides=(12, 1), writeable=False)
    assert np.all(between == rs.FILL)
    pixels = rs.pixels_view(out, 2, 3, 2, 12, 5)
    assert np.array_equal(pixels, rs.resize(rs.pixels_view(x, 2, 2, 3, 8, 5), 3, 2, False))
    assert set(np.unique(rs.pixels_view(x, 2, 2, 3, 8, 5)[..., 2])) <= {0, 255}
    assert rs.kernel_for(32, (0, 16), (32, 48)) == "u8_resize_x16"
    assert rs.kernel_for(32, (0, 4), (32, 32)) == "u8_resize_x4"
    assert rs.kernel_for(32, (0, 0), (36, 32)) == "u8_resize_x4"
    assert rs.kernel_for(21, (1, 3), (21, 21)) == "u8_resize_x4"
    assert rs.kernel_for(4, (1, 3), (5, 7)) == "u8_resize_x4"
    assert rs.kernel_for(3, (0, 0), (16, 16)) == "u8_resize_x1"
    assert rs.kernel_for(1, (0, 0), (1, 1)) == "u8_resize_x1"


# ---- 4. host code under the sanitizers -------------------------------------------------------------------------------
def test_resize_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-resize"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_resize_test")
    # the ASan runtime is linked statically (Makefile asan-resize), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-resize-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


# ---- 5. kernel resources ---------------------------------------------------------------------------------------------
def test_resize_kernels_use_no_scratch_and_fit_their_launch_bounds(tmp_path):
    """the checks of tests/test_kernel_resources.py for hip/u8resize.hip"""
    from test_kernel_resources import READELF, _code_objects
    lib = os.path.join(ROOT, "qnnpack_amd", "libqnnpack_gfx950.so")
    if not os.path.exists(lib) or not os.path.exists(READELF):
        pytest.skip("library or llvm-readelf not available")
    found = {}
    for k, elf in enumerate(_code_objects(open(lib, "rb").read())):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(elf)
        notes = subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
        for entry in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry).group(1)
            if "u8_resize_" in name:
                found[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.sgpr_spill_count:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", entry).group(1)),
                               int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1)))
    # 16-byte pieces with and without the streaming hint on the store, dwords at any alignment, single bytes
    assert len(found) == 4, sorted(found)
    assert sum("ILi16ELb1E" in n for n in found) == 1 and sum("ILi16ELb0E" in n for n in found) == 1, sorted(found)
    assert sum("ILi4ELb0E" in n for n in found) == 1 and sum("ILi1ELb0E" in n for n in found) == 1, sorted(found)
    for name, (vgpr, scratch, vspill, sspill, wg, lds) in found.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, scratch, vspill, sspill)
        # the built kernels take 61 / 52 / 30 VGPRs: all inside the 64-register step, 8 waves per SIMD
        assert wg == 256 and vgpr <= 64, (name, vgpr, wg)
        assert lds == 0, (name, lds)
