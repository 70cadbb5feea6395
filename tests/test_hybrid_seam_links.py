"""CPU tier: the INTEGRATION section 2 seam library (oracle/_ref/libqnnpack_hybrid.so: the reference objects + the
product's objects + one patched statement, oracle/Makefile) must resolve every symbol at load time. Its object lists
used to be written out in oracle/Makefile; when a product source file was added and the list was not, the link
succeeded (shared libraries may carry undefined symbols) and the first dlopen on the GPU box failed -- the link now runs
with --no-undefined, both Makefiles take the lists from qnnpack_amd/csrc/sources.mk, and this test loads the library
the way tests/test_gpu_hybrid_seam.py will."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYBRID = os.path.join(ROOT, "oracle", "_ref", "libqnnpack_hybrid.so")


def test_hybrid_library_resolves_every_symbol():
    if not os.path.exists(HYBRID):
        pytest.skip("oracle/_ref/libqnnpack_hybrid.so not built (needs /root/reference)")
    try:
        import torch  # noqa: F401  -- the HIP runtime the product binds to (qnnpack_amd.load does the same)
    except Exception:
        pass
    lib = ctypes.CDLL(HYBRID, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for sym in ("qnnp_initialize", "qnnp_run_operator", "qnnp_create_convolution2d_nhwc_q8",
                "qnnp_create_fully_connected_nc_q8", "qnnp_create_max_pooling2d_nhwc_u8", "qnnp_delete_operator"):
        assert hasattr(lib, sym), sym


def test_oracle_makefile_lists_every_product_object():
    """the seam's object lists against the product's source lists, as make evaluates them in either Makefile: both come
    from qnnpack_amd/csrc/sources.mk and from nowhere else"""
    import re
    import subprocess

    def words(directory, var):
        out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, directory), "--eval", f"print-{var}: ; @echo $({var})",
                              f"print-{var}"], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split()

    c_srcs = {os.path.splitext(os.path.basename(w))[0] for w in words("qnnpack_amd/csrc", "C_SRCS")}
    hip_srcs = {os.path.splitext(os.path.basename(w))[0] for w in words("qnnpack_amd/csrc", "HIP_SRCS")}
    assert c_srcs and hip_srcs
    assert set(words("oracle", "PRODUCT_C_OBJS")) == c_srcs, (sorted(c_srcs), words("oracle", "PRODUCT_C_OBJS"))
    assert set(words("oracle", "PRODUCT_HIP_OBJS")) == hip_srcs, (sorted(hip_srcs), words("oracle", "PRODUCT_HIP_OBJS"))
    for makefile in ("qnnpack_amd/csrc/Makefile", "oracle/Makefile"):
        text = open(os.path.join(ROOT, makefile)).read()
        assert re.search(r"^include .*sources\.mk$", text, re.M), makefile
        assert not re.search(r"^(C_SRCS|HIP_SRCS)\s*[:+?]?=", text, re.M), makefile
    # every listed source exists, and every depthwise unit on disk is listed
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    for w in words("qnnpack_amd/csrc", "C_SRCS") + words("qnnpack_amd/csrc", "HIP_SRCS"):
        assert os.path.exists(os.path.join(csrc, w)), w
    on_disk = {os.path.splitext(f)[0] for f in os.listdir(os.path.join(csrc, "hip")) if re.fullmatch(r"q8dw\w+\.hip", f)}
    assert on_disk - {"q8dwconv_pc"} <= hip_srcs, sorted(on_disk - hip_srcs)
