"""CPU tier of the output table behind a convolution (qnnp_gfx950_attach_output_table / qnnp_gfx950_operator_table_folded:
output-table.c, the table flavours of hip/q8pwconv.hip's kernel units, hip/q8dwcol.hip and hip/q8dwcol5.hip):

 * interface: the prototypes in include/qnnpack_gfx950_output_table.h are the specified ones, qnnpack_gfx950.h includes
   that header, binding.OUTPUT_TABLE_API is its image while API stays the 65 functions of the three older headers, the
   library exports the two entry points, and without a GPU attach answers uninitialized (no CPU fallback);
 * the argument blocks grew at their ends only: what was there keeps its offset;
 * the cases of tests/test_output_table_gpu.py: the oracle's expectation of every case is not degenerate and every class
   case is in the class it names, without a GPU;
 * host code under AddressSanitizer + UBSan as a stand-alone program (Makefile target asan-table) over
   tests/hip_stub_table.c: every status in its order, the attach / replace / detach / delete lifecycles, no leak of the
   device table, the in-place launch behind the three operator kinds;
 * the table flavours of the depthwise column walks: no scratch, no vector spills, 256 B of LDS (the table), registers
   for the residency their launches are planned for, and the plain flavours no LDS, as before.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from _headers import HEADERS, prototypes
from qnnpack_amd import Status, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "qnnpack_gfx950_output_table.h"
FUNCTIONS = ["qnnp_gfx950_attach_output_table", "qnnp_gfx950_operator_table_folded"]
PROTOTYPES = [
    "enum qnnp_status qnnp_gfx950_attach_output_table(qnnp_operator_t convolution, qnnp_operator_t table);",
    "int qnnp_gfx950_operator_table_folded(qnnp_operator_t op);"]


def test_entry_points_are_declared_as_specified():
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)).replace("( ", "(")
    for prototype in PROTOTYPES:
        assert prototype in text, prototype
    assert sorted(prototypes(HEADER)) == sorted(FUNCTIONS)
    # a caller of qnnpack_gfx950.h has them, beside the residual add
    assert '#include "qnnpack_gfx950_output_table.h"' in open(os.path.join(ROOT, "include", "qnnpack_gfx950.h")).read()
    # and the three older headers declare neither
    for header in HEADERS:
        assert not set(prototypes(header)) & set(FUNCTIONS), header


def test_output_table_api_is_the_image_of_the_header_and_api_is_untouched():
    from test_binding_signatures import SCALARS, is_c_pointer, is_pointer, python_name
    declared = prototypes(HEADER)
    assert [f.symbol for f in binding.OUTPUT_TABLE_API] == FUNCTIONS
    for f in binding.OUTPUT_TABLE_API:
        ret, params = declared[f.symbol]
        assert f.restype is SCALARS[ret], (f.symbol, ret)
        assert f.bound == binding.IF_PRESENT
        assert len(f.params) == len(params), f.symbol
        for (c_type, header_name), p, ctype in zip(params, f.params, f.argtypes):
            assert is_c_pointer(c_type) and is_pointer(ctype), (f.symbol, header_name, c_type, ctype)
            assert p.name == python_name(f, c_type, header_name), (f.symbol, p.name, header_name)
            assert p.kind == "ptr"
    attach, folded = binding.OUTPUT_TABLE_API
    assert attach.methods and not folded.methods
    assert len(binding.API) == 65 and not set(FUNCTIONS) & set(binding.API)
    for method in ("attach_output_table", "attach_output_table_status", "operator_table_folded"):
        assert method in vars(binding.Gfx950Library) and not hasattr(binding.QnnpackLibrary, method), method


def test_library_exports_the_entry_points(product):
    for name in FUNCTIONS:
        assert hasattr(product.lib, name), name
        assert getattr(product.lib, name).argtypes == binding.OUTPUT_TABLE_API[FUNCTIONS.index(name)].argtypes


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="CPU-only behaviour")
def test_without_a_gpu_attach_is_uninitialized(product):
    assert product.initialize_status() == Status.unsupported_hardware
    assert product.attach_output_table_status(None, None) == Status.uninitialized
    assert product.operator_table_folded(None) == -1


def test_the_argument_blocks_grew_at_their_ends_only():
    """`table` and `table_folded` are the last two members of the two launch blocks, the table pointer the last member of
    the two kernel-argument blocks: nothing that was there moves (tests/golden/launch_args.txt stays valid)"""
    seam = open(os.path.join(ROOT, "qnnpack_amd", "csrc", "hip", "qnnp_hip.h")).read()
    for struct in ("qnnp_hip_igemm_args", "qnnp_hip_dwconv_args"):
        body = re.search(r"struct %s \{(.*?)\n\};" % struct, seam, flags=re.S).group(1)
        members = [m for m in re.findall(r"^\s+(?:const\s+)?(?:struct\s+)?[\w]+[\s\*]+(\w+(?:,\s*\w+)*);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)]
        assert members[-2:] == ["table", "table_folded"], (struct, members[-4:])
        assert members[-3] == "rq_pc", (struct, members[-4:])
    for path, struct in (("igemm_params.h", "IgemmParams"), ("dwconv_params.h", "DwParams")):
        text = open(os.path.join(ROOT, "qnnpack_amd", "csrc", "hip", path)).read()
        body = re.search(r"struct %s \{(.*?)\n\};" % struct, text, flags=re.S).group(1)
        lines = [l for l in re.sub(r"//.*", "", body).splitlines() if l.strip()]
        assert re.match(r"\s*const uint8_t\* table;", lines[-1]), (struct, lines[-1])


def _gpu_cases():
    import test_output_table_gpu as G
    return G.POINTWISE + G.AUTO + G.DEPTHWISE + G.CLASSES + G.NOT_FOLDED + [G.LIFE, G.LIFE_UNFOLDED]


def test_the_oracle_expectation_of_every_gpu_case_is_not_degenerate():
    """what tests/test_output_table_gpu.py asserts before it runs anything, here without a GPU; building a class case
    asserts that its stage is in the class it names (tests/_fused.py stage_class)"""
    import _fused as F
    import _output_table as T
    cases = _gpu_cases()
    assert len({c.name for c in cases}) == len(cases)
    for case in cases:
        p = T.problem(case)
        p.not_degenerate()
        assert not np.array_equal(p.expected(), p.plain()), case.name
        # the expectation is a pure function of the case
        again = T.Problem(case)
        assert np.array_equal(again.expected(), p.expected()) and np.array_equal(again.table, p.table), case.name
    import test_output_table_gpu as G
    # every class of the table in every folding kernel family, and a clamp case and a hardswish case per family
    assert {(c.name.rsplit("_mode", 1)[0], c.mode) for c in G.CLASSES} == \
           {("class_" + fam, mode) for fam in G.CLASS_FAMILIES for mode in F.MODES}
    for want in T.PW_KERNELS[:3] + (T.DW_KERNELS[1], T.DW_KERNELS[3]):
        family = [c for c in G.POINTWISE + G.DEPTHWISE if c.want == want]
        assert any(c.clamp == (10, 200) for c in family) and any(c.table == "hardswish" for c in family), want
    assert sorted(T.problem(G.LIFE).table.tolist()) == list(range(256))      # the permutation is one


def test_output_table_host_code_is_clean_under_asan_and_ubsan():
    csrc = os.path.join(ROOT, "qnnpack_amd", "csrc")
    build = subprocess.run(["make", "-C", csrc, "asan-table"], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    exe = os.path.join(csrc, "build", "asan", "host_asan_table_test")
    # the ASan runtime is linked statically (Makefile asan-table), so it comes first whatever else the process loads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0 and "host-sanitizers-table-ok" in run.stdout, run.stdout[-2000:] + run.stderr[-6000:]


def test_column_walk_table_flavours_use_no_scratch_and_256_bytes_of_lds(tmp_path):
    """the checks of tests/test_kernel_resources.py for the table flavours of kernels G and H"""
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
            if "q8_dwconv_col3x3_kernel" in name or "q8_dwconv_col5x5_kernel" in name:
                found[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1)) for key in
                                    ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count", "group_segment_fixed_size"))
    # the last template argument is the flavour: Lb1E with the table, Lb0E without
    tab = {n: v for n, v in found.items() if re.search(r"Lb1EEEvN4qnnp8DwParamsE$", n)}
    plain = {n: v for n, v in found.items() if re.search(r"Lb0EEEvN4qnnp8DwParamsE$", n)}
    # kernel G: seven shapes in five requantization flavours, kernel H: two strides in five; each with and without
    assert len(tab) == 45 and len(plain) == 45 and len(found) == 90, (len(tab), len(plain), len(found))
    for name, (scratch, vspill, vgprs, lds) in found.items():
        # (scalar registers that do not fit go to lanes of a vector register, in the plain flavours as well: no memory)
        assert scratch == 0 and vspill == 0, (name, scratch, vspill)
        assert lds == (256 if name in tab else 0), (name, lds)
        if name in tab:
            waves = lambda v: min(8, 512 // (-(-v // 8) * 8))          # 512 registers in blocks of eight
            if "col3x3" in name:
                # the six waves per SIMD dwcol_plan sizes its launches for (five at stride 1); the lookup costs 0 .. 4 registers
                assert waves(vgprs) >= 6, (name, vgprs)
            else:
                # kernel H runs at its register limit: as many waves per SIMD as the plain flavour
                twin = found[re.sub(r"Lb1E(EEvN4qnnp8DwParamsE)$", r"Lb0E\1", name)]
                assert waves(vgprs) == waves(twin[2]), (name, vgprs, twin[2])
