"""CPU: the C-ABI library builds for gfx950, loads, and exports exactly what include/*.h declares.
No kernel is launched here; only argument validation paths (which return before any launch) are called."""
import ctypes as C
import os
import re

from coma_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = []
    for f in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if f.endswith(".h"):
            txt = open(os.path.join(ROOT, "include", f)).read()
            txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
            names += re.findall(r"\b((?:coma|sd|seg)_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(names))


def test_every_declared_symbol_is_exported_and_bound(hip_lib):
    decl = _declared()
    assert "coma_contact_accumulate_f32" in decl and len(decl) >= 10
    for name in decl:
        assert hasattr(hip_lib, name), f"{name} declared in include/ but not exported"
    # _declared() is a second, cruder reading of the headers than the parser the binding comes from: they must find the same names
    assert sorted(_abi.FUNCTIONS) == decl == sorted(_lib.SIGNATURES) == sorted(_lib.PARAMS), "coma_amd/_abi.py and the headers disagree"


def test_abi_version_11_and_error_text(hip_lib):
    # 11: seg_conv_gemm_describe joined the ABI; seg_conv_gemm_f32 refuses a forced split_k whose slabs the workspace does not hold
    # 10: sd_conv_gemm_describe joined the ABI; sd_conv_gemm_f16 refuses a column bias with SD_EPI_PERM16_N / SD_EPI_PERM32_N and colstats in
    # a phase launch with in_h * in_w % 32 != 0
    assert hip_lib.coma_abi_version() == 11 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "coma_hip.h")).read()
    assert re.search(r"#define COMA_ABI_VERSION (\d+)", hdr).group(1) == "11"
    rc = hip_lib.coma_nearest_vertex_i64(None, None, 1, 1, None, None)
    assert rc == -1 and b"null pointer" in hip_lib.coma_last_error()
    one = C.c_void_p(8)   # never dereferenced: size validation fails first
    rc = hip_lib.coma_contact_accumulate_f32(one, one, one, one, 5, one, 1, 2, 3, 4, _lib.vec3([0, 0, 1]),
                                             _lib.vec3([0, 1, 0]), 0.07, 0.03, 0.25, 1e-10, one, one, one, one, one, None)
    assert rc == -1 and b"obj_sample_stride" in hip_lib.coma_last_error()
    rc = hip_lib.coma_occupancy_splat(one, 1, 0, 8, one, 0.3, 0.9, one, None)
    assert rc == -1


def test_library_is_in_tree():
    assert os.path.dirname(_lib.LIB_PATH) == os.path.join(ROOT, "coma_amd")
