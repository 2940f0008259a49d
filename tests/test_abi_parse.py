"""CPU, no library: coma_amd/_abi.py reads C header text into the ctypes binding.  parse() on small header strings (what it reads, and
every construct it must refuse with the offending text), then rows, struct layouts and constants of the real headers pinned to numbers
and types a person wrote down."""
import ctypes as C

import pytest

from coma_amd import _abi, _lib
from coma_amd.sd import ops as sd_ops
from coma_amd.seg import ops as seg_ops

_vp, _i, _i64, _f, _d, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t

HEADER = """
/* a header in the style of include/ */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define X_VERSION 7   /* a comment
                         over two lines */
#define X_E_BAD (-2)
#define X_HEX 0x10
#define X_ALL (X_VERSION | X_HEX)
enum { SD_OP_A = 3, SD_OP_B, SD_OP_C,
       SD_OP_D = 9, SD_OP_E };
typedef struct sd_desc {
  const void* a;      /* a pointer */
  int a0, a1;
  long long big;
  int tail;
  float* f;
} sd_desc;
typedef struct sd_choice { int bm, bn; size_t bytes; } sd_choice;
/* int sd_in_a_comment(int a); */
int sd_scalars(int a, int32_t b, int64_t c, long long d, size_t e, float f, double g, uint8_t h, uint64_t i, int8_t j,
               const int k, const double l);
int sd_pointers(const float* a, float* b, void** c, const char* d, const sd_desc* e, sd_choice* f, const uint8_t* g /*host*/,
                uint64_t* h, void* stream);
const char* sd_text(void);
size_t sd_bytes(void);
void sd_nothing(int a);
int
seg_split(const double* verts,
          int V, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* X_H */
"""


def test_parse_reads_the_style_of_the_headers():
    fn, st, de = _abi.parse(HEADER)
    assert list(fn) == ["sd_scalars", "sd_pointers", "sd_text", "sd_bytes", "sd_nothing", "seg_split"]     # header order, the comment ignored
    assert fn["sd_scalars"] == (_i, list(zip("abcdefghijkl", [_i, C.c_int32, _i64, C.c_longlong, _sz, _f, _d, C.c_uint8, C.c_uint64, C.c_int8, _i, _d])))
    assert fn["sd_pointers"] == (_i, [("a", _vp), ("b", _vp), ("c", _vp), ("d", C.c_char_p), ("e", _vp), ("f", _vp), ("g", _vp), ("h", _vp),
                                      ("stream", _vp)])
    assert fn["sd_text"] == (C.c_char_p, []) and fn["sd_bytes"] == (_sz, []) and fn["sd_nothing"] == (None, [("a", _i)])
    assert fn["seg_split"] == (_i, [("verts", _vp), ("V", _i), ("stream", _vp)])
    assert st == {"sd_desc": [("a", _vp), ("a0", _i), ("a1", _i), ("big", C.c_longlong), ("tail", _i), ("f", _vp)],
                  "sd_choice": [("bm", _i), ("bn", _i), ("bytes", _sz)]}
    # X_ALL and the include guard have no integer body: left out, not an error; the enum counts on from its explicit values
    assert de == {"X_VERSION": 7, "X_E_BAD": -2, "X_HEX": 16, "SD_OP_A": 3, "SD_OP_B": 4, "SD_OP_C": 5, "SD_OP_D": 9, "SD_OP_E": 10}


@pytest.mark.parametrize("text, offending", [
    ("int sd_f(unsigned a);", "unsigned a"),                                        # a type outside the map
    ("int sd_f(const short* a);", "const short* a"),                                # ... behind a pointer too
    ("long sd_f(int a);", "long sd_f"),                                             # ... and as the return type
    ("typedef struct sd_s { int a; char c; } sd_s;", "char c"),
    ("int sd_f(int a, float);", "float"),                                           # a parameter without a name
    ("int sd_f(const float*, int n);", "const float*"),
    ("int sd_f(int a[3]);", "int a[3]"),                                            # an array parameter
    ("int sd_f(void (*cb)(int), int n);", "void (*cb)(int)"),                       # a function pointer
    ("int sd_f(int a, ...);", "..."),                                               # variadic
    ("typedef struct sd_s { int a : 3; } sd_s;", "int a : 3"),                      # a bit-field
    ("typedef struct sd_s { struct { int x; } in; int y; } sd_s;", "struct { int x;"),                 # a nested struct
    ("typedef struct sd_s { int a[4]; } sd_s;", "int a[4]"),
    ("int sd_f(int a);\nint other_f(int a);", "int other_f(int a)"),                # leftovers: a name outside the ABI's prefixes,
    ("int sd_f(int a)\nint sd_g(int b);", "int sd_g(int b"),                        # a lost semicolon,
    ("struct sd_s { int a; };", "struct sd_s { int a"),                             # a struct that is no typedef,
    ("int sd_f(int a); // a comment in another style", "// a comment"),             # a comment the stripper does not know,
    ("static inline int sd_f(int a) { return a; }", "return a"),                    # a definition,
    ("typedef int sd_t;", "typedef int sd_t"),                                      # a typedef that is no struct
    ("enum { SD_A = SD_B + 1 };", "SD_A = SD_B + 1"),                               # an enum value that is no literal
    ("int sd_f(int a);\nint sd_f(int a);", "sd_f"),                                 # one name twice
])
def test_parse_refuses_what_it_does_not_understand(text, offending):
    with pytest.raises(_abi.AbiError) as e:
        _abi.parse(text, "bad.h")
    assert "bad.h" in str(e.value) and offending in str(e.value), str(e.value)


# rows of the hand-written table this binding replaced, pointers (it had POINTER(c_int64) and the like for host arrays) as c_void_p
PINNED = {
    "coma_last_error": (C.c_char_p, []),
    "coma_occupancy_fused": (_i, [_vp, _i, _i, _i, _vp, _d, _d, _d, _i, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "coma_entropy_f32": (_i, [_vp, _i64, _i, _f, _f, _vp, _vp]),
    "seg_point_sample_f32": (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, C.c_longlong, _vp]),
    "coma_intersection_status": (_i, [_vp, _vp, _vp]),
    "sd_model_create": (_i, [_vp]),
    "sd_model_bind": (_i, [_vp, C.c_char_p, _vp, _sz]),
    "coma_smplx_forward_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "sd_layernorm_f16": (_i, [_vp, _i64, _i, _f, _vp, _vp, _vp, _vp]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_rows_of_the_real_headers(name):
    assert _lib.SIGNATURES[name] == PINNED[name]
    assert len(_lib.PARAMS[name]) == len(PINNED[name][1]) and all(p.isidentifier() for p in _lib.PARAMS[name])


def test_parameter_names_of_the_real_headers():
    assert _lib.PARAMS["sd_layernorm_f16"] == ("x", "rows", "c", "eps", "gamma", "beta", "out", "stream")
    assert _lib.PARAMS["coma_intersection_status"] == ("workspace", "stream", "needed") and _lib.PARAMS["coma_last_error"] == ()
    assert list(_lib.SIGNATURES) == list(_lib.PARAMS) == list(_abi.FUNCTIONS) and len(_abi.FUNCTIONS) >= 132
    assert all(v[1] == [t for _, t in _abi.FUNCTIONS[k][1]] and v[0] is _abi.FUNCTIONS[k][0] for k, v in _lib.SIGNATURES.items())


@pytest.mark.parametrize("cls, cname, size, last, offset", [
    (sd_ops.ConvGemmDesc, "sd_conv_gemm_desc", 216, "phase", 212),
    (sd_ops.ConvGemmChoice, "sd_conv_gemm_choice", 48, "grid_y", 44),
    (seg_ops.SegConvDesc, "seg_conv_desc", 160, "split_k", 152),
    (seg_ops.SegConvChoice, "seg_conv_choice", 56, "slab_elems", 48),
])
def test_struct_layouts_are_the_hand_written_ones(cls, cname, size, last, offset):
    assert cls._fields_ == _abi.STRUCTS[cname] and cls._fields_[-1][0] == last
    assert C.sizeof(cls) == size and getattr(cls, last).offset == offset


def test_struct_fields_of_mixed_width():
    d = dict(_abi.STRUCTS["sd_conv_gemm_desc"])
    assert len(d) == 36 and d["a0"] is _vp and d["c1"] is _i and d["stride_res"] is _i64 and d["workspace_bytes"] is _sz and d["colstats"] is _vp
    assert sd_ops.ConvGemmDesc.stride_a.offset == 136 and sd_ops.ConvGemmDesc.workspace_bytes.offset == 176
    assert len(_abi.STRUCTS["seg_conv_desc"]) == 29 and dict(_abi.STRUCTS["seg_conv_choice"])["slab_elems"] is C.c_longlong
    assert sd_ops.ConvGemmChoice().asdict().keys() == dict(_abi.STRUCTS["sd_conv_gemm_choice"]).keys()


def test_constants_of_the_real_headers():
    D = _abi.DEFINES
    assert [D["SD_EPI_" + k] for k in ("NONE", "GEGLU", "SILU", "BIAS_ROWS", "PERM16_N", "PERM32_N", "QUICK_GELU")] == [0, 1, 2, 4, 8, 16, 32]
    assert (sd_ops.EPI_NONE, sd_ops.EPI_GEGLU, sd_ops.EPI_SILU, sd_ops.EPI_BIAS_ROWS, sd_ops.EPI_PERM16_N, sd_ops.EPI_PERM32_N,
            sd_ops.EPI_QUICK_GELU) == (0, 1, 2, 4, 8, 16, 32)
    assert "SD_EPI_ALL" not in D and "COMA_HIP_H" not in D
    from coma_amd.sd import model
    assert (D["SD_BUF_PERSISTENT"], D["SD_BUF_ZEROED"], D["SD_BUF_IF_NEW"]) == (1, 2, 4) == (model.BUF_PERSISTENT, model.BUF_ZEROED, model.BUF_IF_NEW)
    assert (D["COMA_OK"], D["COMA_E_INVALID"], D["COMA_E_LAUNCH"], D["COMA_E_DEVICE"]) == (0, -1, -2, -3)
    assert D["SEG_OP_CONV"] == 1 and D["SEG_OP_RESIZE"] == 2 and D["SEG_OP_PASTE"] == 16 and D["SEG_OP_RPN_SELECT_LEVELS"] == 17
    assert D["COMA_ABI_VERSION"] == 11 == _lib.ABI_VERSION
