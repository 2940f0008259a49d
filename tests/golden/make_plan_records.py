#!/usr/bin/env python3
"""Golden launch records: tests/golden/plan_records.json, the layout of every recordable entry point's PlanRec in an SDMODEL3 file.

Each of the 40 recordable entry points (include/sd_hip.h, include/seg_hip.h) is called once, through the C ABI, inside one recording
of a model whose single registered range is a fake address with flags 0 -- recording and sd_model_save are host code that never reads
that memory, so this runs without a GPU.  Arguments are distinct sentinels (pointers = base + distinct offsets, distinct small integers,
floats exact in binary), so a swapped or dropped slot changes the file.  The saved plan section is parsed back and every record's kind,
p (as stored: ((buf + 1) << 48) | offset), i and f written out.   Run: python tests/golden/make_plan_records.py
"""
import ctypes as C
import json
import os
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "plan_records.json")

BASE, SPAN = 0x100000000, 1 << 20          # the fake registered range: never dereferenced
REC_BYTES = 8 + 16 * 8 + 24 * 8 + 4 * 8    # kind, reserved, p[16], i[24], f[4]


RECORDABLE = [          # in PlanKind order, then the PK_SEG operators in SEG_OP_* order
    "sd_conv_gemm_f16", "sd_groupnorm_f16", "sd_groupnorm_colstats_f16", "sd_layernorm_f16", "sd_attention_f16", "sd_softmax_f16",
    "sd_timestep_embedding_f16", "sd_copy_d2d", "sd_attention_wide_f16", "sd_xattn_chain_f16", "sd_xfront_f16", "sd_groupnorm_table_f16",
    "sd_xtail_f16", "sd_conv3x3_small_n_f16", "sd_winograd_input_f16", "sd_winograd_output_f16", "sd_gn_winograd_input_f16",
    "sd_im2col3x3_c3_f16", "sd_groupnorm_table_cat_f16", "sd_conv3x3_halo_f16", "sd_conv3x3_c3_f16", "sd_text_embed_f16",
    "sd_attention_causal_f16",
    "seg_conv_gemm_f32", "seg_resize_normalize_u8", "seg_maxpool3x3s2_f32", "seg_subsample2_f32", "seg_memset", "seg_rpn_select",
    "seg_sort_candidates", "seg_nms", "seg_roi_align_f32", "seg_box_predict", "seg_finalize_detections", "seg_point_sample_f32",
    "seg_upsample2x_f32", "seg_topk_points", "seg_point_logit_scatter", "seg_paste_masks", "seg_rpn_select_levels",
]


class _Sentinels:
    def __init__(self):
        self.np = self.ni = self.nf = 0

    def p(self):
        self.np += 1
        return C.c_void_p(BASE + 64 * self.np)

    def i(self):
        self.ni += 1
        return self.ni + 1

    def f(self):
        self.nf += 1
        return 0.25 * self.nf + 0.5


def _calls(h, s):
    """(name, thunk) for every recordable entry point; argument kinds follow _lib.SIGNATURES."""
    from coma_amd import _lib
    from coma_amd.sd.ops import ConvGemmDesc
    from coma_amd.seg.ops import SegConvDesc

    def plain(name):
        def run():
            args = []
            for t in _lib.SIGNATURES[name][1][:-1]:       # the trailing stream stays NULL
                if t in (C.c_float, C.c_double):
                    args.append(s.f())
                elif t is C.c_void_p:
                    args.append(s.p())
                else:
                    args.append(s.i())
            return getattr(h, name)(*args, None)
        return run

    def conv():
        d = ConvGemmDesc()
        for name, t in d._fields_:
            setattr(d, name, s.p() if t is C.c_void_p else s.i())
        d.phase = 3
        return h.sd_conv_gemm_f16(C.byref(d), None)

    def seg_conv():
        d = SegConvDesc()
        for name, t in d._fields_:
            setattr(d, name, s.p() if t is C.c_void_p else s.i())
        return h.seg_conv_gemm_f32(C.byref(d), None)

    def rpn_levels():
        n = 3
        preds = (C.c_void_p * n)(*[s.p().value for _ in range(n)])
        cells = (C.c_void_p * n)(*[s.p().value for _ in range(n)])
        fh = (C.c_int * n)(*[s.i() for _ in range(n)])
        fw = (C.c_int * n)(*[s.i() for _ in range(n)])
        return h.seg_rpn_select_levels(preds, cells, fh, fw, n, s.i(), s.i(), s.i(), s.i(), s.f(), s.f(), s.i(), s.p(), s.p(), s.p(),
                                       s.p(), None)

    def xchain():      # debug_out / debug_stage are not part of the record: NULL, 0
        return h.sd_xattn_chain_f16(*[s.p() for _ in range(15)], s.i(), s.i(), s.i(), s.i(), s.f(), None, 0, None)

    special = {"sd_conv_gemm_f16": conv, "sd_xattn_chain_f16": xchain, "seg_conv_gemm_f32": seg_conv, "seg_rpn_select_levels": rpn_levels}
    return [(n, special.get(n) or plain(n)) for n in RECORDABLE]


def record_all():
    """Record every entry point once and return [{"call", "kind", "p", "i", "f"}] parsed from the saved model."""
    from coma_amd import _lib
    h = _lib.lib()
    m = C.c_void_p()
    assert h.sd_model_create(C.byref(m)) == 0
    try:
        assert h.sd_model_register_buffer(m, C.c_void_p(BASE), SPAN, 0) == 0
        assert h.sd_model_record_begin(m, b"all") == 0
        names = []
        try:
            for name, run in _calls(h, _Sentinels()):
                rc = run()
                assert rc == 0, f"{name}: {rc} {h.coma_last_error().decode()}"
                names.append(name)
        finally:
            h.sd_model_record_end(m)
        assert h.sd_model_num_launches(m, b"all") == len(names)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "m.sdm")
            assert h.sd_model_save(m, path.encode()) == 0, h.coma_last_error().decode()
            blob = open(path, "rb").read()
    finally:
        h.sd_model_destroy(m)
    return [dict(call=n, **r) for n, r in zip(names, parse_plan(blob), strict=True)]


def parse_plan(blob):
    """The records of the single plan of an SDMODEL3 file with no bindings (format: coma_amd/csrc/sd_plan.hip)."""
    assert blob[:8] == b"SDMODEL3"
    off = 24
    (nbuf,) = struct.unpack_from("<I", blob, off)
    off += 4 + 12 * nbuf
    (nbind,) = struct.unpack_from("<I", blob, off)
    assert nbind == 0
    (nplans,) = struct.unpack_from("<I", blob, off + 4)
    assert nplans == 1
    (nrec,) = struct.unpack_from("<I", blob, off + 8 + 32)
    off += 8 + 32 + 4
    recs = []
    for k in range(nrec):
        v = struct.unpack_from("<ii16Q24q4d", blob, off + k * REC_BYTES)
        recs.append({"kind": v[0], "p": list(v[2:18]), "i": list(v[18:42]), "f": list(v[42:46])})
    assert off + nrec * REC_BYTES == len(blob)
    return recs


def dumps(recs):
    return "[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in recs) + "\n]\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    recs = record_all()
    with open(OUT, "w") as f:
        f.write(dumps(recs))
    print(f"{len(recs)} records -> {OUT}")
