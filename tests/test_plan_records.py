"""CPU: the launch-record layout of every recordable entry point, as sd_model_save writes it, against tests/golden/plan_records.json.

Where each argument sits in a PlanRec is part of the SDMODEL3 format; this pins it for all 40 recorded entry points (recording and
saving are host code: the model's one registered range is a fake address and nothing is launched).  The fixture is written by
tests/golden/make_plan_records.py."""
import ctypes as C
import json
import os

import pytest
import torch

from tests.domain_kit import COMA_E_INVALID
from tests.golden import make_plan_records as gen

SD_EPI_ALL = 1 | 2 | 4 | 8 | 16 | 32        # include/sd_hip.h: GEGLU | SILU | BIAS_ROWS | PERM16_N | PERM32_N | QUICK_GELU


@pytest.mark.skipif(torch.cuda.is_available(), reason="a record site that launched would touch the fake addresses on a real device")
def test_plan_records_match_golden(hip_lib):
    got = gen.record_all()
    assert len(got) == len(gen.RECORDABLE) == 40
    with open(gen.OUT) as f:
        want = json.load(f)
    assert [r["call"] for r in got] == [r["call"] for r in want]
    for g, w in zip(got, want):
        assert g == w, f"{g['call']}: record differs from the golden layout"


def _conv_desc(epi):
    from coma_amd.sd.ops import ConvGemmDesc
    d = ConvGemmDesc()
    d.a0, d.w, d.out = gen.BASE, gen.BASE + 64, gen.BASE + 128
    d.c0, d.batch, d.in_h, d.in_w, d.out_h, d.out_w, d.taps, d.stride, d.pad, d.n = 64, 1, 8, 8, 8, 8, 9, 1, 1, 64
    d.epi = epi
    return d


def test_conv_record_rejects_epi_bits_outside_sd_epi_all(hip_lib):
    """Kernel choice is a function of the descriptor alone: a bit outside SD_EPI_ALL (such as a former tuning bit) is refused when the
    launch is recorded, so no saved model can carry one.  Recording is host code: nothing is launched."""
    m = C.c_void_p()
    assert hip_lib.sd_model_create(C.byref(m)) == 0
    try:
        assert hip_lib.sd_model_register_buffer(m, C.c_void_p(gen.BASE), gen.SPAN, 0) == 0
        assert hip_lib.sd_model_record_begin(m, b"p") == 0
        try:
            assert hip_lib.sd_conv_gemm_f16(C.byref(_conv_desc(SD_EPI_ALL)), None) == 0, hip_lib.coma_last_error()
            for bit in (6, 20, 24, 28, 31):
                rc = hip_lib.sd_conv_gemm_f16(C.byref(_conv_desc(SD_EPI_ALL | (1 << bit))), None)
                assert rc == COMA_E_INVALID and b"SD_EPI_ALL" in hip_lib.coma_last_error(), bit
        finally:
            hip_lib.sd_model_record_end(m)
        assert hip_lib.sd_model_num_launches(m, b"p") == 1
    finally:
        hip_lib.sd_model_destroy(m)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a launch that got past the check would touch the fake addresses on a real device")
def test_conv_call_rejects_epi_bits_outside_sd_epi_all(hip_lib):
    rc = hip_lib.sd_conv_gemm_f16(C.byref(_conv_desc(1 << 20)), None)
    assert rc == COMA_E_INVALID and b"SD_EPI_ALL" in hip_lib.coma_last_error()
