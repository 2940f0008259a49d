"""CPU: the launch-record layout of every recordable entry point, as sd_model_save writes it, against tests/golden/plan_records.json.

Where each argument sits in a PlanRec is part of the SDMODEL3 format; this pins it for all 40 recorded entry points (recording and
saving are host code: the model's one registered range is a fake address and nothing is launched).  The fixture is written by
tests/golden/make_plan_records.py."""
import json
import os

import pytest
import torch

from tests.golden import make_plan_records as gen


@pytest.mark.skipif(torch.cuda.is_available(), reason="a record site that launched would touch the fake addresses on a real device")
def test_plan_records_match_golden(hip_lib):
    got = gen.record_all()
    assert len(got) == len(gen.RECORDABLE) == 40
    with open(gen.OUT) as f:
        want = json.load(f)
    assert [r["call"] for r in got] == [r["call"] for r in want]
    for g, w in zip(got, want):
        assert g == w, f"{g['call']}: record differs from the golden layout"
