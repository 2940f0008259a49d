"""CPU: the batched SMPL-X body model's host half.  The f64 restatement tests/smplx_ref.py called once per body against the third-party
package's own lbs and SMPLX class at batch_size = 3 (R64 of tests/golden/smplx_batch_golden.npz) to the project's 1e-12; the
`batch_size` argument of coma_amd.body_model.DeviceSMPLX and what it refuses; the refusals of the batched C entry points, which all
return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import domain_kit as K
from tests import smplx_batch_ref as B
from tests import smplx_ref as S


@pytest.fixture(scope="module")
def golden():
    return B.load_golden()


@pytest.mark.parametrize("case", B.CASES)
def test_restatement_per_body_agrees_with_the_package_at_batch_size_3(golden, case):
    inp = B.case_inputs(case)
    for key in ("coefficients", "theta", "transl"):
        assert np.array_equal(golden[f"{case}__{key}"], inp[key]), key            # the seeded inputs are the stored ones
    assert inp["coefficients"].shape[0] == (B.N if case.endswith("per_body") else 1)
    assert not inp["theta"][0].any() and abs(np.linalg.norm(inp["theta"][2, 9:12]) - np.pi) < 1e-6 and inp["theta"][1].any()
    got = B.restated(case)
    want = {q: golden[f"{case}__r64_{q}"] for q in B.QUANTITIES + ("full_pose",)}
    want["joints"] = B.golden_joints(golden, case)
    for q in want:
        assert got[q].shape == want[q].shape and got[q].shape[0] == B.N, q
        dev = S.rel_dev(got[q], want[q])
        print(f"{case} {q}: {dev:.3e}")
        assert np.all(np.isfinite(got[q])) and dev <= 1e-12, (q, dev)
    if case.startswith("class"):                                                  # the package's 21 vertex picks are vertices of their body
        picks = golden[f"{case}__r64_joints"][:, 55:76]
        assert picks.shape == (B.N, 21, 3)


def test_pooled_reference_error_is_the_generator_s_definition(golden):
    for q in B.QUANTITIES:
        pool = max(S.rel_dev(golden[f"{case}__r32_{q}"], golden[f"{case}__r64_{q}"]) for case in B.CASES)
        assert float(golden[f"e_ref_{q}"]) == pool and 0 < pool < 1e-5, q


def test_batch_size_validation():
    from coma_amd.body_model import MAX_BATCH, DeviceSMPLX
    model, _ = B.model_of("lbs")
    assert DeviceSMPLX(model, n_pca=6).batch_size == 1
    assert DeviceSMPLX(model, n_pca=6, batch_size=3).batch_size == 3 and MAX_BATCH == 1024
    assert DeviceSMPLX(model, n_pca=6, batch_size=np.int64(MAX_BATCH)).batch_size == MAX_BATCH
    for bad in (0, -1, MAX_BATCH + 1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="batch_size"):
            DeviceSMPLX(model, n_pca=6, batch_size=bad)


def test_shape_gradient_is_refused_at_batch_size_2():
    from coma_amd.body_model import DeviceSMPLX
    model, _ = B.model_of("lbs")
    with pytest.raises(ValueError, match=r'"shape" with batch_size=2'):
        DeviceSMPLX(model, n_pca=6, batch_size=2, differentiable=("joints", "shape"))
    assert DeviceSMPLX(model, n_pca=6, batch_size=2, differentiable=("joints", "full_pose")).differentiable == {"joints", "full_pose"}
    assert DeviceSMPLX(model, n_pca=6, batch_size=1, differentiable=("shape",)).batch_size == 1


def test_default_object_still_refuses_two_rows():
    from coma_amd.body_model import DeviceSMPLX
    model, _ = B.model_of("lbs")
    for body in (DeviceSMPLX(model, n_pca=6), DeviceSMPLX(model, n_pca=6, batch_size=1)):
        with pytest.raises(ValueError, match="batch size 1"):
            body(body_pose=torch.zeros(2, 63))
        with pytest.raises(ValueError, match="batch size 1"):
            body(betas=torch.zeros(2, 10))


def test_batched_object_names_both_sizes_when_a_leading_dimension_fits_neither():
    """Shapes are looked at before anything touches the device, so this runs on a machine without one."""
    from coma_amd.body_model import DeviceSMPLX
    model, _ = B.model_of("lbs")
    body = DeviceSMPLX(model, n_pca=6, batch_size=3)
    with pytest.raises(ValueError, match=r"body_pose: leading dimension 2 is neither 1 nor batch_size=3"):
        body(body_pose=torch.zeros(2, 63))
    with pytest.raises(ValueError, match=r"transl: leading dimension 4 is neither 1 nor batch_size=3"):
        body(body_pose=torch.zeros(3, 63), transl=torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"betas: leading dimension 2 is neither 1 nor batch_size=3"):
        body(body_pose=torch.zeros(3, 63), betas=torch.zeros(2, 10))
    with pytest.raises(ValueError, match=r"left_hand_pose: expected \[3,6\] or \[1,6\]"):
        body(left_hand_pose=torch.zeros(3, 45))


def test_from_file_passes_batch_size_on(tmp_path):
    from coma_amd.body_model import DeviceSMPLX
    model, _ = B.model_of("lbs")
    np.savez(tmp_path / "SMPLX_NEUTRAL.npz", **model)
    assert DeviceSMPLX.from_file(str(tmp_path / "SMPLX_NEUTRAL.npz"), num_pca_comps=6, batch_size=5).batch_size == 5
    assert DeviceSMPLX.from_file(str(tmp_path / "SMPLX_NEUTRAL.npz"), num_pca_comps=6).batch_size == 1


def test_size_functions_and_refusals_before_any_launch(hip_lib):
    """Every row of the refusal table is refused with its text; on a machine without a device the accepted base passes every argument
    check and fails only at the launch."""
    L = hip_lib
    V, J = 300, 55
    one = L.coma_smplx_saved_bytes(V, J)
    assert [L.coma_smplx_batch_saved_bytes(V, J, n) for n in (1, 2, 1024)] == [one, 2 * one, 1024 * one] and one % 16 == 0
    for f in (L.coma_smplx_batch_saved_bytes, L.coma_smplx_batch_workspace_bytes, L.coma_smplx_batch_grad_workspace_bytes):
        assert f(V, J, 1) > 0 and f(V, J, 9) > f(V, J, 8) and f(V, J, 9) % 16 == 0
        assert f(V, J, 0) == f(V, J, 1025) == f(0, J, 2) == f(V, 65, 2) == f(V, 0, 2) == 0
    P = 9 * (J - 1)
    assert L.coma_smplx_batch_workspace_bytes(V, J, 3) == 3 * 8 * P + 3 * 8 * 8 * 3 * V        # features, eight partial offsets per body
    _, fm = B.model_of("lbs")
    parents = (ctypes.c_int32 * J)(*[max(int(p), 0) for p in fm["parents"]])
    bad = (ctypes.c_int32 * J)(*parents)
    bad[7] = 9
    table = B.refusal_table(L, parents, bad)
    n = K.check_refusals(L, table, K.host_resolver(), expect_control=not torch.cuda.is_available())
    assert n == sum(len(rows) for _, rows in table.values()) >= 60
    assert L.coma_smplx_extra_joints_batch_f32(None, None, None, None, V, 0, 3, None, None) == 0      # E = 0: nothing to do, as the single-body call
