"""GPU: coma_coap_encode_f32 / coma_coap_query_f32 / coma_coap_collision_f32 / coma_depth_optimize_coap_f64 through the C ABI and
coma_amd.coap on the fixture's seeded model (55 joints, 330 vertices, K = 15 parts), against the reference's own f64 results
(tests/golden/coap_golden.npz, R64) and, where the fixture holds no R64 value (a shifted body, per-point decisions), against the
restatement tests/coap_ref.py, which tests/test_coap_host.py pins to R64 at 1e-10.

Bounds: 4 e_ref_* of the fixture (the reference's own f32-versus-f64 error, max|R32 - R64| / max|R64|), times max|R64| of the
quantity.  Discrete outcomes (inside a part's box, occ > 0.01, occ > 0.5, the bounding-box prefilter) are compared only at points
whose R64 margin exceeds that bound (coap_ref.undecided); at most 2 % of a case's points may be excluded, and sums are compared after
the restatement is evaluated with the device's own decisions there.  Every call is made twice: the bits must be equal."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from tests import coap_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 15
_state = {}


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _model():
    from coma_amd import coap
    if "model" not in _state:
        M = R.model_arrays()
        body = dict(v_template=M["v_template"], faces=M["faces"], lbs_weights=M["lbs_weights"], parents=M["parents"])
        _state["model"] = coap.DeviceCOAP(body, M["weights"], n_samples=64, seed=0, device=DEV)
    return _state["model"]


def _parse(code):
    """The code block's fields as NumPy (layout: include/coma_hip.h)."""
    raw = code.cpu().numpy()
    hdr = raw[:16].view(np.int32)
    geo = raw[16:16 + K * 24 * 8].view(np.float64).reshape(K, 24)
    at = 16 + K * 24 * 8
    vbox = raw[at:at + 48].view(np.float64)
    latent = raw[at + 48:at + 48 + K * 128 * 4].view(np.float32).reshape(K, 128)
    Rm, o = geo[:, :9].reshape(K, 3, 3), geo[:, 9:12]
    Rt = np.swapaxes(Rm, 1, 2)
    return dict(hdr=hdr, bone_trans=np.concatenate([Rt, -np.einsum("krc,kc->kr", Rt, o)[:, :, None]], 2), centre=geo[:, 12:15], half=geo[:, 15:18],
                bbox_min=geo[:, 18:21], bbox_max=geo[:, 21:24], vmin=vbox[:3], vmax=vbox[3:], latent=latent.astype(np.float64))


def _encoded(name):
    """(DeviceCOAP with the case's body encoded, the code block's bytes of two encodes)."""
    m, c = _model(), R.case_inputs(name)
    if _state.get("encoded") != name:
        so = dict(full_pose=c["full_pose"], joints=c["joints"], vertices=c["vertices"])
        first = m.encode_body(so, samples=(c["ids"], c["bary"])).clone()
        second = m.encode_body(so, samples=(c["ids"], c["bary"]))
        _state.update(encoded=name, codes=(first, second))
    return m, _state["codes"]


def _bound(golden, q, ref):
    return 4.0 * float(golden[f"e_ref_{q}"]) * float(np.abs(ref).max())


@pytest.mark.parametrize("name", R.CASE_NAMES)           # n_samples 64, and 1000: ragged against every tile
def test_encode(hip_lib, golden, name):
    m, (first, second) = _encoded(name)
    assert torch.equal(first, second), "two encodes, different bits"
    got, want = _parse(first), R.case_code(name)
    assert got["hdr"].tolist() == [0x434F4150, K, 0, 0]
    for q in ("bone_trans", "bbox_min", "bbox_max", "latent"):
        ref = golden[f"{name}__r64_{q}"]
        gap, bound = float(np.abs(got[q] - ref).max()), _bound(golden, q, ref)
        print(f"{name} {q}: max |device - R64| {gap:.3e}, bound {bound:.3e}")
        assert gap <= bound, q
    assert np.abs(got["centre"] - want["centre"]).max() <= _bound(golden, "bbox_max", want["bbox_max"])
    assert np.abs(got["half"] - want["size"] * 0.5).max() <= _bound(golden, "bbox_max", want["bbox_max"]) * R.BBOX_PADDING
    c = R.case_inputs(name)
    assert np.array_equal(got["vmin"], c["vertices"].min(0).astype(np.float64)) and np.array_equal(got["vmax"], c["vertices"].max(0).astype(np.float64))


def _raw_query(hip_lib, m, points, d, front, derivative):
    """coma_coap_query_f32 through the C ABI -> (occ, docc or None, list length)."""
    from coma_amd import _lib
    p = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32), device=DEV)
    T = p.shape[0]
    occ = torch.full([T], 7.5, dtype=torch.float32, device=DEV)
    docc = torch.full([T], 7.5, dtype=torch.float32, device=DEV)
    ws = torch.zeros([hip_lib.coma_coap_query_workspace_bytes(K, T)], dtype=torch.uint8, device=DEV)
    dd = None if d is None else torch.tensor([d], dtype=torch.float64, device=DEV)
    with _lib.on_device(DEV) as stream:
        rc = hip_lib.coma_coap_query_f32(_lib.ptr(m.weights), m.weights.numel(), _lib.ptr(m.code), K, _lib.ptr(p), T, _lib.ptr(dd), _lib.vec3(front),
                                         1 if derivative else 0, _lib.ptr(occ), _lib.ptr(docc), _lib.ptr(ws), ws.numel(), stream)
    _lib.check(rc, "coma_coap_query_f32")
    return occ.cpu().numpy(), docc.cpu().numpy() if derivative else None, int(ws[:4].cpu().numpy().view(np.int32)[0])


def _check_query(hip_lib, golden, name, points, d, derivative):
    m, _ = _encoded(name)
    M, c, code = R.model_arrays(), R.case_inputs(name), R.case_code(name)
    front = c["front"].astype(np.float64)
    occ, docc, count = _raw_query(hip_lib, m, points, d, c["front"], derivative)
    again = _raw_query(hip_lib, m, points, d, c["front"], derivative)
    assert np.array_equal(occ.view(np.uint32), again[0].view(np.uint32)) and count == again[2]
    shifted = np.asarray(points, np.float64) - (d or 0.0) * front
    ref = R.query(M["weights"], code, shifted, direction=-front)
    skip = R.undecided(ref, code, golden)
    assert skip.mean() <= 0.02
    b_occ, b_docc = _bound(golden, "occupancy", golden[f"{name}__r64_occupancy"]), _bound(golden, "docc", golden[f"{name}__r64_docc"])
    gap = float(np.abs(occ - ref["occupancy"])[~skip].max(initial=0.0))
    print(f"{name} T={len(points)} d={d} derivative={derivative}: list {count}, max |occ - ref| {gap:.3e} (bound {b_occ:.3e}), excluded {int(skip.sum())}")
    assert gap <= b_occ
    assert np.array_equal((occ > 0)[~skip], ref["inside"].any(0)[~skip])
    if not skip.any():
        assert count == int(ref["inside"].sum())
    if derivative:
        assert np.array_equal(docc.view(np.uint32), again[1].view(np.uint32))
        gap = float(np.abs(docc - ref["docc"])[~skip].max(initial=0.0))
        print(f"    max |docc - ref| {gap:.3e} (bound {b_docc:.3e})")
        assert gap <= b_docc and (docc[~skip][~ref["inside"].any(0)[~skip]] == 0).all()
    return occ, docc, count, ref


@pytest.mark.parametrize("T", [1, 63, 65, 1000])
def test_query(hip_lib, golden, T):
    pts = R.case_inputs("small")["points"][:T]
    for d, derivative in ((None, False), (None, True), (0.0, True), (0.04, False), (0.04, True), (-0.07, True)):
        occ, docc, _, ref = _check_query(hip_lib, golden, "small", pts, d, derivative)
    if T == 1000:        # the unshifted query against the reference's own numbers, not only the restatement's
        occ, docc, _, _ = _check_query(hip_lib, golden, "small", pts, None, True)
        assert np.abs(occ - golden["small__r64_occupancy"]).max() <= _bound(golden, "occupancy", golden["small__r64_occupancy"])
        assert np.abs(docc - golden["small__r64_docc"]).max() <= _bound(golden, "docc", golden["small__r64_docc"])
        assert (occ > 0.5).sum() > 100 and (occ == 0).sum() > 100


def test_query_special_sets(hip_lib, golden):
    M, c, code = R.model_arrays(), R.case_inputs("small"), R.case_code("small")
    ref = R.query(M["weights"], code, c["points"])
    outside = c["points"][~ref["inside"].any(0)]
    assert len(outside) >= 100
    occ, docc, count, _ = _check_query(hip_lib, golden, "small", outside[:100], None, True)
    assert count == 0 and not occ.any() and not docc.any()                       # bit patterns: +0.0 everywhere, an empty list
    alone = ref["inside"].sum(0) == 1
    part = int(np.bincount(ref["inside"][:, alone].argmax(0)).argmax())
    mine = c["points"][alone & ref["inside"][part]]
    assert len(mine) >= 3
    occ, docc, count, r = _check_query(hip_lib, golden, "small", mine, None, True)
    assert count == len(mine) and (r["inside"].sum(0) == 1).all() and r["inside"][part].all()
    _check_query(hip_lib, golden, "ragged", R.case_inputs("ragged")["points"], 0.04, True)      # the other body: n_samples = 1000


def _raw_collision(hip_lib, m, points, d, front):
    from coma_amd import _lib
    p = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32), device=DEV)
    T = p.shape[0]
    result = torch.full([2], 7.5, dtype=torch.float64, device=DEV)
    kept = torch.full([1], -1, dtype=torch.int64, device=DEV)
    ws = torch.zeros([hip_lib.coma_coap_query_workspace_bytes(K, T)], dtype=torch.uint8, device=DEV)
    dd = torch.tensor([d], dtype=torch.float64, device=DEV)
    with _lib.on_device(DEV) as stream:
        rc = hip_lib.coma_coap_collision_f32(_lib.ptr(m.weights), m.weights.numel(), _lib.ptr(m.code), K, _lib.ptr(p), T, _lib.ptr(dd), _lib.vec3(front),
                                             R.FILTER_THRESHOLD, _lib.ptr(result), _lib.ptr(kept), _lib.ptr(ws), ws.numel(), stream)
    _lib.check(rc, "coma_coap_collision_f32")
    return result.cpu().numpy(), int(kept.cpu().numpy()[0])


def _device_decisions(hip_lib, m, code, ref, skip, points, d, front):
    """The discrete outcomes for the restatement: its own, except at the excluded points, where the device's (read off its occupancy)."""
    if not skip.any():
        return None
    occ, _, _ = _raw_query(hip_lib, m, points, d, front, False)
    pre = ((points >= code["vmin"] + d * front) & (points <= code["vmax"] + d * front)).all(-1)
    kept = np.where(skip, occ > R.FILTER_THRESHOLD, pre & (ref["occupancy"] > R.FILTER_THRESHOLD))
    return dict(kept=kept, above=np.where(skip, occ > R.LEVEL_SET, ref["occupancy"] > R.LEVEL_SET))


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_collision(hip_lib, golden, name):
    m, _ = _encoded(name)
    M, c, code = R.model_arrays(), R.case_inputs(name), R.case_code(name)
    front, pts = c["front"].astype(np.float64), c["points"].astype(np.float64)
    b_loss, b_dloss = _bound(golden, "loss", golden[f"{name}__r64_loss"]), _bound(golden, "dloss", golden[f"{name}__r64_dloss"])
    for i, d in enumerate(R.DISPLACEMENTS):
        got, kept = _raw_collision(hip_lib, m, c["points"], d, c["front"])
        again, kept2 = _raw_collision(hip_lib, m, c["points"], d, c["front"])
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64)) and kept == kept2
        ref = R.query(M["weights"], code, pts - d * front, direction=-front)
        skip = R.undecided(ref, code, golden, points=pts, d=d, f=front)
        assert skip.mean() <= 0.02
        want = R.collision(M["weights"], code, pts, d, front, R.FILTER_THRESHOLD, _device_decisions(hip_lib, m, code, ref, skip, pts, d, front))
        print(f"{name} d={d}: loss {got[0]:.6f} (ref {want['loss']:.6f}, R64 {golden[f'{name}__r64_loss'][i]:.6f}, bound {b_loss:.2e}), "
              f"dloss {got[1]:+.6f} (ref {want['dloss']:+.6f}, bound {b_dloss:.2e}), kept {kept} (ref {int(want['kept'].sum())}), excluded {int(skip.sum())}")
        assert abs(got[0] - want["loss"]) <= b_loss and abs(got[1] - want["dloss"]) <= b_dloss and kept == int(want["kept"].sum())
        if not skip.any():
            assert abs(got[0] - golden[f"{name}__r64_loss"][i]) <= b_loss and abs(got[1] - golden[f"{name}__r64_dloss"][i]) <= b_dloss
            assert kept == int(golden[f"{name}__r64_kept"][i].sum())


def test_depth_optimisation_trajectory(hip_lib, golden):
    from coma_amd import depth_opt as D
    tr, ti = R.TRAJECTORY, R.trajectory_inputs()
    m, _ = _encoded(tr["case"])
    pts = R.case_inputs(tr["case"])["points"]
    run = lambda: D.optimize_displacement_coap(m, pts, ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"], tr["d0"], tr["lr"],
                                               tr["w_multiview"], tr["w_collision"], tr["E"], R.FILTER_THRESHOLD)
    got, again = run(), run()
    for q in ("traj", "Ctraj", "losses"):
        assert np.array_equal(got[q].view(np.uint64), again[q].view(np.uint64)), q
    for q in ("traj", "Ctraj"):
        ref = golden[f"trajectory__r64_{q}"]
        gap, bound = float(np.abs(got[q] - ref).max()), _bound(golden, q, ref)
        print(f"{q}: max |device - R64| {gap:.3e}, bound {bound:.3e} (R32's own gap {np.abs(golden[f'trajectory__r32_{q}'] - ref).max():.3e})")
        assert gap <= bound, q
    assert np.array_equal(got["losses"][:, 1], got["Ctraj"][:, 0]) and got["traj"][0] == 0.0 and got["d"] == got["traj"][-1]
    assert np.abs(got["losses"][:, 0] - golden["trajectory__r64_losses"][:, 0]).max() <= 1e-6 * golden["trajectory__r64_losses"][:, 0].max()
    off = D.optimize_displacement_coap(m, pts, ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"], 0.0, tr["lr"], tr["w_multiview"], 0.0, 5)
    assert not off["Ctraj"].any() and not off["losses"][:, 1].any()


def test_parent_entry_point_keeps_its_bits(hip_lib):
    """coma_depth_optimize_f64 shares its multiview term and its Adam step with the new entry point: still bit-identical to shift_ref."""
    from coma_amd import depth_opt as D
    from tests import shift_ref as SR
    ti = R.trajectory_inputs()
    want = SR.optimize(None, ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"], 0.0, 0.01, 1e-3, 0.0, 20)
    got = D.optimize_displacement(None, ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"], 0.0, 0.01, 1e-3, 0.0, 20, device=DEV)
    assert np.array_equal(got["traj"].view(np.uint64), want["traj"].view(np.uint64)) and np.array_equal(got["losses"].view(np.uint64), want["losses"].view(np.uint64))
    coap = D.optimize_displacement_coap(None, None, ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"], 0.0, 0.01, 1e-3, 0.4, 20)
    assert np.array_equal(coap["traj"].view(np.uint64), want["traj"].view(np.uint64))      # no points: the same multiview-only run


def test_bad_table_is_reported_by_status(hip_lib):
    from coma_amd import _lib
    m, c = _model(), R.case_inputs("small")
    ids = c["ids"].copy()
    ids[3, 5, 1] = R.MODEL_V
    with pytest.raises(_lib.ComaHipError, match="outside \\[0, V\\)"):
        m.encode_body(dict(full_pose=c["full_pose"], joints=c["joints"], vertices=c["vertices"]), samples=(ids, c["bary"]))
    _state["encoded"] = None


def test_cli_end_to_end(hip_lib, golden, tmp_path):
    from PIL import Image
    from coma_amd import coap as P, depth_opt as D
    from oracle import triangulation_oracle as T
    from src.generation import optimize_depth as cli
    from src.generation.initialize_depth import asset_world
    from tests import metrics_common as MC
    from tests import raster_ref as RR
    from tests import smplx_ref as S
    root = str(tmp_path)
    M, c = R.model_arrays(), R.case_inputs("small")
    np.savez(f"{root}/SMPLX_NEUTRAL.npz", **M["file"])
    torch.save({"state_dict": {k: torch.as_tensor(v) for k, v in M["weights"].items()}}, f"{root}/coap.ckpt")
    sc, cat, asset, mask, prompt = "BEHAVE", "backpack", "behave_asset", "mask:000", "sitting on the backpack, full body"
    ball = RR.icosphere(3, 0.45)
    MC.write_obj(f"{root}/data/BEHAVE/objects/{cat}/{cat}_canon_lowres_in_gen_coord.obj", ball[0] + np.array([0.0, 0.5, 0.0]), ball[1])
    centre = np.array([0.0, 0.0, 0.5])
    eyes = [np.array([0.0, -3.0, 0.5]), np.array([2.5, -1.5, 0.9]), np.array([-2.2, -2.0, 1.4]), np.array([1.0, -2.8, 1.8])]
    cams = [dict(R=RR.look_at(e, centre), t=e, scale=2.4, resolution=(64, 64), obj_R=np.eye(3), obj_t=np.zeros((3, 1))) for e in eyes]
    for v, cam in enumerate(cams):
        MC.write_pickle(f"{root}/cam/{sc}/{cat}/{asset}/view:{v:05}.pickle", cam)
    front = cams[0]["R"][:, 2]
    conv = dict(focals=(80.0, 80.0), princpt=(32.0, 32.0), z_mean=4.0)
    transl = np.array([[0.0, 0.0, 4.0]], dtype=np.float32)
    extra = np.random.default_rng(11).normal(scale=0.3, size=(137 - 55, 3)).astype(np.float32)

    def body_model(smplx_data, smplx_path, full_pose=False):
        v, j = c["vertices"] - c["vertices"].mean(0), np.concatenate([c["joints"] - c["vertices"].mean(0), extra])
        return (v, j, c["full_pose"]) if full_pose else (v, j)
    probe = D.convert_cam2real(np.zeros((1, 3), np.float32), transl, (64, 64), cams[0], conv).astype(np.float64)
    placed = np.array([0.0, -0.25, 0.5]) - probe
    below = f"{sc}/{cat}/{asset}/view:00000/{mask}/{prompt}"
    os.makedirs(f"{root}/inpaint/{below}", exist_ok=True)
    Image.new("RGB", (64, 64)).save(f"{root}/inpaint/{below}/0.png")
    faces = M["faces"].astype(np.int64)
    MC.write_pickle(f"{root}/init/{below}/000000.pickle", dict(faces=faces, displacement=placed))
    smplx_data = dict(transl=transl)
    V0, J0 = (D.convert_cam2real(x, transl, (64, 64), cams[0], conv).astype(np.float64) + placed for x in body_model(smplx_data, None))
    MC.write_pickle(f"{root}/pred/{below}/000000.pickle", dict(smplx_data=smplx_data, convert_data=conv, joints_proj=T.render(J0.copy(), cams[0]).astype(np.float32)))
    for v in (1, 2, 3):
        MC.write_pickle(f"{root}/pred/{sc}/{cat}/{asset}/view:{v:05}/{mask}/{prompt}/000000.pickle",
                        dict(joints_proj=T.render(J0 - 0.08 * front, cams[v]).astype(np.float32)))
    args = cli.build_parser().parse_args(["--inpaint_dir", f"{root}/inpaint", "--camera_dir", f"{root}/cam", "--human_preds_dir", f"{root}/pred",
                                          "--human_initial_dir", f"{root}/init", "--save_dir", f"{root}/opt", "--asset_obj_root", f"{root}/data",
                                          "--num_epoch", "10", "--w_multiview", "1e-4", "--ransac_threshold", "2", "--smplx_path", f"{root}/SMPLX_NEUTRAL.npz",
                                          "--collision", "coap", "--coap_ckpt", f"{root}/coap.ckpt", "--coap_samples", "64", "--coap_seed", "4"])
    done = cli.main(args, body_model=body_model)
    assert [os.path.basename(p) for p in done] == ["000000.pickle"]
    with open(done[0], "rb") as fh:
        saved = pickle.load(fh)
    # the same run through the product's calls, and its first epoch through the restatement with the same sample table
    world = asset_world(ball[0] + np.array([0.0, 0.5, 0.0]), cams[0], "BEHAVE")
    with open(f"{root}/pred/{below}/000000.pickle", "rb") as fh:
        pred = pickle.load(fh)
    item = dict(inpaint_pth=f"{root}/inpaint/{below}/0.png")
    inliers = cli.find_inliers(pred["joints_proj"], item, f"{root}/pred", f"{root}/cam", 400, 2, 100, False, ["original", "full body"], None, "cuda")
    views, cand_view, cand_xy = D.inlier_views(inliers)
    body = dict(v_template=M["v_template"], faces=M["faces"], lbs_weights=M["lbs_weights"], parents=M["parents"])
    m = P.DeviceCOAP(body, f"{root}/coap.ckpt", n_samples=64, seed=4, device=DEV)
    m.encode_body(dict(full_pose=c["full_pose"], joints=J0, vertices=V0))
    want = D.optimize_displacement_coap(m, world, views, J0[D.BODY_INDICES], front, cand_view, cand_xy, 0.0, 0.01, 1e-4, 0.4, 10)
    assert saved["num_inliers"] == len(inliers) == 3 and want["Ctraj"][0, 0] > 0.0 and want["d"] != 0.0
    assert np.array_equal(saved["verts"], (V0 + want["d"] * front.reshape((1, 3))).astype(np.float32)) and saved["faces"].dtype == np.uint32
    V32, J32 = V0.astype(np.float32), J0.astype(np.float32)
    ids, bary = P.draw_samples(np.random.RandomState(4), V32, M["part"], 64)
    code = R.encode(M["weights"], M["part"], M["parents"], c["full_pose"], J32, V32, ids, bary)
    first = R.collision(M["weights"], code, world.astype(np.float32), 0.0, front, R.FILTER_THRESHOLD)
    print(f"d {want['d']!r}; COAP loss {want['Ctraj'][0, 0]:.6f} (restated {first['loss']:.6f}) -> {want['Ctraj'][-1, 0]:.6f}; kept {int(first['kept'].sum())} of {len(world)}")
    w64 = world.astype(np.float32).astype(np.float64)
    r = R.query(M["weights"], code, w64, direction=-front)
    if not R.undecided(r, code, golden, points=w64, d=0.0, f=front).any():
        # a sum over the colliding points of terms that each carry the per-point bound
        n = int((first["kept"] & first["above"]).sum())
        assert abs(want["Ctraj"][0, 0] - first["loss"]) <= n * 4.0 * float(golden["e_ref_occupancy"])
        assert abs(want["Ctraj"][0, 1] - first["dloss"]) <= n * 4.0 * float(golden["e_ref_docc"]) * np.abs(r["docc"]).max()
