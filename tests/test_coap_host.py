"""CPU: COAP's restatement (tests/coap_ref.py) against the reference's own COAPBodyModel in f64 (tests/golden/coap_golden.npz), the
product's partition, checkpoint loader and weight packing, the refusals of the new entry points (argument checks, which return before
any launch) and the depth-optimisation CLI's new flags."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import coap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def model():
    return R.model_arrays()


def test_partition_equals_the_references(golden, model):
    part = model["part"]
    assert len(part["tight_faces"]) == 15 and len(part["joint_mapper"]) == 22
    for key in ("tight_faces", "extended_faces", "tight_vert_selector", "joint_mapper"):
        assert np.array_equal(part[key], golden[f"partition__{key}"]), key
    assert (part["tight_faces"][:, 0, 0] >= 0).all(), "every part has a tight face"


def test_product_partition_equals_the_restatement(model):
    from coma_amd import coap
    got = coap.partition(model["v_template"], model["faces"], model["lbs_weights"], model["parents"], "smplx")
    for key, want in model["part"].items():
        assert np.array_equal(got[key], want) and got[key].dtype == want.dtype, key
    rng = np.random.RandomState(5)
    W = rng.rand(40, 24)
    faces = np.stack([rng.choice(40, 3, replace=False) for _ in range(60)])
    parents = np.array([-1] + [int(rng.randint(0, i)) for i in range(1, 24)])
    W[np.arange(40), np.arange(40) % 24] += 2.0                      # every joint owns a vertex
    a, b = coap.partition(rng.rand(40, 3), faces, W, parents, "smpl"), R.partition(rng.rand(40, 3), faces, W, parents, "smpl")
    assert all(np.array_equal(a[k], b[k]) for k in b) and len(a["tight_faces"]) == 16
    orphan = np.eye(40, 24)
    orphan[5, 5] = 0.0                                                 # joint 5 (not a merged one) owns no vertex
    with pytest.raises(ValueError, match="no vertex"):
        coap.partition(rng.rand(40, 3), faces, orphan, np.arange(-1, 23), "smpl")        # a chain: nothing merges into joint 5


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_restatement_matches_r64(golden, model, name):
    c, code = R.case_inputs(name), R.case_code(name)
    got = dict(bone_trans=code["bone_trans"], bbox_min=code["bbox_min"], bbox_max=code["bbox_max"], latent=code["latent"])
    r = R.query(model["weights"], code, c["points"], direction=-c["front"].astype(np.float64))
    got.update(part_occupancy=r["part_occupancy"], occupancy=r["occupancy"])
    for q, v in got.items():
        dev = R.rel_dev(v, golden[f"{name}__r64_{q}"])
        print(f"{name} {q}: {dev:.2e}")
        assert dev <= 1e-10, (q, dev)
    assert R.rel_dev(r["docc"], golden[f"{name}__r64_docc"]) <= 1e-9
    assert np.array_equal(r["inside"].any(0), golden[f"{name}__r64_part_occupancy"].max(0) > 0)
    for i, d in enumerate(R.DISPLACEMENTS):
        t = R.collision(model["weights"], code, c["points"], d, c["front"], R.FILTER_THRESHOLD)
        assert abs(t["loss"] - golden[f"{name}__r64_loss"][i]) <= 1e-10 * abs(golden[f"{name}__r64_loss"][i])
        assert abs(t["dloss"] - golden[f"{name}__r64_dloss"][i]) <= 1e-9 * abs(golden[f"{name}__r64_dloss"][i])
        assert np.array_equal(t["kept"], golden[f"{name}__r64_kept"][i]) and np.array_equal(t["kept"] & t["above"], golden[f"{name}__r64_mask"][i])


def test_restated_trajectory_matches_r64(golden):
    tr, ti = R.TRAJECTORY, R.trajectory_inputs()
    got = R.optimize(R.restated_term(tr["case"], ti["front"]), ti["views"], ti["joints0"], ti["front"], ti["cand_view"], ti["cand_xy"], tr["d0"], tr["lr"],
                     tr["w_multiview"], tr["w_collision"], tr["E"])
    for q in ("traj", "Ctraj", "losses"):
        assert R.rel_dev(got[q], golden[f"trajectory__r64_{q}"]) <= 1e-9, q
    assert golden["e_ref_traj"] > 0 and golden["e_ref_Ctraj"] > 0


def test_loader_round_trip(tmp_path, model):
    from coma_amd import coap
    K = 15
    state = {k: torch.as_tensor(v) for k, v in model["weights"].items()}
    state["k_one_hot"] = torch.eye(K)                                                 # buffers of the reference's module are dropped
    state["partitioner.joint_mapper"] = torch.ones(22, dtype=torch.bool)
    pth = str(tmp_path / "coap.ckpt")
    torch.save({"state_dict": state}, pth)
    for source in (pth, {"state_dict": state}, state):
        got = coap.load_coap_state(source)
        assert sorted(got) == sorted(model["weights"])
        assert all(np.array_equal(got[k], model["weights"][k]) and got[k].dtype == np.float32 for k in got)
    assert sorted(coap.layer_shapes(K)) == sorted(R.layer_shapes(K))
    broken = dict(state)
    del broken["decoder.lin3.bias"]
    with pytest.raises(ValueError, match="lacks decoder.lin3.bias"):
        coap.load_coap_state(broken)
    with pytest.raises(ValueError, match="shape"):
        coap.load_coap_state(state, K=14)
    with pytest.raises(ValueError, match="not a COAP"):
        coap.load_coap_state({"state_dict": {}})


def _unfragment(vec, at, nb, g):
    """The [8 g, 32 nb] matrix of a fragment field."""
    return vec[at:at + nb * g * 256].reshape(nb, g, 2, 32, 4).transpose(1, 2, 4, 0, 3).reshape(8 * g, 32 * nb)


def test_packed_weights_reproduce_the_query(model, hip_lib):
    """The device's algorithm (per-part biases for the one-hot, inside and latent inputs, q beside the hidden layer at the skips,
    1 / sqrt 2 folded into the weights) evaluated in f64 NumPy on the PACKED vector gives the restatement's occupancy."""
    from coma_amd import coap
    K = 15
    for k in (1, 15, 28, 32):
        assert coap.weights_layout(k)["total"] == hip_lib.coma_coap_weights_floats(k), k
    vec = coap.pack_weights(model["weights"], K)
    lay = coap.weights_layout(K)
    assert vec.dtype == np.float32 and len(vec) == lay["total"]
    c, code = R.case_inputs("small"), R.case_code("small")
    want = R.query(model["weights"], code, c["points"][:200])
    f = lambda name: vec[lay[name][0]:lay[name][0] + lay[name][1]].astype(np.float64)
    n1, g2 = 124 - K, (124 - K + 3 + 7) // 8
    shapes = ((8, 1), ((n1 + 31) // 32, 32), (8, g2), (4, 32), (8, 17), (8, 32), (4, 32), (8, 32), (8, 32), (8, 32))
    Wm = [_unfragment(vec.astype(np.float64), lay[f"w_{i}"][0], nb, g) for i, (nb, g) in enumerate(shapes)]
    bias = [f(f"b_{i}") for i in range(10)]
    part_bias = [(f(f"q{i}_b") + f(f"q{i}_in"))[None] + f(f"q{i}_hot").reshape(K, 256) + code["latent"] @ f(f"q{i}_lat").reshape(128, 256) for i in (0, 2)]
    occ = np.zeros((K, 200))
    for k in range(K):
        q = want["local"][k]
        pad = lambda a, n: np.concatenate([a, np.zeros((len(a), n - a.shape[1]))], 1)
        h = R.softplus(pad(q, 8) @ Wm[0] + part_bias[0][k])
        h = R.softplus(h @ Wm[1] + bias[1])[:, :n1]
        h = R.softplus(pad(np.concatenate([h, q], 1), 8 * g2) @ Wm[2] + part_bias[1][k])
        z = h @ Wm[3] + bias[3]
        skip = np.concatenate([q, z], 1)
        h = R.softplus(pad(skip, 136) @ Wm[4] + bias[4])
        h = R.softplus(h @ Wm[5] + bias[5])
        h = R.softplus(h @ Wm[6] + bias[6])[:, :125]
        h = R.softplus(np.concatenate([h, skip], 1) @ Wm[7] + bias[7])
        h = R.softplus(h @ Wm[8] + bias[8])
        h = R.softplus(h @ Wm[9] + bias[9])
        occ[k] = 1.0 / (1.0 + np.exp(h @ f("w6") + f("b6")[0])) * want["inside"][k]
    assert R.rel_dev(occ, want["part_occupancy"]) <= 1e-6          # the 1 / sqrt 2 of the skips is folded in f32


def test_packed_weights_reproduce_the_encoder(model):
    from coma_amd import coap
    K = 15
    vec = coap.pack_weights(model["weights"], K).astype(np.float64)
    lay = coap.weights_layout(K)
    f = lambda name: vec[lay[name][0]:lay[name][0] + lay[name][1]]
    code = R.case_code("small")
    relu = lambda a: np.maximum(a, 0.0)
    x = np.concatenate([code["local_samples"], np.zeros(code["local_samples"].shape[:2] + (5,))], -1)
    net = x @ _unfragment(vec, lay["e_pos_w"][0], 8, 1) + f("e_pos_b")
    for i in range(4):
        g = 32 if i == 0 else 16
        W0, Ws, W1 = (_unfragment(vec, lay[f"{n}_{i}"][0], 4, g if n != "e_fc1" else 16) for n in ("e_fc0", "e_sc", "e_fc1"))
        c0, cs = f(f"e_b0_{i}")[None, None], 0.0
        if i:
            pooled = net.max(1, keepdims=True)
            c0 = c0 + relu(pooled) @ f(f"e_fc0p_{i}").reshape(128, 128)
            cs = pooled @ f(f"e_scp_{i}").reshape(128, 128)
        net = (net @ Ws + cs) + (relu(relu(net) @ W0 + c0) @ W1 + f(f"e_b1_{i}"))
    latent = relu(net.max(1)) @ f("e_fcc_w").reshape(128, 128) + f("e_fcc_b")
    assert R.rel_dev(latent, code["latent"]) <= 1e-12


def test_exports_refuse_bad_arguments_before_any_launch(hip_lib):
    one = C.c_void_p(16)          # never dereferenced: argument validation fails first
    err = lambda: hip_lib.coma_last_error().decode()
    parents, mapper = (C.c_int32 * 22)(*([0] + list(range(21)))), (C.c_uint8 * 22)(*([1] * 15 + [0] * 7))
    front, dfront = (C.c_float * 3)(0.0, 0.0, 1.0), (C.c_double * 3)(0.0, 0.0, 1.0)
    big = 1 << 40

    def encode(weights=one, wn=big, V=100, par=parents, mp=mapper, mK=22, K=15, S=10, n=64, code=one, ws=one, wsn=big):
        return hip_lib.coma_coap_encode_f32(weights, wn, one, one, one, V, par, mp, mK, K, one, S, one, one, n, code, ws, wsn, None)
    assert encode(weights=None) == -1 and "null pointer" in err()
    assert encode(K=0) == -1 and encode(K=33) == -1 and "K=33 outside [1, 32]" in err()
    assert encode(mK=65) == -1 and encode(mK=14) == -1 and "mK" in err()
    assert encode(n=1) == -1 and encode(n=4097) == -1 and "n_samples=4097 outside [2, 4096]" in err()
    assert encode(V=0) == -1 and encode(S=101) == -1 and "S=101" in err()
    assert encode(wn=10) == -1 and "weights of 10 floats" in err()
    bad_parents = (C.c_int32 * 22)(*([0] + list(range(21))))
    bad_parents[5] = 5
    assert encode(par=bad_parents) == -1 and "parents[5]=5" in err()
    assert encode(mp=(C.c_uint8 * 22)(*([1] * 14 + [0] * 8))) == -1 and "selects 14 joints, K=15" in err()
    assert encode(code=C.c_void_p(24)) == -1 and "code block must be 16-byte aligned" in err()
    assert encode(wsn=16) == -1 and "workspace of 16 bytes" in err()
    assert hip_lib.coma_coap_code_bytes(0) == 0 and hip_lib.coma_coap_code_bytes(15) > 15 * 24 * 8
    assert hip_lib.coma_coap_encode_workspace_bytes(15, 1) == 0 and hip_lib.coma_coap_encode_workspace_bytes(15, 1000) >= 15 * 1000 * 128 * 4
    assert hip_lib.coma_coap_query_workspace_bytes(15, 0) == 0 and hip_lib.coma_coap_query_workspace_bytes(33, 5) == 0
    assert hip_lib.coma_coap_query_workspace_bytes(15, (1 << 22) + 1) == 0 and hip_lib.coma_coap_weights_floats(33) == 0
    assert hip_lib.coma_coap_status(None, None) == -1

    def query(weights=one, wn=big, K=15, T=10, d=None, fr=front, deriv=0, occ=one, docc=one, ws=one, wsn=big):
        return hip_lib.coma_coap_query_f32(weights, wn, one, K, one, T, d, fr, deriv, occ, docc, ws, wsn, None)
    assert query(occ=None) == -1 and "null pointer" in err()
    assert query(K=40) == -1 and query(T=0) == -1 and query(T=(1 << 22) + 1) == -1 and "outside" in err()
    assert query(d=one, fr=None) == -1 and query(deriv=1, fr=None) == -1 and "front" in err()
    assert query(deriv=1, fr=(C.c_float * 3)(0.0, float("nan"), 1.0)) == -1 and "front" in err()
    assert query(deriv=1, docc=None) == -1 and "docc" in err()
    assert query(wn=5) == -1 and "weights of 5 floats" in err()
    assert query(weights=C.c_void_p(20)) == -1 and query(d=C.c_void_p(20)) == -1 and "aligned" in err()
    assert query(wsn=8) == -1 and "workspace of 8 bytes" in err()

    def collide(K=15, T=10, fr=front, thr=0.01, result=one, wn=big, wsn=big):
        return hip_lib.coma_coap_collision_f32(one, wn, one, K, one, T, None, fr, thr, result, None, one, wsn, None)
    assert collide(result=None) == -1 and collide(fr=None) == -1 and "null pointer" in err()
    assert collide(K=0) == -1 and collide(T=0) == -1 and "outside" in err()
    assert collide(thr=-0.1) == -1 and collide(thr=1.0) == -1 and collide(thr=float("nan")) == -1 and "filter_threshold" in err()
    assert collide(wn=3) == -1 and "weights of 3 floats" in err()
    assert collide(wsn=0) == -1 and "workspace of 0 bytes" in err()

    def optimise(E=5, N=0, J=25, w_col=0.4, K=15, T=10, traj=one, Ctraj=one, wsn=big, d0=0.0, fr=dfront):
        return hip_lib.coma_depth_optimize_coap_f64(one, big, one, K, one, T, 0.01, one, wsn, None, 0, None, fr, None, None, N, J, d0, 0.01, 1e-3, w_col, E,
                                                    traj, Ctraj, one, one, None)
    assert optimise(traj=None) == -1 and "null pointer" in err()
    assert optimise(E=0) == -1 and optimise(E=4097) == -1 and "E=4097 outside [1, 4096]" in err()
    assert optimise(N=-1) == -1 and optimise(J=0) == -1 and optimise(N=3) == -1 and "null pointer (views" in err()
    assert optimise(d0=float("inf")) == -1 and "finite" in err()
    assert optimise(Ctraj=None) == -1 and "Ctraj is written" in err()
    assert optimise(K=33) == -1 and optimise(T=0) == -1 and optimise(wsn=4) == -1 and "workspace of 4 bytes" in err()


def test_device_coap_builds_without_a_device(model):
    from coma_amd import _lib, coap
    body = dict(v_template=model["v_template"], faces=model["faces"], lbs_weights=model["lbs_weights"], parents=model["parents"])
    m = coap.DeviceCOAP(body, {"state_dict": model["weights"]}, n_samples=64, seed=3)
    assert (m.K, m.mK, m.n_samples) == (15, 22, 64) and m.weights is None and m.code is None and m.device.index is None
    assert len(m.packed) == coap.weights_layout(15)["total"]
    c = R.case_inputs("small")
    ids, bary = coap.draw_samples(np.random.RandomState(7), c["vertices"], m.part, 65)
    want_ids, want_bary = R.draw_samples(np.random.RandomState(7), c["vertices"], model["part"], 65)
    assert ids.shape == (15, 65, 3) and np.array_equal(ids, want_ids) and np.array_equal(bary, want_bary.astype(np.float32))
    tight = {tuple(f) for f in m.part["tight_faces"][4] if f[0] >= 0}
    assert all(tuple(f) in tight for f in ids[4, :32]) and np.allclose(bary.sum(-1), 1.0, atol=1e-6)
    with pytest.raises(_lib.ComaHipError, match="HIP device"):
        coap.DeviceCOAP(body, model["weights"], device="cpu")
    with pytest.raises(_lib.ComaHipError, match="n_samples"):
        coap.DeviceCOAP(body, model["weights"], n_samples=1)
    with pytest.raises(_lib.ComaHipError, match="no encoded body"):
        m.query(np.zeros((1, 3)))


def test_cli_collision_flags():
    from src.generation import optimize_depth as cli
    from src.application import optimize as app
    a = cli.build_parser().parse_args([])
    assert (a.collision, a.coap_ckpt, a.coap_samples, a.coap_seed) == ("columns", None, 1000, 0)
    b = cli.build_parser().parse_args(["--collision", "coap", "--coap_ckpt", "/nowhere/coap.ckpt", "--coap_samples", "64", "--coap_seed", "5"])
    assert (b.collision, b.coap_ckpt, b.coap_samples, b.coap_seed) == ("coap", "/nowhere/coap.ckpt", 64, 5)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--collision", "learned"])
    with pytest.raises(SystemExit, match="does not exist"):
        cli.main(b)
    with pytest.raises(SystemExit, match="needs --coap_ckpt"):
        cli.main(cli.build_parser().parse_args(["--collision", "coap"]))
    assert "coap" in cli.__doc__ and "never been executed" in cli.__doc__
    assert hasattr(app, "build_parser") or hasattr(app, "main")          # --use_collision keeps its refusal: tests/test_app_objective_host.py pins its text
