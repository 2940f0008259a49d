"""GPU: N starts of the fitting app at once (src/application/optimize.py::fit(starts=...), --num_starts) through the three batched
device models and the batched ComaObjective, on case `app` of tests/fit_ref.py (its synthetic body model, decoder fit_ref.DECODER,
fit_ref.WEIGHTS), 5 iterations.

What is pinned is bit-identity, not a tolerance: every library call gives body n the single call's bits, the loss that goes backward
is a sum over starts (each start's gradient is its own) and torch.optim.Adam is element-wise, so start n of a batched run is the run
of start n alone -- parameters after every step, the last forward's vertices, each iteration's loss, and the first iteration's .grad of
all five parameters."""
import json
import pickle
import sys

import numpy as np
import pytest
import torch

from tests import fit_ref as R
from tests import smplx_ref as S
from tests import vposer_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERS, N = 5, 3
PARAMETERS = ("global_orient", "transl", "left_hand_pose", "right_hand_pose")


class _RecordingBody:
    """The device body model with a handle on the parameters fit() builds."""

    def __init__(self, body):
        self.body, self.faces, self.batch_size = body, body.faces, body.batch_size

    def __call__(self, **kw):
        self.kw = kw
        return self.body(**kw)


class _RecordingDecoder:
    def __init__(self, decoder):
        self.decoder = decoder

    def encode(self, pose):
        return self.decoder.encode(pose)

    def decode(self, embedding, output_type="aa"):
        self.embedding = embedding
        return self.decoder.decode(embedding, output_type=output_type)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class Rig:
    """The models of case `app` at one batch size, and fit() on them."""

    def __init__(self, batch_size):
        from coma_amd.app import ComaObjective
        from coma_amd.body_model import DeviceSMPLX
        from coma_amd.pose_prior import DeviceAnglePrior, DeviceVPoser
        model, _, w, n_pca, _, _ = R.case_models("app")
        c = V.case_shape(R.DECODER)
        o = R.golden_objective(*R.load_golden(), "app")
        self.body = _RecordingBody(DeviceSMPLX(model, n_pca=n_pca, device=DEV, extra_joint_vertex_ids=[], batch_size=batch_size))
        self.decoder = _RecordingDecoder(DeviceVPoser(w, c["H"], c["D"], [1, c["NJ"], 3], device=DEV))
        self.prior = DeviceAnglePrior(DEV)
        self.objective = ComaObjective(o["faces"], o["gt"], o["obj_normal"], o["sel"], o["targets"], o["p"], o["sub_p"], o["eps"], device=DEV)

    def fit(self, num_iters, **kw):
        from src.application import optimize as app
        w = R.WEIGHTS
        return app.fit(lambda v: self.objective.loss(v, w["orientation_weight"], w["contact_weight"]), self.body, self.decoder, self.prior, lr=w["lr"],
                       body_pose_weight=w["body_pose_weight"], bending_prior_weight=w["bending_prior_weight"], pprior_weight=w["pprior_weight"],
                       scale_factor=w["scale_factor"], num_iters=num_iters, device=DEV, record=True, **kw)

    def first_gradients(self, **kw):
        """One iteration: the .grad of the five parameters, rows = starts."""
        self.fit(1, **kw)
        grads = {name: self.body.kw[name].grad.detach().cpu().numpy() for name in PARAMETERS}
        grads["embedding"] = self.decoder.embedding.grad.detach().cpu().numpy()
        return grads


@pytest.fixture(scope="module")
def runs():
    """Every run the tests compare, once: the batched one, each start alone, and today's starts=None path; left unchanged."""
    from src.application.optimize import default_starts
    from tests.domain_kit import device_guard
    starts = default_starts(N)
    with device_guard("the fits of the multi-start tests"):
        many, one = Rig(N), Rig(1)
        out = dict(starts=starts, batched=many.fit(ITERS, starts=starts), batched_grads=many.first_gradients(starts=starts),
                   solo=[one.fit(ITERS, starts=starts[n:n + 1]) for n in range(N)],
                   solo_grads=[one.first_gradients(starts=starts[n:n + 1]) for n in range(N)], default=one.fit(ITERS))
    return out


def test_each_start_equals_its_solo_run(runs):
    got = runs["batched"]
    V_ = got["vertices_all"].shape[1]
    assert got["trajectory"].shape == (ITERS + 1, N, 6) and got["vertices_all"].shape == (N, V_, 3) and got["vertices_all"].dtype == np.float32
    assert len(got["losses"]) == ITERS and all(row.shape == (N,) for row in got["losses"]) and got["start_losses"].shape == (N,)
    assert np.array_equal(got["trajectory"][0], np.float32(runs["starts"]).astype(np.float64))            # the parameters are f32
    # the gradients of the first iteration, all five parameters: the library's part
    for name, batched in runs["batched_grads"].items():
        assert batched.shape[0] == N and np.all(np.isfinite(batched)), name
        for n in range(N):
            solo = runs["solo_grads"][n][name]
            ulp = np.max(np.abs(_bits(batched[n]).astype(np.int64) - _bits(solo[0]).astype(np.int64)))
            print(f"{name}, start {n}: max|g| {np.abs(solo).max():.3e}, largest difference {ulp} ulp")
    for name, batched in runs["batched_grads"].items():
        for n in range(N):
            assert np.abs(batched[n]).max() > 0, (name, n)
            assert _equal(batched[n], runs["solo_grads"][n][name][0]), (name, n)
    # ... and what torch's Adam makes of them
    losses = np.stack(got["losses"])
    for n in range(N):
        solo = runs["solo"][n]
        assert solo["trajectory"].shape == (ITERS + 1, 1, 6) and solo["best"] == 0
        rows = np.flatnonzero(np.any(_bits(got["trajectory"][:, n]) != _bits(solo["trajectory"][:, 0]), axis=1))
        print(f"start {n}: trajectory rows that differ from the solo run: {rows.tolist()}")
        assert rows.size == 0, (n, rows)
        assert _equal(got["vertices_all"][n], solo["vertices_all"][0]), n
        assert _equal(losses[:, n], np.stack(solo["losses"])[:, 0]), n
        assert np.all(np.abs(np.diff(got["trajectory"][:, n], axis=0)).max(axis=1) > 0)            # every iteration stepped
    assert not np.array_equal(got["vertices_all"][0], got["vertices_all"][1])                       # other starts, other bodies


def test_the_default_path_is_untouched(runs):
    """Row 0 of default_starts is the reference's start, and its solo run is the starts=None run bit for bit."""
    assert np.array_equal(runs["starts"][0], [0.0, 0.0, 0.0, 3.0, 1.0, 0.0])
    solo, default = runs["solo"][0], runs["default"]
    assert set(default) == {"vertices", "losses", "trajectory"}
    traj = np.asarray(default["trajectory"])
    assert traj.shape == (ITERS + 1, 6) and _equal(traj, solo["trajectory"][:, 0])
    assert default["vertices"].shape == solo["vertices"].shape and _equal(default["vertices"], solo["vertices"])
    assert all(isinstance(x, float) for x in default["losses"])
    assert _equal(np.asarray(default["losses"], dtype=np.float32), np.stack(solo["losses"])[:, 0])


def test_the_best_start_is_returned(runs):
    from src.application.optimize import best_start
    got = runs["batched"]
    losses = got["start_losses"]
    assert np.all(np.isfinite(losses)) and len(np.unique(losses)) == N
    assert got["best"] == best_start(losses) == int(np.argmin(losses))
    assert _equal(got["vertices"], got["vertices_all"][got["best"]])
    assert _equal(losses, got["losses"][-1])                        # the last iteration's forward
    print(f"start losses {losses}, best {got['best']}")


def test_a_body_model_of_another_batch_size_raises_before_any_launch():
    from coma_amd.body_model import DeviceSMPLX
    from src.application.optimize import default_starts, fit
    model, _, _, n_pca, _, _ = R.case_models("app")
    body = DeviceSMPLX(model, n_pca=n_pca, device=DEV, extra_joint_vertex_ids=[], batch_size=2)

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError(f"the pose decoder was asked for .{name}: fit() went past its batch-size check")

    def never(*a):
        raise AssertionError("called")
    with pytest.raises(ValueError, match="3 starts, but the body model was built with batch_size=2"):
        fit(never, body, Untouched(), never, lr=1e-2, body_pose_weight=1.0, bending_prior_weight=1.0, pprior_weight=1.0, scale_factor=1.0,
            num_iters=2, device=DEV, starts=default_starts(3))


def _experiment_dir(path, name):
    c = V.case_shape(name)
    (path / "snapshots").mkdir(parents=True)
    (path / "synthetic.ini").write_text(f"[All]\nnum_neurons : {c['H']}\nlatentD : {c['D']}\ndata_shape : [1, {c['NJ']}, 3]\nuse_cont_repr : True\n")
    torch.save({k: torch.from_numpy(v) for k, v in V.case_weights(name).items()}, path / "snapshots" / "synthetic_E001.pt")


def test_cli_runs_three_starts(tmp_path, monkeypatch):
    """--body_model device --pose_prior device --num_starts 3 on the synthetic model files of test_app_fit_gpu.py's CLI test: the best
    start is optimized.obj, every start has its file, starts.json says which; --loop device with two starts stops with the pinned text."""
    from src.application import optimize as app
    model, fm = S.case_model("moderate")
    (tmp_path / "smplx").mkdir()
    np.savez(tmp_path / "smplx" / "SMPLX_NEUTRAL.npz", **model)
    _experiment_dir(tmp_path / "vposer", "near_rest")
    monkeypatch.setattr(app, "BODY_MOCAP_PATH", str(tmp_path))
    monkeypatch.setattr(app, "VPOSER_PATH", str(tmp_path / "vposer"))
    Vn, O, k = fm["V"], 20, 30
    rng = np.random.default_rng(5)
    unit = lambda n: (lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))
    prob = np.zeros((Vn, O, Vn), np.float32)
    prob[np.arange(Vn), 0, np.arange(Vn)] = 1.0
    nom = np.full((Vn, O), 0.1, np.float32)
    nom[rng.choice(Vn, size=k, replace=False), rng.integers(0, O, size=k)] = 1.0
    state = dict(prob_grid_canon_human_wrt_obj=prob, canon_normal_grid=unit(Vn), contact_dist_expectation_grid_nom=nom,
                 contact_dist_expectation_grid_denom=np.ones((Vn, O), np.float32))
    asset = dict(downsampled_pcd_points_raw=(rng.uniform(-1, 1, size=(O, 3)) + [3.0, 1.0, 0.0]).astype(np.float32), downsampled_pcd_normal_raw=unit(O))
    for pth, obj in ((tmp_path / "coma.pickle", state), (tmp_path / "asset.pickle", asset)):
        with open(pth, "wb") as fh:
            pickle.dump(obj, fh)
    flags = ["--supercategory", "super", "--category", "cat", "--coma_path", str(tmp_path / "coma.pickle"), "--asset_downsample_pth",
             str(tmp_path / "asset.pickle"), "--num_iters", "3", "--body_model", "device", "--pose_prior", "device"]
    for package in ("smplx", "configer", "torchgeometry"):
        monkeypatch.setitem(sys.modules, package, None)
    out = app.main(app.build_parser().parse_args(flags + ["--save_dir", str(tmp_path / "out"), "--num_starts", "3"]))
    directory = tmp_path / "out" / "super" / "cat"
    assert out["path"] == str(directory / "optimized.obj") and out["vertices_all"].shape == (3, Vn, 3) and np.all(np.isfinite(out["vertices_all"]))
    assert sorted(p.name for p in directory.iterdir()) == ["optimized.obj", "optimized_start00.obj", "optimized_start01.obj", "optimized_start02.obj", "starts.json"]
    with open(directory / "starts.json") as fh:
        said = json.load(fh)
    assert said["best"] == out["best"] and np.array_equal(np.float32(said["start_losses"]), out["start_losses"]) and np.array_equal(said["starts"], app.default_starts(3))
    assert (directory / "optimized.obj").read_bytes() == (directory / f"optimized_start{out['best']:02d}.obj").read_bytes()
    from coma_amd.downsample import load_obj
    for n in range(3):
        v, f = load_obj(str(directory / f"optimized_start{n:02d}.obj"))
        assert np.array_equal(f, fm["faces"]) and np.array_equal(v.astype(np.float32), out["vertices_all"][n])
    with pytest.raises(SystemExit) as e:
        app.main(app.build_parser().parse_args(flags + ["--loop", "device", "--num_starts", "2"]))
    assert str(e.value) == app.LOOP_RUNS_ONE_START
