"""CPU: the multi-start surface of src/application/optimize.py -- default_starts, --num_starts, the best-start policy, fit()'s
batch-size check -- and the refusals of coma_app_objective_batch_f32 (argument checks return before any launch)."""
import numpy as np
import pytest

from src.application import optimize as app


def test_default_starts():
    for N in (1, 2, 3, 8, 64):
        rows = app.default_starts(N)
        assert rows.shape == (N, 6) and rows.dtype == np.float64
        assert np.array_equal(rows[0], [0.0, 0.0, 0.0, 3.0, 1.0, 0.0])                       # the reference's start
        assert np.array_equal(rows[:, [0, 2]], np.zeros((N, 2))) and np.array_equal(rows[:, 3:], np.tile([3.0, 1.0, 0.0], (N, 1)))
        assert np.array_equal(rows[:, 1], 2.0 * np.pi * np.arange(N) / N)
    assert app.default_starts(4)[2, 1] == np.pi and len(np.unique(app.default_starts(64)[:, 1])) == 64
    for bad in (0, -1):
        with pytest.raises(ValueError, match="must be positive"):
            app.default_starts(bad)
    assert "reference" in app.default_starts.__doc__ and "THIS project" in app.default_starts.__doc__


FLAGS = ["--supercategory", "s", "--category", "c", "--coma_path", "a.pickle", "--asset_downsample_pth", "b.pickle"]


def test_num_starts_is_absent_unless_given():
    parse = app.build_parser().parse_args
    assert "num_starts" not in vars(parse([])) and app.num_starts_choice(parse([])) == 1
    given = vars(parse(FLAGS + ["--num_starts", "5"]))
    assert given.pop("num_starts") == 5 and given == vars(parse(FLAGS))
    assert app.num_starts_choice(parse(["--num_starts", "7"])) == 7
    with pytest.raises(SystemExit):
        parse(["--num_starts", "two"])


@pytest.mark.parametrize("value", ("0", "65", "-3"))
def test_num_starts_out_of_range_is_refused_up_front(value, monkeypatch):
    touched = []
    for name in ("device_body_model", "device_pose_prior", "optimize_smpl", "default_body_model"):
        monkeypatch.setattr(app, name, lambda *a, _n=name, **k: touched.append(_n))
    args = app.build_parser().parse_args(FLAGS + ["--body_model", "device", "--pose_prior", "device", "--num_starts", value])
    with pytest.raises(SystemExit) as e:
        app.main(args)
    assert str(e.value) == app.NUM_STARTS_RANGE and "[1, 64]" in app.NUM_STARTS_RANGE and not touched
    from coma_amd import pose_prior
    assert app.MAX_STARTS == pose_prior.MAX_BATCH


def test_loop_device_runs_one_start(monkeypatch):
    touched, optimize_smpl = [], app.optimize_smpl
    for name in ("device_body_model", "device_pose_prior", "optimize_smpl"):
        monkeypatch.setattr(app, name, lambda *a, _n=name, **k: touched.append(_n))
    args = app.build_parser().parse_args(FLAGS + ["--loop", "device", "--num_starts", "2"])
    with pytest.raises(SystemExit) as e:
        app.main(args)
    assert str(e.value) == app.LOOP_RUNS_ONE_START and not touched
    with pytest.raises(ValueError) as e:
        optimize_smpl("s", "c", {}, {}, 1e-6, [0, 0, 1], [0, 1, 0], 0, 1e-2, 1.0, 1.0, 1.0, 1.0, 1.0, 0.3, 1.0, False, loop="device", num_starts=2)
    assert str(e.value) == app.LOOP_RUNS_ONE_START


def test_main_builds_the_body_model_for_the_starts(monkeypatch):
    seen = {}
    monkeypatch.setattr(app, "device_body_model", lambda **kw: seen.setdefault("body", kw) and "body")
    monkeypatch.setattr(app, "device_pose_prior", lambda: ("decoder", "prior"))
    monkeypatch.setattr(app, "optimize_smpl", lambda **kw: seen.setdefault("call", kw))
    app.main(app.build_parser().parse_args(FLAGS + ["--body_model", "device", "--pose_prior", "device", "--num_starts", "4"]))
    assert seen["body"] == dict(batch_size=4) and seen["call"]["num_starts"] == 4 and "loop" not in seen["call"]
    seen.clear()
    monkeypatch.setattr(app, "device_body_model", lambda **kw: seen.setdefault("body", kw or {"none": True}) and "body")
    app.main(app.build_parser().parse_args(FLAGS + ["--body_model", "device", "--pose_prior", "device"]))
    assert seen["body"] == {"none": True} and "num_starts" not in seen["call"]              # one start: today's calls, argument for argument


def test_best_start_policy():
    nan, inf = float("nan"), float("inf")
    assert app.best_start([3.0, 1.0, 2.0]) == 1
    assert app.best_start([2.0, 1.0, 1.0, 5.0]) == 1                                         # the first of equal losses
    assert app.best_start([nan, 4.0, 3.0]) == 2 and app.best_start([1.0, nan]) == 0
    assert app.best_start([nan, -inf, inf, 7.0]) == 3                                        # an infinite loss is no result either
    assert app.best_start(np.float32([5.0])) == 0 and isinstance(app.best_start(np.float32([5.0, 4.0])), int)
    with pytest.raises(FloatingPointError, match=r"none of the 3 starts .* start 0: nan, start 1: inf, start 2: nan"):
        app.best_start([nan, inf, nan])


class _Body:
    def __init__(self, batch_size=None):
        if batch_size is not None:
            self.batch_size = batch_size

    def __call__(self, **kw):
        raise AssertionError("the body model was called")


class _Untouched:
    def __getattr__(self, name):
        raise AssertionError(f"the pose decoder was asked for .{name}")


def _fit(body, starts, decoder=None):
    never = lambda *a: (_ for _ in ()).throw(AssertionError("called"))
    return app.fit(never, body, decoder or _Untouched(), never, lr=1e-2, body_pose_weight=1.0, bending_prior_weight=1.0, pprior_weight=1.0,
                   scale_factor=1.0, num_iters=2, device="cpu", starts=starts)


def test_fit_checks_the_batch_size_before_anything_runs():
    with pytest.raises(ValueError, match="3 starts, but the body model was built with batch_size=1"):
        _fit(_Body(1), app.default_starts(3))
    with pytest.raises(ValueError, match="1 starts, but the body model was built with batch_size=2"):
        _fit(_Body(2), app.default_starts(3)[:1])
    for bad in (np.zeros(6), np.zeros((2, 5)), np.zeros((0, 6))):
        with pytest.raises(ValueError, match=r"starts must be \[N,6\]"):
            _fit(_Body(2), bad)
    # a matching batch size, and a hook without the attribute (a third-party model), pass the check: the decoder is reached
    for body in (_Body(3), _Body()):
        with pytest.raises(AssertionError, match="pose decoder was asked for .encode"):
            _fit(body, app.default_starts(3))


def test_batched_objective_refusals(hip_lib):
    from tests import app_batch_ref as AB
    from tests import domain_kit as K
    table = AB.refusal_table(hip_lib)
    assert K.check_refusals(hip_lib, table, K.host_resolver(AB.HOST_ARGS), expect_control=False) == 30
    size = hip_lib.coma_app_objective_batch_workspace_bytes
    assert size(145, 242, 20, 0) == size(145, 242, 20, 1025) == size(145, 242, 146, 3) == size(0, 242, 0, 3) == 0
    for V, F, k in ((145, 242, 20), (10475, 20908, 1000), (10475, 20908, 0)):
        assert size(V, F, k, 1) == hip_lib.coma_app_objective_workspace_bytes(V, F, k) > 0
