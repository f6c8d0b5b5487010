"""LiveSession ego-motion, the parts that need no GPU: self-checks of the fp64 restatement in tests/live_ego_ref.py (it
recovers the planted camera motion and separates the mover), the fp32 evaluation that sets that module's constants,
degenerate inputs, the trajectory helper, LiveSession / command-line validation and the argument checks of
codd_ego_motion (every call is rejected before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ego_ref as le  # noqa: E402

from codd_amd import _abi  # noqa: E402

EINVAL = -1  # CODD_EINVAL
case_id = lambda s: "%dx%d" % s[0]  # noqa: E731
_CACHE = {}
# what the reference recovers at the defaults, per crop height: (static pixels' residual <=, movers' residual >=) in pixels
RESIDUALS = {37: (0.08, 4.1), 40: (0.35, 23.0), 128: (0.25, 13.7)}


def _case(shape, mover):
    """(scene, its fp64 reference), computed once and never modified."""
    key = (shape[0], mover)
    if key not in _CACHE:
        s = le.scene(shape, mover)
        _CACHE[key] = (s, le.reference(s["T"], s["depth"], s["K"], s["crop"], scale=le.SCALE))
    return _CACHE[key]


@pytest.mark.parametrize("mover", (False, True), ids=("static", "mover"))
@pytest.mark.parametrize("shape", le.CASES, ids=case_id)
def test_reference_recovers_the_planted_motion(shape, mover):
    s, ref = _case(shape, mover)
    (h, w), G = s["crop"], ref["G"]
    assert ref["ok"] and ref["steps"] == 5 and ref["n_valid"] == h * w - 6  # the six planted invalid pixels
    dt, dq = float((G[:3] - s["G"][:3]).norm()), le.rotation_angle(G[3:], s["G"][3:])
    print(f"{h}x{w} mover={mover}: |dt| {dt:.3g}, angle {dq:.3g} rad")
    assert dt <= (7e-4 if mover else 1e-5) and dq <= (8.5e-4 if mover else 2.1e-5)
    res, valid = ref["residual"], ref["valid"]
    static_max, mover_min = RESIDUALS[h]
    assert float(res[valid & ~s["mover"]].max()) <= static_max
    assert bool((ref["moving"][valid & ~s["mover"]] == 0).all())
    if mover:
        share = float(s["mover"].sum()) / (h * w)
        assert 0.2 < share < 0.3
        assert float(res[valid & s["mover"]].min()) >= mover_min
        assert bool((ref["moving"][valid & s["mover"]] == 1).all())
    assert bool((ref["moving"][~valid] == 255).all()) and bool(torch.isnan(res[~valid]).all())
    # no pixel sits anywhere near a threshold
    assert not bool(ref["und_valid"].any()) and not bool(ref["und_mask"].any())


@pytest.mark.parametrize("mover", (False, True), ids=("static", "mover"))
@pytest.mark.parametrize("shape", le.CASES, ids=case_id)
def test_fp32_evaluation_within_a_quarter_of_every_bound(shape, mover):
    """Re-measures MEASURED: per-pixel fp32 terms with fp64 sums stay within C / 4 of the fp64 reference."""
    s, ref = _case(shape, mover)
    rec, moving, residual = le.evaluate32(s["T"], s["depth"], s["K"], s["crop"], scale=le.SCALE)
    res = le.compare(rec, moving, residual, ref, f"fp32 evaluation {case_id(shape)}")
    print(res)
    le.within(res, 0.25, case_id(shape))
    for k, v in le.MEASURED.items():
        assert res[k] <= v * 1.005, (k, res[k])  # (MEASURED is the worst over the cases)
    # fp32 and fp64 agree on validity and on the mask, and nearly on the residual
    assert torch.equal(moving, ref["moving"])
    assert float((residual.double() - ref["residual"])[ref["valid"]].abs().max()) <= 6.3e-5
    assert float((rec[3:7].double() - ref["G"][3:]).abs().max()) <= 1e-7
    assert float((rec[:3].double() - le.SCALE * ref["G"][:3]).abs().max()) <= 1e-7
    assert int(rec[8]) == ref["n_valid"] and int(rec[7]) == 1 and int(rec[11]) == 5


def test_constants_are_four_times_the_measurement():
    for k, v in le.MEASURED.items():
        assert 4 * v <= le.C[k] < 4 * v * 1.06, k  # rounded UP to two digits
    assert le.C["induced_flow"] == le.lm.C["induced_flow"] and le.C["sceneflow"] == le.lm.C["sceneflow"]


def test_padding_never_reaches_the_reference():
    s, ref = _case(le.CASES[0], True)
    (h, w), T, depth = s["crop"], s["T"].clone(), s["depth"].clone()
    T[0, h:], T[0, :, w:], depth[0, h:], depth[0, :, w:] = 0.25, 0.25, 7.0, 7.0
    again = le.reference(T, depth, s["K"], s["crop"], scale=le.SCALE)
    assert torch.equal(again["G"], ref["G"]) and torch.equal(again["moving"], ref["moving"])


def test_one_iteration_is_the_l2_step():
    """iters=1 is one plain weighted least-squares step from identity: the mover drags it away from the camera."""
    s, ref = _case(le.CASES[0], True)
    one = le.reference(s["T"], s["depth"], s["K"], s["crop"], scale=le.SCALE, iters=1)
    assert one["ok"] and one["steps"] == 1
    assert float((one["G"][:3] - s["G"][:3]).norm()) > 10 * float((ref["G"][:3] - s["G"][:3]).norm())


@pytest.mark.parametrize("kind", ("all_invalid", "few_valid", "one_ray"))
def test_degenerate_inputs_stop_at_identity(kind):
    s = le.degenerate(kind)
    ref = le.reference(s["T"], s["depth"], s["K"], s["crop"])
    rec, moving, residual = le.evaluate32(s["T"], s["depth"], s["K"], s["crop"])
    identity = torch.tensor([0.0, 0, 0, 0, 0, 0, 1], dtype=torch.float64)
    assert not ref["ok"] and ref["steps"] == 0 and torch.equal(ref["G"], identity) and ref["n_valid"] == s["valid"]
    assert torch.equal(rec[:8], torch.tensor([0.0, 0, 0, 0, 0, 0, 1, 0])) and bool(torch.isfinite(rec).all())
    assert int(rec[8]) == s["valid"] and int(rec[11]) == 0
    # the field is identity: every valid pixel is static under the identity pose
    assert int((moving == 0).sum()) == s["valid"] and int((moving == 255).sum()) == moving.numel() - s["valid"]
    le.compare(rec, moving, residual, ref, kind)
    if kind == "one_ray":  # enough pixels, and still singular: the pivot test is what stops it
        X0, _, valid = le._geometry(s["T"], s["depth"], s["K"], s["crop"], torch.float64)
        Y = X0[valid]
        Hm, _ = le._normal_equations64(Y, torch.zeros_like(Y), 1 / Y[:, 2] ** 2)
        d = le.pivots(Hm)
        assert s["valid"] >= 16 and not bool((d > le.PIVOT * float(Hm.trace())).all())
    # one more valid pixel than "few_valid" and the fit runs
    if kind == "few_valid":
        depth = s["depth"].clone()
        depth[0, 11, 29] = 2.0
        assert le.reference(s["T"], depth, s["K"], s["crop"])["ok"]


def test_trajectory_helper():
    from codd_amd import live
    from oracle import se3
    G = se3.exp(torch.tensor(le.G_TWIST, dtype=torch.float64))
    Gi = se3.exp(-torch.tensor(le.G_TWIST, dtype=torch.float64))
    M = live.pose_matrix(G.numpy())
    # the matrix acts like the pose
    X = torch.tensor([0.3, -1.2, 2.5], dtype=torch.float64)
    assert np.allclose(M[:3, :3] @ X.numpy() + M[:3, 3], se3.act(G, X).numpy(), rtol=0, atol=1e-15)
    W0 = live.trajectory_step(np.eye(4), None)
    assert np.array_equal(W0, np.eye(4))
    W1 = live.trajectory_step(W0, G.numpy())
    assert np.allclose(W1 @ M, np.eye(4), rtol=0, atol=1e-15)  # W_t = W_{t-1} G^-1
    W2 = live.trajectory_step(W1, Gi.numpy())  # composing G and then G^-1 returns to identity
    assert np.allclose(W2, np.eye(4), rtol=0, atol=1e-15)
    assert np.array_equal(live.trajectory_step(W1, Gi.numpy(), ok=False), W1)  # a degenerate fit carries W forward
    assert np.array_equal(live.trajectory_step(W1, None), np.eye(4))  # a frame without a field restarts it


def test_session_validates_the_egomotion_argument():
    from codd_amd import configs, live
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd()).eval()  # on the CPU
    stereo = build_estimator(configs.stereo_only()).eval()
    assert live.LiveSession(est, (40, 50)).ego is None and live.LiveSession(stereo, (40, 50), egomotion=False).ego is None
    for bad in ("yes", 1, dict(iters=0), dict(iters=33), dict(iters=2.5), dict(delta_px=0.0), dict(tau_px=-1.0),
                dict(tau_px=float("nan")), dict(unknown=1)):
        with pytest.raises(ValueError):
            live.LiveSession(est, (40, 50), egomotion=bad)
    for good in (True, dict(iters=3)):
        with pytest.raises(ValueError):
            live.LiveSession(stereo, (40, 50), egomotion=good)  # no motion stage: refused before the device is touched
    s = live.LiveSession(est, (40, 50), egomotion=True, intrinsics=(500.0, 500.0, 25.0, 20.0), calib=100.0)
    assert s.ego == live.EGO_DEFAULTS == le.DEFAULTS and s.motion is None and not s._open_done and s.pending() == 0
    assert s._K == [500.0, 500.0, 25.0, 20.0] and s._bf == le.lm.bf_of(500.0)
    s = live.LiveSession(est, (40, 50), motion="flow2d", egomotion=dict(iters=3, tau_px=1.5))
    assert s.ego == dict(iters=3, delta_px=1.0, tau_px=1.5, min_valid=16) and s.motion == "flow2d"
    assert live.Ego._fields == ("pose", "ok", "valid", "inliers", "rms_px", "moving", "residual", "camera_to_world")


def test_cli_accepts_ego_only_with_live():
    from codd_amd import inference
    assert inference.parse_args(["--live"]).ego is False
    assert inference.parse_args(["--live", "--ego"]).ego is True
    assert inference.parse_args(["--live", "--ego", "--motion", "flow2d"]).motion == "flow2d"
    with pytest.raises(SystemExit):
        inference.parse_args(["--ego"])


def test_ego_motion_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    lib = _abi.load()
    assert "codd_ego_motion" in _abi.SIGNATURES and "codd_ego_motion_scratch" in _abi.SIGNATURES
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = buf.ctypes.data_as(C.c_void_p)
    need = lib.codd_ego_motion_scratch(40, 50)

    def call(T=p, depth=p, H=64, W=64, h=40, w=50, fx=70.0, fy=70.0, iters=5, delta=1.0, tau=2.0, scratch=p, nbytes=need,
             record=p, moving=p, residual=p):
        return lib.codd_ego_motion(T, depth, H, W, h, w, fx, fy, 32.0, 32.0, 1.0, iters, delta, tau, 16, scratch, nbytes,
                                   record, moving, residual, None)

    for name in ("T", "depth", "scratch", "record", "moving"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("H", "W", "h", "w"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL, name
    assert call(h=65) == EINVAL and call(w=65) == EINVAL  # the crop exceeds the padded grid
    for iters in (0, -1, 33):
        assert call(iters=iters) == EINVAL
    for name in ("fx", "fy", "delta", "tau"):
        for bad in (0.0, -1.0, float("nan")):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    assert call(nbytes=need - 1) == EINVAL and call(nbytes=0) == EINVAL


def test_ego_motion_scratch_is_positive_and_monotone():
    lib = _abi.load()
    sizes = [lib.codd_ego_motion_scratch(h, w) for h, w in ((1, 1), (37, 53), (40, 301), (128, 192), (540, 960))]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.codd_ego_motion_scratch(54, 960) == lib.codd_ego_motion_scratch(540, 96)  # a function of h * w
    assert lib.codd_ego_motion_scratch(0, 5) < 0 and lib.codd_ego_motion_scratch(5, -1) < 0
    for h, w in ((1, 1), (37, 53), (540, 960)):  # the layout is part of the contract: rows, states, ticket; X1 behind them
        assert lib.codd_ego_motion_scratch(h, w) == 82208 + 12 * h * w


def test_run_live_streams_the_ego_file(tmp_path, monkeypatch):
    """--live --ego --show with a stand-in session: frame 0 (no field) is NaN / 255, the others as returned; with
    --motion the tuple is taken apart in the order result, motion, ego."""
    from PIL import Image
    from codd_amd import inference, live
    h, w, n = 6, 10, 4
    for side in ("l", "r"):
        os.makedirs(tmp_path / side)
        for i in range(n):
            Image.fromarray(np.full((h, w, 3), 10 * i + (100 if side == "r" else 0), np.uint8)).save(tmp_path / side / f"{i}.png")

    class Session:  # push / pop / pending / reset / close of LiveSession
        def __init__(self, model, shape, motion=None, egomotion=False, **kw):
            self.motion, self.ego, self.q, self.frames = motion, egomotion, [], 0

        def pending(self):
            return len(self.q)

        def push(self, left, right):
            i = self.frames
            out = [left[..., 0].astype(np.float32)]
            if self.motion is not None:
                out.append(None if i == 0 else np.full((h, w, 3), float(i), np.float32))
            if self.ego:
                pose = np.array([i, 0, 0, 0, 0, 0, 1], np.float32)
                out.append(None if i == 0 else live.Ego(pose, i != 2, 50 + i, 40 + i, 0.5 * i, np.full((h, w), i, np.uint8),
                                                        np.zeros((h, w), np.float32), np.eye(4) * i))
            self.q.append(out[0] if len(out) == 1 else tuple(out))
            self.frames += 1

        def pop(self):
            return self.q.pop(0)

        def reset(self):
            self.frames = 0

        def close(self):
            pass

    monkeypatch.setattr(live, "LiveSession", Session)
    videos = inference.list_videos(str(tmp_path / "l"), str(tmp_path / "r"), ".png")
    base = ["--img-dir", str(tmp_path / "l"), "--r-img-dir", str(tmp_path / "r"), "--live", "--show"]
    inference.run_live(inference.parse_args(base + ["--show-dir", str(tmp_path / "a")]), None, videos)
    inference.run_live(inference.parse_args(base + ["--show-dir", str(tmp_path / "b"), "--ego"]), None, videos)
    inference.run_live(inference.parse_args(base + ["--show-dir", str(tmp_path / "c"), "--ego", "--motion", "sceneflow"]), None, videos)
    assert sorted(os.listdir(tmp_path / "a")) == ["l.disp.pred.npz"]
    assert sorted(os.listdir(tmp_path / "b")) == ["l.disp.pred.npz", "l.ego.pred.npz"]
    assert sorted(os.listdir(tmp_path / "c")) == ["l.disp.pred.npz", "l.ego.pred.npz", "l.motion.pred.npz"]
    a = np.load(tmp_path / "a" / "l.disp.pred.npz")["disp"]
    for d in ("b", "c"):
        assert np.array_equal(np.load(tmp_path / d / "l.disp.pred.npz")["disp"], a)
        z = np.load(tmp_path / d / "l.ego.pred.npz")
        assert sorted(z.files) == ["camera_to_world", "moving", "pose", "stats"]
        pose, stats, world, moving = z["pose"], z["stats"], z["camera_to_world"], z["moving"]
        assert pose.shape == (1, n, 7) and pose.dtype == np.float32 and stats.shape == (1, n, 4)
        assert world.shape == (1, n, 4, 4) and world.dtype == np.float64
        assert moving.shape == (1, n, h, w) and moving.dtype == np.uint8
        assert np.isnan(pose[0, 0]).all() and np.isnan(stats[0, 0]).all() and np.isnan(world[0, 0]).all()
        assert (moving[0, 0] == 255).all()
        for i in range(1, n):
            assert pose[0, i, 0] == i and (moving[0, i] == i).all() and np.array_equal(world[0, i], np.eye(4) * i)
            assert stats[0, i].tolist() == [float(i != 2), 50.0 + i, 40.0 + i, 0.5 * i]
    m = np.load(tmp_path / "c" / "l.motion.pred.npz")["motion"]
    assert np.isnan(m[0, 0]).all() and (m[0, 3] == 3.0).all()
    # without --show nothing is written and the tuples are still taken apart
    inference.run_live(inference.parse_args(base[:-1] + ["--show-dir", str(tmp_path / "d"), "--ego"]), None, videos)
    assert not os.path.exists(tmp_path / "d")
