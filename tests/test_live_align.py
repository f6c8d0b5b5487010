"""Depth registered to another camera without a GPU: every call codd_align_depth rejects before a launch, AlignTarget
(validation, files, the rig's own cameras against StereoCalibration), fold_radius2, auto_footprint, the validation of
LiveSession(align_to=, align=) and of the command line, and the restatements of tests/live_align_ref.py: the exact plants
against the brute-force reference, the measured deviation of the fp32 operation order that sets DELTA, and the share of
target pixels the reference alone leaves ambiguous on the inputs the GPU test uses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_align_ref as la  # noqa: E402
import live_calib_ref as cr  # noqa: E402

from codd_amd import calibration as cal  # noqa: E402

# ---- calls rejected before any launch (the library loads without a GPU) ---------------------------------------------
P = 0x1000  # a dummy non-NULL pointer: nothing below reaches a launch
EINVAL = -1


def _view(**over):
    from codd_amd import _abi
    s = _abi.AlignView()
    s.R[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    s.T[:] = [0.1, 0, 0]
    s.K[:] = [60, 60, 30, 20]
    s.dist[:] = [0] * 8
    s.r2_max, s.model = 1e6, 0
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(s, k)[v[0]] = v[1]
        else:
            setattr(s, k, v)
    return s


def _call(disp=P, H=64, W=64, h=37, w=53, f=48.0, cx=26.0, cy=18.0, calib=5.0, view=True, ht=40, wt=60, footprint=1,
          depth_out=P, uv_out=P, **over):
    from codd_amd import _abi
    v = C.byref(_view(**over)) if view else None
    return _abi.load().codd_align_depth(disp, H, W, h, w, f, cx, cy, calib, v, ht, wt, footprint, depth_out, uv_out, None)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw", [
    dict(disp=None), dict(view=False), dict(depth_out=None),
    dict(h=0), dict(w=0), dict(h=-1), dict(H=0, h=0), dict(W=0), dict(ht=0), dict(wt=-3), dict(h=65), dict(w=65),
    dict(f=0.0), dict(f=-1.0), dict(f=NAN), dict(calib=0.0), dict(calib=-2.0), dict(calib=NAN),
    dict(model=2), dict(model=-1),
    dict(R=(4, NAN)), dict(T=(2, INF)), dict(K=(2, NAN)), dict(dist=(7, -INF)), dict(r2_max=NAN), dict(r2_max=INF),
    dict(K=(0, 0.0)), dict(K=(1, -60.0)), dict(r2_max=0.0), dict(r2_max=-1.0),
    dict(footprint=0), dict(footprint=5), dict(footprint=-1),
    dict(H=1 << 16, W=1 << 15, h=1 << 16, w=1 << 15), dict(ht=1 << 16, wt=1 << 15),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_calls_are_rejected(kw):
    assert _call(**kw) == EINVAL


def test_header_names_the_limits():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_hip.h")).read()
    from codd_amd import ops
    assert "#define CODD_ALIGN_MAX_FOOTPRINT 4" in header and ops.ALIGN_MAX_FOOTPRINT == cal.MAX_FOOTPRINT == 4


# ---- AlignTarget ------------------------------------------------------------------------------------------------------
def _camera(model="brown", size=(40, 60)):
    return la.as_camera(la.make_target(model, size, 50.0))


def test_align_target_validation():
    cam = _camera()
    t = cal.AlignTarget(cam)
    assert np.array_equal(t.R, np.eye(3)) and np.array_equal(t.T, np.zeros(3)) and not t.rectified
    for kw in (dict(camera="cam"), dict(R=np.eye(3) * 2), dict(R=np.diag([1.0, 1.0, -1.0])), dict(R=[[1, 0], [0, 1]]),
               dict(T=[0, 0]), dict(T=[0, NAN, 0]), dict(T="abc")):
        with pytest.raises(ValueError):
            cal.AlignTarget(**dict(dict(camera=cam, R=np.eye(3), T=np.zeros(3)), **kw))
    with pytest.raises(ValueError, match="calibration"):
        cal.AlignTarget.resolve("left", None)
    with pytest.raises(ValueError, match="align_to"):
        cal.AlignTarget.resolve(3.5)
    with pytest.raises(ValueError, match="json or .npz"):
        cal.AlignTarget.resolve("target.txt")
    assert cal.AlignTarget.resolve(t) is t


@pytest.mark.parametrize("ext", (".json", ".npz"))
@pytest.mark.parametrize("model", ("brown", "fisheye"))
def test_align_target_file_round_trip(tmp_path, ext, model):
    t = cal.AlignTarget(_camera(model), cr.rot(la.OM), la.T)
    path = tmp_path / ("target" + ext)
    t.save(path)
    back = cal.AlignTarget.load(path)
    assert back == t and back.camera.size == (40, 60) and back.camera.model == model
    assert cal.AlignTarget.resolve(str(path)) == t
    d = t.to_dict()
    assert sorted(d) == ["R", "T", "camera", "rectified", "size"] and cal.AlignTarget.from_dict(d) == t
    with pytest.raises(ValueError, match="missing"):
        cal.AlignTarget.from_dict({k: v for k, v in d.items() if k != "R"})
    with pytest.raises(ValueError, match="json or .npz"):
        t.save(tmp_path / "target.yaml")


def _rig(model="brown", size=(40, 60)):
    (Kl, dl), (Kr, dr), R, T = cr.make_rig(model, size)
    n = 8 if model == "brown" else 4
    return cal.StereoCalibration(cal.CameraModel(size, Kl, model, dl[:n]), cal.CameraModel(size, Kr, model, dr[:n]), R, T)


@pytest.mark.parametrize("model", ("brown", "fisheye"))
def test_of_rig_against_the_stereo_calibration(model):
    """A point seen at rectified pixel (u, v) with disparity d is seen by the rectified RIGHT camera at (u - d, v): the
    physical right camera sees it where source_points(1, u - d, v) says, and of_rig("right") must project it there; the
    left one at source_points(0, u, v) whatever d is.  And of_rig agrees with the calibration's own R, T."""
    sc = _rig(model)
    rect = sc.rectify()
    f, _, cx, cy = rect.intrinsics
    rng = np.random.default_rng(3)
    u, v, d = rng.uniform(5, 55, 200), rng.uniform(5, 35, 200), rng.uniform(0.5, 9.0, 200)
    Z = rect.calib / d
    X = np.stack([(u - cx) / f * Z, (v - cy) / f * Z, Z])
    for side, view, ur in (("left", 0, u), ("right", 1, u - d)):
        t = cal.AlignTarget.of_rig(rect, side)
        assert t.rectified and t.camera is rect.views[view].camera
        R, T = t.pose_from(rect)  # (rectified: its own pose, no second R1^T)
        Xt = R @ X + T[:, None]
        sx, sy = t.camera.distort(Xt[0] / Xt[2], Xt[1] / Xt[2])
        wx, wy = rect.source_points(view, ur, v)
        assert np.abs(sx - wx).max() < 1e-9 and np.abs(sy - wy).max() < 1e-9
    # the physical right camera from the physical left one is the calibration itself
    right = cal.AlignTarget.of_rig(rect, "right")
    assert np.abs(right.R @ rect.R1 - sc.R).max() < 1e-12 and np.abs(right.T - sc.T).max() < 1e-12
    # a target given from the physical left camera is taken through R1^T
    t = cal.AlignTarget(sc.right, sc.R, sc.T)
    R, T = t.pose_from(rect)
    assert np.abs(R - right.R).max() < 1e-12 and np.abs(T - right.T).max() < 1e-12
    R, T = t.pose_from(None)
    assert np.array_equal(R, sc.R)
    with pytest.raises(ValueError):
        cal.AlignTarget.of_rig(rect, "middle")
    with pytest.raises(ValueError):
        cal.AlignTarget.of_rig(sc, "left")


def test_align_view_struct():
    from codd_amd import ops
    sc = _rig()
    rect = sc.rectify()
    t = cal.AlignTarget(sc.right, sc.R, sc.T)
    s = ops.align_view(t, rect)
    assert np.abs(np.array(s.R[:]).reshape(3, 3) - sc.R @ rect.R1.T).max() < 1e-15 and list(s.T) == list(sc.T)
    assert tuple(s.K) == sc.right.K and tuple(s.dist) == sc.right.dist8 and s.model == 0
    assert s.r2_max == cal.fold_radius2(sc.right)
    assert list(ops.align_view(t).R) == list(sc.R.reshape(-1))


def test_fold_radius2():
    """rd = r (1 + k1 r^2) with k1 < 0 peaks at r^2 = 1 / (3 |k1|); beyond it the polynomial folds back."""
    for k1 in (-0.3, -0.05):
        cam = cal.CameraModel((40, 60), (50, 50, 30, 20), "brown", (k1, 0, 0, 0))
        r2 = cal.fold_radius2(cam)
        peak = 1 / (3 * abs(k1))
        assert 0.98 * peak <= r2 <= 1.02 * peak
        # a point beyond the fold lands nearer the centre than the fold itself: what r2_max keeps out
        far, edge = 1.5 * np.sqrt(peak), np.sqrt(r2)
        assert abs(cam.distort(far, 0.0)[0] - 30) < abs(cam.distort(edge, 0.0)[0] - 30)
    assert cal.fold_radius2(cal.CameraModel((40, 60), (50, 50, 30, 20))) == cal.R2_CAP
    assert cal.fold_radius2(cal.CameraModel((40, 60), (50, 50, 30, 20), "fisheye", (0.01, 0, 0, 0))) == cal.R2_CAP
    th = np.sqrt(1 / (3 * 0.2))  # theta_d = theta (1 - 0.2 theta^2) peaks there
    r2 = cal.fold_radius2(cal.CameraModel((40, 60), (50, 50, 30, 20), "fisheye", (-0.2, 0, 0, 0)))
    assert 0.97 * np.tan(th) ** 2 <= r2 <= 1.03 * np.tan(th) ** 2
    assert np.isfinite(cal.R2_CAP) and np.isfinite(np.float32(cal.R2_CAP))


def test_auto_footprint():
    plain = cal.CameraModel((40, 60), (50, 50, 29.5, 19.5))
    K = (50, 50, 29.5, 19.5)
    assert cal.auto_footprint(np.eye(3), plain, (40, 60), K) == 1  # an identity target
    assert cal.auto_footprint(np.eye(3), cal.CameraModel((80, 120), (100, 100, 59.5, 39.5)), (40, 60), K) == 2
    assert cal.auto_footprint(np.eye(3), cal.CameraModel((80, 120), (100.2, 100.2, 59.5, 39.5)), (40, 60), K) == 3
    assert cal.auto_footprint(np.eye(3), cal.CameraModel((20, 30), (25, 25, 14.5, 9.5)), (40, 60), K) == 1
    assert cal.auto_footprint(np.eye(3), cal.CameraModel((400, 600), (500, 500, 300, 200)), (40, 60), K) == 4  # clamped
    assert cal.auto_footprint(np.diag([-1.0, 1.0, -1.0]), plain, (40, 60), K) == 1  # everything behind the target


# ---- LiveSession(align_to=, align=) and the command line: no device call ------------------------------------------------
class NoDevice:  # an estimator stand-in that fails on any use
    def __getattr__(self, name):
        raise AssertionError(f"the estimator was touched ({name}) before the option was validated")


def test_session_argument_validation(tmp_path):
    from codd_amd import live
    assert live.ALIGN_DEFAULTS == dict(footprint=None, uv=False) and live.Aligned._fields == ("depth", "uv")
    t = cal.AlignTarget(_camera(), cr.rot(la.OM), la.T)
    K = dict(intrinsics=(50.0, 50.0, 30.0, 20.0), calib=5.0)
    for name in ("left", "right"):
        with pytest.raises(ValueError, match="calibration"):
            live.LiveSession(NoDevice(), (40, 60), align_to=name, **K)
    with pytest.raises(ValueError, match="align_to"):
        live.LiveSession(NoDevice(), (40, 60), align=dict(footprint=2), **K)
    for bad in (dict(foot=1), dict(footprint=0), dict(footprint=5), dict(footprint=2.0), dict(footprint=True), dict(uv=1),
                "auto", 2):
        with pytest.raises(ValueError, match="align"):
            live.LiveSession(NoDevice(), (40, 60), align_to=t, align=bad, **K)
    with pytest.raises(ValueError, match="align_to"):
        live.LiveSession(NoDevice(), (40, 60), align_to=7, **K)
    with pytest.raises(ValueError, match="one focal length"):
        live.LiveSession(NoDevice(), (40, 60), align_to=t, intrinsics=(50.0, 51.0, 30.0, 20.0), calib=5.0)
    with pytest.raises((ValueError, OSError)):
        live.LiveSession(NoDevice(), (40, 60), align_to=str(tmp_path / "missing.json"), **K)
    assert live._check_align(None, None) == live.ALIGN_DEFAULTS
    assert live._check_align(dict(uv=True), t) == dict(footprint=None, uv=True)
    assert live._check_align(dict(footprint=3), t) == dict(footprint=3, uv=False)


def test_session_resolves_the_target_on_a_cpu_estimator(tmp_path):
    """Everything the constructor derives (the target, the struct, the automatic footprint) without a device: the session
    on a CPU estimator is built and fails only at its first frame."""
    from codd_amd import _abi, configs, live
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.stereo_only()).eval()
    sc = _rig(size=(128, 192))
    sc.save(tmp_path / "rig.json")
    s = live.LiveSession(est, (128, 192), calibration=str(tmp_path / "rig.json"), align_to="right")
    assert s.align_target == cal.AlignTarget.of_rig(s.rect, "right") and s.align["footprint"] in (1, 2) and not s.align["uv"]
    assert list(s._align_view.R) == list(s.rect.R2.T.reshape(-1))
    t = cal.AlignTarget(_camera(size=(256, 384)), cr.rot(la.OM), la.T)
    t.save(tmp_path / "colour.npz")
    s2 = live.LiveSession(est, (128, 192), calibration=sc, align_to=tmp_path / "colour.npz", align=dict(uv=True))
    assert s2.align_target == t and s2.align == dict(footprint=cal.auto_footprint(
        t.R @ s2.rect.R1.T, t.camera, (128, 192), s2.rect.intrinsics), uv=True)
    assert np.abs(np.array(s2._align_view.R[:]).reshape(3, 3) - t.R @ s2.rect.R1.T).max() < 1e-15
    s3 = live.LiveSession(est, (128, 192), intrinsics=(170.0, 170.0, 95.5, 63.5), calib=20.0, align_to=t, align=dict(footprint=4))
    assert s3.align["footprint"] == 4 and list(s3._align_view.R) == list(t.R.reshape(-1))
    frame = np.zeros((128, 192, 3), np.uint8)
    with pytest.raises(_abi.CoddHipError):
        s3.step(frame, frame)


def test_cli_flags_need_each_other():
    from codd_amd import inference
    base = ["--img-dir", "l", "--r-img-dir", "r"]
    a = inference.parse_args(base + ["--live", "--calibration", "rig.json", "--align", "right", "--align-footprint", "2"])
    assert a.align == "right" and a.align_footprint == 2
    a = inference.parse_args(base + ["--live", "--align", "colour.json"])
    assert a.align == "colour.json" and a.align_footprint is None
    assert inference.parse_args(base + ["--live"]).align is None
    for argv in (["--align", "colour.json"], ["--live", "--align", "left"], ["--live", "--align", "right"],
                 ["--live", "--align-footprint", "2"], ["--live", "--align", "c.json", "--align-footprint", "5"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)


# ---- the restatements ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("a", "b"))
@pytest.mark.parametrize("shape", la.SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_reference_reproduces_the_exact_plants(shape, which):
    c, want, (by0, by1, bx0, bx1) = la.plant_case(shape, which)
    ref = la.reference(c)
    assert np.array_equal(ref["depth"], want.astype(np.float64))
    p32 = la.positions_fp32(c)
    assert np.array_equal(la.splat_fp32(c, p32), want)  # every operation of the plants is exact in fp32
    assert np.array_equal(p32["sx"], ref["uv"][..., 0].astype(np.float32)) and p32["ok"].all()
    if which == "b" and shape[0] == (37, 53):
        assert (want[by0:by1, bx0 + 8:bx1 + 8] == 2).all()  # the block, 8 columns on, in front of the background it covers
        assert np.isinf(want[by0:by1, bx0 + 2:bx0 + 8]).all()  # the band it uncovered
        assert (want[by0:by1, 2:bx0 + 2] == 8).all() and (want[:by0] == 8)[:, 2:-7].all()


_GEN = {}


def _general(spec):
    if spec not in _GEN:
        c = la.general_case(spec)
        _GEN[spec] = (c, la.reference(c))
    return _GEN[spec]


def test_delta_is_derived_from_the_measured_deviation():
    """MEASURED_DEV covers the deviation of the fp32 restatement from fp64 over every general case, DELTA is 8 times it and
    at least 2^-10; the two restatements skip the same pixels, and the fp32 depth stays inside DEPTH_C."""
    worst, worst_ratio = 0.0, 0.0
    for spec in la.GENERAL:
        c, ref = _general(spec)
        p32 = la.positions_fp32(c)
        ok = ref["pos"]["ok"]
        assert np.array_equal(p32["ok"], ok), la.case_id(spec)
        dev = max(np.abs(p32[k].astype(np.float64)[ok] - ref["pos"][k][ok]).max() for k in ("sx", "sy"))
        worst = max(worst, float(dev))
        worst_ratio = max(worst_ratio, float((np.abs(p32["Zt"].astype(np.float64)[ok] - ref["pos"]["Zt"][ok]) / ref["pos"]["bound"][ok]).max()))
    print(f"largest position deviation of the fp32 restatement: {worst:.3e} px; largest Zt error / bound: {worst_ratio:.3f}")
    assert worst <= la.MEASURED_DEV <= 2 * worst  # the recorded figure is the measured one, not a loose stand-in
    assert la.DELTA == max(8 * la.MEASURED_DEV, 2.0 ** -10)
    assert worst_ratio <= 1.0


@pytest.mark.parametrize("spec", la.GENERAL, ids=la.case_id)
def test_general_cases_stay_under_the_cap(spec):
    """On the inputs the GPU test uses the reference alone masks at most CAP of the covered pixels, the fp32 restatement
    passes the checks the kernel has to pass, and each case exercises what it is there for."""
    c, ref = _general(spec)
    (h, w), (ht, wt) = c["crop"], c["target"]["size"]
    amb = la.ambiguous(ref["pos"], c["k"], (ht, wt), la.DELTA)
    covered = int(np.isfinite(ref["depth"]).sum())
    assert covered >= 1 and int(amb.sum()) <= la.CAP * covered, (int(amb.sum()), covered)
    p32 = la.positions_fp32(c)
    la.check_depth(la.splat_fp32(c, p32), ref, amb, la.case_id(spec))
    la.check_uv(np.stack([p32["sx"], p32["sy"]], -1), ref, la.DELTA / 2, la.case_id(spec))
    assert ref["pos"]["ok"].all()
    if (h, w) == (37, 53):
        sx, sy = ref["uv"][..., 0], ref["uv"][..., 1]
        outside = (sx < -0.5) | (sx > wt - 0.5) | (sy < -0.5) | (sy > ht - 0.5)
        assert outside.any() or spec[2] >= 1.4  # some pixels leave the smaller targets
        assert covered >= 0.5 * min(h * w, ht * wt)
        if c["k"] == 1 and spec[2] > 1:
            assert np.isinf(ref["depth"]).sum() > 0
