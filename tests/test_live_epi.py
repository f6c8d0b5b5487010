"""LiveSession rectification health check on the CPU: the restatement of tests/live_epi_ref.py recovers planted vertical
disparities, its cases leave few near-ties, LiveSession's epipolar= validation makes no device call, combine_epipolar pools
normal equations exactly, and calibration.Rectification.corrected takes a fitted misalignment out of a rig."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_epi_ref as le  # noqa: E402

from codd_amd import calibration as cal, live  # noqa: E402

_CACHE = {}
# The parabola through three SAD costs is biased towards whole rows.  Where the window's grey difference is linear in the
# offset t in [-1/2, 1/2] from the best row, C(v) = S |v - t| and the estimate is t / (2 (1 - |t|)): its error has the maximum
# 0.0858 px at |t| = 1 - 1/sqrt(2).  A least-squares fit is a projection, so the rms of (fitted - planted) over the pixels it
# was fitted to is at most that of the bias field; 8-bit quantisation and window edges add to it: 0.1 px.
BIAS_PX = 0.1


def _ref(i, plant=None):
    key = (i, plant)
    if key not in _CACHE:
        c = le.case(le.CASES[i], plant)
        _CACHE[key] = (c, le.reference(c))
    return _CACHE[key]


def _corner_px(c, dcoef):
    """|coefficient error| expressed as pixels of dy at the image corner (0, 0), term by term."""
    fx, fy, cx, cy = c["K"]
    xr, yn = -cx / fx, -cy / fy
    return np.abs(np.asarray(dcoef) * fy * np.array([1 + yn * yn, xr * yn, xr, yn]))


@pytest.mark.parametrize("plant", [(le.PLANT_OFFSET_PX / le.K_FIT[1], 0.0, 0.0, 0.0), le.PLANT_MIX], ids=["offset", "mix"])
def test_plant_recovery(plant):
    c, ref = _ref(le.FIT_CASE, plant)
    f = ref["f64"]
    assert f["ok"] and f["n"] >= 1000 and f["steps"] == c["par"]["iters"]
    ys, xs = np.nonzero(ref["measurable64"])
    d = c["disp"][ys, xs].astype(np.float64)
    planted, fitted = le.model_dy(plant, c["K"], xs - d, ys), le.model_dy(f["coef"], c["K"], xs - d, ys)
    rms = float(np.sqrt(np.mean((fitted - planted) ** 2)))
    print(f"planted {plant}: fitted {f['coef'].tolist()}, n {f['n']}, inliers {f['inliers']}, rms dy {f['rms']:.4f}, rms fit "
          f"{f['rms_fit']:.4f}; coefficient errors as px at the corner {_corner_px(c, f['coef'] - np.array(plant)).tolist()}; "
          f"rms (fitted - planted) {rms:.4f} px, planted |dy| max {np.abs(planted).max():.3f}")
    assert np.abs(planted).max() >= 0.5
    assert rms <= BIAS_PX
    # the measured map itself: the median error of a pixel stays inside the same bias
    err = np.abs(ref["m64"]["dy"][ys, xs] - planted)
    print(f"  per-pixel |dy - planted|: median {np.median(err):.4f}, 90 % {np.quantile(err, 0.9):.4f}")
    assert np.median(err) <= BIAS_PX


@pytest.mark.parametrize("i", range(len(le.CASES)), ids=[le.case_id(s) for s in le.CASES])
def test_near_ties_are_rare(i):
    c, ref = _ref(i)
    n, und = int(ref["measurable64"].sum()), int((ref["undecided"] & ref["measurable64"]).sum())
    print(f"{le.case_id(le.CASES[i])}: measurable {n}, undecided {und} (all candidates: {int(ref['undecided'].sum())}), devC "
          f"{ref['devC']:.3e}, dev dy {ref['dev_dy']:.3e}, dev coef {ref['dev_coef']:.3e}")
    if c["crop"] == (5, 3):
        assert n == 0 and not ref["f64"]["ok"] and not np.any(ref["f64"]["coef"])
        return
    assert n >= 50
    assert und <= 0.01 * n and int(ref["undecided"].sum()) <= 0.01 * n
    # the restatement takes the reference's decisions outside the undecided pixels
    same = np.isnan(ref["m32"]["dy"]) == np.isnan(ref["m64"]["dy"])
    assert same[~ref["undecided"]].all()


def test_tie_order_and_gates():
    assert le.candidate_order(2) == [0, -1, 1, -2, 2]
    c, _ = _ref(0)
    flat = dict(c, right=np.zeros_like(c["right"]), left=np.zeros_like(c["left"]))  # every cost ties at 0: v* = 0, no curvature
    m = le.measure(flat, np.float32)
    assert m["idx"][0].size > 0 and (m["vstar"] == 0).all() and np.isnan(m["dy"]).all()
    m = le.measure(c, np.float32, tau=-1.0)  # no match is good enough
    assert np.isnan(m["dy"]).all()


BAD = [3, "yes", dict(speed=1), dict(range_px=0), dict(range_px=5), dict(range_px=2.0), dict(range_px=True), dict(step=0),
       dict(step=9), dict(step="2"), dict(iters=0), dict(iters=33), dict(iters=None), dict(tau=float("nan")), dict(tau="x"),
       dict(min_curv=float("nan")), dict(min_curv=None), dict(delta_px=0.0), dict(delta_px=-1.0), dict(delta_px=float("nan")),
       dict(min_valid=2.5), dict(min_valid=None), dict(map=1), dict(map="yes")]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_check_epi_rejects(bad):
    with pytest.raises(ValueError, match="epipolar"):
        live._check_epi(bad)
    with pytest.raises(ValueError, match="epipolar"):  # before the estimator is looked at: no device call
        live.LiveSession(None, (8, 8), epipolar=bad)


def test_check_epi_accepts():
    assert live._check_epi(False) is None and live._check_epi(None) is None
    assert live._check_epi(True) == live.EPI_DEFAULTS and live._check_epi(True) is not live.EPI_DEFAULTS
    assert live.EPI_DEFAULTS == dict(range_px=2, step=2, tau=24.0, min_curv=0.5, iters=4, delta_px=0.25, min_valid=256, map=False)
    p = live._check_epi(dict(step=4, map=True, tau=30))
    assert p == dict(live.EPI_DEFAULTS, step=4, map=True, tau=30.0) and isinstance(p["tau"], float)
    assert live.Epipolar._fields == ("coef", "ok", "valid", "inliers", "rms_px", "rms_fit_px", "A", "b", "dy")


def test_record_layout():
    rec = np.zeros(32)
    rec[:10] = [1e-3, 2e-3, 3e-3, 4e-3, 1, 500, 400, 0.5, 0.1, 4]
    rec[10:20] = np.arange(1, 11)
    rec[20:24] = [7, 8, 9, 10]
    e = live.epipolar_from_record(rec)
    assert e.coef.tolist() == [1e-3, 2e-3, 3e-3, 4e-3] and e.ok is True and (e.valid, e.inliers) == (500, 400)
    assert (e.rms_px, e.rms_fit_px) == (0.5, 0.1) and e.dy is None and e.b.tolist() == [7, 8, 9, 10]
    assert e.A.tolist() == [[1, 2, 3, 4], [2, 5, 6, 7], [3, 6, 8, 9], [4, 7, 9, 10]]


def test_combine_epipolar_pools_the_equations():
    c, ref = _ref(le.FIT_CASE)
    h, w = c["crop"]
    dy = ref["m64"]["dy"]
    full = le.fit(c, dy, np.float64, iters=1)
    parts = []
    for rows in (slice(0, h // 2), slice(h // 2, h)):
        half = np.full_like(dy, np.nan)
        half[rows] = dy[rows]
        f = le.fit(c, half, np.float64, iters=1, min_valid=10 ** 9)  # (its own fit fails: ok False, equations kept)
        assert not f["ok"]
        parts.append(live.Epipolar(f["coef"], f["ok"], f["n"], f["inliers"], f["rms"], f["rms_fit"], f["A"], f["b"], None))
    coef, ok = live.combine_epipolar(parts + [None])
    assert ok and full["ok"]
    rel = np.abs(coef - full["coef"]).max() / np.abs(full["coef"]).max()
    print("combined vs full fit, relative:", rel)
    assert rel <= 1e-12
    none, ok0 = live.combine_epipolar([])
    assert not ok0 and not none.any()
    # the library's solver against the restatement's
    a, oka = live.solve_epipolar(full["A"], full["b"])
    assert oka and np.abs(a - full["coef"]).max() <= 1e-12 * np.abs(full["coef"]).max()
    assert live.solve_epipolar(np.zeros((4, 4)), np.zeros(4))[1] is False


def test_entry_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    import ctypes as C
    from codd_amd import _abi
    lib = _abi.load()
    assert not _abi.MISSING and lib.codd_epipolar_scratch(0, 4) == -1 and lib.codd_epipolar_scratch(4, -1) == -1
    assert lib.codd_epipolar_scratch(65536, 32768) == -1 and lib.codd_epipolar_scratch(37, 61) > 12 * 37 * 61
    for h, w in ((1, 1), (37, 53), (540, 960)):  # the layout is part of the contract: rows, states, ticket; three planes
        assert lib.codd_epipolar_scratch(h, w) == 65696 + 12 * h * w
    need = lib.codd_epipolar_scratch(24, 40)
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = buf.ctypes.data_as(C.c_void_p)
    std = (C.c_float * 3)(*le.STD)
    nan = float("nan")

    def call(disp=p, left=p, right=p, H=64, W=64, h=24, w=40, stdv=std, fx=60.0, fy=60.0, cx=20.0, cy=12.0, range_px=2, step=2,
             tau=24.0, min_curv=0.5, iters=4, delta_px=0.25, min_valid=16, scratch=p, nbytes=need, record=p, dy_map=None):
        return lib.codd_epipolar_check(disp, left, right, H, W, h, w, stdv, fx, fy, cx, cy, range_px, step, tau, min_curv, iters,
                                       delta_px, min_valid, scratch, nbytes, record, dy_map, None)

    for name in ("disp", "left", "right", "stdv", "scratch", "record"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(h=0), dict(w=0), dict(H=0), dict(W=-3), dict(h=65), dict(w=65), dict(range_px=0), dict(range_px=5),
                dict(step=0), dict(step=9), dict(iters=0), dict(iters=33), dict(fx=0.0), dict(fx=nan), dict(fy=-1.0),
                dict(delta_px=0.0), dict(delta_px=nan), dict(tau=nan), dict(min_curv=nan), dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**bad) == -1, bad


# ---- Rectification.corrected on a rig whose right camera has moved ------------------------------------------------------
def _rig():
    size = (480, 640)
    left = cal.CameraModel(size, (520.0, 520.0, 319.5, 239.5))
    right = cal.CameraModel(size, (525.0, 525.0, 322.0, 238.0))
    R = cal.rodrigues([0.01, -0.02, 0.005])
    return cal.StereoCalibration(left, right, R, [-0.12, 0.002, 0.001])


def _rectified_rows(rect, calib, R_extra, ratio, X):
    """Rectified positions (ul, vl, ur, vr) of the 3-D points X [n,3] (left camera frame) seen by the TRUE rig -- the
    nominal ``calib`` whose right camera is rotated by ``R_extra`` and has ``ratio`` times the focal length -- and
    un-rectified in closed form with ``rect`` (pinhole cameras: ray = K^-1 pixel; rectified = P R ray)."""
    out = []
    Xr = (R_extra @ (calib.R @ X.T + calib.T[:, None])).T
    for view, pts, scale in ((0, X, 1.0), (1, Xr, ratio)):
        fx, fy, cx, cy = (calib.left if view == 0 else calib.right).K
        sx, sy = scale * fx * pts[:, 0] / pts[:, 2] + cx, scale * fy * pts[:, 1] / pts[:, 2] + cy  # the true camera's pixel
        Rv, (f, _, pcx, pcy), cam = rect.views[view]
        kx, ky, kcx, kcy = cam.K  # what the rectification believes
        ray = np.stack([(sx - kcx) / kx, (sy - kcy) / ky, np.ones_like(sx)])
        r = np.asarray(Rv) @ ray
        out += [f * r[0] / r[2] + pcx, f * r[1] / r[2] + pcy]
    return out


def test_corrected_takes_the_misalignment_out(tmp_path):
    calib = _rig()
    rect = calib.rectify()
    R_extra, ratio = cal.rodrigues([2e-3, -1.5e-3, 1e-3]), 1.001
    rng = np.random.default_rng(3)
    pts = []
    for z in (0.8, 2.0, 6.0):  # three depth planes, seen by both cameras
        u, v = rng.uniform(80, 560, 400), rng.uniform(40, 440, 400)
        pts.append(np.stack([(u - 319.5) / 520.0 * z, (v - 239.5) / 520.0 * z, np.full(400, z)], 1))
    X = np.concatenate(pts)

    def dy_of(r):
        ul, vl, ur, vr = _rectified_rows(r, calib, R_extra, ratio, X)
        return ul, vl, ur, vr - vl

    ul, vl, ur, dy0 = dy_of(rect)
    ideal = _rectified_rows(rect, calib, np.eye(3), 1.0, X)
    assert np.abs(ideal[3] - ideal[1]).max() < 1e-9  # the nominal rig is rectified exactly
    # the reference least squares on (x - d = ur, y = vl, dy0)
    fx, fy, cx, cy = rect.intrinsics
    xr, yn = (ur - cx) / fx, (vl - cy) / fy
    p = np.stack([fy * (1 + yn * yn), fy * xr * yn, fy * xr, fy * yn])
    A, b = le.normal_equations(p, np.ones_like(dy0), dy0)
    coef, ok = le.solve(A, b)
    assert ok
    fixed = rect.corrected(coef)
    _, _, _, dy1 = dy_of(fixed)
    ratio_left = np.abs(dy1).max() / np.abs(dy0).max()
    print(f"max |dy0| {np.abs(dy0).max():.4f} px, max |dy1| {np.abs(dy1).max():.5f} px, ratio {ratio_left:.5f}; coef {coef.tolist()}")
    assert 0.3 <= np.abs(dy0).max() <= 5.0
    assert np.abs(dy1).max() <= 0.02 * np.abs(dy0).max()
    # the left view, P, shape and baseline are untouched; the right view and camera changed
    assert fixed.views[0] is rect.views[0] and fixed.intrinsics == rect.intrinsics and fixed.shape == rect.shape
    assert fixed.baseline == rect.baseline and fixed.views[1].camera != rect.views[1].camera
    assert rect.corrected(np.zeros(4)).views[1].camera == rect.views[1].camera
    assert np.array_equal(rect.corrected(np.zeros(4)).R2, rect.R2)
    # round trip through to_dict / save / load, both formats
    for name in ("fixed.json", "fixed.npz"):
        fixed.save(tmp_path / name)
        back = cal.load(tmp_path / name)
        assert isinstance(back, cal.Rectification) and back.shape == fixed.shape
        assert np.abs(back.R2 - fixed.R2).max() <= 1e-15 and np.array_equal(back.R1, fixed.R1)
        assert back.views[1].camera == fixed.views[1].camera and back.views[0].camera == fixed.views[0].camera
        assert abs(back.baseline - fixed.baseline) <= 1e-15 * fixed.baseline and back.intrinsics == fixed.intrinsics
    for bad in ([1, 2, 3], [0, 0, 0, float("nan")], [0, 0, 0, -1.0]):
        with pytest.raises(ValueError):
            rect.corrected(bad)
