"""Rectification from a stereo calibration, the parts that need no GPU: the geometry of StereoCalibration.rectify, what
the map function means (against an independent projection through both cameras), from_opencv, the two file formats,
every ValueError of codd_amd/calibration.py and of LiveSession(calibration=), and the argument checks of the two C-ABI
entries (every call is rejected before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_calib_ref as cr  # noqa: E402

from codd_amd import _abi, calibration as cal, ops  # noqa: E402
from codd_amd.calibration import CameraModel, Rectification, StereoCalibration  # noqa: E402

EINVAL = -1  # CODD_EINVAL


def _rig(model="brown", size=(48, 70)):
    (Kl, dl), (Kr, dr), R, T = cr.make_rig(model, size)
    return StereoCalibration(CameraModel(size, Kl, model, dl), CameraModel(size, Kr, model, dr), R, T)


def _points(n=1000, seed=0):
    """3-D points in front of the rig, in the LEFT camera's frame."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(0.8, 12.0, n)
    return np.stack([rng.uniform(-0.45, 0.45, n) * Z, rng.uniform(-0.3, 0.3, n) * Z, Z], axis=1)


# ---- geometry ---------------------------------------------------------------------------------------------------------
def test_rectified_rows_agree_and_disparity_is_baseline_over_depth():
    rig = _rig()
    rect = rig.rectify((37, 53))
    Xl = _points()
    Xr = Xl @ rig.R.T + rig.T
    Pl, Pr = Xl @ rect.R1.T, Xr @ rect.R2.T  # in the two rectified frames
    xl, yl, xr, yr = Pl[:, 0] / Pl[:, 2], Pl[:, 1] / Pl[:, 2], Pr[:, 0] / Pr[:, 2], Pr[:, 1] / Pr[:, 2]
    rows, disp = np.abs(yl - yr).max(), np.abs(Pl[:, 2] * (xl - xr) - np.linalg.norm(rig.T)).max()
    print(f"rows agree to {rows:.2e}; Z (x_l - x_r) = |T| to {disp:.2e}; |Z_l - Z_r| {np.abs(Pl[:, 2] - Pr[:, 2]).max():.2e}")
    assert rows <= 1e-12 and disp <= 1e-12
    assert rect.baseline == pytest.approx(np.linalg.norm(rig.T), rel=1e-15)
    assert rect.calib == rect.intrinsics[0] * rect.baseline and rect.intrinsics[0] == rect.intrinsics[1]
    # the default rectified camera: f' = zoom * min(f) * min(h / hs, w / ws), the principal point at the image centre
    fmin = min(rig.left.K[:2] + rig.right.K[:2])
    assert rect.intrinsics == pytest.approx((fmin * min(37 / 48, 53 / 70),) * 2 + (26.0, 18.0), rel=1e-15)
    assert rig.rectify((37, 53), zoom=1.25).intrinsics[0] == pytest.approx(1.25 * rect.intrinsics[0], rel=1e-15)
    assert rig.rectify().shape == rig.size  # default: the source size


def test_rectify_agrees_with_the_restatement_of_bouguets_method():
    rig = _rig()
    rect = rig.rectify((37, 53), zoom=0.9)
    R1, R2, f, cx, cy, b = cr.rectify_ref(rig.left.K, rig.right.K, rig.R, rig.T, rig.size, (37, 53), zoom=0.9)
    assert np.abs(rect.R1 - R1).max() <= 1e-14 and np.abs(rect.R2 - R2).max() <= 1e-14
    assert rect.intrinsics == pytest.approx((f, f, cx, cy), rel=1e-15) and rect.baseline == pytest.approx(b, rel=1e-15)
    # both are rotations, and the split is even: each camera turns by half the relative angle (before the common alignment)
    for R in (rect.R1, rect.R2):
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
    assert np.abs(rect.R2.T @ rect.R1 - rig.R).max() <= 1e-14  # R2^T R1 = R: what is left between the views is a translation


def test_already_rectified_rig_gives_identity_maps_exactly():
    # f, cx, cy dyadic: every operation of the map function is then exact in fp64, so "identity" can be asserted to the bit
    size, K = (40, 64), (64.0, 64.0, 31.5, 19.5)
    cam = CameraModel(size, K)
    rect = StereoCalibration(cam, cam, np.eye(3), (-0.1, 0.0, 0.0)).rectify(principal=(31.5, 19.5))
    assert np.array_equal(rect.R1, np.eye(3)) and np.array_equal(rect.R2, np.eye(3))
    assert rect.intrinsics == K and rect.baseline == 0.1 and rect.shape == size
    uu, vv = cr.grid(size)
    for view in (0, 1):
        mx, my = rect.maps(view)
        assert np.array_equal(mx, uu) and np.array_equal(my, vv)
        rx, ry, _ = cr.map_fp64(cr.as_view(rect.views[view]), uu, vv)
        assert np.array_equal(rx, uu) and np.array_equal(ry, vv)
        fx_, fy_ = cr.map_fp32(cr.as_view(rect.views[view]), uu, vv)  # ... and in the kernels' fp32 order
        assert np.array_equal(fx_, uu.astype(np.float32)) and np.array_equal(fy_, vv.astype(np.float32))
    # a general focal length: (u - cx) / f * f + cx is the identity up to rounding only
    cam = CameraModel(size, (61.7, 61.7, 30.9, 20.3))
    rect = StereoCalibration(cam, cam, np.eye(3), (-0.1, 0.0, 0.0)).rectify(principal=(30.9, 20.3))
    mx, my = rect.maps(0)
    assert max(np.abs(mx - uu).max(), np.abs(my - vv).max()) <= 1e-12


@pytest.mark.parametrize("model", cal.MODELS)
def test_map_sends_the_rectified_projection_to_the_source_projection(model):
    """What the map means, without the map function: project a 3-D point through the real camera (K, dist) -> source pixel
    s, and through the rectified camera -> u; map(u) must be s."""
    rig = _rig(model)
    rect = rig.rectify((37, 53), zoom=0.8)
    Xl = _points(400, seed=1)
    f, _, cx, cy = rect.intrinsics
    worst = 0.0
    for view, X, cam in ((0, Xl, rig.left), (1, Xl @ rig.R.T + rig.T, rig.right)):
        s = cr.distort(dict(K=cam.K, dist=cam.dist8, model=model), X[:, 0] / X[:, 2], X[:, 1] / X[:, 2])  # the real camera
        Xrect = X @ rect.views[view].R.T
        u, v = f * Xrect[:, 0] / Xrect[:, 2] + cx, f * Xrect[:, 1] / Xrect[:, 2] + cy  # the rectified camera
        for got in (rect.source_points(view, u, v), cr.map_fp64(cr.as_view(rect.views[view]), u, v)[:2]):
            worst = max(worst, np.abs(got[0] - s[0]).max(), np.abs(got[1] - s[1]).max())
    print(f"{model}: map(u) = s to {worst:.2e} px")
    assert worst <= 1e-9


@pytest.mark.parametrize("model", cal.MODELS)
def test_fp32_restatement_stays_close_to_fp64(model):
    """The fp32 operation order of the header, restated in numpy, against fp64 at the small GPU case (the issue measured
    about 1.1e-5 px here); its product-size deviation sets the GPU test's bound."""
    rect = _rig(model).rectify((37, 53))
    uu, vv = cr.grid(rect.shape)
    for view in (0, 1):
        v = cr.as_view(rect.views[view])
        rx, ry, _ = cr.map_fp64(v, uu, vv)
        fx_, fy_ = cr.map_fp32(v, uu, vv)
        dev = max(np.abs(fx_ - rx).max(), np.abs(fy_ - ry).max())
        inside = np.mean((rx > -1) & (rx < 70) & (ry > -1) & (ry < 48))
        print(f"{model} view {view}: fp32 restatement deviates {dev:.2e} px; {100 * inside:.0f} % of the pixels inside; "
              f"shift up to {max(np.abs(rx - uu * 70 / 53).max(), np.abs(ry - vv * 48 / 37).max()):.1f} px")
        assert dev < 1.0 / 32 / 5


# ---- from_opencv and files ------------------------------------------------------------------------------------------------
def _same_rect(a, b):
    assert a.shape == b.shape and a.size == b.size and a.intrinsics == b.intrinsics
    assert a.baseline == pytest.approx(b.baseline, rel=1e-15) and a.calib == pytest.approx(b.calib, rel=1e-15)
    for va, vb in zip(a.views, b.views):
        assert np.array_equal(np.asarray(va.R), np.asarray(vb.R)) and tuple(va.P) == tuple(vb.P) and va.camera == vb.camera


def test_from_opencv_round_trips_rectify():
    rig = _rig()
    rect = rig.rectify((37, 53), zoom=1.1)
    assert rect.P2[0, 3] == -rect.intrinsics[0] * rect.baseline and not rect.P1[:, 3].any()
    _same_rect(Rectification.from_opencv(rect.R1, rect.R2, rect.P1, rect.P2, rig.left, rig.right, (37, 53)), rect)


@pytest.mark.parametrize("ext", [".json", ".npz"])
@pytest.mark.parametrize("model", cal.MODELS)
def test_files_round_trip(tmp_path, ext, model):
    rig = _rig(model)
    rig.save(tmp_path / ("rig" + ext))
    back = cal.load(tmp_path / ("rig" + ext))
    assert isinstance(back, StereoCalibration) and back.size == rig.size
    assert back.left == rig.left and back.right == rig.right
    assert np.array_equal(back.R, rig.R) and np.array_equal(back.T, rig.T)
    rect = rig.rectify((37, 53))
    rect.save(tmp_path / ("rect" + ext))
    back = cal.load(str(tmp_path / ("rect" + ext)))
    assert isinstance(back, Rectification)
    _same_rect(back, rect)
    assert cal.resolve(tmp_path / ("rig" + ext), (37, 53)).intrinsics == rect.intrinsics
    with pytest.raises(ValueError):
        rig.save(tmp_path / "rig.yaml")
    with pytest.raises(ValueError):
        cal.load(tmp_path / "rig.yml")


def test_short_distortion_tuples_are_zero_extended():
    K = (60.0, 60.0, 30.0, 20.0)
    assert CameraModel((40, 64), K, dist=(0.1, 0.2, 0.3, 0.4)).dist8 == (0.1, 0.2, 0.3, 0.4, 0, 0, 0, 0)
    assert CameraModel((40, 64), K, dist=(0.1, 0.2, 0.3, 0.4, 0.5)).dist8 == (0.1, 0.2, 0.3, 0.4, 0.5, 0, 0, 0)
    assert CameraModel((40, 64), np.array([[60.0, 0, 30], [0, 61, 20], [0, 0, 1]])).K == (60.0, 61.0, 30.0, 20.0)
    assert CameraModel((40, 64), K, "fisheye", (0.1, 0.2, 0.3, 0.4)).dist8[:4] == (0.1, 0.2, 0.3, 0.4)


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_calibration_errors():
    K, size = (60.0, 60.0, 30.0, 20.0), (40, 64)
    cam = CameraModel(size, K)
    for bad in ((1, 2, 3), (1,) * 6, (1,) * 7, (1,) * 9):  # wrong coefficient counts
        with pytest.raises(ValueError):
            CameraModel(size, K, "brown", bad)
    for bad in ((1, 2, 3), (1,) * 5, (1,) * 8):
        with pytest.raises(ValueError):
            CameraModel(size, K, "fisheye", bad)
    with pytest.raises(ValueError):
        CameraModel(size, K, "mei")
    with pytest.raises(ValueError):
        CameraModel(size, (60.0, float("nan"), 30.0, 20.0))  # non-finite entries
    with pytest.raises(ValueError):
        CameraModel(size, K, dist=(0.1, float("inf"), 0, 0))
    with pytest.raises(ValueError):
        CameraModel(size, (60.0, -60.0, 30.0, 20.0))
    with pytest.raises(ValueError):
        CameraModel((0, 64), K)
    T = (-0.1, 0.0, 0.0)
    with pytest.raises(ValueError):
        StereoCalibration(cam, CameraModel((40, 66), K), np.eye(3), T)  # size mismatch
    with pytest.raises(ValueError):
        StereoCalibration(cam, cam, np.eye(3) * 1.001, T)  # not a rotation to 1e-6
    with pytest.raises(ValueError):
        StereoCalibration(cam, cam, np.diag([1.0, 1.0, -1.0]), T)  # a reflection
    StereoCalibration(cam, cam, np.eye(3) + 1e-8, T)  # ... inside the tolerance
    with pytest.raises(ValueError):
        StereoCalibration(cam, cam, np.eye(3), (-0.1, float("nan"), 0.0))
    with pytest.raises(ValueError):
        StereoCalibration(cam, cam, np.eye(3), (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="vertical"):
        StereoCalibration(cam, cam, np.eye(3), (-0.01, -0.1, 0.0))  # a baseline mostly along y
    with pytest.raises(ValueError, match="on the left"):
        StereoCalibration(cam, cam, np.eye(3), (0.1, 0.0, 0.0))  # a right camera on the left
    rig = StereoCalibration(cam, cam, np.eye(3), T)
    for kw in (dict(zoom=0.0), dict(zoom=float("nan")), dict(shape=(0, 10)), dict(principal=(1.0, float("inf")))):
        with pytest.raises(ValueError):
            rig.rectify(**kw)
    # from_opencv: a rectified baseline that is not along +x, in its three disguises
    rect = rig.rectify()
    P2 = rect.P2
    P2[0, 3] = -P2[0, 3]
    with pytest.raises(ValueError, match=r"\+x"):
        Rectification.from_opencv(rect.R1, rect.R2, rect.P1, P2, cam, cam, size)
    P2 = rect.P2
    P2[1, 3] = -6.0
    with pytest.raises(ValueError, match="vertical"):
        Rectification.from_opencv(rect.R1, rect.R2, rect.P1, P2, cam, cam, size)
    P2 = rect.P2
    P2[0, 2] += 3.0  # not CALIB_ZERO_DISPARITY
    with pytest.raises(ValueError):
        Rectification.from_opencv(rect.R1, rect.R2, rect.P1, P2, cam, cam, size)
    with pytest.raises(ValueError):
        Rectification.from_opencv(rect.R1 * 1.01, rect.R2, rect.P1, rect.P2, cam, cam, size)
    with pytest.raises(ValueError):
        Rectification.from_opencv(rect.R1, rect.R2, rect.P1, rect.P2, cam, CameraModel((40, 66), K), size)


def _cpu_session(shape=(37, 53), **kw):
    from codd_amd import configs
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.stereo_only()).eval()  # on the CPU: any device call would raise CoddHipError
    return LiveSession(est, shape, **kw)


def test_session_constructor_errors_and_derived_numbers(tmp_path):
    rig = _rig()
    rect = rig.rectify((37, 53))
    ident = np.zeros((37, 53), np.float32)
    for kw in (dict(intrinsics=(1.0, 1.0, 2.0, 3.0)), dict(calib=10.0), dict(rectify=((ident, ident), None))):
        with pytest.raises(ValueError, match="calibration"):
            _cpu_session(calibration=rig, **kw)
    with pytest.raises(ValueError):
        _cpu_session(zoom=1.5)  # zoom without a calibration
    with pytest.raises(ValueError):
        _cpu_session(calibration=rect, zoom=1.5)  # a Rectification is taken as it is
    with pytest.raises(ValueError):
        _cpu_session(shape=(40, 64), calibration=rect)  # made for another shape
    with pytest.raises(ValueError):
        _cpu_session(calibration=42)
    with pytest.raises(ValueError):
        _cpu_session(calibration=str(tmp_path / "rig.yaml"))
    with pytest.raises(ValueError):
        _cpu_session(calibration=rig, pixel_format="nv12", pitch=60)  # the pitch is checked against the SOURCE width 70
    with pytest.raises(ValueError):
        _cpu_session(shape=(38, 54), calibration=_rig(size=(47, 70)), pixel_format="nv12")  # nv12: the SOURCE height is odd
    rig.save(tmp_path / "rig.json")
    for c in (rig, rect, tmp_path / "rig.json", str(tmp_path / "rig.json")):
        s = _cpu_session(calibration=c)
        meta = s.metas[0]
        assert s.shape == (37, 53) and s.src_shape == (48, 70) and s.padded == (64, 64)
        assert meta["img_shape"] == (37, 53, 3) and meta["calib"] == s.calib == rect.calib
        assert tuple(meta["intrinsics"]) == rect.intrinsics
    assert _cpu_session(calibration=rig, zoom=1.5).calib == pytest.approx(1.5 * rect.calib, rel=1e-15)
    plain = _cpu_session()  # calibration=None: the defaults of before
    assert plain.rect is None and plain.src_shape == plain.shape and plain.calib == 210.0
    assert tuple(plain.metas[0]["intrinsics"]) == (1050.0, 1050.0, 480.0, 270.0)


def test_session_validates_frames_against_the_source_size():
    s = _cpu_session(calibration=_rig())
    src = np.zeros((48, 70, 3), np.uint8)
    with pytest.raises(ValueError):
        s.push(np.zeros((37, 53, 3), np.uint8), src)  # the rectified size is not the frame size
    with pytest.raises(ValueError):
        s.push(src, np.zeros((48, 71, 3), np.uint8))
    assert s.pending() == 0 and not s._open_done
    with pytest.raises(_abi.CoddHipError):  # a valid pair gets past validation; the CPU estimator is then refused
        s.push(src, src)
    s = _cpu_session(shape=(38, 54), calibration=_rig(), pixel_format="nv12", pitch=72)
    assert s._layout == (72, 70, 72, 72 * 72)  # rows 3 hs / 2 of the source, its row bytes, pitch, bytes
    with pytest.raises(ValueError):
        s.push(np.zeros((57, 72), np.uint8), np.zeros((72, 72), np.uint8))
    assert not s._open_done


# ---- the C-ABI entries: every call below is rejected before any launch ------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_entries_reject_bad_arguments():
    lib = _abi.load()
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = _ptr(buf)
    m, s = (C.c_float * 3)(1, 2, 3), (C.c_float * 3)(1, 1, 1)
    rect = _rig().rectify((37, 53))
    good = ops.calib_structs(rect)

    def view(**kw):
        v = ops.calib_structs(rect)[0]
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(v, k)[val[0]] = val[1]
            else:
                setattr(v, k, val)
        return C.byref(v)

    L, R_ = C.byref(good[0]), C.byref(good[1])
    bad_views = [view(model=2), view(model=-1), view(f=0.0), view(f=-3.0), view(f=float("nan")), view(f=float("inf")),
                 view(K=(0, 0.0)), view(K=(1, -1.0)), view(K=(0, float("inf"))), view(K=(2, float("nan"))),
                 view(R=(4, float("nan"))), view(dist=(7, float("inf"))), view(cx=float("nan"))]

    def maps(l=L, r=R_, h=37, w=53, lx=p, ly=p, rx=p, ry=p):
        return lib.codd_rectify_maps(l, r, h, w, lx, ly, rx, ry, None)

    assert maps(l=None, r=None) == EINVAL
    assert maps(h=0) == EINVAL and maps(w=-1) == EINVAL
    assert maps(lx=None) == EINVAL and maps(ly=None) == EINVAL and maps(rx=None) == EINVAL and maps(ry=None) == EINVAL
    for b in bad_views:
        assert maps(l=b) == EINVAL and maps(r=b) == EINVAL and maps(l=None, r=b) == EINVAL

    def ingest(left=p, right=p, fmt=0, yuv=0, hs=48, ws=70, pitch=0, l=L, r=R_, h=37, w=53, mean=m, std=s, H=64, W=64,
               ol=p, orr=p):
        return lib.codd_ingest_calibrated(left, right, fmt, 0, yuv, hs, ws, pitch, l, r, h, w, mean, std, H, W, ol, orr, None)

    for k in ("left", "right", "mean", "std", "ol", "orr"):
        assert ingest(**{k: None}) == EINVAL, k
    assert ingest(l=None, r=None) == EINVAL
    assert ingest(fmt=9) == EINVAL and ingest(fmt=-1) == EINVAL
    assert ingest(fmt=4, yuv=3) == EINVAL and ingest(fmt=2, yuv=-1) == EINVAL
    assert ingest(fmt=2, ws=69) == EINVAL and ingest(fmt=4, hs=47) == EINVAL and ingest(fmt=5, hs=1) == EINVAL  # size rules on hs, ws
    assert ingest(hs=0) == EINVAL and ingest(ws=0) == EINVAL
    assert ingest(pitch=209) == EINVAL and ingest(fmt=1, pitch=69) == EINVAL and ingest(fmt=2, pitch=139) == EINVAL
    assert ingest(H=36) == EINVAL and ingest(W=52) == EINVAL and ingest(h=32, H=64) == EINVAL and ingest(w=32, W=64) == EINVAL
    assert ingest(h=0) == EINVAL and ingest(w=0) == EINVAL
    assert ingest(l=None) == EINVAL and ingest(r=None) == EINVAL  # a view without calibration needs hs, ws == h, w
    for b in bad_views:
        assert ingest(l=b) == EINVAL and ingest(r=b) == EINVAL
