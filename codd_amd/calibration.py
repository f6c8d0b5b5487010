"""Stereo calibration -> rectification, on the host in numpy fp64 (no device call anywhere in this module).

A user of a live stereo rig has a calibration: two camera models (intrinsics and lens distortion) and the pose of the
right camera against the left, ``X_right = R X_left + T`` -- what ``cv2.stereoCalibrate`` returns.  ``StereoCalibration
.rectify`` turns it into a ``Rectification``: per view the rectifying rotation ``R_rect`` and the pinhole camera ``P =
(f', f', cx', cy')`` of the rectified image, plus what the session needs of the rectified rig -- ``baseline``,
``intrinsics`` and ``calib = f' * baseline``.  The rectifying map itself is a closed-form function of these numbers,
stated once in include/codd_hip.h (THE MAP FUNCTION) and evaluated on the GPU (ops.rectify_maps writes it out as map
arrays, ops.ingest_calibrated evaluates it inside the ingest launch); ``Rectification.source_points`` is the same
function in fp64 for use on the host.

``AlignTarget`` describes one more calibrated camera -- a physical camera of the rig or a separate colour camera -- to
which ``LiveSession(align_to=)`` registers the depth map (ops.align_depth); ``fold_radius2`` and ``auto_footprint`` derive
the two parameters of that launch the user does not have to think about.

Files: ``.json`` and ``.npz`` with the plain keys listed in INTEGRATION.md ("Rectification from a calibration", "Depth on
another camera's grid").
"""
import json
import os
from collections import namedtuple

import numpy as np

MODELS = ("brown", "fisheye")  # CODD_CALIB_BROWN, CODD_CALIB_FISHEYE of include/codd_hip.h, in this order
BROWN_COUNTS = (0, 4, 5, 8)  # k1 k2 p1 p2 [k3 [k4 k5 k6]], zero-extended to 8
FISHEYE_COUNTS = (0, 4)  # k1 k2 k3 k4
ROTATION_TOL = 1e-6

# One view of a rectification: R the 3x3 rectifying rotation (X_rect = R X_cam), P = (f', f', cx', cy') the rectified
# pinhole camera, camera the source CameraModel.
RectifiedView = namedtuple("RectifiedView", "R P camera")


def _finite(a, name, shape=None):
    try:
        a = np.array(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: numbers expected, got {a!r}") from None
    if shape is not None and a.shape != shape:
        raise ValueError(f"{name}: shape {shape} expected, got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name}: finite entries expected, got {a.tolist()}")
    return a


def _size(size, name):
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: (height, width) expected, got {size!r}") from None
    if h <= 0 or w <= 0 or (h, w) != tuple(size):
        raise ValueError(f"{name}: positive integers (height, width) expected, got {size!r}")
    return h, w


def _rotation(R, name):
    R = _finite(R, name, (3, 3))
    if np.abs(R @ R.T - np.eye(3)).max() > ROTATION_TOL or abs(np.linalg.det(R) - 1.0) > ROTATION_TOL:
        raise ValueError(f"{name}: a rotation matrix is expected (R R^T = I and det R = 1 to {ROTATION_TOL:g})")
    return R


def rodrigues(om):
    """Rotation vector [3] -> rotation matrix [3,3]."""
    om = np.asarray(om, np.float64)
    th = float(np.linalg.norm(om))
    if th < 1e-300:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def rotation_vector(R):
    """Rotation matrix [3,3] -> rotation vector [3] (angle in [0, pi])."""
    R = np.asarray(R, np.float64)
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * float(np.linalg.norm(axis)), 0.5 * (float(np.trace(R)) - 1.0)
    th = float(np.arctan2(s, c))
    if s > 1e-8:
        return axis * (th / (2.0 * s))
    if c > 0:  # near the identity: R - R^T = 2 [om]_x to first order
        return 0.5 * axis
    # near pi: the axis from the symmetric part, R + I = 2 k k^T
    B = 0.5 * (R + np.eye(3))
    i = int(np.argmax(np.diag(B)))
    k = B[:, i] / np.sqrt(B[i, i])
    return k * th


class CameraModel:
    """One camera: ``size`` (height, width) of its frames, ``K`` = (fx, fy, cx, cy), and the lens: ``model`` "brown"
    (OpenCV's rational model, ``dist`` = (k1, k2, p1, p2[, k3[, k4, k5, k6]]): 4, 5 or 8 coefficients, zero-extended) or
    "fisheye" (Kannala-Brandt as ``cv2.fisheye``, ``dist`` = (k1, k2, k3, k4)).  No ``dist`` is a lens without distortion."""

    def __init__(self, size, K, model="brown", dist=()):
        self.size = _size(size, "size")
        K = _finite(K, "K")
        if K.shape == (3, 3):  # the camera matrix as OpenCV has it
            if K[0, 1] != 0.0:
                raise ValueError("K: a camera matrix with skew is not supported")
            K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        if K.shape != (4,):
            raise ValueError(f"K: (fx, fy, cx, cy) or a 3x3 camera matrix expected, got shape {K.shape}")
        if not (K[0] > 0 and K[1] > 0):
            raise ValueError(f"K: positive fx, fy expected, got {K[0]}, {K[1]}")
        if model not in MODELS:
            raise ValueError(f"model: one of {MODELS} expected, got {model!r}")
        d = _finite(dist, "dist").reshape(-1)
        counts = BROWN_COUNTS if model == "brown" else FISHEYE_COUNTS
        if d.size not in counts:
            raise ValueError(f"dist: {model} takes {' / '.join(map(str, counts[1:]))} coefficients, got {d.size}")
        self.K, self.model = tuple(float(v) for v in K), model
        self.dist = tuple(float(v) for v in d)
        self.dist8 = self.dist + (0.0,) * (8 - len(self.dist))

    def distort(self, x, y):
        """Normalised pinhole coordinates (x, y) = (X/Z, Y/Z) -> source pixel position (sx, sy), fp64 arrays."""
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        r2 = x * x + y * y
        fx, fy, cx, cy = self.K
        if self.model == "brown":
            k1, k2, p1, p2, k3, k4, k5, k6 = self.dist8
            kr = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
            xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        else:
            k1, k2, k3, k4 = self.dist8[:4]
            r = np.sqrt(r2)
            t = np.arctan(r)
            t2 = t * t
            td = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where(r > 1e-8, td / r, 1.0)
            xd, yd = x * s, y * s
        return fx * xd + cx, fy * yd + cy

    def to_dict(self):
        return dict(K=list(self.K), model=self.model, dist=list(self.dist))

    def __eq__(self, other):
        return isinstance(other, CameraModel) and (self.size, self.K, self.model, self.dist8) == (
            other.size, other.K, other.model, other.dist8)

    __hash__ = None

    def __repr__(self):
        return f"CameraModel(size={self.size}, K={self.K}, model={self.model!r}, dist={self.dist})"


class Rectification:
    """What the session needs of a rectified rig: ``views`` (left, right: ``RectifiedView``), ``size`` (hs, ws) of the
    source frames, ``shape`` (h, w) of the rectified image, ``baseline`` in the unit of T, ``intrinsics`` = (f', f', cx',
    cy') of the rectified virtual camera and ``calib`` = f' * baseline.  Both views share one rectified camera (the same
    f' and the same principal point: zero disparity at infinity), which is what depth = calib / disparity assumes."""

    def __init__(self, left, right, shape, baseline):
        self.shape = _size(shape, "shape")
        self.views = (left, right)
        for name, v in zip(("left", "right"), self.views):
            if not isinstance(v.camera, CameraModel):
                raise ValueError(f"{name}: a CameraModel is expected, got {type(v.camera).__name__}")
            _rotation(v.R, f"{name} R_rect")
            P = _finite(v.P, f"{name} P", (4,))
            if not (P[0] > 0 and P[0] == P[1]):
                raise ValueError(f"{name} P: (f', f', cx', cy') with one positive focal length expected, got {P.tolist()}")
        if left.camera.size != right.camera.size:
            raise ValueError(f"size: both cameras must have the same frame size, got {left.camera.size} and {right.camera.size}")
        if tuple(left.P) != tuple(right.P):
            raise ValueError("P: both rectified views must share f', cx', cy' (zero disparity at infinity; with "
                             f"cv2.stereoRectify pass CALIB_ZERO_DISPARITY), got {tuple(left.P)} and {tuple(right.P)}")
        self.size = left.camera.size
        self.baseline = float(_finite(baseline, "baseline", ()))
        if not self.baseline > 0:
            raise ValueError(f"baseline: the rectified baseline must lie along +x (the right camera to the right of the "
                             f"left one), got {self.baseline}")
        self.intrinsics = tuple(float(v) for v in left.P)
        self.calib = self.intrinsics[0] * self.baseline

    # ---- the matrices of cv2.stereoRectify -------------------------------------------------------------
    @property
    def R1(self):
        return np.array(self.views[0].R, np.float64)

    @property
    def R2(self):
        return np.array(self.views[1].R, np.float64)

    def _P(self, tx):
        f, _, cx, cy = self.intrinsics
        return np.array([[f, 0.0, cx, tx * f], [0.0, f, cy, 0.0], [0.0, 0.0, 1.0, 0.0]])

    @property
    def P1(self):
        return self._P(0.0)

    @property
    def P2(self):
        return self._P(-self.baseline)

    @classmethod
    def from_opencv(cls, R1, R2, P1, P2, left, right, shape):
        """The four matrices of ``cv2.stereoRectify`` as they are (``left``, ``right``: the two ``CameraModel``s, ``shape``:
        the (h, w) the matrices were computed for, stereoRectify's newImageSize).  The baseline is -P2[0,3] / P2[0,0]."""
        P1, P2 = _finite(P1, "P1", (3, 4)), _finite(P2, "P2", (3, 4))
        for name, P in (("P1", P1), ("P2", P2)):
            if P[0, 1] != 0 or P[1, 0] != 0 or tuple(P[2]) != (0.0, 0.0, 1.0, 0.0) or not P[0, 0] > 0:
                raise ValueError(f"{name}: a projection matrix [[f, 0, cx, tx f], [0, f, cy, 0], [0, 0, 1, 0]] is expected")
            if abs(P[0, 0] - P[1, 1]) > 1e-9 * P[0, 0]:
                raise ValueError(f"{name}: one focal length is expected (fx' = fy'), got {P[0, 0]} and {P[1, 1]}")
        if P1[0, 3] != 0 or P1[1, 3] != 0:
            raise ValueError("P1: the left view is the reference (P1[:, 3] = 0)")
        if P2[1, 3] != 0:
            raise ValueError("P2: a baseline along y (a vertical rig) is not supported")
        baseline = -P2[0, 3] / P2[0, 0]
        if not baseline > 0:
            raise ValueError(f"P2: the rectified baseline -P2[0,3] / P2[0,0] = {baseline} must be positive (along +x: "
                             f"the right camera to the right of the left one)")
        views = [RectifiedView(_rotation(R, n), (P[0, 0], P[0, 0], P[0, 2], P[1, 2]), cam)
                 for R, n, P, cam in ((R1, "R1", P1, left), (R2, "R2", P2, right))]
        return cls(views[0], views[1], shape, baseline)

    # ---- the map function in fp64 (include/codd_hip.h: THE MAP FUNCTION) -------------------------------
    def source_points(self, view, u, v):
        """Rectified pixel positions (u, v) of ``view`` (0 left, 1 right) -> source positions (sx, sy), fp64; NaN where the
        ray does not point into the source camera's half space (W <= 0)."""
        R, (f, _, cx, cy), cam = self.views[view]
        u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
        xr, yr = (u - cx) / f, (v - cy) / f
        Rt = np.asarray(R, np.float64).T
        X, Y, W = (Rt[i, 0] * xr + Rt[i, 1] * yr + Rt[i, 2] for i in range(3))
        ok = (W > 0) & np.isfinite(W)
        Ws = np.where(ok, W, 1.0)
        sx, sy = cam.distort(X / Ws, Y / Ws)
        return np.where(ok, sx, np.nan), np.where(ok, sy, np.nan)

    def maps(self, view):
        """(map_x, map_y), fp64 [h,w], of one view: ``source_points`` on the rectified pixel grid."""
        h, w = self.shape
        vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        return self.source_points(view, uu, vv)

    # ---- the correction a live session's rectification check found (live.Epipolar, live.combine_epipolar) ---------
    def corrected(self, coef):
        """A new ``Rectification`` that takes out the vertical disparity ``dy = f' (c0 (1 + yn^2) + c1 xr yn + c2 xr + c3 yn)``
        which a session rectified with THIS one measured (``coef`` = (c0, c1, c2, c3): ``live.Epipolar.coef`` or
        ``live.combine_epipolar``).  That map says that the right rectified view shows every ray rotated by ``R_w =
        rodrigues((-c0, c1, c2))`` and magnified by ``1 + c3``; so the right view's rectifying rotation becomes ``R_w^T R2``
        (the inverse of the fitted rotation on its ``R``) and the right ``CameraModel``'s ``fx`` and ``fy`` are multiplied
        by ``1 + c3`` (the focal length the lens really has, which divides the magnification out of the map).  The left
        view, ``P``, ``shape`` and ``baseline`` are untouched.  First order: what is left is of the order ``|coef|`` times
        what was there; check again with the corrected rectification and apply ``corrected`` to the result if need be."""
        c = _finite(coef, "coef", (4,))
        if not 1.0 + c[3] > 0:
            raise ValueError(f"coef: a focal ratio 1 + c3 > 0 is expected, got c3 = {c[3]}")
        left, right = self.views
        fx, fy, cx, cy = right.camera.K
        camera = CameraModel(right.camera.size, (fx * (1.0 + c[3]), fy * (1.0 + c[3]), cx, cy), right.camera.model,
                             right.camera.dist)
        R = rodrigues([-c[0], c[1], c[2]]).T @ np.asarray(right.R, np.float64)
        return Rectification(left, RectifiedView(R, right.P, camera), self.shape, self.baseline)

    # ---- files -----------------------------------------------------------------------------------------
    def to_dict(self):
        return dict(size=list(self.size), left=self.views[0].camera.to_dict(), right=self.views[1].camera.to_dict(),
                    shape=list(self.shape), R1=self.R1.tolist(), R2=self.R2.tolist(), P1=self.P1.tolist(), P2=self.P2.tolist())

    def save(self, path):
        _save(self.to_dict(), path)


class StereoCalibration:
    """``left``, ``right``: ``CameraModel``s of one frame size; ``R`` [3,3], ``T`` [3]: ``X_right = R X_left + T``, the
    convention of ``cv2.stereoCalibrate``.  The right camera sits to the right of the left one (T mostly along -x)."""

    def __init__(self, left, right, R, T):
        for name, cam in (("left", left), ("right", right)):
            if not isinstance(cam, CameraModel):
                raise ValueError(f"{name}: a CameraModel is expected, got {type(cam).__name__}")
        if left.size != right.size:
            raise ValueError(f"size: both cameras must have the same frame size, got {left.size} and {right.size}")
        self.left, self.right, self.size = left, right, left.size
        self.R = _rotation(R, "R")
        self.T = _finite(T, "T").reshape(-1)
        if self.T.shape != (3,):
            raise ValueError(f"T: 3 entries expected, got {self.T.size}")
        if not np.linalg.norm(self.T) > 0:
            raise ValueError("T: a non-zero baseline is expected")
        self._half_rotations()  # (a vertical or mirrored rig is rejected here, not at the first frame)

    def _half_rotations(self):
        """Bouguet's method: each camera takes half of the relative rotation, then both take the smallest rotation that
        brings the baseline onto the x axis.  -> (R1, R2, baseline)."""
        r_r = rodrigues(-0.5 * rotation_vector(self.R))  # R^(-1/2): the right camera's half; the left takes its transpose
        t = r_r @ self.T  # the baseline between the two half-rotated cameras
        if abs(t[1]) > abs(t[0]):
            raise ValueError(f"T: the baseline lies mostly along y ({t.tolist()} after the half rotations): vertical "
                             f"rigs are not supported")
        if t[0] > 0:
            raise ValueError(f"T: the right camera is on the left of the left one (X_right = R X_left + T has T mostly "
                             f"along +x: {self.T.tolist()}); swap the cameras")
        nt = float(np.linalg.norm(t))
        uu = np.array([-1.0, 0.0, 0.0])
        ww = np.cross(t, uu)
        nw = float(np.linalg.norm(ww))
        if nw > 0:
            ww = ww * (np.arctan2(nw, float(t @ uu)) / nw)  # the angle between t and uu, robust near 0
        wR = rodrigues(ww)
        R1, R2 = wR @ r_r.T, wR @ r_r
        t_rect = R2 @ self.T  # X_right_rect = X_left_rect + t_rect
        if not (t_rect[0] < 0 and np.abs(t_rect[1:]).max() <= 1e-9 * nt):
            raise ValueError(f"T: the rectified baseline {(-t_rect).tolist()} does not lie along +x")
        return R1, R2, nt

    def rectify(self, shape=None, zoom=1.0, principal=None):
        """-> ``Rectification`` for a rectified image of ``shape`` (h, w) (default: the source size).  The rectified focal
        length is ``zoom * min(fx_l, fy_l, fx_r, fy_r) * min(h / hs, w / ws)``: at ``zoom`` 1 the rectified image shows the
        source at its own scale (times the resize factor), a larger ``zoom`` magnifies about the principal point, a smaller
        one shows more of the border.  ``principal`` (cx', cy'), the same in both views, defaults to the image centre
        ((w-1)/2, (h-1)/2)."""
        hs, ws = self.size
        h, w = _size(self.size if shape is None else shape, "shape")
        try:
            zoom = float(zoom)
        except (TypeError, ValueError):
            raise ValueError(f"zoom: a positive number expected, got {zoom!r}") from None
        if not (zoom > 0 and np.isfinite(zoom)):
            raise ValueError(f"zoom: a positive number expected, got {zoom!r}")
        cx, cy = ((w - 1) / 2.0, (h - 1) / 2.0) if principal is None else _finite(principal, "principal", (2,))
        f = zoom * min(self.left.K[:2] + self.right.K[:2]) * min(h / hs, w / ws)
        R1, R2, baseline = self._half_rotations()
        P = (f, f, float(cx), float(cy))
        return Rectification(RectifiedView(R1, P, self.left), RectifiedView(R2, P, self.right), (h, w), baseline)

    def to_dict(self):
        return dict(size=list(self.size), left=self.left.to_dict(), right=self.right.to_dict(), R=self.R.tolist(),
                    T=self.T.tolist())

    def save(self, path):
        _save(self.to_dict(), path)


# ---- another calibrated camera to register the depth map to -------------------------------------------------
R2_CAP = 1e6  # fold_radius2 of a lens that never folds: a radius of 1000 focal lengths, 89.94 degrees off the axis
FOOTPRINT_GRID, MAX_FOOTPRINT = 33, 4  # (CODD_ALIGN_MAX_FOOTPRINT of include/codd_hip.h)


def fold_radius2(camera, samples=4096):
    """The ``r2_max`` of codd_align_depth for ``camera``: the squared normalised radius up to which the lens model is
    monotonic.  The distorted radius of a point at radius r -- brown: r (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4
    + k6 r^6), the radial part; fisheye: theta_d(atan r) -- is scanned outward in fp64 at r = tan(theta), theta uniform in
    (0, atan sqrt(R2_CAP)]; the answer is r^2 at the last sample before it first stops increasing (a polynomial with a
    negative leading coefficient turns back there and would project far-off points into the image), or ``R2_CAP``."""
    th = np.arctan(np.sqrt(R2_CAP)) * np.arange(0, samples + 1, dtype=np.float64) / samples
    r = np.tan(th)
    r2 = r * r
    with np.errstate(all="ignore"):
        if camera.model == "brown":
            k1, k2, _, _, k3, k4, k5, k6 = camera.dist8
            rd = r * (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
        else:
            k1, k2, k3, k4 = camera.dist8[:4]
            t2 = th * th
            rd = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        rising = np.diff(rd) > 0  # (False for a NaN or an infinity on either side)
    stop = np.flatnonzero(~rising)
    if stop.size == 0:
        return R2_CAP
    if stop[0] == 0:
        raise ValueError(f"camera: the lens model does not increase from the centre on ({camera!r})")
    return float(min(r2[stop[0]], R2_CAP))


def auto_footprint(R, camera, shape, intrinsics, r2_max=None):
    """The footprint ``k`` that leaves no hole lines: ``clamp(ceil(m - 1e-3), 1, 4)``, ``m`` the largest ``|dsx/du|`` or
    ``|dsy/dv|`` of the map rectified pixel -> target position for points at infinity (``X_t = R X``: no translation), by
    central differences of half a pixel either way on a 33 x 33 grid over the rectified image of ``shape`` (h, w) with
    ``intrinsics`` (f', f', cx', cy').  Positions behind the target or beyond ``r2_max`` take no part; none at all: 1."""
    R = _rotation(R, "R")
    h, w = _size(shape, "shape")
    f, _, cx, cy = (float(v) for v in intrinsics)
    r2_max = fold_radius2(camera) if r2_max is None else float(r2_max)
    vv, uu = np.meshgrid(np.linspace(0.0, h - 1.0, FOOTPRINT_GRID), np.linspace(0.0, w - 1.0, FOOTPRINT_GRID), indexing="ij")

    def at(u, v):
        X = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)])
        Xt = np.tensordot(R, X, 1)
        ok = Xt[2] > 0
        z = np.where(ok, Xt[2], 1.0)
        x, y = Xt[0] / z, Xt[1] / z
        ok &= x * x + y * y <= r2_max
        sx, sy = camera.distort(np.where(ok, x, 0.0), np.where(ok, y, 0.0))
        return np.where(ok, sx, np.nan), np.where(ok, sy, np.nan)

    du = np.abs(at(uu + 0.5, vv)[0] - at(uu - 0.5, vv)[0])
    dv = np.abs(at(uu, vv + 0.5)[1] - at(uu, vv - 0.5)[1])
    m = np.concatenate([du[np.isfinite(du)], dv[np.isfinite(dv)]])
    if m.size == 0:
        return 1
    return int(min(max(np.ceil(m.max() - 1e-3), 1), MAX_FOOTPRINT))


class AlignTarget:
    """A calibrated camera to register the session's depth map to (``LiveSession(align_to=)``): ``camera`` its
    ``CameraModel`` and its pose ``X_target = R X_left + T``, the convention of ``cv2.stereoCalibrate`` between the left
    camera and this one.  ``X_left`` is the PHYSICAL left camera when the session has ``calibration=`` and the rectified
    left camera (the only one there is) otherwise; ``T`` is in the unit of the rig's baseline.  ``rectified=True`` says
    that the pose refers to the rectified left camera although the session has a calibration: what ``of_rig`` builds."""

    def __init__(self, camera, R=None, T=None, rectified=False):
        if not isinstance(camera, CameraModel):
            raise ValueError(f"camera: a CameraModel is expected, got {type(camera).__name__}")
        self.camera = camera
        self.R = _rotation(np.eye(3) if R is None else R, "R")
        self.T = _finite(np.zeros(3) if T is None else T, "T").reshape(-1)
        if self.T.shape != (3,):
            raise ValueError(f"T: 3 entries expected, got {self.T.size}")
        self.rectified = bool(rectified)

    @classmethod
    def of_rig(cls, rect, side):
        """The rig's own ``side`` ("left" or "right") physical camera as a target, from a ``Rectification`` alone: relative
        to the rectified left camera, left: ``R = R1^T, T = 0``; right: ``R = R2^T, T = -baseline R2^T e_x``."""
        if not isinstance(rect, Rectification):
            raise ValueError(f"rect: a Rectification is expected, got {type(rect).__name__}")
        if side not in ("left", "right"):
            raise ValueError(f"side: 'left' or 'right' expected, got {side!r}")
        if side == "left":
            return cls(rect.views[0].camera, rect.R1.T, np.zeros(3), rectified=True)
        Rt = rect.R2.T
        return cls(rect.views[1].camera, Rt, -rect.baseline * Rt[:, 0], rectified=True)

    def pose_from(self, rect=None):
        """``(R, T)`` with ``X_target = R X_rect + T``, ``X_rect`` in the rectified left camera of ``rect`` (None: the
        session has no calibration, or the target is ``rectified``: its own pose)."""
        if rect is None or self.rectified:
            return self.R.copy(), self.T.copy()
        return self.R @ rect.R1.T, self.T.copy()  # X_left = R1^T X_rect

    def to_dict(self):
        return dict(size=list(self.camera.size), camera=self.camera.to_dict(), R=self.R.tolist(), T=self.T.tolist(),
                    rectified=self.rectified)

    def save(self, path):
        path = os.fspath(path)
        ext = os.path.splitext(path)[1].lower()
        d = self.to_dict()
        if ext == ".json":
            with open(path, "w") as f:
                json.dump(d, f, indent=1)
        elif ext == ".npz":
            cam = d["camera"]
            with open(path, "wb") as f:  # (np.savez appends .npz to a name, not to a file object)
                np.savez(f, size=np.asarray(d["size"], np.int64), R=self.R, T=self.T, rectified=np.asarray(self.rectified),
                         camera_K=np.asarray(cam["K"], np.float64), camera_model=np.asarray(cam["model"]),
                         camera_dist=np.asarray(cam["dist"], np.float64))
        else:
            raise ValueError(f"align target file: .json or .npz expected, got {path!r}")

    @classmethod
    def from_dict(cls, d):
        missing = [k for k in ("size", "camera", "R", "T") if k not in d]
        if missing:
            raise ValueError(f"align target file: missing keys {missing}")
        size = tuple(int(v) for v in np.asarray(d["size"]).reshape(-1))
        c = d["camera"]
        if "K" not in c:
            raise ValueError("align target file: missing key camera K")
        camera = CameraModel(size, c["K"], str(c.get("model", "brown")), c.get("dist", ()))
        return cls(camera, d["R"], d["T"], rectified=bool(np.asarray(d.get("rectified", False))))

    @classmethod
    def load(cls, path):
        """A ``.json`` or ``.npz`` file written by ``save`` (keys size, camera {K, model, dist}, R, T[, rectified]; in an
        ``.npz`` the camera's as camera_K, camera_model, camera_dist)."""
        path = os.fspath(path)
        ext = os.path.splitext(path)[1].lower()
        if ext == ".json":
            with open(path) as f:
                return cls.from_dict(json.load(f))
        if ext == ".npz":
            with np.load(path) as z:
                d = {k: z[k] for k in z.files if not k.startswith("camera_")}
                if "camera_K" in z.files:
                    d["camera"] = dict(K=z["camera_K"], model=str(z["camera_model"]) if "camera_model" in z.files else "brown",
                                       dist=z["camera_dist"] if "camera_dist" in z.files else ())
            return cls.from_dict(d)
        raise ValueError(f"align target file: .json or .npz expected, got {path!r}")

    @classmethod
    def resolve(cls, align_to, rect=None):
        """What ``LiveSession(align_to=)`` accepts -> an ``AlignTarget``: one is taken as it is, a path is loaded, and
        "left" / "right" name the rig's own cameras, which only a session with ``calibration=`` (``rect``) has."""
        if isinstance(align_to, cls):
            return align_to
        if align_to in ("left", "right"):
            if rect is None:
                raise ValueError(f"align_to={align_to!r} names a camera of the rig: it needs calibration=")
            return cls.of_rig(rect, align_to)
        if isinstance(align_to, (str, os.PathLike)):
            return cls.load(align_to)
        raise ValueError(f"align_to: an AlignTarget, 'left', 'right' or a path to a .json / .npz file expected, got "
                         f"{type(align_to).__name__}")

    def __eq__(self, other):
        return isinstance(other, AlignTarget) and self.camera == other.camera and self.rectified == other.rectified and \
            np.array_equal(self.R, other.R) and np.array_equal(self.T, other.T)

    __hash__ = None

    def __repr__(self):
        return f"AlignTarget({self.camera!r}, R={self.R.tolist()}, T={self.T.tolist()}, rectified={self.rectified})"


# ---- files: plain keys, .json or .npz --------------------------------------------------------------------
_MATRICES = ("R", "T", "R1", "R2", "P1", "P2")


def _save(d, path):
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".json":
        with open(path, "w") as f:
            json.dump(d, f, indent=1)
    elif ext == ".npz":
        flat = {k: np.asarray(d[k], np.int64 if k in ("size", "shape") else np.float64) for k in d if k not in ("left", "right")}
        for side in ("left", "right"):
            flat[side + "_K"] = np.asarray(d[side]["K"], np.float64)
            flat[side + "_model"] = np.asarray(d[side]["model"])
            flat[side + "_dist"] = np.asarray(d[side]["dist"], np.float64)
        with open(path, "wb") as f:  # (np.savez appends .npz to a name, not to a file object)
            np.savez(f, **flat)
    else:
        raise ValueError(f"calibration file: .json or .npz expected, got {path!r}")


def _from_dict(d):
    missing = [k for k in ("size", "left", "right") if k not in d]
    if missing:
        raise ValueError(f"calibration file: missing keys {missing}")
    size = tuple(int(v) for v in np.asarray(d["size"]).reshape(-1))
    cams = []
    for side in ("left", "right"):
        c = d[side]
        cams.append(CameraModel(size, c["K"], str(c.get("model", "brown")), c.get("dist", ())))
    if "R1" in d:
        shape = tuple(int(v) for v in np.asarray(d.get("shape", size)).reshape(-1))
        return Rectification.from_opencv(d["R1"], d["R2"], d["P1"], d["P2"], cams[0], cams[1], shape)
    if "R" not in d or "T" not in d:
        raise ValueError("calibration file: R and T (a calibration) or R1, R2, P1, P2 (a rectification) expected")
    return StereoCalibration(cams[0], cams[1], d["R"], d["T"])


def load(path):
    """A ``.json`` or ``.npz`` file -> ``StereoCalibration`` (keys R, T) or ``Rectification`` (keys R1, R2, P1, P2)."""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".json":
        with open(path) as f:
            return _from_dict(json.load(f))
    if ext == ".npz":
        with np.load(path) as z:
            d = {k: z[k] for k in z.files if "_" not in k or k in _MATRICES}
            for side in ("left", "right"):
                if side + "_K" not in z.files:
                    raise ValueError(f"calibration file: missing key {side}_K")
                d[side] = dict(K=z[side + "_K"], model=str(z[side + "_model"]) if side + "_model" in z.files else "brown",
                               dist=z[side + "_dist"] if side + "_dist" in z.files else ())
        return _from_dict(d)
    raise ValueError(f"calibration file: .json or .npz expected, got {path!r}")


def resolve(calibration, shape, zoom=1.0):
    """What ``LiveSession(calibration=, zoom=)`` accepts -> the ``Rectification`` for a rectified image of ``shape``: a
    ``StereoCalibration`` (or a file holding one) is rectified with ``zoom``; a ``Rectification`` (or a file holding one)
    is taken as it is and must have been made for ``shape``, with ``zoom`` left at 1."""
    if isinstance(calibration, (str, os.PathLike)):
        calibration = load(calibration)
    if isinstance(calibration, StereoCalibration):
        return calibration.rectify(shape, zoom=zoom)
    if isinstance(calibration, Rectification):
        if calibration.shape != tuple(shape):
            raise ValueError(f"calibration: the Rectification was made for shape {calibration.shape}, the session has {tuple(shape)}")
        if float(zoom) != 1.0:
            raise ValueError("zoom: applies when the session rectifies a StereoCalibration; a Rectification is taken as it is")
        return calibration
    raise ValueError(f"calibration: a StereoCalibration, a Rectification or a path to a .json / .npz file expected, got "
                     f"{type(calibration).__name__}")
