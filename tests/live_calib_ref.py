"""numpy restatements of the calibration map function (include/codd_hip.h: THE MAP FUNCTION) and of
StereoCalibration.rectify (Bouguet's method), written from the header's text and the method's description, not from
codd_amd/calibration.py or the kernels: the map in fp64 (``map_fp64``), the host's fp32 constants (``constants``) and the
map in the header's fp32 operation order (``map_fp32``), whose own deviation from fp64 sets the bound of the GPU test.
A view is a plain dict: R [3,3] (R_rect), f, cx, cy (the rectified camera), K (fx, fy, cx, cy), dist (8 numbers, zero-
extended), model ("brown" | "fisheye")."""
import numpy as np

RIG_OM = (0.02, -0.035, 0.015)  # the relative rotation of the test rig (rotation vector, rad) and its baseline
RIG_T = (-0.12, 0.004, -0.006)
BROWN = (-0.28, 0.09, 1.2e-3, -8e-4, -0.012, 0.02, 0.01, 1e-3)
FISHEYE = (-0.03, 8e-3, -4e-3, 9e-4)


def rot(om):
    """Rotation vector -> matrix, as the exponential series' closed form (Rodrigues)."""
    om = np.asarray(om, np.float64)
    th = np.sqrt(om @ om)
    if th == 0:
        return np.eye(3)
    n = om / th
    S = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * np.outer(n, n)


def rotvec(R):
    """Matrix -> rotation vector, for angles well inside (0, pi) (the test rigs)."""
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-12:
        return np.zeros(3)
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def rectify_ref(Kl, Kr, R, T, size, shape, zoom=1.0, principal=None):
    """Bouguet: split R in half between the cameras, then the smallest rotation that brings the baseline onto -x (the right
    camera to the right).  -> (R1, R2, f, cx, cy, baseline)."""
    R, T = np.asarray(R, np.float64), np.asarray(T, np.float64)
    half = rot(-0.5 * rotvec(R))  # applied to the right camera; its transpose to the left one
    t = half @ T
    e = np.array([-1.0, 0.0, 0.0])
    axis = np.cross(t, e)
    s, c = np.linalg.norm(axis), t @ e
    align = rot(axis / s * np.arctan2(s, c)) if s > 0 else np.eye(3)
    (hs, ws), (h, w) = size, shape
    f = zoom * min(Kl[0], Kl[1], Kr[0], Kr[1]) * min(h / hs, w / ws)
    cx, cy = ((w - 1) / 2, (h - 1) / 2) if principal is None else principal
    return align @ half.T, align @ half, f, cx, cy, np.linalg.norm(T)


def distort(view, x, y):
    """Normalised (x, y) -> source pixel (sx, sy), fp64, as the header states the two models."""
    k = view["dist"]
    r2 = x ** 2 + y ** 2
    if view["model"] == "brown":
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        kr = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
        yd = y * kr + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    else:
        r = np.sqrt(r2)
        t = np.arctan(r)
        td = t * (1 + k[0] * t ** 2 + k[1] * t ** 4 + k[2] * t ** 6 + k[3] * t ** 8)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(r > 1e-8, td / r, 1.0)
        xd, yd = x * s, y * s
    fx, fy, cx, cy = view["K"]
    return fx * xd + cx, fy * yd + cy


def map_fp64(view, u, v):
    """(sx, sy) and W of rectified pixels (u, v) in fp64; NaN where W <= 0."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    xr, yr = (u - view["cx"]) / view["f"], (v - view["cy"]) / view["f"]
    Rt = np.asarray(view["R"], np.float64).T
    X, Y, W = (Rt[i, 0] * xr + Rt[i, 1] * yr + Rt[i, 2] for i in range(3))
    ok = W > 0
    Wd = np.where(ok, W, 1.0)
    sx, sy = distort(view, X / Wd, Y / Wd)
    return np.where(ok, sx, np.nan), np.where(ok, sy, np.nan), W


def grid(shape):
    h, w = shape
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return uu, vv


def constants(view):
    """The fp32 constants as the header defines them: fp64, each rounded once."""
    R, f, cx, cy = np.asarray(view["R"], np.float64), view["f"], view["cx"], view["cy"]
    m = np.empty(9)
    for i in range(3):
        m[3 * i], m[3 * i + 1] = R[0, i] / f, R[1, i] / f
        m[3 * i + 2] = R[2, i] - (R[0, i] * cx + R[1, i] * cy) / f
    return m.astype(np.float32), np.asarray(view["K"], np.float64).astype(np.float32), np.asarray(view["dist"], np.float64).astype(np.float32)


def _fma(a, b, c):
    """One fused multiply-add in fp32: the product of two fp32 numbers is exact in fp64, the sum is rounded to fp64 and then
    to fp32 (a double rounding that differs from the fused result in rare ties only; this function sets a bound, no bits)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def map_fp32(view, u, v):
    """The header's fp32 operation order in numpy float32 -> (sx, sy) fp32."""
    f32 = np.float32
    m, K, k = constants(view)
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    X = _fma(m[0], u, _fma(m[1], v, m[2]))
    Y = _fma(m[3], u, _fma(m[4], v, m[5]))
    W = _fma(m[6], u, _fma(m[7], v, m[8]))
    ok = (W > 0) & np.isfinite(W)
    with np.errstate(all="ignore"):
        iw = f32(1) / np.where(ok, W, f32(1))
        x, y = X * iw, Y * iw
        xx, yy, r2 = x * x, y * y, _fma(y, y, x * x)
        if view["model"] == "brown":
            num = _fma(_fma(_fma(k[4], r2, k[1]), r2, k[0]), r2, f32(1))
            den = _fma(_fma(_fma(k[7], r2, k[6]), r2, k[5]), r2, f32(1))
            kr, xy2 = num / den, (x + x) * y
            xd = _fma(x, kr, _fma(k[2], xy2, k[3] * _fma(f32(2), xx, r2)))
            yd = _fma(y, kr, _fma(k[3], xy2, k[2] * _fma(f32(2), yy, r2)))
        else:
            r = np.sqrt(r2)
            t = np.arctan(r)
            t2 = t * t
            td = t * _fma(_fma(_fma(_fma(k[3], t2, k[2]), t2, k[1]), t2, k[0]), t2, f32(1))
            s = np.where(r > f32(1e-8), td / np.where(r > 0, r, f32(1)), f32(1))
            xd, yd = x * s, y * s
        sx, sy = _fma(K[0], xd, K[2]), _fma(K[1], yd, K[3])
    assert sx.dtype == sy.dtype == np.float32
    return np.where(ok, sx, f32(np.nan)), np.where(ok, sy, f32(np.nan))


def make_rig(model, size, jitter=1.0):
    """The cameras of the test rig for source frames of ``size``: a different K and dist per view, f about 0.9 ws (about
    60 px at the small shapes).  -> ((K, dist) left, (K, dist) right, R, T)."""
    hs, ws = size
    base = np.array(BROWN if model == "brown" else FISHEYE)
    f = 0.9 * ws
    Kl = (f * 1.01, f * 0.985, (ws - 1) / 2 + 0.013 * ws, (hs - 1) / 2 - 0.011 * hs)
    Kr = (f * 0.995, f * 1.02, (ws - 1) / 2 - 0.009 * ws, (hs - 1) / 2 + 0.016 * hs)
    return (Kl, tuple(base)), (Kr, tuple(base * 1.07 * jitter)), rot(RIG_OM), np.array(RIG_T)


def as_view(rv):
    """A codd_amd.calibration.RectifiedView as the plain dict this module takes."""
    return dict(R=np.asarray(rv.R, np.float64), f=rv.P[0], cx=rv.P[2], cy=rv.P[3], K=rv.camera.K, dist=rv.camera.dist8,
                model=rv.camera.model)
