"""Restatement of codd_epipolar_check (include/codd_hip.h) shared by the CPU and the GPU tests: grey, measure and fit once
in float64 (the reference) and once in np.float32 in the header's operation order (what the kernel computes), the
near-tie analysis that says which pixels the reference alone cannot decide, and the cases.

Reference and restatement are ONE vectorised numpy routine run at two precisions: every step the header fixes to an fp32
operation is one numpy operation on arrays of ``dtype``, which for np.float32 rounds as the hardware does (no fused
multiply-add exists in numpy); sums over pixels and the 4x4 solve are float64 in both.  u = x - d and a = u - floor(u) are
exact in fp32 for the quarter-pixel disparities of the cases, so both precisions start from the same taps.

Undecided pixels.  The measure step takes decisions on fp32 costs: the arg-min over the candidates and three gates.  With
devC = max |C32(v) - C64(v)| over all candidates of all measured pixels of a case (the restatement's own deviation), the
reference cannot decide a pixel when
    the arg-min's margin (second smallest cost - smallest) is <= 2 devC   (either cost may move by devC),
    |c0 - 27 tau| <= devC,                                                (the match gate)
    |den - 27 min_curv| <= 4 devC with den = cm - 2 c0 + cp               (the texture gate: four costs)
(|v*| == V is decided with the arg-min).  Outside these pixels the measurable mask is compared exactly; tests/test_live_epi.py
asserts on the reference alone that they are at most 1 % of a case's measurable pixels.

Cases.  The left image is an analytic texture -- a sum of 8 oriented sinusoids -- so the scene can be sampled exactly at
any real position; the disparity is piecewise constant in quarter pixels (a background and one or two fronto-parallel
boxes) plus a band of invalid values; the right image shows, at (xr, yr), the left point (xr + d, yr - dy) of the nearest
surface that lands there, dy from the planted coefficients; both images go through 8-bit quantisation and the
normalisation codd_preprocess applies.
"""
import numpy as np

RX, RY = 4, 1
NWIN = (2 * RX + 1) * (2 * RY + 1)  # 27
STD = (58.395, 57.12, 57.375)  # ops.IMAGENET_STD
MEAN = (123.675, 116.28, 103.53)
PIVOT = 1e-12
DEFAULTS = dict(range_px=2, step=2, tau=24.0, min_curv=0.5, iters=4, delta_px=0.25, min_valid=256)

PLANT_OFFSET_PX = 0.6  # a pure offset: c0 = 0.6 / fy
# ((h, w), (H, W), K, overrides of DEFAULTS, planted coefficients or None for PLANT_MIX)
K_SMALL, K_FIT = (60.0, 60.0, 19.5, 11.5), (200.0, 200.0, 79.5, 47.5)
# +-0.5 px of roll at the left and right borders (fy c2 xr = 200 * 0.00625 * 0.4), 0.3 px of pitch, a focal term of 0.19 px
# at the top and bottom rows and a small cross term: |dy| <= 1.04 px
PLANT_MIX = (0.0015, 0.002, 0.00625, 0.004)
CASES = [
    dict(crop=(24, 40), padded=(64, 64), K=K_SMALL, par=dict(min_valid=16), plant=(0.005, 0.0, 0.004, 0.0)),
    dict(crop=(37, 61), padded=(64, 64), K=(90.0, 90.0, 30.0, 18.0), par=dict(step=1, min_valid=16), plant=(0.004, 0.002, 0.006, 0.003)),
    dict(crop=(37, 61), padded=(64, 64), K=(90.0, 90.0, 30.0, 18.0), par=dict(step=3, min_valid=16), plant=(0.004, 0.002, 0.006, 0.003)),
    dict(crop=(96, 160), padded=(128, 192), K=K_FIT, par=dict(range_px=2), plant=PLANT_MIX),
    dict(crop=(96, 160), padded=(128, 192), K=K_FIT, par=dict(range_px=4), plant=PLANT_MIX),
    dict(crop=(5, 3), padded=(64, 64), K=(60.0, 60.0, 1.0, 2.0), par=dict(min_valid=16), plant=(0.0, 0.0, 0.0, 0.0)),  # nothing measurable
]
FIT_CASE = 3


def case_id(spec):
    return "%dx%d-s%d-v%d" % (spec["crop"] + (params(spec)["step"], params(spec)["range_px"]))


def params(spec):
    return dict(DEFAULTS, **spec["par"])


# ---- the scene ------------------------------------------------------------------------------------------------------
def _waves(seed=7, n=8):
    rng = np.random.default_rng(seed)
    lam = rng.uniform(5.0, 23.0, n)  # wavelengths in pixels
    th = rng.uniform(0.0, np.pi, n)
    th[::2] = rng.uniform(np.pi / 4, 3 * np.pi / 4, (n + 1) // 2)  # every other wave varies mostly along y
    return lam, th, rng.uniform(0.0, 2 * np.pi, n), rng.uniform(9.0, 14.0, n)


_WAVES = _waves()


def texture(c, y, x):
    """Grey level (float64) of the scene's surface at the real left-image position (x, y), channel c: 128 +- at most 112."""
    lam, th, ph, amp = _WAVES
    g = np.full(np.broadcast(x, y).shape, 128.0)
    for k in range(len(lam)):
        g = g + amp[k] * np.sin(2 * np.pi * (np.cos(th[k]) * x + np.sin(th[k]) * y) / lam[k] + ph[k] + 0.4 * c * (k % 3))
    return g


def model_dy(coef, K, xr_pix, y_pix):
    """dy_model (float64) at right-image column ``xr_pix`` = x - d and row ``y_pix`` of the LEFT image."""
    fx, fy, cx, cy = K
    xr, yn = (np.asarray(xr_pix, np.float64) - cx) / fx, (np.asarray(y_pix, np.float64) - cy) / fy
    return fy * (coef[0] * (1 + yn * yn) + coef[1] * xr * yn + coef[2] * xr + coef[3] * yn)


def regions(h, w):
    """(d, y0, y1, x0, x1) of the background and the fronto-parallel boxes, nearest last; quarter-pixel disparities."""
    if w < 16 or h < 8:
        return [(1.25, 0, h, 0, w)]
    out = [(min(6.25, np.floor(w / 8.0) + 0.25), 0, h, 0, w)]
    out.append((out[0][0] + 4.5, h // 5, (3 * h) // 5, w // 2, w // 2 + w // 4))
    if w >= 100:
        out.append((out[0][0] + 9.25, h // 2 + 4, h - 6, w // 4, w // 4 + w // 5))
    return out


def invalid_band(h, w):
    """Rows [y0, y1) whose disparities cycle through 0, NaN, +inf, -2."""
    y0 = max(h - 8, 0) if h >= 16 else h // 2
    return y0, min(y0 + 2, h)


def normalise(g):
    """8-bit quantisation, then the fp32 normalisation of codd_preprocess: [3,H,W] float64 grey levels -> fp32."""
    u8 = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    m, s = (np.array(v, np.float32)[:, None, None] for v in (MEAN, STD))
    return ((u8.astype(np.float32) - m) / s).astype(np.float32)


def case(spec, plant=None):
    """dict(disp fp32 [H,W], left / right fp32 [3,H,W] normalised, crop, padded, K, par, plant)."""
    (h, w), (H, W), K = spec["crop"], spec["padded"], spec["K"]
    plant = tuple(spec["plant"] if plant is None else plant)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    disp = np.zeros((H, W), np.float32)
    regs = regions(h, w)
    for d, y0, y1, x0, x1 in regs:
        disp[y0:y1, x0:x1] = d
    disp[:h, w:] = disp[:h, w - 1:w]
    disp[h:] = disp[h - 1:h]
    b0, b1 = invalid_band(h, w)
    bad = np.array([0.0, np.nan, np.inf, -2.0], np.float32)
    disp[b0:b1, :w] = bad[(np.arange(w)[None, :] + np.arange(b0, b1)[:, None]) % 4]
    left = np.stack([texture(c, yy, xx) for c in range(3)])
    right = np.zeros_like(left)
    for d, y0, y1, x0, x1 in regs:  # nearest last: it overwrites what it occludes
        yl = yy.copy()
        for _ in range(4):  # dy is defined at the left row: a contraction with factor ~1e-2
            yl = yy - model_dy(plant, K, xx, yl)
        xl = xx + d
        inside = (xl >= x0 - 0.5) & (xl < x1 - 0.5) & (yl >= y0 - 0.5) & (yl < y1 - 0.5)
        if (y0, y1, x0, x1) == (0, h, 0, w):
            inside = np.ones_like(inside)  # the background continues behind the borders
        for c in range(3):
            right[c][inside] = texture(c, yl, xl)[inside]
    return dict(disp=disp, left=normalise(left), right=normalise(right), crop=(h, w), padded=(H, W), K=K,
                par=params(spec), plant=plant)


# ---- grey, measure, fit at one precision --------------------------------------------------------------------------------
def grey(c, dtype):
    h, w = c["crop"]
    s = np.array(STD, np.float32).astype(dtype)
    third = (np.float32(1.0) / np.float32(3.0)).astype(dtype) if dtype == np.float32 else np.float64(1.0) / 3.0
    out = []
    for img in (c["left"], c["right"]):
        p = img[:, :h, :w].astype(dtype)
        out.append(((p[0] * s[0] + p[1] * s[1]) + p[2] * s[2]) * third)
    assert out[0].dtype == dtype
    return out


def candidate_order(V):
    """Candidates in the order that resolves ties: the smaller |v|, then the smaller v."""
    return [0] + [s * m for m in range(1, V + 1) for s in (-1, 1)]


def measure(c, dtype, **over):
    """dict(dy [h,w] of ``dtype`` (NaN: not measured or not measurable), idx (ys, xs) of the pixels whose taps stay inside
    the crop, C [n, 2V+1] their costs (column v + V), margin / c0 / den [n]: what the decisions were taken on)."""
    par = dict(c["par"], **over)
    h, w = c["crop"]
    V, step = par["range_px"], par["step"]
    gL, gR = grey(c, dtype)
    ys, xs = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    d = c["disp"][ys, xs]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d > 0)
        u = (xs.astype(np.float32) - np.where(ok, d, np.float32(0))).astype(np.float32)  # one fp32 subtraction
        fl = np.floor(u)
        ok &= (xs - RX >= 0) & (xs + RX < w) & (ys - RY - V >= 0) & (ys + RY + V < h) & (fl >= RX)
        ok &= np.where(ok, fl, 0).astype(np.int64) + RX + 1 < w
    ys, xs, u, fl = ys[ok], xs[ok], u[ok], fl[ok]
    f = fl.astype(np.int64)
    a = (u - fl).astype(np.float32).astype(dtype)
    b = (np.float32(1.0) - a.astype(np.float32)).astype(dtype) if dtype == np.float32 else 1.0 - a
    n = ys.size
    dy = np.full((h, w), np.nan, dtype)
    if n == 0:
        z = np.zeros(0, dtype)
        return dict(dy=dy, idx=(ys, xs), C=np.zeros((0, 2 * V + 1), dtype), margin=z, c0=z, den=z, vstar=np.zeros(0, np.int64))
    cols = np.arange(-RX, RX + 1)
    R = {}
    for r in range(-RY - V, RY + V + 1):
        q0, q1 = gR[(ys + r)[:, None], f[:, None] + cols], gR[(ys + r)[:, None], f[:, None] + cols + 1]
        R[r] = q0 * b[:, None] + q1 * a[:, None]
    L = {j: gL[(ys + j)[:, None], xs[:, None] + cols] for j in range(-RY, RY + 1)}
    C = np.zeros((n, 2 * V + 1), dtype)
    for v in range(-V, V + 1):
        rows = []
        for j in range(-RY, RY + 1):
            t = np.abs(L[j] - R[j + v])
            s = t[:, 0]
            for i in range(1, 2 * RX + 1):
                s = s + t[:, i]
            rows.append(s)
        C[:, v + V] = (rows[0] + rows[1]) + rows[2]
    assert C.dtype == dtype
    order = np.array(candidate_order(V))
    Co = C[:, order + V]
    vstar = order[np.argmin(Co, axis=1)]  # the first minimum in tie order
    srt = np.sort(C, axis=1)
    margin = srt[:, 1] - srt[:, 0]
    inner = np.abs(vstar) < V
    vi = np.where(inner, vstar, 0)
    rows_ = np.arange(n)
    cm, c0, cp = C[rows_, vi + V - 1], C[rows_, vi + V], C[rows_, vi + V + 1]
    two, thr_c, thr_t = dtype(2.0), dtype(np.float32(27.0) * np.float32(par["min_curv"])), dtype(np.float32(27.0) * np.float32(par["tau"]))
    den = (cm - two * c0) + cp
    good = inner & (den > thr_c) & (den > 0) & (c0 <= thr_t)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = vi.astype(dtype) + (cm - cp) / (two * den)
    dy[ys[good], xs[good]] = val[good]
    return dict(dy=dy, idx=(ys, xs), C=C, margin=margin, c0=c0, den=den, vstar=vstar, inner=inner, good=good,
                thr=(thr_c, thr_t))


def terms(c, dy_map, coef, dtype):
    """(ys, xs, dy, p [4,n], e) of the measurable pixels of ``dy_map`` in the header's operation order."""
    h, w = c["crop"]
    fx, fy, cx, cy = (dtype(np.float32(v)) for v in c["K"])
    ys, xs = np.nonzero(~np.isnan(dy_map[:h, :w]))
    dy = dy_map[ys, xs].astype(dtype)
    d = c["disp"][ys, xs]
    u = (xs.astype(np.float32) - d).astype(np.float32).astype(dtype) if dtype == np.float32 else xs.astype(np.float64) - d.astype(np.float64)
    xr, yn = (u - cx) / fx, (ys.astype(dtype) - cy) / fy
    one = dtype(1.0)
    p = np.stack([fy * (one + yn * yn), fy * (xr * yn), fy * xr, fy * yn])
    cc = [dtype(np.float32(v)) if dtype == np.float32 else np.float64(v) for v in coef]
    e = dy - (((cc[0] * p[0] + cc[1] * p[1]) + cc[2] * p[2]) + cc[3] * p[3])
    assert p.dtype == dtype and e.dtype == dtype
    return ys, xs, dy, p, e


def solve(A, b):
    """(c, ok): 4x4 Cholesky in float64 with the header's pivot rule."""
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        return np.zeros(4), False
    floor_ = PIVOT * np.trace(A)
    L = np.zeros((4, 4))
    for j in range(4):
        dd = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not dd > floor_:
            return np.zeros(4), False
        L[j, j] = np.sqrt(dd)
        for i in range(j + 1, 4):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.linalg.solve(L, b)
    cc = np.linalg.solve(L.T, y)
    return (cc, True) if np.all(np.isfinite(cc)) else (np.zeros(4), False)


def normal_equations(p, wt, dy):
    """A [4,4], b [4]: products in the dtype of ``p``, sums in float64."""
    q = wt * p
    A = np.zeros((4, 4))
    for i in range(4):
        for j in range(i, 4):
            A[i, j] = A[j, i] = (q[i] * p[j]).astype(np.float64).sum()
    return A, np.array([(q[i] * dy).astype(np.float64).sum() for i in range(4)])


def fit(c, dy_map, dtype, **over):
    """The IRLS of the header on ``dy_map``: dict(coef, ok, n, inliers, rms, rms_fit, steps, A, b)."""
    par = dict(c["par"], **over)
    delta = dtype(np.float32(par["delta_px"]))
    coef, alive, steps = np.zeros(4), True, 0
    A, b = np.zeros((4, 4)), np.zeros(4)
    for k in range(par["iters"]):
        _, _, dy, p, e = terms(c, dy_map, coef, dtype)
        wt = np.ones_like(dy) if k == 0 else dtype(1.0) / (dtype(1.0) + (e * e) / (delta * delta))
        A, b = normal_equations(p, wt, dy)
        if not alive:
            continue
        new, ok = solve(A, b) if dy.size >= par["min_valid"] else (None, False)
        if ok:
            coef, steps = new, steps + 1
        else:
            alive = False
    _, _, dy, p, e = terms(c, dy_map, coef, dtype)
    inl = np.abs(e) <= delta
    n, ni = dy.size, int(inl.sum())
    return dict(coef=coef, ok=alive, n=n, inliers=ni, steps=steps, A=A, b=b,
                rms=float(np.sqrt((dy * dy).astype(np.float64).sum() / n)) if n else 0.0,
                rms_fit=float(np.sqrt((e[inl] * e[inl]).astype(np.float64).sum() / ni)) if ni else 0.0)


# ---- the reference of a case, the restatement's deviation, the undecided pixels ---------------------------------------
def reference(c):
    """Everything the tests compare against, computed once per case: m64 / m32 (measure), f64 / f32 (fit), devC, dev_dy,
    dev_coef, undecided [h,w] bool, measurable64 [h,w] bool."""
    h, w = c["crop"]
    m64, m32 = measure(c, np.float64), measure(c, np.float32)
    ys, xs = m64["idx"]
    devC = float(np.abs(m32["C"].astype(np.float64) - m64["C"]).max()) if ys.size else 0.0
    und = np.zeros((h, w), bool)
    if ys.size:
        thr_c, thr_t = m64["thr"]
        u = m64["margin"] <= 2 * devC
        u |= m64["inner"] & ((np.abs(m64["c0"] - thr_t) <= devC) | (np.abs(m64["den"] - thr_c) <= 4 * devC))
        und[ys[u], xs[u]] = True
    f64, f32 = fit(c, m64["dy"], np.float64), fit(c, m32["dy"], np.float32)
    both = ~np.isnan(m64["dy"]) & ~np.isnan(m32["dy"]) & ~und
    dev_dy = float(np.abs(m32["dy"].astype(np.float64) - m64["dy"])[both].max()) if both.any() else 0.0
    return dict(m64=m64, m32=m32, f64=f64, f32=f32, devC=devC, dev_dy=dev_dy, undecided=und,
                dev_coef=float(np.abs(f32["coef"] - f64["coef"]).max()), measurable64=~np.isnan(m64["dy"]))
