"""Restatement of codd_ground_plane (include/codd_hip.h) shared by the CPU and the GPU tests: fit, metric plane, labels,
heights and grid once in float64 (the reference) and once in np.float32 in the header's operation order (what the kernel
computes), the analysis that says which pixels the reference alone cannot decide, and the cases.

Reference and restatement are ONE vectorised numpy routine run at two precisions: every step the header fixes to an fp32
operation is one numpy operation on arrays of ``dtype``, which for np.float32 rounds as the hardware does (no fused
multiply-add exists in numpy); sums over pixels, the 3x3 solve and the metric plane are float64 in both.  Parameters are
rounded to fp32 first in both (the entry takes floats), so thresholds are the same numbers.

Undecided pixels.  The last pass takes discrete decisions on fp32 values: the label bands (|e| against tol_px, |hgt|
against ground_tol, hgt against clearance) and the cell index (gx / cell + gw / 2 and gz / cell against an integer).  With
dev_e, dev_h, dev_u the largest deviations of the restatement's e, hgt and cell coordinates from the reference's over the
valid pixels of a case, either side of a comparison may move by that much: a pixel is undecided when a compared value
lies within 2 dev of its threshold.  Outside these pixels labels are compared exactly; tests/test_live_ground.py asserts
on the reference alone that they are fewer than 1 % of a case's valid pixels.

Scenes, in closed form: a camera of height ``cam_h`` above a floor, pitched down and rolled, sees the plane d = c.p with
c = -(calib / cam_h) (u_x / fx, u_y / fy, u_z), u the up vector in camera coordinates; where that disparity is not positive
there is sky (disp = 0); fronto-parallel boxes (constant disparity: that of the floor under the middle of their bottom
edge) stand on the floor; a pit lies below it; a band of NaN crosses the image; Gaussian noise of 0.05 px is added to every
valid pixel; the padding holds 99, which a kernel that reads outside the crop would fit.
"""
import numpy as np

PIVOT = 1e-12
NOISE_PX = 0.05
DEFAULTS = dict(step=2, iters=8, delta_px=0.25, delta0_px=4.0, asym=4.0, min_valid=256, max_tilt_deg=45.0, tol_px=0.5,
                ground_tol=0.05, clearance=2.0, cell=0.25)
FLOOR, OBSTACLE, OVERHEAD, BELOW, INVALID = 0, 1, 2, 3, 255
UP = (0.0, -1.0, 0.0)
K_FIT, CALIB_FIT, CAM_H, PITCH, ROLL = (120.0, 120.0, 80.0, 40.0), 60.0, 1.2, 0.15, 0.03

# boxes: (x0, x1, y_top, y_bottom), columns [x0, x1), rows [y_top, y_bottom)
SCENES = dict(
    easy=dict(boxes=[(96, 132, 30, 64)], pit=(20, 44, 80, 88)),
    clutter=dict(boxes=[(8, 52, 24, 66), (60, 104, 30, 80), (112, 156, 26, 58)]),
    wall=dict(boxes=[(0, 160, 0, 56)]),
    heavy=dict(boxes=[(6, 78, 6, 90), (88, 154, 10, 84)]),
    plain=dict(boxes=[]),
    odd=dict(boxes=[(34, 52, 12, 28)]),
    none=dict(boxes=[], nothing=True),
    large=dict(boxes=[(150, 220, 90, 200)]),
)
BIG = dict(crop=(96, 160), padded=(128, 192), K=K_FIT, calib=CALIB_FIT, cam_h=CAM_H, pitch=PITCH, roll=ROLL)
SEED_HEAVY = dict(height=1.0, pitch=PITCH + 0.08)  # the mount as the integrator believes it: both wrong
CASES = [
    dict(BIG, name="easy", scene="easy", par={}, seed=None, grid=((32, 32), 0.25)),
    dict(BIG, name="clutter", scene="clutter", par={}, seed=None, grid=((7, 5), 1.0)),
    dict(BIG, name="clutter-seeded", scene="clutter", par={}, seed=dict(height=CAM_H, pitch=PITCH), grid=None),
    dict(BIG, name="wall", scene="wall", par=dict(clearance=0.6), seed=None, grid=((32, 32), 0.25)),
    dict(BIG, name="wall-seeded", scene="wall", par={}, seed=dict(height=CAM_H, pitch=PITCH), grid=((7, 5), 1.0)),
    dict(BIG, name="heavy-seeded", scene="heavy", par={}, seed=SEED_HEAVY, grid=((32, 32), 0.25)),
    dict(BIG, name="heavy-unseeded", scene="heavy", par={}, seed=None, grid=((32, 32), 0.25), fails="tilt"),
    dict(crop=(24, 40), padded=(64, 64), K=(40.0, 40.0, 20.0, 8.0), calib=20.0, cam_h=1.0, pitch=0.1, roll=0.0, name="plain",
         scene="plain", par=dict(min_valid=16), seed=None, grid=((7, 5), 1.0)),
    dict(crop=(37, 61), padded=(64, 64), K=(60.0, 60.0, 30.0, 14.0), calib=30.0, cam_h=1.0, pitch=0.12, roll=-0.04,
         name="odd-s1", scene="odd", par=dict(step=1, min_valid=16), seed=None, grid=((32, 32), 0.25)),
    dict(crop=(37, 61), padded=(64, 64), K=(60.0, 60.0, 30.0, 14.0), calib=30.0, cam_h=1.0, pitch=0.12, roll=-0.04,
         name="odd-s3", scene="odd", par=dict(step=3, min_valid=16), seed=None, grid=None),
    dict(crop=(5, 3), padded=(64, 64), K=(60.0, 60.0, 1.0, 2.0), calib=30.0, cam_h=1.0, pitch=0.1, roll=0.0, name="none",
         scene="none", par=dict(min_valid=16), seed=None, grid=((7, 5), 1.0), fails="nothing"),
    # 210 fit pixels pass min_valid at every step, the 180 inliers of the final plane do not: ok = 0 is known only when the
    # last pass's sums are in, after the labels and the grid have been written
    dict(crop=(37, 61), padded=(64, 64), K=(60.0, 60.0, 30.0, 14.0), calib=30.0, cam_h=1.0, pitch=0.12, roll=-0.04,
         name="few-inliers", scene="odd", par=dict(step=3, min_valid=200), seed=None, grid=((7, 5), 1.0), fails="inliers"),
    # 260 x 256 = 66560 pixels: with step 1 both the fit passes' and the last pass's stride loops (256 workgroups x 256
    # threads = 65536 elements a trip) take two trips; on every shape above they take one
    dict(crop=(260, 256), padded=(320, 256), K=(200.0, 200.0, 128.0, 100.0), calib=100.0, cam_h=1.5, pitch=0.2, roll=0.02,
         name="two-trips", scene="large", par=dict(step=1, iters=3), seed=None, grid=((32, 32), 0.25)),
]


def case_id(spec):
    return spec["name"]


def params(spec):
    return dict(DEFAULTS, **spec["par"], **({} if spec["grid"] is None else dict(cell=spec["grid"][1])))


def up_vector(pitch, roll=0.0, up=UP):
    """The unit up vector in camera coordinates of a camera pitched down by ``pitch`` and rolled by ``roll`` (radians)."""
    u = np.array(up, np.float64)
    u = np.array([u[0], u[1] * np.cos(pitch) - u[2] * np.sin(pitch), u[1] * np.sin(pitch) + u[2] * np.cos(pitch)])
    return np.array([u[0] * np.cos(roll) - u[1] * np.sin(roll), u[0] * np.sin(roll) + u[1] * np.cos(roll), u[2]])


def plane_coef(height, K, calib, u):
    """c of the floor a camera ``height`` above it sees, u its unit up vector: the closed form of live.ground_seed."""
    return -(calib / height) * np.array([u[0] / K[0], u[1] / K[1], u[2]])


def plane_disp(coef, K, xs, ys):
    return coef[0] * (np.asarray(xs, np.float64) - K[2]) + coef[1] * (np.asarray(ys, np.float64) - K[3]) + coef[2]


def case(spec):
    """dict(disp fp32 [H,W], crop, padded, K, calib, par, seed (float64 [3] or None), grid, plant (the planted c), floor
    [h,w] bool (the pixels that show the floor), name, fails (None, or the rule through which ok must come back 0))."""
    (h, w), (H, W), K, calib = spec["crop"], spec["padded"], spec["K"], spec["calib"]
    sc = SCENES[spec["scene"]]
    plant = plane_coef(spec["cam_h"], K, calib, up_vector(spec["pitch"], spec["roll"]))
    yy, xx = np.mgrid[0:h, 0:w]
    d = plane_disp(plant, K, xx, yy)
    floor = d > 0.25  # (the far floor, below a quarter pixel, is sky too: 1 / d has no use there)
    d = np.where(floor, d, 0.0)
    for x0, x1, y0, y1 in sc["boxes"]:
        db = plane_disp(plant, K, 0.5 * (x0 + x1 - 1), y1 - 1)
        box = np.zeros((h, w), bool)
        box[y0:y1, x0:x1] = True
        box &= db > d  # (the box hides the floor behind it, not the floor in front of it)
        d = np.where(box, db, d)
        floor &= ~box
    if sc.get("pit"):
        x0, x1, y0, y1 = sc["pit"]
        d[y0:y1, x0:x1] -= 1.5
        floor[y0:y1, x0:x1] = False
    rng = np.random.default_rng(11)
    d = np.where(d > 0, d + NOISE_PX * rng.standard_normal((h, w)), d)
    if h >= 16:  # a band of NaN across the floor
        d[h - 12:h - 10, :] = np.nan
        floor[h - 12:h - 10, :] = False
    if sc.get("nothing"):
        d = np.array([0.0, np.nan, np.inf, -2.0])[(xx + yy) % 4]
        floor[:] = False
    disp = np.full((H, W), 99.0, np.float32)
    disp[:h, :w] = d.astype(np.float32)
    seed = None
    if spec["seed"] is not None:
        seed = plane_coef(spec["seed"]["height"], K, calib, up_vector(spec["seed"]["pitch"]))
    return dict(disp=disp, crop=(h, w), padded=(H, W), K=K, calib=calib, par=params(spec), seed=seed, grid=spec["grid"],
                plant=plant, floor=floor, name=spec["name"], fails=spec.get("fails"))


# ---- fit, metric plane, pixels at one precision -------------------------------------------------------------------------
def _f(dtype, v):
    """A parameter as the entry receives it (a float), in the working precision."""
    return dtype(np.float32(v))


def valid_mask(c):
    h, w = c["crop"]
    d = c["disp"][:h, :w]
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def residual(c, coef, dtype, ys, xs):
    """(p0, p1, d, e) at the pixels (ys, xs) in the header's operation order."""
    fx, fy, cx, cy = (_f(dtype, v) for v in c["K"])
    d = c["disp"][ys, xs].astype(dtype)
    p0, p1 = xs.astype(dtype) - cx, ys.astype(dtype) - cy
    cc = [dtype(np.float32(v)) if dtype == np.float32 else np.float64(v) for v in coef]
    e = d - ((cc[0] * p0 + cc[1] * p1) + cc[2])
    assert e.dtype == dtype
    return p0, p1, d, e


def solve(A, b):
    """(c, ok): 3x3 Cholesky in float64 with the header's pivot rule."""
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        return np.zeros(3), False
    floor_ = PIVOT * np.trace(A)
    L = np.zeros((3, 3))
    for j in range(3):
        dd = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not dd > floor_:
            return np.zeros(3), False
        L[j, j] = np.sqrt(dd)
        for i in range(j + 1, 3):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    cc = np.linalg.solve(L.T, np.linalg.solve(L, b))
    return (cc, True) if np.all(np.isfinite(cc)) else (np.zeros(3), False)


def normal_equations(p0, p1, wt, d):
    """A [3,3], b [3]: products in the dtype of the terms, sums in float64."""
    q0, q1 = wt * p0, wt * p1
    s = lambda v: float(v.astype(np.float64).sum())  # noqa: E731
    A = np.array([[s(q0 * p0), s(q0 * p1), s(q0)], [0.0, s(q1 * p1), s(q1)], [0.0, 0.0, s(wt)]])
    A = A + np.triu(A, 1).T
    return A, np.array([s(q0 * d), s(q1 * d), s(wt * d)])


def weights(c, e, k, dtype, **over):
    par = dict(c["par"], **over)
    f32 = np.float32
    if dtype == np.float32:  # s_k, s_k / asym and their squares are fp32 operations of the entry
        sk = max(f32(par["delta_px"]), f32(par["delta0_px"]) * f32(0.5 ** k))
        sp = sk / f32(par["asym"])
        s2n, s2p = sk * sk, sp * sp
    else:
        sk = max(float(f32(par["delta_px"])), float(f32(par["delta0_px"])) * 0.5 ** k)
        sp = sk / float(f32(par["asym"]))
        s2n, s2p = np.float64(sk * sk), np.float64(sp * sp)
    one = dtype(1.0)
    wt = one / (one + (e * e) / np.where(e > 0, s2p, s2n).astype(dtype))
    assert wt.dtype == dtype
    return wt


def fit(c, dtype, **over):
    """The IRLS of the header: dict(coef, alive, n, inliers, rms, steps, A, b, idx)."""
    par = dict(c["par"], **over)
    h, w = c["crop"]
    step = par["step"]
    ys, xs = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
    v = valid_mask(c)[ys, xs]
    ys, xs = ys[v], xs[v]
    n = ys.size
    seeded = c["seed"] is not None
    coef = np.array(c["seed"], np.float64) if seeded else np.zeros(3)
    alive, steps = True, 0
    A, b = np.zeros((3, 3)), np.zeros(3)
    for k in range(par["iters"]):
        p0, p1, d, e = residual(c, coef, dtype, ys, xs)
        if k == 0 and not seeded:
            wt = (ys.astype(dtype) >= _f(dtype, c["K"][3])).astype(dtype)
        else:
            wt = weights(c, e, k, dtype, **over)
        A, b = normal_equations(p0, p1, wt, d)
        if not alive:
            continue
        new, ok = solve(A, b) if n >= par["min_valid"] else (None, False)
        if ok:
            coef, steps = new, steps + 1
        else:
            alive = False
            if steps == 0:
                coef = np.zeros(3)
    _, _, _, e = residual(c, coef, dtype, ys, xs)
    inl = np.abs(e) <= _f(dtype, par["delta_px"])
    ni = int(inl.sum())
    return dict(coef=coef, alive=alive, n=n, inliers=ni, steps=steps, A=A, b=b, idx=(ys, xs),
                rms=float(np.sqrt((e[inl] * e[inl]).astype(np.float64).sum() / ni)) if ni else 0.0)


def metric(c, f, up=UP, **over):
    """The metric plane of a fit, float64: dict(ok, normal, Hc, tilt, forward, right)."""
    par = dict(c["par"], **over)
    z = np.zeros(3)
    out = dict(ok=False, normal=z.copy(), Hc=0.0, tilt=0.0, forward=z.copy(), right=z.copy())
    if not f["alive"]:
        return out
    fx, fy = float(np.float32(c["K"][0])), float(np.float32(c["K"][1]))
    N = np.array([f["coef"][0] * fx, f["coef"][1] * fy, f["coef"][2]])
    nn = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
    if not (nn > 0 and np.isfinite(nn)):
        return out
    Hc = float(np.float32(c["calib"])) / nn
    if not (Hc > 0 and np.isfinite(Hc)):
        return out
    n = -N / nn
    u = np.array([float(np.float32(v)) for v in up])
    u = u / np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    tilt = float(np.degrees(np.arccos(np.clip((n[0] * u[0] + n[1] * u[1]) + n[2] * u[2], -1.0, 1.0))))
    ok = tilt <= float(np.float32(par["max_tilt_deg"]))
    g = np.array([-n[2] * n[0], -n[2] * n[1], 1.0 - n[2] * n[2]])
    gl = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    fwd, right = z.copy(), z.copy()
    if gl < 1e-3:
        ok = False
    else:
        fwd = g / gl
        right = np.cross(fwd, n)
    ok = ok and f["inliers"] >= par["min_valid"]
    return dict(ok=bool(ok), normal=n, Hc=Hc, tilt=tilt, forward=fwd, right=right)


def pixels(c, f, m, dtype, **over):
    """Labels, heights and the grid under the fit ``f`` and its metric plane ``m``: dict(labels, height, e, u, v (the cell
    coordinates before floorf, NaN where the pixel does not go to the grid), grid_count, grid_height)."""
    par = dict(c["par"], **over)
    h, w = c["crop"]
    labels = np.full((h, w), INVALID, np.uint8)
    height = np.full((h, w), np.nan, dtype)
    e_map, u_map, v_map = (np.full((h, w), np.nan, dtype) for _ in range(3))
    gc = gh_ = None
    if c["grid"] is not None:
        (gh, gw), _ = c["grid"]
        gc, gh_ = np.zeros((2, gh, gw), np.int32), np.zeros((gh, gw), np.float32)
    out = dict(labels=labels, height=height, e=e_map, u=u_map, v=v_map, grid_count=gc, grid_height=gh_)
    if not m["ok"]:
        return out
    ys, xs = np.nonzero(valid_mask(c))
    p0, p1, d, e = residual(c, f["coef"], dtype, ys, xs)
    Hc = dtype(np.float32(m["Hc"])) if dtype == np.float32 else np.float64(m["Hc"])
    hgt = (Hc * e) / d
    tol, gtol, clr = _f(dtype, par["tol_px"]), _f(dtype, par["ground_tol"]), _f(dtype, par["clearance"])
    lab = np.where((np.abs(e) <= tol) | (np.abs(hgt) <= gtol), FLOOR,
                   np.where(hgt > clr, OVERHEAD, np.where(hgt > 0, OBSTACLE, BELOW))).astype(np.uint8)
    labels[ys, xs], height[ys, xs], e_map[ys, xs] = lab, hgt, e
    if gc is not None:
        fx, fy = _f(dtype, c["K"][0]), _f(dtype, c["K"][1])
        r, fw = ([dtype(np.float32(t)) if dtype == np.float32 else np.float64(t) for t in m[k]] for k in ("right", "forward"))
        cell, half = _f(dtype, par["cell"]), dtype(0.5) * dtype(gw)
        Z = _f(dtype, c["calib"]) / d
        X0, X1 = Z * (p0 / fx), Z * (p1 / fy)
        gx, gz = (r[0] * X0 + r[1] * X1) + r[2] * Z, (fw[0] * X0 + fw[1] * X1) + fw[2] * Z
        u, v = gx / cell + half, gz / cell
        assert u.dtype == dtype and v.dtype == dtype
        go = lab <= OBSTACLE
        u_map[ys[go], xs[go]], v_map[ys[go], xs[go]] = u[go], v[go]
        fi, fz = np.floor(u), np.floor(v)
        ins = go & (fi >= 0) & (fi < gw) & (fz >= 0) & (fz < gh)
        ix, iz = fi[ins].astype(np.int64), fz[ins].astype(np.int64)
        np.add.at(gc, (lab[ins].astype(np.int64), iz, ix), 1)
        ob = lab[ins] == OBSTACLE
        np.maximum.at(gh_, (iz[ob], ix[ob]), hgt[ins][ob].astype(np.float32))
    return out


def run(c, dtype, up=UP, **over):
    f = fit(c, dtype, **over)
    m = metric(c, f, up, **over)
    return dict(fit=f, plane=m, pix=pixels(c, f, m, dtype, **over))


def record(r):
    """The 32 doubles of the header from a ``run``."""
    f, m = r["fit"], r["plane"]
    rec = np.zeros(32)
    rec[0:3], rec[3], rec[4], rec[5], rec[6], rec[7] = f["coef"], m["ok"], f["n"], f["inliers"], f["rms"], f["steps"]
    rec[8:11], rec[11], rec[12] = m["normal"], m["Hc"], m["tilt"]
    rec[13:19], rec[19:22], rec[22:25] = f["A"][np.triu_indices(3)], f["b"], m["forward"]
    return np.where(np.isfinite(rec), rec, 0.0)


# ---- the reference of a case, the restatement's deviation, the undecided pixels ---------------------------------------
def reference(c):
    """Everything the tests compare against, computed once per case: r64 / r32 (``run``), dev_coef, dev_normal, dev_Hc,
    dev_e, dev_h, dev_u (the restatement's deviations), undecided [h,w] bool, reach [gh,gw] (how many undecided pixels can
    land in each cell) or None, valid [h,w] bool."""
    h, w = c["crop"]
    r64, r32 = run(c, np.float64), run(c, np.float32)
    p64, p32 = r64["pix"], r32["pix"]
    valid = valid_mask(c)
    par = c["par"]

    def dev(a, b):
        both = ~np.isnan(a) & ~np.isnan(b)
        return float(np.abs(a[both].astype(np.float64) - b[both]).max()) if both.any() else 0.0

    dev_e, dev_h = dev(p32["e"], p64["e"]), dev(p32["height"], p64["height"])
    dev_u = max(dev(p32["u"], p64["u"]), dev(p32["v"], p64["v"]))
    und = np.zeros((h, w), bool)
    reach = None
    if r64["plane"]["ok"]:
        e, hg = p64["e"], p64["height"]
        tol, gtol, clr = (float(np.float32(par[k])) for k in ("tol_px", "ground_tol", "clearance"))
        with np.errstate(invalid="ignore"):
            und |= np.abs(np.abs(e) - tol) <= 2 * dev_e
            und |= (np.abs(np.abs(hg) - gtol) <= 2 * dev_h) | (np.abs(hg - clr) <= 2 * dev_h)
            if c["grid"] is not None:
                (gh, gw), _ = c["grid"]
                u, v = p64["u"], p64["v"]
                edge = (np.abs(u - np.rint(u)) <= 2 * dev_u) | (np.abs(v - np.rint(v)) <= 2 * dev_u)
                # a pixel whose label is undecided may enter or leave the grid: it needs its cell coordinates too
                und |= edge
                reach = np.zeros((gh, gw), np.int64)
                ys, xs = np.nonzero(und & valid)
                if ys.size:  # the cell coordinates of ANY valid pixel: those of pixels(), without the label's gate
                    uu, vv = _cell_coordinates(c, r64, ys, xs)
                    for du in (-1, 0, 1):
                        for dv in (-1, 0, 1):
                            ix, iz = np.floor(uu) + du, np.floor(vv) + dv
                            ins = (ix >= 0) & (ix < gw) & (iz >= 0) & (iz < gh)
                            np.add.at(reach, (iz[ins].astype(np.int64), ix[ins].astype(np.int64)), 1)
        und &= valid
    return dict(r64=r64, r32=r32, valid=valid, undecided=und, reach=reach, dev_e=dev_e, dev_h=dev_h, dev_u=dev_u,
                dev_coef=float(np.abs(r32["fit"]["coef"] - r64["fit"]["coef"]).max()),
                dev_normal=float(np.abs(r32["plane"]["normal"] - r64["plane"]["normal"]).max()),
                dev_Hc=abs(r32["plane"]["Hc"] - r64["plane"]["Hc"]))


def _cell_coordinates(c, r, ys, xs):
    fx, fy, cx, cy = (float(np.float32(v)) for v in c["K"])
    (gh, gw), _ = c["grid"]
    m = r["plane"]
    d = c["disp"][ys, xs].astype(np.float64)
    Z = float(np.float32(c["calib"])) / d
    X = np.stack([Z * ((xs - cx) / fx), Z * ((ys - cy) / fy), Z])
    cell = float(np.float32(c["par"]["cell"]))
    return m["right"] @ X / cell + 0.5 * gw, m["forward"] @ X / cell
