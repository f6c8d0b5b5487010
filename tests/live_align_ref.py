"""Restatements of codd_align_depth (include/codd_hip.h) shared by the CPU and the GPU tests, written from the header's
text: the contract in fp64 by brute force (``reference``: every source pixel is tested, no acceleration structure), the
header's fp32 operation order in numpy float32 (``positions_fp32``), the target pixels whose footprint membership hangs
on a rounding boundary (``ambiguous``), and the inputs of the tests.

A target is a plain dict: R [3,3], T [3] (X_t = R X_rect + T), K (fx, fy, cx, cy), dist (8 numbers), model ("brown" |
"fisheye"), r2_max, size (ht, wt).  A case is a dict: disp fp32 [H,W], crop (h, w), f, cx, cy, calib (floats that fp32
holds exactly), target, k.

THE DEPTH BOUND.  Z_t = fma(R6, X, fma(R7, Y, fma(R8, Z, T2))) with u = 2^-24 the unit roundoff of fp32, to first order:
  Z = (1 / d) * calib                      2 roundings
  X = ((u - cx) / f) * Z                   3 roundings + Z's 2 = 5;  Y likewise 5
  R6, R7, R8, T2 rounded once to fp32      1 each
  the products inside the fmas are exact; the three fmas round their sums once each: the innermost sum holds the Z and T
  terms, the middle one also the Y term, the outer one all four
  => |dZ_t| <= u ((5 + 1 + 1) |R6 X| + (5 + 1 + 2) |R7 Y| + (2 + 1 + 3) |R8 Z| + (1 + 3) |T2|) <= 8 u (|R2.| . |X| + |T2|)
so DEPTH_C = 8 (the largest of 7, 8, 6, 4).  A target pixel takes the minimum over its contributors; two minima over the
same contributors differ by at most the largest contributor's bound, which is what ``reference`` records per pixel.

DELTA.  The position (sx, sy) of the fp32 restatement deviates from fp64 by at most MEASURED_DEV pixels over the general
cases below (tests/test_live_align.py measures it and asserts the constant covers it); DELTA = max(8 MEASURED_DEV, 2^-10):
the margin is over this restatement, the factor 8 for a division or an atanf that differs by an ulp on the device."""
import zlib

import numpy as np

import live_calib_ref as cr

DEPTH_C = 8
U32 = 2.0 ** -24
MEASURED_DEV = 1.3e-5  # pixels: the largest |fp32 restatement - fp64| position over GENERAL (test_live_align.py prints it)
DELTA = max(8 * MEASURED_DEV, 2.0 ** -10)
CAP = 0.02  # at most this share of the covered target pixels may be excluded as ambiguous, per case

SHAPES = (((2, 2), (3, 3)), ((4, 6), (6, 8)), ((37, 53), (64, 64)))  # (crop, padded) of the source
BROWN = (-0.21, 0.06, 1.1e-3, -7e-4, -0.008, 0.015, 0.008, 8e-4)
FISHEYE = (-0.03, 8e-3, -4e-3, 9e-4)
OM, T = (0.03, -0.05, 0.02), (0.05, -0.02, 0.03)
# (model, target size / source size, footprint): target larger and smaller than the source, k = 1, 2, 3
VARIANTS = (("brown", 1.5, 2), ("fisheye", 0.75, 1), ("brown", 1.6, 3), ("fisheye", 1.4, 3), ("brown", 1.0, 1))
GENERAL = tuple((s, m, z, k) for s in SHAPES for m, z, k in VARIANTS)


def case_id(c):
    (h, w), _ = c[0]
    return "%dx%d-%s-x%g-k%d" % ((h, w) + tuple(c[1:]))


# ---- the contract ------------------------------------------------------------------------------------------------
def first_index(s, k):
    """The first of the k columns (rows) nearest to s: odd k rint(s) - (k-1)/2 (ties to even), even k floor(s) - (k/2 - 1)."""
    return (np.rint(s) - (k - 1) // 2 if k % 2 else np.floor(s) - (k // 2 - 1)).astype(np.int64)


def positions_fp64(c):
    """Per source pixel of the crop, fp64: ok (not skipped), sx, sy, Zt and the first-order bound of Zt in fp32."""
    (h, w), t = c["crop"], c["target"]
    d = c["disp"][:h, :w].astype(np.float64)
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ok = np.isfinite(d) & (d > 0)
    with np.errstate(all="ignore"):
        Z = c["calib"] / np.where(ok, d, 1.0)
        X = np.stack([(uu - c["cx"]) / c["f"] * Z, (vv - c["cy"]) / c["f"] * Z, Z])
        R, T3 = np.asarray(t["R"], np.float64), np.asarray(t["T"], np.float64)
        Xt = np.tensordot(R, X, 1) + T3[:, None, None]
        ok &= (Xt[2] > 0) & np.isfinite(Xt[2])
        Zt = np.where(ok, Xt[2], 1.0)
        x, y = Xt[0] / Zt, Xt[1] / Zt
        ok &= x * x + y * y <= t["r2_max"]
        sx, sy = cr.distort(t, np.where(ok, x, 0.0), np.where(ok, y, 0.0))
        ok &= np.isfinite(sx) & np.isfinite(sy)
    bound = DEPTH_C * U32 * (np.tensordot(np.abs(R[2]), np.abs(X), 1) + abs(T3[2]))
    nan = np.nan
    return dict(ok=ok, sx=np.where(ok, sx, nan), sy=np.where(ok, sy, nan), Zt=np.where(ok, Zt, nan), bound=np.where(ok, bound, nan))


def reference(c, pos=None):
    """-> dict(depth fp64 [ht,wt] (+inf: nothing landed), bound [ht,wt] (the largest contributor's), uv fp64 [h,w,2], pos)."""
    pos = positions_fp64(c) if pos is None else pos
    (h, w), (ht, wt), k = c["crop"], c["target"]["size"], c["k"]
    depth, bound = np.full((ht, wt), np.inf), np.zeros((ht, wt))
    fx, fy = first_index(np.where(pos["ok"], pos["sx"], 0.0), k), first_index(np.where(pos["ok"], pos["sy"], 0.0), k)
    for v in range(h):
        for u in range(w):
            if not pos["ok"][v, u]:
                continue
            for ty in range(max(fy[v, u], 0), min(fy[v, u] + k, ht)):
                for tx in range(max(fx[v, u], 0), min(fx[v, u] + k, wt)):
                    depth[ty, tx] = min(depth[ty, tx], pos["Zt"][v, u])
                    bound[ty, tx] = max(bound[ty, tx], pos["bound"][v, u])
    return dict(depth=depth, bound=bound, uv=np.stack([pos["sx"], pos["sy"]], -1), pos=pos)


def ambiguous(pos, k, size, delta):
    """bool [ht,wt]: the target pixels that enter or leave some source pixel's footprint when its sx or sy moves by
    ``delta`` either way."""
    ht, wt = size
    out = np.zeros((ht, wt), bool)
    ok = pos["ok"]
    sx, sy = np.where(ok, pos["sx"], 0.0), np.where(ok, pos["sy"], 0.0)
    ax, bx, ay, by = first_index(sx - delta, k), first_index(sx + delta, k), first_index(sy - delta, k), first_index(sy + delta, k)
    for v, u in zip(*np.nonzero(ok & ((ax != bx) | (ay != by)))):
        box = np.zeros((ht, wt), bool)
        box[max(ay[v, u], 0):max(by[v, u] + k, 0), max(ax[v, u], 0):max(bx[v, u] + k, 0)] = True   # in a footprint for some shift
        box[max(by[v, u], 0):max(ay[v, u] + k, 0), max(bx[v, u], 0):max(ax[v, u] + k, 0)] = False  # in it for every shift
        out |= box
    return out


# ---- the header's fp32 operation order ---------------------------------------------------------------------------
def positions_fp32(c):
    """ok, sx, sy, Zt as numpy float32 evaluates the header's operation order (fma: live_calib_ref._fma)."""
    f32, fma = np.float32, cr._fma
    (h, w), t = c["crop"], c["target"]
    R, T3 = np.asarray(t["R"], np.float64).astype(f32).reshape(-1), np.asarray(t["T"], np.float64).astype(f32)
    K, k = np.asarray(t["K"], np.float64).astype(f32), np.asarray(t["dist"], np.float64).astype(f32)
    d = c["disp"][:h, :w]
    vv, uu = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    ok = np.isfinite(d) & (d > 0)
    with np.errstate(all="ignore"):
        Z = (f32(1) / np.where(ok, d, f32(1))) * f32(c["calib"])
        X = ((uu - f32(c["cx"])) / f32(c["f"])) * Z
        Y = ((vv - f32(c["cy"])) / f32(c["f"])) * Z
        Xt = fma(R[0], X, fma(R[1], Y, fma(R[2], Z, T3[0])))
        Yt = fma(R[3], X, fma(R[4], Y, fma(R[5], Z, T3[1])))
        Zt = fma(R[6], X, fma(R[7], Y, fma(R[8], Z, T3[2])))
        ok &= (Zt > 0) & np.isfinite(Zt)
        Zs = np.where(ok, Zt, f32(1))
        x, y = Xt / Zs, Yt / Zs
        xx, yy, r2 = x * x, y * y, fma(y, y, x * x)
        ok &= r2 <= f32(t["r2_max"])
        if t["model"] == "brown":
            num = fma(fma(fma(k[4], r2, k[1]), r2, k[0]), r2, f32(1))
            den = fma(fma(fma(k[7], r2, k[6]), r2, k[5]), r2, f32(1))
            kr, xy2 = num / den, (x + x) * y
            xd = fma(x, kr, fma(k[2], xy2, k[3] * fma(f32(2), xx, r2)))
            yd = fma(y, kr, fma(k[3], xy2, k[2] * fma(f32(2), yy, r2)))
        else:
            r = np.sqrt(r2)
            th = np.arctan(r)
            t2 = th * th
            td = th * fma(fma(fma(fma(k[3], t2, k[2]), t2, k[1]), t2, k[0]), t2, f32(1))
            s = np.where(r > f32(1e-8), td / np.where(r > 0, r, f32(1)), f32(1))
            xd, yd = x * s, y * s
        sx, sy = fma(K[0], xd, K[2]), fma(K[1], yd, K[3])
        ok &= np.isfinite(sx) & np.isfinite(sy)
    assert sx.dtype == sy.dtype == Zt.dtype == np.float32
    nan = f32(np.nan)
    return dict(ok=ok, sx=np.where(ok, sx, nan), sy=np.where(ok, sy, nan), Zt=np.where(ok, Zt, nan))


def splat_fp32(c, p32):
    """The depth map the fp32 restatement gives: fp32 [ht,wt]."""
    (h, w), (ht, wt), k = c["crop"], c["target"]["size"], c["k"]
    depth = np.full((ht, wt), np.inf, np.float32)
    for v, u in zip(*np.nonzero(p32["ok"])):
        fx, fy = int(first_index(p32["sx"][v, u], k)), int(first_index(p32["sy"][v, u], k))
        sl = depth[max(fy, 0):max(fy + k, 0), max(fx, 0):max(fx + k, 0)]
        np.minimum(sl, p32["Zt"][v, u], out=sl)
    return depth


def check_depth(got, ref, amb, name=""):
    """``got`` fp32 [ht,wt] against ``reference``'s result outside ``amb``: +inf exactly where the reference has it, every
    other pixel within its bound.  -> the largest error / bound."""
    keep = ~amb
    rinf = np.isinf(ref["depth"])
    ginf = np.isposinf(got)
    assert np.array_equal(ginf[keep], rinf[keep]), f"{name}: {int((ginf != rinf)[keep].sum())} pixels differ in being reached"
    m = keep & ~rinf
    if not m.any():
        return 0.0
    err = np.abs(got.astype(np.float64)[m] - ref["depth"][m])
    ratio = float((err / ref["bound"][m]).max())
    assert ratio <= 1.0, f"{name}: depth error {ratio:.3f} x the bound of {DEPTH_C} * 2^-24 * (|R2.| |X| + |T2|)"
    return ratio


def check_uv(got, ref, tol, name=""):
    """``got`` fp32 [h,w,2]: NaN exactly where the reference skips the pixel, within ``tol`` pixels elsewhere.  -> max error."""
    ok = ref["pos"]["ok"]
    gnan = np.isnan(got)
    assert np.array_equal(gnan[..., 0], ~ok) and np.array_equal(gnan[..., 1], ~ok), f"{name}: uv is NaN at other pixels than the reference skips"
    if not ok.any():
        return 0.0
    err = float(np.abs(got.astype(np.float64)[ok] - ref["uv"][ok]).max())
    assert err <= tol, f"{name}: uv deviates by {err:.3e} px, more than {tol:.3e}"
    return err


# ---- inputs ------------------------------------------------------------------------------------------------------
def make_target(model, size, f, om=OM, T3=T, dist=None, shift=(0.3, -0.4), r2_max=None):
    """A target camera of ``size`` (ht, wt) with focal lengths about ``f``; r2_max from the library's own scan unless given."""
    ht, wt = size
    dist = tuple(BROWN if model == "brown" else FISHEYE + (0.0,) * 4) if dist is None else tuple(dist)
    K = (f * 1.02, f * 0.97, (wt - 1) / 2 + shift[0], (ht - 1) / 2 + shift[1])
    t = dict(R=cr.rot(om), T=np.asarray(T3, np.float64), K=K, dist=dist, model=model, size=(ht, wt))
    t["r2_max"] = fold_radius2(t) if r2_max is None else r2_max
    return t


def fold_radius2(t):
    from codd_amd import calibration
    return calibration.fold_radius2(as_camera(t))


def as_camera(t):
    from codd_amd import calibration
    n = 8 if t["model"] == "brown" else 4
    return calibration.CameraModel(t["size"], t["K"], t["model"], tuple(t["dist"])[:n])


def as_align_target(t):
    """The plain dict as a codd_amd.calibration.AlignTarget (pose from the grid of the disparity)."""
    from codd_amd import calibration
    return calibration.AlignTarget(as_camera(t), t["R"], t["T"])


def scene(shape, seed, lo=1.0, hi=6.0):
    """fp32 [H,W] disparity: a slanted background with ripples and a foreground box in the crop, junk in the padding."""
    (h, w), (H, W) = shape
    rng = np.random.default_rng(zlib.crc32(("align " + seed).encode()))
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = lo + (hi - lo) * (0.25 + 0.2 * uu / max(w, 1) + 0.1 * vv / max(h, 1)) + 0.05 * np.sin(0.7 * uu + 0.4 * vv)
    d[h // 3:max(2 * h // 3, h // 3 + 1), w // 3:max(2 * w // 3, w // 3 + 1)] = 0.8 * hi
    d += rng.uniform(-0.02, 0.02, d.shape)
    d[h:, :] = 99.0
    d[:, w:] = -5.0
    return d.astype(np.float32)


def general_case(spec):
    """One of GENERAL: a rotated and translated target of ``zoom`` times the source size."""
    shape, model, zoom, k = spec
    (h, w), _ = shape
    f = float(np.float32(0.9 * max(w, 4)))
    ht, wt = max(int(round(zoom * h)), 1), max(int(round(zoom * w)), 1)
    return dict(disp=scene(shape, case_id(spec)), crop=(h, w), f=f, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0,
                calib=float(np.float32(f * 0.12)), target=make_target(model, (ht, wt), zoom * f), k=k)


def plant_case(shape, which):
    """The exact plants: f = 64, R = I, no distortion, depths that are powers of two -> (case, expected fp32 [ht,wt]).
    'a': T = 0, the target's principal point 5 columns right and 2 rows up of the source's, a target of another size: pixel
    (u, v) lands on (u + 5, v - 2).  'b': T = (0.25, 0, 0), the same principal point: a shift of f Tx / Z = 16 / Z columns,
    2 for the background at Z = 8 and 8 for the block at Z = 2, which wins where both land."""
    (h, w), (H, W) = shape
    f, cx, cy, calib = 64.0, 3.0, 2.0, 16.0
    Zs = np.full((h, w), 8.0)
    by0, by1, bx0, bx1 = h // 4, max(3 * h // 4, h // 4 + 1), w // 4, max(w // 2, w // 4 + 1)
    if which == "a":
        Zs[::2, 1::3], Zs[1::2, ::4] = 4.0, 1.0
        size, K, T3, dx, dy = (h + 3, w + 4), (64.0, 64.0, cx + 5, cy - 2), (0.0, 0.0, 0.0), 5, -2
    else:
        Zs[by0:by1, bx0:bx1] = 2.0
        size, K, T3, dx, dy = (h, w + 9), (64.0, 64.0, cx, cy), (0.25, 0.0, 0.0), 0, 0
    disp = np.full((H, W), 7.0, np.float32)
    disp[:h, :w] = (calib / Zs).astype(np.float32)
    want = np.full(size, np.inf, np.float32)
    for v in range(h):
        for u in range(w):
            ty, tx = v + dy, u + dx + (int(16 / Zs[v, u]) if which == "b" else 0)
            if 0 <= ty < size[0] and 0 <= tx < size[1]:
                want[ty, tx] = min(want[ty, tx], np.float32(Zs[v, u]))
    t = dict(R=np.eye(3), T=np.asarray(T3), K=K, dist=(0.0,) * 8, model="brown", size=size, r2_max=1e6)
    c = dict(disp=disp, crop=(h, w), f=f, cx=cx, cy=cy, calib=calib, target=t, k=1)
    return c, want, (by0, by1, bx0, bx1)
