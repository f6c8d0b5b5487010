"""Restatement of codd_objects (include/codd_hip.h) shared by the CPU and the GPU tests, in numpy only, and the cases.

Every decision of the contract is an fp32 comparison of fp32 values, each formed by the operations the header names, one
numpy operation on np.float32 arrays per operation (numpy has no fused multiply-add and its division is correctly
rounded); minima and maxima are taken over the header's order-preserving integer image of the floats, and there is no
sum.  So this restatement equals the kernel bit for bit, with no excluded pixel and no tolerance.

Components: every foreground pixel starts with its own raster index; each round takes the minimum over the pixel and its
joined 4-neighbours, then replaces every label by the label of the pixel it names (a label is the raster index of a pixel
of the same component, so this only shortens the walk); the rounds stop at the fixed point, where every pixel of a
component carries the component's smallest raster index: its key.

Cases: the ground record is fabricated in closed form by ``record`` from a camera height, a pitch and a roll -- a camera
``cam_h`` above the floor with the unit up vector u sees the plane c = -(calib / cam_h) (u_x / fx, u_y / fy, u_z), whose unit
normal towards the camera is u and whose forward axis is the optical axis projected onto the plane -- so that reference
and kernel read the same 32 doubles and no case needs codd_ground_plane.  The padding of the disparity holds 99, which a
kernel that reads outside the crop would join.
"""
import numpy as np

f32 = np.float32
FLOOR, OBSTACLE, OVERHEAD, BELOW, INVALID = 0, 1, 2, 3, 255
DEFAULTS = dict(select=1 << OBSTACLE, gap_px=1.0, gap_rel=0.05, min_pixels=64, min_height=0.15, max_objects=256)
NONE = 0xFFFF
CROP, PADDED = (70, 150), (128, 192)  # at least three 16 x 64 tiles each way, with a remainder
K, CALIB = (100.0, 100.0, 74.5, 20.25), 50.0
ANY_HEIGHT = -1e30  # min_height of the cases whose shapes are not about height


def up_vector(pitch, roll=0.0):
    u = np.array([0.0, -np.cos(pitch), -np.sin(pitch)])
    return np.array([u[0] * np.cos(roll) - u[1] * np.sin(roll), u[0] * np.sin(roll) + u[1] * np.cos(roll), u[2]])


def record(cam_h=1.2, pitch=0.15, roll=0.03, ok=1.0, K=K, calib=CALIB):
    """The 32 doubles of codd_ground_plane for the floor a camera ``cam_h`` above it sees (the fields codd_objects reads:
    c [0:3], ok [3], n [8:11], Hc [11], f [22:25]; the others zero)."""
    u = up_vector(pitch, roll)
    rec = np.zeros(32)
    rec[0:3] = -(calib / cam_h) * np.array([u[0] / K[0], u[1] / K[1], u[2]])
    rec[3] = ok
    rec[8:11], rec[11] = u, cam_h
    g = np.array([-u[2] * u[0], -u[2] * u[1], 1.0 - u[2] * u[2]])
    rec[22:25] = g / np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    return rec


def make(name, labels, disp, rec=None, crop=None, padded=PADDED, K=K, calib=CALIB, **par):
    """A case: labels uint8 [h,w], disp [h,w] (the crop; the padding is filled with 99), the record, the parameters."""
    labels = np.ascontiguousarray(labels, np.uint8)
    h, w = labels.shape
    assert crop is None or tuple(crop) == (h, w)
    full = np.full(padded, 99.0, f32)
    full[:h, :w] = np.asarray(disp, f32)
    unknown = set(par) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(name=name, crop=(h, w), padded=tuple(padded), K=tuple(K), calib=calib, disp=full, labels=labels,
                rec=record() if rec is None else np.asarray(rec, np.float64), par=dict(DEFAULTS, **par))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def ordered(v):
    """The order-preserving integer image (uint32) of fp32 values."""
    u = np.ascontiguousarray(v, f32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unordered(o):
    o = np.ascontiguousarray(o, np.uint32)
    return np.where(o >> 31 != 0, o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(f32)


def foreground(c):
    h, w = c["crop"]
    d, lab = c["disp"][:h, :w], c["labels"]
    if c["rec"][3] == 0:
        return np.zeros((h, w), bool)
    sel = (np.uint64(c["par"]["select"]) >> np.minimum(lab, 31).astype(np.uint64)) & np.uint64(1)
    with np.errstate(invalid="ignore"):
        return (lab < 32) & (sel == 1) & np.isfinite(d) & (d > 0)


def edges(c, fg=None):
    """(right [h,w-1], down [h-1,w]) bool: the pixel is joined to its right / lower neighbour."""
    h, w = c["crop"]
    d = c["disp"][:h, :w]
    fg = foreground(c) if fg is None else fg
    gap_px, gap_rel = f32(c["par"]["gap_px"]), f32(c["par"]["gap_rel"])

    def joined(a, b, both):
        with np.errstate(invalid="ignore", over="ignore"):
            lim = np.maximum(gap_px, gap_rel * np.minimum(a, b))
            t = np.abs(a - b) <= lim
        assert lim.dtype == f32
        return both & t

    return joined(d[:, :-1], d[:, 1:], fg[:, :-1] & fg[:, 1:]), joined(d[:-1, :], d[1:, :], fg[:-1, :] & fg[1:, :])


def components(c, fg=None):
    """key int64 [h,w]: the smallest raster index of the pixel's component, -1 for background."""
    h, w = c["crop"]
    fg = foreground(c) if fg is None else fg
    right, down = edges(c, fg)
    big = h * w
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    L = np.where(fg, idx, big)
    while True:
        N = L.copy()
        N[:, :-1] = np.where(right, np.minimum(N[:, :-1], L[:, 1:]), N[:, :-1])
        N[:, 1:] = np.where(right, np.minimum(N[:, 1:], L[:, :-1]), N[:, 1:])
        N[:-1, :] = np.where(down, np.minimum(N[:-1, :], L[1:, :]), N[:-1, :])
        N[1:, :] = np.where(down, np.minimum(N[1:, :], L[:-1, :]), N[1:, :])
        flat = np.append(N.ravel(), big)  # (background names the sentinel, which names itself)
        N = flat[N]
        if np.array_equal(N, L):
            break
        L = N
    return np.where(fg, L, -1)


def pixel_terms(c, ys, xs):
    """(d, hgt, gx, gz) fp32 at the pixels (ys, xs), in the header's operation order."""
    fx, fy, cx, cy = (f32(v) for v in c["K"])
    calib, rec = f32(c["calib"]), c["rec"]
    c0, c1, c2, Hc = f32(rec[0]), f32(rec[1]), f32(rec[2]), f32(rec[11])
    n, f = rec[8:11], rec[22:25]
    r = [f32(f[1] * n[2] - f[2] * n[1]), f32(f[2] * n[0] - f[0] * n[2]), f32(f[0] * n[1] - f[1] * n[0])]  # fp64, then rounded
    f = [f32(v) for v in f]
    d = c["disp"][ys, xs]
    with np.errstate(all="ignore"):
        p0, p1 = xs.astype(f32) - cx, ys.astype(f32) - cy
        e = d - ((c0 * p0 + c1 * p1) + c2)
        hgt = (Hc * e) / d
        Z = calib / d
        X0, X1 = Z * (p0 / fx), Z * (p1 / fy)
        gx, gz = (r[0] * X0 + r[1] * X1) + r[2] * Z, (f[0] * X0 + f[1] * X1) + f[2] * Z
    assert all(v.dtype == f32 for v in (d, hgt, gx, gz))
    return d, hgt, gx, gz


def reference(c):
    """dict(count int32 [4], obj_i int32 [m,8], obj_f fp32 [m,8], ids uint16 [h,w], key int64 [h,w]) of the contract."""
    h, w = c["crop"]
    par = c["par"]
    m = par["max_objects"]
    fg = foreground(c)
    key = components(c, fg)
    ys, xs = np.nonzero(fg)
    count, obj_i, obj_f = np.zeros(4, np.int32), np.zeros((m, 8), np.int32), np.zeros((m, 8), f32)
    ids = np.full((h, w), NONE, np.uint16)
    out = dict(count=count, obj_i=obj_i, obj_f=obj_f, ids=ids, key=key)
    if ys.size == 0:
        return out
    keys, comp = np.unique(key[ys, xs], return_inverse=True)  # ascending keys
    nc = keys.size
    d, hgt, gx, gz = pixel_terms(c, ys, xs)
    idx = ys.astype(np.int64) * w + xs
    pixels = np.bincount(comp, minlength=nc)
    big = np.iinfo(np.int64).max
    x0, y0 = np.full(nc, big), np.full(nc, big)
    x1, y1 = np.full(nc, -1, np.int64), np.full(nc, -1, np.int64)
    np.minimum.at(x0, comp, xs), np.minimum.at(y0, comp, ys), np.maximum.at(x1, comp, xs), np.maximum.at(y1, comp, ys)
    near = np.zeros(nc, np.uint64)
    np.maximum.at(near, comp, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64))
    near_idx = (~(near & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64)
    lo, hi = {}, {}
    for name, v in (("d", d), ("hgt", hgt), ("gx", gx), ("gz", gz)):
        o = ordered(v)
        lo[name], hi[name] = np.full(nc, 0xFFFFFFFF, np.uint32), np.zeros(nc, np.uint32)
        np.minimum.at(lo[name], comp, o), np.maximum.at(hi[name], comp, o)
        lo[name], hi[name] = unordered(lo[name]), unordered(hi[name])
    with np.errstate(invalid="ignore"):
        passes = (pixels >= par["min_pixels"]) & (hi["hgt"] >= f32(par["min_height"]))
    number = np.cumsum(passes) - 1
    chosen = passes & (number < m)
    n = int(chosen.sum())
    count[:] = (n, int(passes.sum()), nc, ys.size)
    k = np.nonzero(chosen)[0]
    obj_i[:n] = np.stack([pixels[k], x0[k], y0[k], x1[k], y1[k], near_idx[k] % w, near_idx[k] // w, keys[k]], 1)
    obj_f[:n] = np.stack([lo["gx"][k], hi["gx"][k], lo["gz"][k], hi["gz"][k], lo["hgt"][k], hi["hgt"][k], lo["d"][k],
                          hi["d"][k]], 1)
    ids[ys, xs] = np.where(chosen[comp], number[comp], NONE).astype(np.uint16)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _blank(crop=CROP, d=8.0):
    return np.zeros(crop, np.uint8), np.full(crop, d, f32)


def _serpentine(crop=CROP):
    """A one-pixel-wide path through the whole crop: every other row, joined at alternating ends."""
    lab, d = _blank(crop)
    h, w = crop
    lab[0::2, :] = OBSTACLE
    for y in range(1, h, 2):
        lab[y, w - 1 if (y // 2) % 2 == 0 else 0] = OBSTACLE
    return lab, d


def _comb(crop=CROP):
    lab, d = _blank(crop)
    lab[:, 0::2] = OBSTACLE  # teeth from the first row down
    lab[-1, :] = OBSTACLE  # that meet only in the last row
    return lab, d


def _u(crop=CROP):
    lab, d = _blank(crop)
    lab[:, 3] = lab[:, crop[1] - 4] = OBSTACLE
    lab[-1, 3:crop[1] - 3] = OBSTACLE
    return lab, d


def _checker(crop=CROP):
    lab, d = _blank(crop)
    yy, xx = np.mgrid[0:crop[0], 0:crop[1]]
    lab[(yy + xx) % 2 == 0] = OBSTACLE
    return lab, d


def _isolated(n, crop=CROP):
    """n isolated pixels spread over the crop (every tile gets some)."""
    lab, d = _blank(crop)
    ys, xs = np.mgrid[1:crop[0]:7, 1:crop[1]:11]
    assert ys.size >= n
    pick = np.linspace(0, ys.size - 1, n).astype(int)
    lab[ys.ravel()[pick], xs.ravel()[pick]] = OBSTACLE
    return lab, d


def _two_boxes(step):
    lab, d = _blank()
    lab[10:50, 20:100] = OBSTACLE
    d[10:50, 20:60], d[10:50, 60:100] = 16.0, f32(16.0) + f32(step)
    return lab, d


def _slant():
    lab, d = _blank()
    lab[5:60, :] = OBSTACLE
    d[:, :] = (5.0 + 0.5 * np.arange(CROP[1]))[None, :]  # 0.5 a pixel under a gap of 1, 74.5 end to end
    return lab, d


def _gap_rel():
    lab, d = _blank()
    lab[10:40, 10:60] = lab[10:40, 90:140] = OBSTACLE
    d[10:40, 10:35], d[10:40, 35:60] = 40.0, 41.5  # 1.5 <= 0.05 * 40: one component
    d[10:40, 90:115], d[10:40, 115:140] = 10.0, 11.5  # 1.5 > 0.05 * 10: two
    return lab, d


def _sizes():
    """An 8 x 8 block (64 pixels) and one with a corner missing (63), across a tile corner each."""
    lab, d = _blank()
    lab[12:20, 60:68] = OBSTACLE
    lab[28:36, 124:132] = OBSTACLE
    lab[28, 124] = FLOOR
    return lab, d


def _heights():
    """Two blocks of one disparity; the lower one in the image is lower above the floor."""
    lab, d = _blank(d=20.0)
    lab[10:30, 20:50] = OBSTACLE
    lab[14:34, 90:120] = OBSTACLE
    return lab, d


def _top(c, box):
    y0, y1, x0, x1 = box
    ys, xs = np.mgrid[y0:y1, x0:x1]
    return pixel_terms(c, ys.ravel(), xs.ravel())[1].max()


def _near_tie():
    lab, d = _blank(d=10.0)
    lab[15:30, 5:40] = OBSTACLE
    d[22, 10] = d[20, 30] = d[20, 25] = 12.0  # three equally near pixels: (20, 25) has the smallest raster index
    return lab, d


def _bad_disparity():
    lab, d = _blank()
    lab[:, :] = OBSTACLE
    yy, xx = np.mgrid[0:CROP[0], 0:CROP[1]]
    d[:, :] = np.array([8.0, np.nan, np.inf, 0.0, -2.0, 8.0, -np.inf], f32)[(xx + 3 * yy) % 7]
    return lab, d


def _two_labels():
    lab, d = _blank()
    lab[:, :] = np.array([FLOOR, OBSTACLE, OVERHEAD, BELOW, INVALID, 40, 33], np.uint8)[(np.arange(CROP[1]) // 9) % 7][None, :]
    return lab, d


def _both_signs():
    """A block across the image centre's column and, under a camera pitched 1.2 rad down, across gz = 0."""
    lab, d = _blank(d=30.0)
    lab[50:70, 60:90] = OBSTACLE
    return lab, d


def build_cases():
    any_h = dict(min_height=ANY_HEIGHT)
    cases = [
        make("serpentine", *_serpentine(), min_pixels=1, **any_h),
        make("comb", *_comb(), min_pixels=1, **any_h),
        make("u", *_u(), min_pixels=1, **any_h),
        make("checkerboard", *_checker(), min_pixels=1, max_objects=256, **any_h),
        make("exactly-max", *_isolated(37), min_pixels=1, max_objects=37, **any_h),
        make("max-plus-one", *_isolated(38), min_pixels=1, max_objects=37, **any_h),
        make("boxes-split", *_two_boxes(1.0 + 2.0 ** -10), gap_px=1.0, gap_rel=0.0, **any_h),
        make("boxes-joined", *_two_boxes(1.0 - 2.0 ** -10), gap_px=1.0, gap_rel=0.0, **any_h),
        make("slant", *_slant(), gap_px=1.0, gap_rel=0.0, **any_h),
        make("gap-rel", *_gap_rel(), gap_px=1e-3, gap_rel=0.05, **any_h),
        make("min-pixels", *_sizes(), min_pixels=64, **any_h),
        make("near-tie", *_near_tie(), gap_px=2.5, **any_h),
        make("bad-disparity", *_bad_disparity(), min_pixels=1, **any_h),
        make("two-labels", *_two_labels(), select=(1 << OBSTACLE) | (1 << OVERHEAD), min_pixels=1, **any_h),
        make("all-foreground", np.full(CROP, OBSTACLE, np.uint8), np.full(CROP, 9.0, f32), **any_h),
        make("no-foreground", *_blank(), **any_h),
        make("no-floor", *_sizes(), rec=record(ok=0.0), min_pixels=1, **any_h),
        make("one-row", *_serpentine((1, 150)), padded=(64, 192), min_pixels=1, **any_h),
        make("one-column", *_serpentine((70, 1)), padded=(128, 64), min_pixels=1, **any_h),
        make("five-by-seven", *_checker((5, 7)), padded=(64, 64), min_pixels=1, **any_h),
        make("both-signs", *_both_signs(), rec=record(pitch=1.2, roll=0.0), **any_h),
    ]
    # min_height exactly the taller block's top, and the next float above it
    probe = make("probe", *_heights())
    top = _top(probe, (10, 30, 20, 50))
    assert _top(probe, (14, 34, 90, 120)) < top
    cases.append(make("min-height-kept", *_heights(), min_height=float(top)))
    cases.append(make("min-height-dropped", *_heights(), min_height=float(np.nextafter(top, f32(np.inf)))))
    return cases


CASES = build_cases()
NAMES = {c["name"]: i for i, c in enumerate(CASES)}


def case_id(c):
    return c["name"]
