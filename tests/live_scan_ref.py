"""Restatement of codd_range_scan (include/codd_hip.h) shared by the CPU and the GPU tests, in numpy only, and the cases.

Every decision of the contract is an fp32 comparison of fp32 values, each formed by the operations the header names, one
numpy operation on np.float32 arrays per operation (numpy has no fused multiply-add; its division and square root are
correctly rounded); the beam is taken by the COUNT of the edges with side >= 0, as the header defines it, not by a
bisection; the sums are integers and the minimum is taken over a 64-bit integer.  So this restatement equals the kernel
bit for bit, with no excluded pixel and no tolerance.  The per-pixel ground-frame terms are those of
tests/live_objects_ref.py (``pixel_terms``), imported, not copied.

Cases: a case is a case of live_objects_ref (``lo.make``: labels, padded disparity, record, K, calib) plus ``scan`` (beams,
bins, angles (radians), range_min, range_max, select, min_pixels), ``edges`` (the table) and ``ids`` (uint16 [h,w] or
None).  The planted cases use the FLAT rig: a level camera (pitch 0, roll 0: r = (1, 0, 0), f = (0, 0, 1)) with K = (64, 64,
74, 20.25) and calib 50, where gz = 50 / d and gx = gz * (x - 74) / 64 are exact for the disparities used (12.5 -> 4, 10 -> 5,
25 -> 2, 50 -> 1, 6.25 -> 8), so that a pixel can be planted exactly on a range, on a bin boundary or on a beam edge.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ground_ref as lg  # noqa: E402
import live_objects_ref as lo  # noqa: E402

f32 = np.float32
FLOOR, OBSTACLE, OVERHEAD, BELOW, INVALID = lo.FLOOR, lo.OBSTACLE, lo.OVERHEAD, lo.BELOW, lo.INVALID
NONE = lo.NONE
CROP, PADDED = lo.CROP, lo.PADDED
DEFAULTS = dict(beams=256, bins=128, angles=None, range_min=0.0, range_max=12.8, select=1 << OBSTACLE, min_pixels=8)
MAX_BEAMS, MAX_BINS = 2048, 1024
FLAT_K, FLAT_CALIB = (64.0, 64.0, 74.0, 20.25), 50.0
SCENE_K = (120.0, 120.0, 75.0, 20.0)  # of the boxes scene: the horizon high in the crop, so that the floor fills most of it
NAN_BITS, INF_BITS = 0x7FC00000, 0x7F800000
HALF_PI = np.pi / 2


def scan_edges(beams, angle_min, angle_max):
    """fp32 [beams+1,2] = (sin a_i, cos a_i), a_i = angle_min + (angle_max - angle_min) * i / beams in float64."""
    a = float(angle_min) + (float(angle_max) - float(angle_min)) * np.arange(beams + 1, dtype=np.float64) / float(beams)
    return np.stack([np.sin(a), np.cos(a)], 1).astype(f32)


def camera_span(K, w):
    return float(np.arctan((0.0 - K[2]) / K[0])), float(np.arctan((float(w) - 1.0 - K[2]) / K[0]))


def make(name, labels, disp, rec=None, ids=None, K=lo.K, calib=lo.CALIB, padded=PADDED, planted=(), **scan):
    """A case.  ``planted``: the (y, x) of pixels planted exactly on a boundary (asserted exactly by the CPU test and left
    out of its float64 comparison)."""
    c = lo.make(name, labels, disp, rec=rec, padded=padded, K=K, calib=calib)
    del c["par"]
    unknown = set(scan) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **scan)
    if p["angles"] is None:
        p["angles"] = camera_span(K, c["crop"][1])
    c["scan"] = p
    c["edges"] = scan_edges(p["beams"], *p["angles"])
    c["ids"] = None if ids is None else np.ascontiguousarray(ids, np.uint16)
    if planted == "all":
        planted = list(zip(*np.nonzero(c["labels"] != INVALID)))
    c["planted"] = tuple((int(y), int(x)) for y, x in planted)
    return c


# ---- the restatement ---------------------------------------------------------------------------------------------------
def assign(c):
    """The pixels that reach a (beam, bin): dict(ys, xs, obst bool, beam, k, rho fp32, gx, gz fp32, idx), in raster order.
    Empty with ok = 0."""
    h, w = c["crop"]
    p = c["scan"]
    d, lab = c["disp"][:h, :w], c["labels"]
    sel = (np.uint64(p["select"]) >> np.minimum(lab, 31).astype(np.uint64)) & np.uint64(1)
    with np.errstate(invalid="ignore"):
        take = (lab < 32) & np.isfinite(d) & (d > 0) & ((lab == FLOOR) | (sel == 1))
    if c["rec"][3] == 0:
        take[:] = False
    ys, xs = np.nonzero(take)
    _, _, gx, gz = lo.pixel_terms(c, ys, xs)
    rmin, rmax = f32(p["range_min"]), f32(p["range_max"])
    bins, beams = p["bins"], p["beams"]
    bin_w = rmax / f32(bins)
    with np.errstate(all="ignore"):
        rho = np.sqrt((gx * gx) + (gz * gz))
        keep = (gz > 0) & (rho >= rmin) & (rho < rmax)
        q = np.floor(rho / bin_w)
        s, co = c["edges"][:, 0], c["edges"][:, 1]
        side = (co[None, :] * gx[:, None]) - (s[None, :] * gz[:, None])
        cnt = (side >= 0).sum(1)
    assert rho.dtype == f32 and q.dtype == f32 and side.dtype == f32 and bin_w.dtype == f32
    keep &= (cnt > 0) & (cnt < beams + 1)
    k = np.where(keep, q, 0).astype(np.int64)
    k = np.where(k >= bins, bins - 1, k)
    g = np.nonzero(keep)[0]
    ys, xs = ys[g], xs[g]
    return dict(ys=ys, xs=xs, obst=lab[ys, xs] != FLOOR, beam=cnt[g] - 1, k=k[g], rho=rho[g], gx=gx[g], gz=gz[g],
                idx=ys.astype(np.int64) * w + xs, bin_w=bin_w)


def tables(c, a=None, drop=None):
    """(O int64 [beams,bins], F, N uint64) from ``assign``; ``drop``: a bool mask over its pixels to leave out."""
    a = assign(c) if a is None else a
    beams, bins = c["scan"]["beams"], c["scan"]["bins"]
    use = np.ones(a["idx"].shape, bool) if drop is None else ~drop
    ob, fl = use & a["obst"], use & ~a["obst"]
    O, F = np.zeros((beams, bins), np.int64), np.zeros((beams, bins), np.int64)
    N = np.full((beams, bins), np.iinfo(np.uint64).max, np.uint64)
    np.add.at(O, (a["beam"][ob], a["k"][ob]), 1)
    np.add.at(F, (a["beam"][fl], a["k"][fl]), 1)
    key = (a["rho"][ob].view(np.uint32).astype(np.uint64) << np.uint64(32)) | a["idx"][ob].astype(np.uint64)
    np.minimum.at(N, (a["beam"][ob], a["k"][ob]), key)
    return O, F, N


def resolve(O, F, min_pixels):
    """Per beam (kh or bins, kf or -1, floor) of the header's "per beam" paragraph."""
    beams, bins = O.shape
    kh, kf, floor_ = np.full(beams, bins), np.full(beams, -1), np.zeros(beams, np.int64)
    for b in range(beams):
        hit = np.nonzero(O[b] >= min_pixels)[0]
        if hit.size:
            kh[b] = hit[0]
        seen = np.nonzero(F[b, :kh[b]] >= min_pixels)[0]
        if seen.size:
            kf[b] = seen[-1]
        floor_[b] = F[b, :kh[b]].sum()
    return kh, kf, floor_


def reference(c):
    """dict(count int32 [4], scan_i int32 [beams,4], scan_f fp32 [beams,4]) of the contract, and the tables."""
    h, w = c["crop"]
    p = c["scan"]
    beams, bins = p["beams"], p["bins"]
    a = assign(c)
    O, F, N = tables(c, a)
    kh, kf, floor_ = resolve(O, F, p["min_pixels"])
    bin_w = a["bin_w"]
    free = np.where(kf >= 0, (kf + 1).astype(f32) * bin_w, f32(0)).astype(f32)
    scan_i, scan_f = np.zeros((beams, 4), np.int32), np.zeros((beams, 4), f32)
    bits = scan_f.view(np.uint32)
    count = np.zeros(4, np.int32)
    for b in range(beams):
        if kh[b] < bins:
            n = int(N[b, kh[b]])
            idx = n & 0xFFFFFFFF
            y, x = divmod(idx, w)
            _, _, gx, gz = lo.pixel_terms(c, np.array([y]), np.array([x]))
            obj = -1
            if c["ids"] is not None and c["ids"][y, x] != NONE:
                obj = int(c["ids"][y, x])
            bits[b, 0] = n >> 32
            scan_f[b, 1:] = (free[b], gx[0], gz[0])
            scan_i[b] = (idx, obj, O[b, kh[b]], floor_[b])
            count[0] += 1
        else:
            clear = free[b] > 0
            bits[b, 0] = INF_BITS if clear else NAN_BITS
            scan_f[b, 1] = free[b] if clear else 0
            scan_i[b] = (-1, -1, 0, floor_[b])
            count[1 if clear else 2] += 1
    count[3] = O.sum()
    return dict(count=count, scan_i=scan_i, scan_f=scan_f, O=O, F=F, N=N, kh=kh, kf=kf, assign=a)


# ---- the cases ---------------------------------------------------------------------------------------------------------
def flat_record(ok=1.0):
    return lo.record(cam_h=1.2, pitch=0.0, roll=0.0, ok=ok, K=FLAT_K, calib=FLAT_CALIB)


def _blank(fill=INVALID, d=8.0):
    return np.full(CROP, fill, np.uint8), np.full(CROP, d, f32)


def flat(name, labels, disp, **kw):
    kw.setdefault("angles", (-HALF_PI, HALF_PI))
    kw.setdefault("range_max", 16.0)
    kw.setdefault("bins", 16)
    return make(name, labels, disp, rec=flat_record(), K=FLAT_K, calib=FLAT_CALIB, **kw)


def boxes_scene():
    """(labels, disp [h,w], record, ids): live_ground_ref's "clutter" -- a noisy floor with three fronto-parallel boxes --
    cut to the crop of these tests, labelled by the fp32 restatement of codd_ground_plane, its obstacles numbered by the
    restatement of codd_objects."""
    spec = dict(crop=CROP, padded=PADDED, K=SCENE_K, calib=lg.CALIB_FIT, cam_h=lg.CAM_H, pitch=lg.PITCH, roll=lg.ROLL,
                name="scan-boxes", scene="clutter", par={}, seed=None, grid=None)
    g = lg.case(spec)
    r = lg.run(g, np.float32)
    assert r["plane"]["ok"]
    labels, rec = r["pix"]["labels"], lg.record(r)
    h, w = CROP
    oc = lo.make("scan-boxes", labels, g["disp"][:h, :w], rec=rec, K=SCENE_K, calib=lg.CALIB_FIT, min_pixels=64, min_height=0.15)
    return labels, g["disp"][:h, :w], rec, lo.reference(oc)["ids"]


def _wall():
    lab, d = _blank()
    lab[:, 80:130] = OBSTACLE
    d[:, 80:130] = 12.5  # gz = 4, gx in (0.375, 3.5): between the edges at 0 and 45 degrees, rho in [4.02, 5.32): bin 2 of 2-wide bins
    return lab, d


def _own_beam():
    lab, d = _blank()
    lab[20, :] = OBSTACLE
    d[20, :] = 12.5
    return lab, d


def _rho_tie():
    lab, d = _blank()
    lab[30, 80] = lab[10, 80] = lab[10, 90] = OBSTACLE
    d[30, 80] = d[10, 80] = 12.5  # the same gx, gz: the same rho
    d[10, 90] = 10.0
    return lab, d


def _threshold(near):
    """``near`` obstacle pixels at rho = 4 exactly (x = 74: gx = 0), twenty at rho = 5."""
    lab, d = _blank()
    lab[10:10 + near, 74], d[10:10 + near, 74] = OBSTACLE, 12.5
    lab[30:50, 74], d[30:50, 74] = OBSTACLE, 10.0
    return lab, d


def _speckle():
    """Column 74 (gx = 0): one obstacle pixel at rho = 2, twenty at rho = 5; floor at rho = 1 and 2 (eight pixels each) and
    three floor pixels at rho = 4."""
    lab, d = _threshold(0)
    lab[5, 74], d[5, 74] = OBSTACLE, 25.0
    lab[50:58, 74], d[50:58, 74] = FLOOR, 50.0
    lab[58:66, 74], d[58:66, 74] = FLOOR, 25.0
    lab[66:69, 74], d[66:69, 74] = FLOOR, 12.5
    return lab, d


def _range_edges():
    lab, d = _blank()
    lab[10, 74], d[10, 74] = OBSTACLE, 12.5  # rho = 4 = range_min
    lab[12, 74], d[12, 74] = OBSTACLE, 3.3   # rho = fl(50 / fl(3.3)), the far pixel
    lab[14, 74], d[14, 74] = OBSTACLE, 25.0  # rho = 2 < range_min
    return lab, d


def far_rho():
    return f32(FLAT_CALIB) / f32(3.3)


def _beam_edges():
    lab, d = _blank()
    for x in (10, 74, 138):  # gx = -gz, 0, gz: on the edges at -45, 0 and 45 degrees of a four-beam table over +-90
        lab[20, x], d[20, x] = OBSTACLE, 12.5
    return lab, d


def _behind():
    lab, d = _blank(d=30.0)
    lab[:, 60:90] = OBSTACLE
    return lab, d


def _two_labels():
    lab, d = lo._two_labels()
    return lab, d


def _floor_and_nothing():
    lab, d = _blank()
    lab[10:40, 30:70], d[10:40, 30:70] = OBSTACLE, 12.5   # x - 74 in [-44, -5]: beam 1 (-45 .. 0 degrees)
    lab[10:40, 80:120], d[10:40, 80:120] = FLOOR, 12.5    # beam 2: floor, no obstacle (no column at 3 : 4 : 5, rho = 5)
    lab[50, 140:143], d[50, 140:143] = FLOOR, 12.5        # beam 3: three floor pixels, fewer than min_pixels
    return lab, d


def _bad_disparity():
    lab, d = lo._bad_disparity()
    lab[::2, :] = FLOOR
    return lab, d


def build_cases():
    labels, disp, rec, ids = boxes_scene()
    scene = dict(rec=rec, K=SCENE_K, calib=lg.CALIB_FIT)
    wl, wd = _wall()
    ids5 = np.full(CROP, 5, np.uint16)
    wall = flat("wall", wl, wd, ids=ids5, beams=4, range_max=32.0)
    hit = int(reference(wall)["scan_i"][2, 0])
    ids_none = ids5.copy()
    ids_none.ravel()[hit] = NONE
    r0 = far_rho()
    return [
        make("boxes", labels, disp, ids=ids, **scene),
        make("boxes-no-ids", labels, disp, **scene),
        make("boxes-1x1", labels, disp, ids=ids, beams=1, bins=1, **scene),
        make("boxes-7x16", labels, disp, ids=ids, beams=7, bins=16, min_pixels=3, **scene),
        make("boxes-wide", labels, disp, ids=ids, beams=64, angles=(-HALF_PI, HALF_PI), range_min=1.5, range_max=6.0, **scene),
        wall,
        flat("wall-none-id", wl, wd, ids=ids_none, beams=4, range_max=32.0),
        flat("own-beam", *_own_beam(), beams=512, angles=(-0.905, 0.9), bins=8, range_max=24.0, min_pixels=1),
        flat("rho-tie", *_rho_tie(), beams=1, min_pixels=2),
        flat("threshold-met", *_threshold(8), beams=1, min_pixels=8, planted="all"),
        flat("threshold-missed", *_threshold(7), beams=1, min_pixels=8, planted="all"),
        flat("speckle", *_speckle(), beams=1, min_pixels=8, planted="all"),
        flat("range-edges", *_range_edges(), beams=1, min_pixels=1, range_min=4.0,
             range_max=float(np.nextafter(r0, f32(np.inf))), planted="all"),
        flat("range-max-excluded", *_range_edges(), beams=1, min_pixels=1, range_min=4.0, range_max=float(r0),
             planted="all"),
        flat("beam-edges", *_beam_edges(), beams=4, min_pixels=1, planted="all"),
        make("behind", *_behind(), rec=lo.record(pitch=1.2, roll=0.0), beams=16, angles=(-HALF_PI, HALF_PI), min_pixels=1),
        make("no-floor", labels, disp, ids=ids, rec=np.where(np.arange(32) == 3, 0.0, rec), K=SCENE_K, calib=lg.CALIB_FIT),
        make("two-labels", *_two_labels(), select=(1 << OBSTACLE) | (1 << OVERHEAD), beams=32, min_pixels=4),
        flat("floor-and-nothing", *_floor_and_nothing(), beams=4, min_pixels=8),
        make("bad-disparity", *_bad_disparity(), beams=16, bins=16, min_pixels=2),
    ]


CASES = build_cases()
NAMES = {c["name"]: i for i, c in enumerate(CASES)}


def case_id(c):
    return c["name"]
