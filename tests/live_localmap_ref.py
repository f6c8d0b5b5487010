"""Restatement of codd_local_map (include/codd_hip.h) shared by the CPU and the GPU tests, in numpy only, and the cases.

The four launches are four functions, each from the state BYTES to the next ones, so that a test can enter at any launch:
``pose`` (launch 1: Python floats are IEEE doubles, the operations stand in the header's order, none is fused; division and
square root are correctly rounded on both sides), ``enter`` (launch 2), ``pixels`` (launch 3: one numpy operation on
np.float32 arrays per fp32 operation of the header; the per-pixel ground-frame terms are those of
tests/live_objects_ref.py, imported, not copied) and ``update`` (launch 4, integers).  ``step`` chains them.  Launches 2 to 4
equal the kernel bit for bit given the state launch 1 left; launch 1 is compared within the fp64 bound of the GPU test.

A case is a case of live_objects_ref (``lo.make``: labels, padded disparity, ground record, K, calib) plus ``par`` (the
parameters of the entry, ``DEFAULTS``), ``ego`` (fp32 [16] or None), ``fresh`` and the planted ``state``, ``logodds``, ``age``
before the call.  The planted cases use the FLAT rig of tests/live_scan_ref.py: a level camera with K = (64, 64, 74, 20.25) and
calib 50, where gz = 50 / d and gx = gz * (x - 74) / 64 are exact for the disparities used.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_objects_ref as lo  # noqa: E402
import live_scan_ref as ls  # noqa: E402

f32 = np.float32
FLOOR, OBSTACLE, OVERHEAD, BELOW, INVALID = lo.FLOOR, lo.OBSTACLE, lo.OVERHEAD, lo.BELOW, lo.INVALID
RESET, HOLD = 0, 1
CROP, PADDED = (37, 70), (64, 128)  # ragged 8 x 8 blocks and 32 x 8 tiles: 5 tile rows, 3 tile columns, the last partial
DEFAULTS = dict(gh=16, gw=24, cell=0.5, range_min=0.0, range_max=12.8, select=1 << OBSTACLE, min_pixels=4, l_occ=4, l_free=2,
                l_min=-32, l_max=64, decay=0, occ_level=8, free_level=-4, lost=RESET)
# the state's 32 doubles
EXISTS, PX, PZ, HX, HZ, IX0, IZ0, FRAMES, RESTARTS, N, HC, F, PIX0, PIZ0, CLEARED, INTEGRATED, LINKED, DX, DZ = (
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 18, 19, 20, 21, 22)
FLAT_K, FLAT_CALIB = ls.FLAT_K, ls.FLAT_CALIB


def ego_record(t=(0.0, 0.0, 0.0), q=(0.0, 0.0, 0.0, 1.0), ok=1.0):
    """The 16 fp32 of codd_ego_motion (the fields codd_local_map reads: t [0:3], q_xyzw [3:7], ok [7]; the others zero)."""
    e = np.zeros(16, f32)
    e[0:3], e[3:7], e[7] = t, q, ok
    return e


def empty_state():
    return np.zeros(32, np.float64)


def planted_state(par, p=(0.0, 0.0), h=(0.0, 1.0), rec=None, frames=3, restarts=1):
    """A state as launch 1 leaves it: a pose, its window origin, the floor frame of the ground record ``rec``."""
    rec = ls.flat_record() if rec is None else rec
    cell = float(f32(par["cell"]))
    st = empty_state()
    st[EXISTS], st[PX], st[PZ], st[HX], st[HZ] = 1.0, p[0], p[1], h[0], h[1]
    st[IX0], st[IZ0] = np.floor(p[0] / cell) - par["gw"] // 2, np.floor(p[1] / cell) - par["gh"] // 2
    st[FRAMES], st[RESTARTS] = frames, restarts
    st[N:N + 3], st[HC], st[F:F + 3] = rec[8:11], rec[11], rec[22:25]
    st[PIX0], st[PIZ0] = st[IX0], st[IZ0]
    return st


# ---- launch 1 ----------------------------------------------------------------------------------------------------------
def rotation(q):
    """R of the unit quaternion q_xyzw, rows (header's expressions)."""
    qx, qy, qz, qw = q
    return ((1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)),
            (2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)),
            (2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)))


def _floor_of(rec):
    return [float(v) for v in rec[8:11]], float(rec[11]), [float(v) for v in rec[22:25]]


def pose(st, ego, rec, fresh, par):
    """Launch 1: the state after it (a new array)."""
    st = np.array(st, np.float64)
    cell = float(f32(par["cell"]))
    exists, cur = st[EXISTS] != 0, rec[3] != 0
    px, pz, hx, hz = (float(st[k]) for k in (PX, PZ, HX, HZ))
    pix0, piz0 = st[IX0], st[IZ0]
    n, Hc, f = [0.0] * 3, 0.0, [0.0] * 3
    dx = dz = 0.0
    linked = False
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    if exists and ego is not None and not fresh and ego[7] != 0:
        t = [float(v) for v in ego[0:3]]
        q = [float(v) for v in ego[3:7]]
        with np.errstate(all="ignore"):
            qn = float(np.sqrt(np.float64(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])))
        good = qn > 0.0 and qn < np.inf
        if good:
            R = rotation([v / qn for v in q])
            col = lambda k: (R[0][k], R[1][k], R[2][k])  # noqa: E731
            n_p, Hp, f_p = [float(v) for v in st[N:N + 3]], float(st[HC]), [float(v) for v in st[F:F + 3]]
            if cur:
                n, Hc, f = _floor_of(rec)
            else:
                n = [dot(R[0], n_p), dot(R[1], n_p), dot(R[2], n_p)]
                Hc = Hp - dot(n, t)
                g = [-n[2] * n[0], -n[2] * n[1], 1.0 - n[2] * n[2]]
                gn = float(np.sqrt(np.float64((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])))
                good = gn >= 1e-3
                with np.errstate(all="ignore"):
                    f = [float(np.float64(v) / np.float64(gn)) for v in g]
            if good:
                r_p = [f_p[1] * n_p[2] - f_p[2] * n_p[1], f_p[2] * n_p[0] - f_p[0] * n_p[2], f_p[0] * n_p[1] - f_p[1] * n_p[0]]
                c = [-dot(col(0), t), -dot(col(1), t), -dot(col(2), t)]
                v = [dot(col(0), f), dot(col(1), f), dot(col(2), f)]
                ddx, ddz = dot(r_p, c), dot(f_p, c)
                a, b = dot(r_p, v), dot(f_p, v)
                m = float(np.sqrt(np.float64(a * a + b * b)))
                if m >= 1e-6:
                    qx1, qz1 = (px + ddx * hz) + ddz * hx, (pz - ddx * hx) + ddz * hz
                    ux, uz = (a * hz + b * hx) / m, (b * hz - a * hx) / m
                    un = float(np.sqrt(np.float64(ux * ux + uz * uz)))
                    if abs(qx1 / cell) < 2.0 ** 30 and abs(qz1 / cell) < 2.0 ** 30 and un > 0.0 and un < np.inf:
                        px, pz, hx, hz, dx, dz = qx1, qz1, ux / un, uz / un, ddx, ddz
                        linked = True
    cleared, now = False, exists
    frames, restarts = float(st[FRAMES]), float(st[RESTARTS])
    if linked:
        integrated = cur
        frames += 1.0
    elif exists and not fresh and par["lost"] == HOLD:
        dx = dz = 0.0
        integrated = cur
        frames += 1.0
        n, Hc, f = _floor_of(rec) if cur else ([float(v) for v in st[N:N + 3]], float(st[HC]), [float(v) for v in st[F:F + 3]])
    else:
        if exists or fresh:
            restarts += 1.0
        cleared = True
        px, pz, hx, hz, dx, dz, frames = 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0
        now = integrated = cur
        n, Hc, f = _floor_of(rec) if cur else ([0.0] * 3, 0.0, [0.0] * 3)
    out = np.zeros(32, np.float64)
    out[EXISTS] = 1.0 if now else 0.0
    out[PX], out[PZ], out[HX], out[HZ] = px, pz, hx, hz
    out[IX0], out[IZ0] = np.floor(px / cell) - float(par["gw"] // 2), np.floor(pz / cell) - float(par["gh"] // 2)
    out[FRAMES], out[RESTARTS] = frames, restarts
    out[N:N + 3], out[HC], out[F:F + 3] = n, Hc, f
    out[PIX0], out[PIZ0] = pix0, piz0
    out[CLEARED], out[INTEGRATED], out[LINKED] = float(cleared), float(bool(integrated)), float(linked)
    out[DX], out[DZ] = dx, dz
    return out


# ---- launches 2 to 4 ---------------------------------------------------------------------------------------------------
def slots(st, par):
    """int64 [gh,gw]: the flat storage index of window cell [j,i] (world cell (ix0 + i, iz0 + j), mathematical modulo)."""
    gh, gw = par["gh"], par["gw"]
    wx = int(st[IX0]) + np.arange(gw, dtype=np.int64)
    wz = int(st[IZ0]) + np.arange(gh, dtype=np.int64)
    return np.mod(wz, gh)[:, None] * gw + np.mod(wx, gw)[None, :]


def enter(st, L, age, par):
    """Launch 2 on copies of the storage: (logodds int16 [gh,gw], age uint8 [gh,gw])."""
    gh, gw = par["gh"], par["gw"]
    L, age = np.array(L, np.int16).reshape(-1), np.array(age, np.uint8).reshape(-1)
    wx = int(st[IX0]) + np.arange(gw, dtype=np.int64)[None, :]
    wz = int(st[IZ0]) + np.arange(gh, dtype=np.int64)[:, None]
    kept = (st[CLEARED] == 0) & (wx >= int(st[PIX0])) & (wx < int(st[PIX0]) + gw) & (wz >= int(st[PIZ0])) & (wz < int(st[PIZ0]) + gh)
    s = slots(st, par)[~kept]
    L[s], age[s] = 0, 255
    return L.reshape(gh, gw), age.reshape(gh, gw)


def pixels(c, st, par):
    """Launch 3: (O, F) int32 [gh,gw] in window order, and the eligible pixels' (ys, xs, jx, jz, obst) that reached a cell."""
    gh, gw = par["gh"], par["gw"]
    O, Fl = np.zeros((gh, gw), np.int32), np.zeros((gh, gw), np.int32)
    none = dict(ys=np.zeros(0, np.int64), xs=np.zeros(0, np.int64), jx=np.zeros(0, np.int64), jz=np.zeros(0, np.int64),
                obst=np.zeros(0, bool))
    if st[INTEGRATED] == 0:
        return O, Fl, none
    h, w = c["crop"]
    d, lab = c["disp"][:h, :w], c["labels"]
    sel = (np.uint64(par["select"]) >> np.minimum(lab, 31).astype(np.uint64)) & np.uint64(1)
    with np.errstate(invalid="ignore"):
        take = ((lab == FLOOR) | ((lab < 32) & (sel == 1))) & np.isfinite(d) & (d > 0)
    ys, xs = np.nonzero(take)
    _, _, gx, gz = lo.pixel_terms(c, ys, xs)
    cellf, rmin, rmax = f32(par["cell"]), f32(par["range_min"]), f32(par["range_max"])
    cell = float(cellf)
    oxf, ozf = f32(st[PX] - st[IX0] * cell), f32(st[PZ] - st[IZ0] * cell)
    hxf, hzf = f32(st[HX]), f32(st[HZ])
    with np.errstate(all="ignore"):
        rho = np.sqrt((gx * gx) + (gz * gz))
        wx, wz = (gx * hzf + gz * hxf) + oxf, (gz * hzf - gx * hxf) + ozf
        jx, jz = np.floor(wx / cellf), np.floor(wz / cellf)
        keep = (rho >= rmin) & (rho < rmax) & (jx >= 0) & (jx < f32(gw)) & (jz >= 0) & (jz < f32(gh))
    assert all(v.dtype == f32 for v in (rho, wx, wz, jx, jz, oxf, hxf))
    g = np.nonzero(keep)[0]
    ys, xs, jx, jz = ys[g], xs[g], jx[g].astype(np.int64), jz[g].astype(np.int64)
    obst = lab[ys, xs] != FLOOR
    np.add.at(O, (jz[obst], jx[obst]), 1)
    np.add.at(Fl, (jz[~obst], jx[~obst]), 1)
    return O, Fl, dict(ys=ys, xs=xs, jx=jx, jz=jz, obst=obst)


def update(st, L, age, O, Fl, par):
    """Launch 4 on copies of the storage: dict(logodds, age (storage), map_out, age_out (window), counts = (pixels, occupied,
    free, never seen))."""
    gh, gw = par["gh"], par["gw"]
    s = slots(st, par)
    Ls, ages = np.array(L, np.int16).reshape(-1), np.array(age, np.uint8).reshape(-1)
    Lw, aw = Ls[s].astype(np.int64), ages[s].astype(np.int64)
    O, Fl = O.astype(np.int64), Fl.astype(np.int64)
    occ = O >= par["min_pixels"]
    free = ~occ & (Fl >= par["min_pixels"])
    rest = ~occ & ~free
    L1 = np.where(occ, np.minimum(Lw + par["l_occ"], par["l_max"]), np.where(free, np.maximum(Lw - par["l_free"], par["l_min"]), Lw))
    if par["decay"] > 0:
        dec = np.where(Lw > 0, np.maximum(Lw - par["decay"], 0), np.minimum(Lw + par["decay"], 0))
        L1 = np.where(rest, dec, L1)
    a1 = np.where(rest, np.where(aw == 255, 255, np.minimum(aw + 1, 254)), 0)
    Ls[s], ages[s] = L1.astype(np.int16), a1.astype(np.uint8)
    counts = (int((O + Fl).sum()), int((L1 >= par["occ_level"]).sum()), int((L1 <= par["free_level"]).sum()), int((a1 == 255).sum()))
    return dict(logodds=Ls.reshape(gh, gw), age=ages.reshape(gh, gw), map_out=L1.astype(np.int16), age_out=a1.astype(np.uint8),
                counts=counts)


def record(st, counts):
    r = np.zeros(16, np.float64)
    r[0], r[1], r[2], r[3] = st[INTEGRATED], st[LINKED], st[RESTARTS], st[FRAMES]
    r[4:8] = st[PX], st[PZ], st[HX], st[HZ]
    r[8:10] = st[IX0], st[IZ0]
    r[10:14] = counts
    r[14:16] = st[DX], st[DZ]
    return r


def after_pose(c, st, L, age, par):
    """Launches 2 to 4 from the state launch 1 left: dict(state, logodds, age, map_out, age_out, O, F, record)."""
    L, age = enter(st, L, age, par)
    O, Fl, px = pixels(c, st, par)
    u = update(st, L, age, O, Fl, par)
    return dict(state=st, logodds=u["logodds"], age=u["age"], map_out=u["map_out"], age_out=u["age_out"], O=O, F=Fl,
                record=record(st, u["counts"]), assign=px)


def step(c, st, L, age, par=None, ego=None, fresh=False):
    """All four launches."""
    par = c["par"] if par is None else par
    return after_pose(c, pose(st, ego, c["rec"], fresh, par), L, age, par)


def reference(c):
    return step(c, c["state"], c["logodds"], c["age"], c["par"], c["ego"], c["fresh"])


# ---- the cases ---------------------------------------------------------------------------------------------------------
def make(name, labels, disp, rec=None, K=FLAT_K, calib=FLAT_CALIB, padded=PADDED, ego=None, fresh=False, state=None, logodds=None,
         age=None, **par):
    """A case.  ``state`` None: the empty state (zeros); ``logodds`` / ``age`` None: a planted pattern that a clear must
    erase and an update must carry."""
    c = lo.make(name, labels, disp, rec=ls.flat_record() if rec is None else rec, padded=padded, K=K, calib=calib)
    unknown = set(par) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **par)
    c["par"] = p
    gh, gw = p["gh"], p["gw"]
    k = np.arange(gh * gw, dtype=np.int64).reshape(gh, gw)
    c["logodds"] = np.ascontiguousarray(((k * 7) % 23 - 11) if logodds is None else logodds, np.int16).reshape(gh, gw)
    c["age"] = np.ascontiguousarray(np.where(k % 5 == 0, 255, (k * 3) % 250) if age is None else age, np.uint8).reshape(gh, gw)
    c["state"] = empty_state() if state is None else np.asarray(state, np.float64)
    c["ego"] = None if ego is None else np.asarray(ego, f32)
    c["fresh"] = bool(fresh)
    return c


def _blank(fill=INVALID, d=8.0):
    return np.full(CROP, fill, np.uint8), np.full(CROP, d, f32)


def _one_cell():
    """Every pixel a floor pixel of one cell: gz = 50 / 0.5 = 100, gx = 100 (x - 74) / 64 in (-116, -6.2), cells of 1024."""
    lab, d = _blank(FLOOR, 0.5)
    return lab, d


def _keys64():
    """One wave's 8 x 8 block (rows 8 .. 15, columns 56 .. 63) whose 64 pixels have 64 distinct keys, with cells of 1 / 8 and a
    camera at (0, 0): 32 depths gz = 1.0625 + k / 8 (the middle of 32 successive cell rows), each at a floor pixel and at an
    obstacle pixel next to it."""
    lab, d = _blank()
    for r in range(8):
        for q in range(8):
            lab[8 + r, 56 + q] = OBSTACLE if q % 2 else FLOOR
            d[8 + r, 56 + q] = 50.0 / (1.0625 + 0.125 * (4 * r + q // 2))
    return lab, d


def _cell_edge():
    """Pixels exactly on cell edges, cells of 0.5 around a camera at (0, 0) (oxf = 6, ozf = 4): column 42 has gx = -gz / 2
    and column 10 gx = -gz, exactly.  gz = 2: (wx, wz) = (5, 6) = cell (10, 12) and (4, 6) = cell (8, 12); gz = 1: (5.5, 5) = cell
    (11, 10) and (5, 5) = cell (10, 10); gz = 4: wz = 8 = 16 cells: outside, the far edge is exclusive."""
    lab, d = _blank()
    for y, dd in ((5, 25.0), (6, 50.0), (7, 12.5)):
        lab[y, 42], d[y, 42] = OBSTACLE, dd
        lab[y + 10, 10], d[y + 10, 10] = FLOOR, dd
    return lab, d


def _bad_disparity():
    lab, d = _blank(FLOOR, 25.0)
    lab[::2, :] = OBSTACLE
    d[3, :] = np.nan
    d[4, :] = np.inf
    d[5, :] = 0.0
    d[6, :] = -25.0
    d[7, :] = -np.inf
    return lab, d


def _range_edges():
    """Column 10 (gx = -gz): rho = sqrtf(2 gz gz), for gz = 4, 6.25 and, between them, 5."""
    lab, d = _blank()
    lab[10:14, 10], d[10:14, 10] = OBSTACLE, 12.5
    lab[20:24, 10], d[20:24, 10] = OBSTACLE, 8.0
    lab[30:34, 10], d[30:34, 10] = OBSTACLE, 10.0
    return lab, d


def rho_at(gz):
    g = f32(gz)
    return np.sqrt((g * g) + (g * g))


def _scene():
    """A floor strip at two depths, two obstacle columns, and labels the map ignores unless selected."""
    lab, d = _blank()
    lab[20:, :], d[20:, :] = FLOOR, 25.0      # gz = 2
    lab[28:, :], d[28:, :] = FLOOR, 50.0      # gz = 1
    lab[2:20, 20:30], d[2:20, 20:30] = OBSTACLE, 25.0
    lab[2:20, 50:66], d[2:20, 50:66] = OBSTACLE, 20.0  # gz = 2.5
    lab[0:2, :], d[0:2, :] = OVERHEAD, 40.0   # gz = 1.25
    lab[2:6, 0:8], d[2:6, 0:8] = BELOW, 25.0
    return lab, d


def build_cases():
    sl, sd = _scene()
    par16 = dict(DEFAULTS)
    ident, fwd = ego_record(), ego_record(t=(0.0, 0.0, -1.25))  # (t = -R c: the camera went 1.25 forward)
    back = ego_record(t=(3.0, 0.0, 2.5))                        # (the camera went 3 to the left and 2.5 back: negative cells)
    jump = ego_record(t=(-100.0, 0.0, -100.0))                  # (a window jump that clears everything)
    q90 = ego_record(t=(0.5, 0.0, -0.25), q=(0.0, np.sqrt(0.5), 0.0, np.sqrt(0.5)))
    r0, r1 = rho_at(4.0), rho_at(6.25)
    st = planted_state(par16, p=(0.3, 0.7))
    st1 = planted_state(dict(par16, cell=1.0), p=(0.3, 2.0))
    no_floor = np.where(np.arange(32) == 3, 0.0, ls.flat_record())
    cases = [
        make("fresh", sl, sd, fresh=True, ego=ident, state=st),
        make("first-from-zeros", sl, sd),
        make("identity", sl, sd, ego=ident, state=st),
        make("forward", sl, sd, ego=fwd, state=st),
        make("negative-cells", sl, sd, ego=back, state=st),
        make("window-jump", sl, sd, ego=jump, state=st),
        make("turn", sl, sd, ego=q90, state=st, decay=1),
        make("ground-lost", sl, sd, rec=no_floor, ego=fwd, state=st, decay=3),
        make("ego-lost-reset", sl, sd, ego=ego_record(t=(0, 0, -1.25), ok=0.0), state=st),
        make("ego-lost-hold", sl, sd, ego=ego_record(t=(0, 0, -1.25), ok=0.0), state=st, lost=HOLD),
        make("ego-null-reset", sl, sd, state=st),
        make("ego-null-hold", sl, sd, state=st, lost=HOLD),
        make("fresh-hold", sl, sd, fresh=True, ego=fwd, state=st, lost=HOLD),
        make("lost-and-no-floor", sl, sd, rec=no_floor, state=st),
        make("one-cell", *_one_cell(), fresh=True, cell=1024.0, range_max=4096.0, min_pixels=37 * 70),
        make("keys64", *_keys64(), ego=ident, state=planted_state(dict(par16, cell=0.125, gh=80), p=(0.0, 0.0)), cell=0.125,
             min_pixels=1, gh=80, gw=24),
        make("cell-edge", *_cell_edge(), ego=ident, state=planted_state(par16, p=(0.0, 0.0)), min_pixels=1),
        make("bad-disparity", *_bad_disparity(), ego=ident, state=st, min_pixels=1),
        make("range-edges", *_range_edges(), ego=ident, state=st1, cell=1.0, min_pixels=1, range_min=float(r0), range_max=float(r1)),
        make("range-edges-in", *_range_edges(), ego=ident, state=st1, cell=1.0, min_pixels=1, range_min=float(np.nextafter(r0, f32(np.inf))),
             range_max=float(np.nextafter(r1, f32(np.inf)))),
        make("two-labels", sl, sd, ego=ident, state=st, select=(1 << OBSTACLE) | (1 << OVERHEAD), min_pixels=2),
        make("floor-only", sl, sd, ego=ident, state=st, select=0),
        make("saturate", sl, sd, ego=ident, state=st, l_occ=30000, l_free=30000, l_min=-32768, l_max=32767,
             logodds=np.where(np.arange(16 * 24) % 2 == 0, 32000, -32000)),
        make("1x1", sl, sd, ego=fwd, state=planted_state(dict(par16, gh=1, gw=1, cell=4.0), p=(-1.0, 0.7)), gh=1, gw=1, cell=4.0),
        make("5x3", sl, sd, ego=fwd, state=planted_state(dict(par16, gh=5, gw=3, cell=1.0), p=(0.3, 0.7)), gh=5, gw=3, cell=1.0),
        make("5x3-fresh", sl, sd, fresh=True, gh=5, gw=3, cell=1.0, min_pixels=1),
    ]
    return cases


CASES = build_cases()
NAMES = {c["name"]: i for i, c in enumerate(CASES)}


def case_id(c):
    return c["name"]


# ---- planted camera poses over a plane (the CPU test of launch 1) ---------------------------------------------------------
def camera_to_world(yaw, pitch, roll):
    """C: camera axes (x right, y down, z forward) in a world with Y up and the floor Y = 0: yaw about the vertical, then
    pitch (down positive) about the camera's x axis, then roll about its z axis."""
    cy_, sy_ = np.cos(yaw), np.sin(yaw)
    cp, sp = np.cos(pitch), np.sin(pitch)
    cr, sr = np.cos(roll), np.sin(roll)
    base = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])  # a level camera: y down
    Ry = np.array([[cy_, 0.0, sy_], [0.0, 1.0, 0.0], [-sy_, 0.0, cy_]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    Rz = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    return Ry @ base @ Rx @ Rz


def floor_record(C, height):
    """The ground record (n, Hc, f, ok) a camera with the axes ``C`` at ``height`` above the floor Y = 0 sees."""
    rec = np.zeros(32)
    n = C.T @ np.array([0.0, 1.0, 0.0])
    g = np.array([-n[2] * n[0], -n[2] * n[1], 1.0 - n[2] * n[2]])
    rec[3], rec[8:11], rec[11], rec[22:25] = 1.0, n, height, g / np.sqrt(g @ g)
    return rec


def quaternion(R):
    """q_xyzw of a rotation matrix (w > 0 for the small rotations used)."""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def ego_between(C0, o0, C1, o1):
    """The fp32 ego record of G: X_cur = R X_prev + t between two planted cameras."""
    R = C1.T @ C0
    t = C1.T @ (o0 - o1)
    return ego_record(t=t, q=quaternion(R))
