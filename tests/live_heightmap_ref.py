"""Restatement of codd_height_map (include/codd_hip.h) shared by the CPU and the GPU tests, in numpy only, and the cases.

The four launches are four functions, each from the state BYTES to the next ones: ``enter`` (launch 1), ``pixels`` (launch 2:
the cell of a pixel is what tests/live_localmap_ref.py's ``pixels`` computes and the height what tests/live_objects_ref.py's
``pixel_terms`` computes -- imported, not copied; the quantisation is one numpy operation on np.float32 per fp32 operation of
the header), ``update`` (launch 3, integers) and ``derive`` (launch 4, integers).  ``after_map`` chains them from the state
codd_local_map's launch 1 left; ``step`` runs the map's restatement first.

A case is a case of live_localmap_ref (``lm.make``) plus ``hpar`` (``DEFAULTS``: the entry's own parameters, the thresholds
already in units of h_res) and ``layers``: the planted top, bot, ceil, hage before the call.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_localmap_ref as lm  # noqa: E402
import live_objects_ref as lo  # noqa: E402
import live_scan_ref as ls  # noqa: E402

f32 = np.float32
FLOOR, OBSTACLE, OVERHEAD, BELOW, INVALID = lm.FLOOR, lm.OBSTACLE, lm.OVERHEAD, lm.BELOW, lm.INVALID
NONE, NO_CEIL, Q_MAX = -32768, 32767, 32000
STEP, HEADROOM, HOLE, UNKNOWN = 1, 2, 4, 255
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SURFACES = (1 << FLOOR) | (1 << OBSTACLE) | (1 << BELOW)
DEFAULTS = dict(h_res=0.005, select=SURFACES, min_pixels=4, alpha=128, max_step_q=20, robot_height_q=200, max_drop_q=20)
LAYERS = ("top", "bot", "ceil", "hage")
TABLES = ("Tmax", "Tmin", "Tn", "Cmin", "Cn")
OUTPUTS = ("top_out", "bot_out", "ceil_out", "hage_out", "step_out", "flags_out")


def quantise(hgt, h_res):
    """q of the header for fp32 heights (finite ones): rintf, the clamp, the conversion."""
    hgt = np.asarray(hgt, f32)
    with np.errstate(all="ignore"):
        r = np.rint(hgt / f32(h_res))
        q = np.minimum(np.maximum(r, f32(-Q_MAX)), f32(Q_MAX))
    assert r.dtype == f32 and q.dtype == f32
    return q.astype(np.int64)


def blend(v, t, alpha):
    """f(v, t) = v + (alpha (t - v)) / 256, the division truncating toward zero."""
    n = int(alpha) * (np.asarray(t, np.int64) - np.asarray(v, np.int64))
    return np.asarray(v, np.int64) + np.sign(n) * (np.abs(n) // 256)


def kept(st, par):
    """bool [gh,gw]: window cells that were in the previous window (launch 1's rule, as live_localmap_ref.enter states it)."""
    gh, gw = par["gh"], par["gw"]
    wx = int(st[lm.IX0]) + np.arange(gw, dtype=np.int64)[None, :]
    wz = int(st[lm.IZ0]) + np.arange(gh, dtype=np.int64)[:, None]
    return ((st[lm.CLEARED] == 0) & (wx >= int(st[lm.PIX0])) & (wx < int(st[lm.PIX0]) + gw) & (wz >= int(st[lm.PIZ0]))
            & (wz < int(st[lm.PIZ0]) + gh))


def enter(st, layers, par):
    """Launch 1 on copies of the storage: dict(top, bot, ceil int16, hage uint8 [gh,gw])."""
    gh, gw = par["gh"], par["gw"]
    out = {k: np.array(layers[k], np.uint8 if k == "hage" else np.int16).reshape(-1) for k in LAYERS}
    s = lm.slots(st, par)[~kept(st, par)]
    out["top"][s], out["bot"][s], out["ceil"][s], out["hage"][s] = NONE, NONE, NO_CEIL, 255
    return {k: v.reshape(gh, gw) for k, v in out.items()}


def pixels(c, st, par, hpar):
    """Launch 2: dict(Tmax, Tmin, Tn, Cmin, Cn int32 [gh,gw]) and the pixels that reached a table: dict(ys, xs, jx, jz, over, q,
    hgt)."""
    gh, gw = par["gh"], par["gw"]
    T = dict(Tmax=np.full((gh, gw), INT_MIN, np.int32), Tmin=np.full((gh, gw), INT_MAX, np.int32), Tn=np.zeros((gh, gw), np.int32),
             Cmin=np.full((gh, gw), INT_MAX, np.int32), Cn=np.zeros((gh, gw), np.int32))
    sel = int(hpar["select"])
    assert not sel & (1 << OVERHEAD) and 0 <= sel < 2 ** 32
    # the map's own launch 3 on every label either table takes (it always takes the floor: dropped again below if unselected)
    _, _, px = lm.pixels(c, st, dict(par, select=(sel | (1 << OVERHEAD)) & ~(1 << FLOOR)))
    ys, xs, jx, jz = px["ys"], px["xs"], px["jx"], px["jz"]
    lab = c["labels"][ys, xs].astype(np.int64)
    over = lab == OVERHEAD
    surf = ((sel >> np.minimum(lab, 31)) & 1).astype(bool) & (lab < 32)
    _, hgt, _, _ = lo.pixel_terms(c, ys, xs)
    g = np.nonzero((surf | over) & np.isfinite(hgt))[0]
    ys, xs, jx, jz, over, hgt = ys[g], xs[g], jx[g], jz[g], over[g], hgt[g]
    q = quantise(hgt, hpar["h_res"])
    s, o = ~over, over
    np.maximum.at(T["Tmax"], (jz[s], jx[s]), q[s].astype(np.int32))
    np.minimum.at(T["Tmin"], (jz[s], jx[s]), q[s].astype(np.int32))
    np.add.at(T["Tn"], (jz[s], jx[s]), 1)
    np.minimum.at(T["Cmin"], (jz[o], jx[o]), q[o].astype(np.int32))
    np.add.at(T["Cn"], (jz[o], jx[o]), 1)
    return T, dict(ys=ys, xs=xs, jx=jx, jz=jz, over=over, q=q, hgt=hgt)


def update_cells(top, bot, ceil, hage, T, hpar):
    """The update rule on int64 arrays of any shape (the window's cells): (top, bot, ceil, hage)."""
    top, bot, ceil, hage = (np.asarray(v, np.int64) for v in (top, bot, ceil, hage))
    Tmax, Tmin, Tn, Cmin, Cn = (np.asarray(T[k], np.int64) for k in TABLES)
    surf, over = Tn >= hpar["min_pixels"], Cn >= hpar["min_pixels"]
    a = hpar["alpha"]
    top1 = np.where(surf, np.where(top == NONE, Tmax, blend(top, Tmax, a)), top)
    bot1 = np.where(surf, np.where(bot == NONE, Tmin, blend(bot, Tmin, a)), bot)
    ceil1 = np.where(over, np.where(ceil == NO_CEIL, Cmin, blend(ceil, Cmin, a)), ceil)
    age1 = np.where(surf | over, 0, np.where(hage == 255, 255, np.minimum(hage + 1, 254)))
    return top1, bot1, ceil1, age1


def update(st, layers, T, par, hpar):
    """Launch 3 on copies of the storage: dict(top, bot, ceil, hage (storage), top_out, bot_out, ceil_out, hage_out (window))."""
    gh, gw = par["gh"], par["gw"]
    s = lm.slots(st, par)
    flat = {k: np.array(layers[k], np.uint8 if k == "hage" else np.int16).reshape(-1) for k in LAYERS}
    new = update_cells(*(flat[k][s] for k in LAYERS), T, hpar)
    out = {}
    for k, v in zip(LAYERS, new):
        flat[k][s] = v.astype(flat[k].dtype)
        out[k] = flat[k].reshape(gh, gw)
        out[k + "_out"] = v.astype(flat[k].dtype)
    return out


def derive(top, bot, ceil, hpar):
    """Launch 4 on the unrolled layers: (step uint16, flags uint8 [gh,gw], counts = (known, STEP, HEADROOM, HOLE), largest top,
    smallest bot)."""
    top, bot, ceil = (np.asarray(v, np.int64) for v in (top, bot, ceil))
    gh, gw = top.shape
    known = top != NONE
    pad = np.full((gh + 2, gw + 2), INT_MAX, np.int64)  # beyond the window's edge there is no neighbour: nothing wraps
    pad[1:-1, 1:-1] = np.where(known, top, INT_MAX)
    low = np.full((gh, gw), INT_MAX, np.int64)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if dj or di:
                low = np.minimum(low, pad[1 + dj:1 + dj + gh, 1 + di:1 + di + gw])
    step = np.where(known & (low != INT_MAX), np.maximum(0, top - low), 0)
    flags = (np.where(step > hpar["max_step_q"], STEP, 0) | np.where((ceil != NO_CEIL) & (ceil - top < hpar["robot_height_q"]), HEADROOM, 0)
             | np.where(bot < -hpar["max_drop_q"], HOLE, 0))
    flags = np.where(known, flags, UNKNOWN)
    counts = (int(known.sum()), int((known & (flags & STEP != 0)).sum()), int((known & (flags & HEADROOM != 0)).sum()),
              int((known & (flags & HOLE != 0)).sum()))
    hi, lo_ = (int(top[known].max()), int(bot[known].min())) if known.any() else (0, 0)
    return step.astype(np.uint16), flags.astype(np.uint8), counts, hi, lo_


def record(st, T, hage_out, counts, hi, lo_):
    r = np.zeros(16, np.float64)
    r[0] = st[lm.INTEGRATED]
    r[1], r[2], r[3] = int(T["Tn"].astype(np.int64).sum()), int(T["Cn"].astype(np.int64).sum()), int((hage_out == 0).sum())
    r[4:8] = counts
    r[8], r[9] = hi, lo_
    r[10:12] = st[lm.IX0], st[lm.IZ0]
    return r


def after_map(c, st, layers, par=None, hpar=None):
    """All four launches from the state codd_local_map left: dict(the layers, the outputs, the tables, record, assign)."""
    par = c["par"] if par is None else par
    hpar = c["hpar"] if hpar is None else hpar
    L = enter(st, layers, par)
    T, px = pixels(c, st, par, hpar)
    u = update(st, L, T, par, hpar)
    step, flags, counts, hi, lo_ = derive(u["top_out"], u["bot_out"], u["ceil_out"], hpar)
    out = dict(u, step_out=step, flags_out=flags, record=record(st, T, u["hage_out"], counts, hi, lo_), assign=px, **T)
    return out


def step(c, st, layers, par=None, hpar=None, ego=None, fresh=False):
    """The map's launch 1 (its restatement), then the four launches: (the state, after_map's dict)."""
    par = c["par"] if par is None else par
    st1 = lm.pose(st, ego, c["rec"], fresh, par)
    return st1, after_map(c, st1, layers, par, hpar)


def reference(c):
    return step(c, c["state"], c["layers"], c["par"], c["hpar"], c["ego"], c["fresh"])


def thresholds(h_res, max_step, robot_height, max_drop):
    """The host's quantisation: (int)rint(v / h_res) in fp64."""
    return tuple(int(np.rint(np.float64(v) / np.float64(h_res))) for v in (max_step, robot_height, max_drop))


# ---- the cases ---------------------------------------------------------------------------------------------------------
def planted_layers(gh, gw):
    """A pattern a clear must erase and an update must carry: sentinels among the values, bot <= top, ceil above top."""
    k = np.arange(gh * gw, dtype=np.int64).reshape(gh, gw)
    top = np.where(k % 7 == 0, NONE, (k * 37) % 600 - 100)
    bot = np.where(top == NONE, NONE, top - (k * 11) % 90)
    ceil = np.where(k % 3 == 0, NO_CEIL, np.where(top == NONE, 400, top) + (k * 13) % 500)
    hage = np.where(top == NONE, np.where(k % 2 == 0, 255, 9), np.where(k % 5 == 0, 254, (k * 3) % 250))
    return dict(top=top.astype(np.int16), bot=bot.astype(np.int16), ceil=ceil.astype(np.int16), hage=hage.astype(np.uint8))


def with_height(c, layers=None, **hpar):
    unknown = set(hpar) - set(DEFAULTS)
    assert not unknown, unknown
    c = dict(c, hpar=dict(DEFAULTS, **hpar))
    c["layers"] = planted_layers(c["par"]["gh"], c["par"]["gw"]) if layers is None else layers
    return c


def _many_heights():
    """lm's one-cell scene (every pixel in one cell of 1024) with a height per row, -23 .. 33, the top rows overhead."""
    lab, d = lm._one_cell()
    lab[:9, :] = OVERHEAD
    lab[9:20, ::3] = OBSTACLE
    lab[30:, 1::2] = BELOW
    return lab, d


def _keys64():
    """lm's keys64 block with its obstacle pixels made overhead ones: 32 cells x (surface | overhead) = 64 distinct keys in
    one wave, each lane alone with its key."""
    lab, d = lm._keys64()
    lab[lab == OBSTACLE] = OVERHEAD
    return lab, d


def _overhead_only():
    """lm's scene plus overhead pixels alone in cells of their own (gz = 3.25, left of the optical axis) and a strip where
    overhead and floor pixels share cells (gz = 1)."""
    lab, d = lm._scene()
    lab[0:2, :], d[0:2, :] = OVERHEAD, 50.0 / 3.25
    lab[2:4, 30:50], d[2:4, 30:50] = OVERHEAD, 50.0
    return lab, d


def _huge_plane():
    """A ground record whose disparity plane has c = (1e37, 0, 0): c0 p0 overflows fp32 for p0 <= -35 (x <= 39: hgt is not
    finite, the pixel is dropped) and is finite and huge for x >= 40 (q clamps at +32000)."""
    rec = ls.flat_record()
    rec[0:3] = 1e37, 0.0, 0.0
    return rec


def build_cases():
    L = {c["name"]: c for c in lm.CASES}
    sl, sd = lm._scene()
    par16 = dict(lm.DEFAULTS)
    st = lm.planted_state(par16, p=(0.3, 0.7))
    ident = lm.ego_record()
    cases = [with_height(L[n]) for n in ("fresh", "first-from-zeros", "identity", "forward", "negative-cells", "window-jump", "turn",
                                         "ground-lost", "lost-and-no-floor", "ego-lost-hold", "cell-edge", "range-edges",
                                         "range-edges-in", "1x1", "5x3", "5x3-fresh")]
    cases += [
        with_height(L["bad-disparity"], min_pixels=1),
        with_height(dict(L["cell-edge"], name="cell-edge-1"), min_pixels=1, alpha=256),
        with_height(lm.make("many-heights", *_many_heights(), fresh=True, cell=1024.0, range_max=4096.0), min_pixels=1, alpha=1),
        with_height(lm.make("keys64-kinds", *_keys64(), ego=ident, state=lm.planted_state(dict(par16, cell=0.125, gh=80), p=(0.0, 0.0)),
                            cell=0.125, gh=80, gw=24), min_pixels=1),
        with_height(lm.make("overhead-only", *_overhead_only(), ego=ident, state=st), min_pixels=2, robot_height_q=2000),
        with_height(lm.make("non-finite-height", sl, sd, rec=_huge_plane(), ego=ident, state=st), min_pixels=1),
        with_height(lm.make("surfaces-obstacle-only", sl, sd, ego=ident, state=st), select=1 << OBSTACLE, alpha=37, h_res=0.0625),
        with_height(lm.make("no-surface-label", sl, sd, ego=ident, state=st), select=0, max_step_q=0, max_drop_q=0, robot_height_q=0),
        with_height(lm.make("thresholds-max", sl, sd, ego=ident, state=st), max_step_q=Q_MAX, max_drop_q=Q_MAX, robot_height_q=Q_MAX,
                    h_res=0.25),
    ]
    return cases


CASES = build_cases()
NAMES = {c["name"]: i for i, c in enumerate(CASES)}


def case_id(c):
    return c["name"]
