"""LiveSession elevation layer on the CPU: the restatement of tests/live_heightmap_ref.py itself -- the rule through the
scrolling toroidal window against a second statement kept in a plain dict by world cell; the update rule (first observation,
blend, truncation, dead band, clamp, ties, ages); the derive rule (edges of the window, unknown neighbours, each flag on its
threshold); a physical scene rendered to disparity in fp64 whose features must come out at their heights -- and
_check_heightmap, the LiveSession constructor, heightmap_from_buffers, the tuple order, the bindings, the entry's argument
checks (no launch) and the command line's arguments.  Nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_heightmap_ref as hm  # noqa: E402
import live_localmap_ref as lm  # noqa: E402
from codd_amd import live, ops  # noqa: E402

f32 = np.float32
HP = dict(hm.DEFAULTS)


# ---- the rule against a dict ----------------------------------------------------------------------------------------------
def _trunc_div(n, d):
    return n // d if n >= 0 else -((-n) // d)


def _dict_cell(old, t, hp):
    """The header's launch 3 for one cell, in plain integers: old = (top, bot, ceil, age), t = (Tmax, Tmin, Tn, Cmin, Cn)."""
    top, bot, ceil, age = old
    tmax, tmin, tn, cmin, cn = t
    f = lambda v, x: v + _trunc_div(hp["alpha"] * (x - v), 256)  # noqa: E731
    seen = False
    if tn >= hp["min_pixels"]:
        top = tmax if top == -32768 else f(top, tmax)
        bot = tmin if bot == -32768 else f(bot, tmin)
        seen = True
    if cn >= hp["min_pixels"]:
        ceil = cmin if ceil == 32767 else f(ceil, cmin)
        seen = True
    age = 0 if seen else (255 if age == 255 else min(age + 1, 254))
    return top, bot, ceil, age


def test_scrolling_window_equals_a_dict_by_world_cell():
    """A planted walk of window origins -- negative steps, a step of exactly gh, a jump beyond the window, sideways steps, a
    CLEARED frame, a frame that is not INTEGRATED -- with random tables: after every frame the storage holds world cell (ix, iz)
    at [iz mod gh, ix mod gw] with the values of a dict that forgets what leaves the window, and the outputs are the window."""
    gh, gw = 6, 5
    par = dict(lm.DEFAULTS, gh=gh, gw=gw)
    hp = dict(HP, alpha=96, min_pixels=3)
    rng = np.random.default_rng(5)
    origins = [(0, 0), (1, 2), (-2, 1), (-2, -5), (-2, -5 + gh), (3, 1), (3, 1), (40, -30), (39, -31), (39, -31 - gh), (39 - gw, -31 - gh)]
    cleared = {0, 6}
    idle = {4}
    layers = {k: np.full((gh, gw), 77, np.uint8 if k == "hage" else np.int16) for k in hm.LAYERS}  # (garbage: frame 0 is CLEARED)
    world, prev, carried = {}, (0, 0), 0
    for n, (ix0, iz0) in enumerate(origins):
        st = lm.empty_state()
        st[lm.IX0], st[lm.IZ0], st[lm.PIX0], st[lm.PIZ0] = ix0, iz0, prev[0], prev[1]
        st[lm.CLEARED], st[lm.INTEGRATED] = float(n in cleared), float(n not in idle)
        T = dict(Tmax=rng.integers(-300, 300, (gh, gw)), Tn=rng.integers(0, 7, (gh, gw)), Cmin=rng.integers(300, 600, (gh, gw)),
                 Cn=rng.integers(0, 6, (gh, gw)))
        T["Tmin"] = T["Tmax"] - rng.integers(0, 80, (gh, gw))
        if n in idle:
            T = dict(Tmax=np.full((gh, gw), hm.INT_MIN), Tmin=np.full((gh, gw), hm.INT_MAX), Tn=np.zeros((gh, gw), int),
                     Cmin=np.full((gh, gw), hm.INT_MAX), Cn=np.zeros((gh, gw), int))
        u = hm.update(st, hm.enter(st, layers, par), T, par, hp)
        layers = {k: u[k] for k in hm.LAYERS}
        # the dict: forget, then update every cell of the window
        inside = lambda c: ix0 <= c[0] < ix0 + gw and iz0 <= c[1] < iz0 + gh  # noqa: E731
        world = {} if n in cleared else {c: v for c, v in world.items() if inside(c)}
        for j in range(gh):
            for i in range(gw):
                c = (ix0 + i, iz0 + j)
                carried += (ix0, iz0) != prev and world.get(c, (-32768,))[0] != -32768  # known before, kept through a move
                world[c] = _dict_cell(world.get(c, (-32768, -32768, 32767, 255)), tuple(int(T[k][j, i]) for k in hm.TABLES), hp)
                got = tuple(int(layers[k][c[1] % gh, c[0] % gw]) for k in hm.LAYERS)
                assert got == world[c], (n, c, got, world[c])
                assert tuple(int(u[k + "_out"][j, i]) for k in hm.LAYERS) == world[c], (n, c)
        prev = (ix0, iz0)
    assert carried > 20 and len(world) == gh * gw


# ---- the update rule ------------------------------------------------------------------------------------------------------
def _one(top, bot, ceil, age, tmax=hm.INT_MIN, tmin=hm.INT_MAX, tn=0, cmin=hm.INT_MAX, cn=0, **hp):
    T = dict(Tmax=np.array([tmax]), Tmin=np.array([tmin]), Tn=np.array([tn]), Cmin=np.array([cmin]), Cn=np.array([cn]))
    return tuple(int(v[0]) for v in hm.update_cells([top], [bot], [ceil], [age], T, dict(HP, **hp)))


def test_update_rule():
    assert _one(hm.NONE, hm.NONE, hm.NO_CEIL, 255, 90, 10, 4) == (90, 10, hm.NO_CEIL, 0)  # the first observation is taken as it is
    assert _one(hm.NONE, hm.NONE, hm.NO_CEIL, 255, 90, 10, 3) == (hm.NONE, hm.NONE, hm.NO_CEIL, 255)  # below min_pixels: nothing
    assert _one(hm.NONE, hm.NONE, hm.NO_CEIL, 255, cmin=400, cn=4) == (hm.NONE, hm.NONE, 400, 0)  # an overhead-only cell
    assert _one(100, 20, 500, 7, 200, 0, 4, 400, 4) == (150, 10, 450, 0)  # alpha 128: half way
    assert _one(100, 20, 500, 7, 200, 0, 4, 400, 4, alpha=256) == (200, 0, 400, 0)  # alpha 256: the target
    assert _one(100, 20, 500, 7, 200, 0, 4, 400, 4, alpha=1) == (100, 20, 500, 0)  # alpha 1: |t - v| < 256 moves nothing
    assert _one(0, 0, 0, 0, 256, -256, 4, -300, 4, alpha=1) == (1, -1, -1, 0)
    # truncation toward zero on both signs: 128 * 3 / 256 = 1.5 -> 1 and -1.5 -> -1 (a floor would give -2)
    assert _one(10, 10, 10, 0, 13, 7, 4, 7, 4) == (11, 9, 9, 0)
    assert int(hm.blend(10, 7, 128)) == 9 and int(hm.blend(-10, -13, 128)) == -11 and int(hm.blend(-10, -7, 128)) == -9
    # the dead band |t - v| < 256 / alpha: alpha 128 rests one unit off, alpha 64 three
    assert int(hm.blend(10, 11, 128)) == 10 and int(hm.blend(10, 9, 128)) == 10 and int(hm.blend(10, 12, 128)) == 11
    assert int(hm.blend(10, 13, 64)) == 10 and int(hm.blend(10, 14, 64)) == 11 and int(hm.blend(10, 6, 64)) == 9
    for alpha in (1, 37, 64, 128, 255, 256):
        v = 0
        for _ in range(4000):
            v = int(hm.blend(v, 1000, alpha))
        assert 0 <= 1000 - v <= -(-256 // alpha) - 1, (alpha, v)
    # ages: 254 saturates, 255 stays, an observation resets; a frame that is not INTEGRATED has empty tables
    assert _one(5, 5, 9, 253)[3] == 254 and _one(5, 5, 9, 254)[3] == 254 and _one(5, 5, 9, 255)[3] == 255
    assert _one(5, 4, 9, 17) == (5, 4, 9, 18) and _one(5, 5, 9, 255, 6, 6, 4)[3] == 0
    # the extremes stay in range and in order
    assert _one(-32000, -32000, 32000, 0, 32000, 32000, 4, -32000, 4, alpha=256) == (32000, 32000, -32000, 0)
    assert _one(32000, -32000, 0, 0, -32000, -32000, 4) == (0, -32000, 0, 0)


def test_quantisation():
    # ties of rintf go to even: with h_res a power of two hgt / h_res is exact
    h = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, 3.0], f32) * f32(0.125)
    assert hm.quantise(h, 0.125).tolist() == [0, 2, 2, 0, -2, -2, 0, 3]
    # the clamp at +-32000, also for a quotient that overflows to infinity
    h = np.array([32000.0, 32000.5, 32001.0, -32000.5, 1e30, -1e30, 3e38, 31999.5], f32) * f32(0.125)
    assert hm.quantise(h, 0.125).tolist() == [32000, 32000, 32000, -32000, 32000, -32000, 32000, 32000]
    assert hm.quantise(np.array([3e38], f32), 1e-3).tolist() == [32000]
    assert hm.thresholds(0.005, 0.10, 1.0, 0.10) == (20, 200, 20) == ops.height_thresholds(0.005, 0.10, 1.0, 0.10)
    assert ops.height_thresholds(0.125, 0.0625, 0.1875, 4000.0) == (0, 2, 32000)  # rint in fp64: ties to even
    for bad in ((0.0, 1, 1, 1), (float("nan"), 1, 1, 1), (0.005, -0.01, 1, 1), (0.005, 1, 160.01, 1), (0.005, 1, 1, float("inf"))):
        with pytest.raises(ValueError):
            ops.height_thresholds(*bad)


def test_bot_never_above_top():
    rng = np.random.default_rng(11)
    n = 4096
    for alpha in (1, 3, 128, 200, 256):
        hp = dict(HP, alpha=alpha, min_pixels=1)
        top, bot = np.full(n, hm.NONE), np.full(n, hm.NONE)
        ceil, age = np.full(n, hm.NO_CEIL), np.full(n, 255)
        for _ in range(60):
            tmax = rng.integers(-hm.Q_MAX, hm.Q_MAX + 1, n)
            tmin = tmax - rng.integers(0, 3000, n) * rng.integers(0, 2, n)
            T = dict(Tmax=tmax, Tmin=np.maximum(tmin, -hm.Q_MAX), Tn=rng.integers(0, 3, n), Cmin=rng.integers(-hm.Q_MAX, hm.Q_MAX, n),
                     Cn=rng.integers(0, 2, n))
            top, bot, ceil, age = hm.update_cells(top, bot, ceil, age, T, hp)
            assert (bot <= top).all() and ((top == hm.NONE) == (bot == hm.NONE)).all()
            assert (np.abs(top[top != hm.NONE]) <= hm.Q_MAX).all() and (np.abs(ceil[ceil != hm.NO_CEIL]) <= hm.Q_MAX).all()


# ---- the derive rule ------------------------------------------------------------------------------------------------------
def _derive(top, bot=None, ceil=None, **hp):
    top = np.array(top, np.int64)
    bot = top.copy() if bot is None else np.array(bot, np.int64)
    ceil = np.full(top.shape, hm.NO_CEIL) if ceil is None else np.array(ceil, np.int64)
    return hm.derive(top, bot, ceil, dict(HP, **hp))


def test_derive_rule():
    N = hm.NONE
    # a high cell in column 0 and a low one in column gw - 1 are no neighbours: nothing wraps
    top = np.full((3, 5), 10)
    top[:, 0], top[:, 4] = 500, -400
    step, flags, counts, hi, lo_ = _derive(top)
    assert step[:, 0].tolist() == [490] * 3 and step[:, 4].tolist() == [0] * 3 and step[:, 3].tolist() == [410] * 3 and step[:, 1].tolist() == [0] * 3
    assert (flags[:, 0] == hm.STEP).all() and (flags[:, 4] == hm.HOLE).all() and (flags[:, 3] == hm.STEP).all() and (flags[:, 1:3] == 0).all()
    assert counts == (15, 6, 0, 3) and (hi, lo_) == (500, -400)
    top = np.full((4, 3), 10)  # likewise the first and the last row
    top[0, :], top[3, :] = 500, -400
    assert _derive(top)[0][0].tolist() == [490] * 3 and _derive(top)[0][3].tolist() == [0] * 3
    # a 1 x 1 grid: no neighbour, no step; an unknown cell is 255 and counts nowhere
    step, flags, counts, hi, lo_ = _derive([[700]])
    assert step.tolist() == [[0]] and flags.tolist() == [[0]] and counts == (1, 0, 0, 0) and (hi, lo_) == (700, 700)
    step, flags, counts, hi, lo_ = _derive([[N]], bot=[[N]], ceil=[[300]])
    assert step.tolist() == [[0]] and flags.tolist() == [[255]] and counts == (0, 0, 0, 0) and (hi, lo_) == (0, 0)
    # unknown neighbours are skipped: the centre stands 100 above its only known neighbour; a cell without one has step 0
    step, flags, _, _, _ = _derive([[N, N, N], [N, 300, N], [N, N, 200]])
    assert step.tolist() == [[0, 0, 0], [0, 100, 0], [0, 0, 0]] and flags[1, 1] == hm.STEP and flags[2, 2] == 0 and flags[0, 0] == 255
    assert _derive([[N, N, N], [N, 300, N], [N, N, N]])[0][1, 1] == 0
    # the upper cell of the edge is the blocked one, whichever side it is on
    _, flags, _, _, _ = _derive([[0, 0, 100, 100]])
    assert flags.tolist() == [[0, 0, hm.STEP, 0]]
    # each flag on its threshold and one unit beside it
    assert _derive([[0, 20]])[1].tolist() == [[0, 0]] and _derive([[0, 21]])[1].tolist() == [[0, hm.STEP]]
    assert _derive([[5]], ceil=[[205]])[1].tolist() == [[0]] and _derive([[5]], ceil=[[204]])[1].tolist() == [[hm.HEADROOM]]
    assert _derive([[5]], ceil=[[hm.NO_CEIL]], robot_height_q=hm.Q_MAX)[1].tolist() == [[0]]
    assert _derive([[0]], bot=[[-20]])[1].tolist() == [[0]] and _derive([[0]], bot=[[-21]])[1].tolist() == [[hm.HOLE]]
    assert _derive([[0, 30]], bot=[[-30, 30]], ceil=[[50, 60]])[1].tolist() == [[hm.HOLE | hm.HEADROOM, hm.STEP | hm.HEADROOM]]
    assert _derive([[0, 30]], max_step_q=0, max_drop_q=0, robot_height_q=0)[1].tolist() == [[0, hm.STEP]]


# ---- a physical scene -----------------------------------------------------------------------------------------------------
SCENE_K, SCENE_CALIB, SCENE_CROP, SCENE_PADDED = (110.0, 110.0, 80.0, 60.0), 50.0, (120, 160), (128, 192)
CELL, GRID = 0.2, 40
BIG = 50.0
BOX, KERB, PIT, BEAM = 0.50, 0.08, -0.30, 2.10
# solids (x0, x1, y0, y1, z0, z1) in the world: Y up, the floor Y = 0; no face lies on a cell edge
BOX_XZ, KERB_XZ, PIT_XZ, BEAM_XZ = (-1.3, -0.5, 2.9, 3.7), (0.7, 1.5, 2.9, 3.7), (-0.3, 0.5, 2.9, 4.1), (-1.5, 1.5, 5.1, 5.5)
SOLIDS = [(-BIG, BIG, -10.0, 0.0, -BIG, PIT_XZ[2]), (-BIG, BIG, -10.0, 0.0, PIT_XZ[3], BIG), (-BIG, PIT_XZ[0], -10.0, 0.0, PIT_XZ[2], PIT_XZ[3]),
          (PIT_XZ[1], BIG, -10.0, 0.0, PIT_XZ[2], PIT_XZ[3]), (PIT_XZ[0], PIT_XZ[1], -10.0, PIT, PIT_XZ[2], PIT_XZ[3]),
          BOX_XZ[:2] + (0.0, BOX) + BOX_XZ[2:], KERB_XZ[:2] + (0.0, KERB) + KERB_XZ[2:], BEAM_XZ[:2] + (BEAM, BEAM + 0.2) + BEAM_XZ[2:]]
# (x, z, height, yaw, pitch, roll): the camera walks towards the features while it pitches and rolls
# (lm.camera_to_world turns the optical axis upwards for a positive pitch: these cameras look down by 0.07 to 0.13)
SCENE_WALK = [(0.00, 0.0, 1.20, 0.00, -0.10, 0.00), (0.03, 0.3, 1.22, 0.03, -0.13, 0.02), (-0.02, 0.6, 1.19, -0.04, -0.08, -0.03),
              (0.04, 0.9, 1.21, 0.05, -0.12, 0.03), (0.00, 1.2, 1.18, -0.02, -0.07, -0.02), (-0.03, 1.5, 1.20, 0.02, -0.11, 0.01)]


def _render(C, o):
    """fp64 depth along the camera's z axis of the nearest solid per pixel (inf: none), by slabs."""
    h, w = SCENE_CROP
    fx, fy, cx, cy = SCENE_K
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ray = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1) @ C.T  # world directions, camera z = 1
    depth = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for x0, x1, y0, y1, z0, z1 in SOLIDS:
            t0 = (np.array([x0, y0, z0]) - o) / ray
            t1 = (np.array([x1, y1, z1]) - o) / ray
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit = (near <= far) & (near > 1e-9)
            depth = np.where(hit & (near < depth), near, depth)
    return depth


def _scene_frames():
    """Per frame: the case (fp32 disparity, labels by codd_ground_plane's rule on the exact plane), the fp64 disparity, the ego
    record."""
    cams = [(lm.camera_to_world(yaw, pitch, roll), np.array([x, hgt, z])) for x, z, hgt, yaw, pitch, roll in SCENE_WALK]
    frames = []
    for i, (C, o) in enumerate(cams):
        rec = lm.floor_record(C, o[1])
        rec[0:3] = -(SCENE_CALIB / o[1]) * np.array([rec[8] / SCENE_K[0], rec[9] / SCENE_K[1], rec[10]])
        with np.errstate(all="ignore"):
            d64 = np.where(np.isfinite(_render(C, o)), SCENE_CALIB / _render(C, o), 0.0)
        c = lm.make(f"scene-{i}", np.full(SCENE_CROP, hm.INVALID, np.uint8), d64.astype(f32), rec=rec, K=SCENE_K, calib=SCENE_CALIB,
                    padded=SCENE_PADDED, gh=GRID, gw=GRID, cell=CELL)
        ys, xs = np.nonzero(d64 > 0)
        _, hgt, _, _ = hm.lo.pixel_terms(c, ys, xs)
        lab = np.where(np.abs(hgt) <= f32(0.05), hm.FLOOR, np.where(hgt > f32(2.0), hm.OVERHEAD, np.where(hgt > 0, hm.OBSTACLE, hm.BELOW)))
        c["labels"][ys, xs] = lab
        frames.append((c, d64, None if i == 0 else lm.ego_between(*cams[i - 1], C, o)))
    C0, o0 = cams[0]
    rec0 = lm.floor_record(C0, o0[1])
    f0, r0 = C0 @ rec0[22:25], C0 @ np.cross(rec0[22:25], rec0[8:11])
    assert np.allclose(r0, (1, 0, 0), atol=1e-15) and np.allclose(f0, (0, 0, 1), atol=1e-15)  # the map's axes are the world's
    return frames


def _cells(x0, x1, z0, z1, margin):
    """World cells (ix, iz) inside the rectangle, ``margin`` cells away from its sides."""
    ix = range(int(np.ceil(x0 / CELL - 1e-9)) + margin, int(np.floor(x1 / CELL + 1e-9)) - margin)
    iz = range(int(np.ceil(z0 / CELL - 1e-9)) + margin, int(np.floor(z1 / CELL + 1e-9)) - margin)
    return [(i, j) for j in iz for i in ix]


def test_physical_scene():
    """A level floor, a 0.50 box, a 0.08 kerb, a pit of -0.30 and a beam whose underside is at 2.10, seen by a camera that walks
    1.5 towards them in six frames while pitch and roll change.  Afterwards the cells inside each feature hold its height within
    h_res / 2 + the dead band (one unit at alpha 128) + the fp32 rounding of hgt, the last measured here against an fp64
    evaluation of the same pixels from the unrounded disparity.  Observed: rounding 4.1e-7 and a largest deviation of 0.0000
    (every feature sits on a whole unit of h_res and every frame's extreme quantises to it) against a bound of 0.0075."""
    hp = dict(HP)
    res = hp["h_res"]
    frames = _scene_frames()
    par = frames[0][0]["par"]
    layers = {k: np.zeros((GRID, GRID), np.uint8 if k == "hage" else np.int16) for k in hm.LAYERS}
    st = lm.empty_state()
    rounding = 0.0
    for i, (c, d64, ego) in enumerate(frames):
        st, r = hm.step(c, st, layers, par, hp, ego, fresh=i == 0)
        assert st[lm.INTEGRATED] == 1 and (i == 0 or st[lm.LINKED] == 1)
        layers = {k: r[k] for k in hm.LAYERS}
        a = r["assign"]
        rec, (fx, fy, cx, cy) = c["rec"], SCENE_K
        d = d64[a["ys"], a["xs"]]
        exact = rec[11] * (d - ((rec[0] * (a["xs"] - cx) + rec[1] * (a["ys"] - cy)) + rec[2])) / d
        rounding = max(rounding, float(np.abs(a["hgt"].astype(np.float64) - exact).max()))
    bound = res / 2 + (-(-256 // hp["alpha"]) - 1) * res + rounding
    ix0, iz0 = int(st[lm.IX0]), int(st[lm.IZ0])
    at = lambda k, cell: int(r[k][cell[1] - iz0, cell[0] - ix0])  # noqa: E731
    worst = 0.0
    checks = (("box", "top_out", _cells(*BOX_XZ, 0), BOX), ("box", "bot_out", _cells(*BOX_XZ, 0), BOX),
              ("kerb", "top_out", _cells(*KERB_XZ, 0), KERB), ("kerb", "bot_out", _cells(*KERB_XZ, 0), KERB),
              ("pit", "bot_out", [(i, 19) for i in (-1, 0, 1)], PIT), ("pit", "top_out", [(i, 19) for i in (-1, 0, 1)], PIT),
              ("beam", "ceil_out", _cells(*BEAM_XZ, 0), BEAM), ("floor under the beam", "top_out", _cells(*BEAM_XZ, 0), 0.0),
              ("floor", "top_out", [(i, 12) for i in range(-6, 7)], 0.0))
    for name, k, cells, want in checks:
        assert len(cells) >= 3, name
        for cell in cells:
            v = at(k, cell)
            assert v not in (hm.NONE, hm.NO_CEIL), f"{name}: {k} of cell {cell} was never observed"
            worst = max(worst, abs(v * res - want))
            assert abs(v * res - want) <= bound, f"{name}: {k} of cell {cell} is {v * res:.4f}, {want} expected within {bound:.2e}"
    print(f"physical scene: fp32 rounding of hgt {rounding:.2e}; largest deviation {worst:.4f} against the bound {bound:.4f}")
    flags = r["flags_out"]
    fl = lambda cell: int(flags[cell[1] - iz0, cell[0] - ix0])  # noqa: E731
    # the box's edge cells towards the camera and towards the free floor on its right carry STEP, the kerb's none
    box_edge = [(-3, j) for j in (15, 16, 17)] + [(i, 14) for i in (-6, -5, -4)]
    assert all(fl(cell) & hm.STEP for cell in box_edge), [fl(cell) for cell in box_edge]
    kerb_all = _cells(KERB_XZ[0] - CELL, KERB_XZ[1] + CELL, KERB_XZ[2] - CELL, KERB_XZ[3] + CELL, 0)
    assert all(fl(cell) in (0, 255) for cell in kerb_all), [fl(cell) for cell in kerb_all]
    assert sum(fl(cell) == 0 for cell in kerb_all) >= 12
    assert all(fl((i, 19)) & hm.HOLE for i in (-1, 0, 1)) and not any(fl(cell) & hm.HOLE for cell in box_edge + kerb_all)
    # the beam: headroom is missing only for a robot taller than 2.10
    under = _cells(*BEAM_XZ, 0)
    assert all(fl(cell) == 0 for cell in under)
    for robot, missing in ((2.10, False), (2.105, True), (2.2, True)):
        q = hm.thresholds(res, 0.10, robot, 0.10)
        _, f2, _, _, _ = hm.derive(r["top_out"], r["bot_out"], r["ceil_out"], dict(hp, robot_height_q=q[1]))
        assert all(bool(f2[cell[1] - iz0, cell[0] - ix0] & hm.HEADROOM) == missing for cell in under), (robot, missing)


# ---- plumbing -------------------------------------------------------------------------------------------------------------
class _WithMotion:
    motion = object()


def test_check_heightmap():
    assert live._check_heightmap(None) is None and live._check_heightmap(False) is None
    assert live._check_heightmap(True) == live.HEIGHTMAP_DEFAULTS and live._check_heightmap(True) is not live.HEIGHTMAP_DEFAULTS
    assert live.HEIGHTMAP_DEFAULTS == dict(h_res=0.005, select=("floor", "obstacle", "below"), min_pixels=4, alpha=128, max_step=0.10,
                                           robot_height=1.0, max_drop=0.10)
    assert live.select_mask(live.HEIGHTMAP_DEFAULTS["select"]) == ops.HEIGHT_PARAMS["select"] == hm.SURFACES
    assert {k: v for k, v in live.HEIGHTMAP_DEFAULTS.items() if k != "select"} == {k: v for k, v in ops.HEIGHT_PARAMS.items() if k != "select"}
    p = live._check_heightmap(dict(select="obstacle", alpha=np.int64(256), h_res=1, max_step=0))
    assert p["select"] == ("obstacle",) and p["alpha"] == 256 and type(p["alpha"]) is int and p["h_res"] == 1.0 and p["max_step"] == 0.0
    assert live._check_heightmap(dict(select=()))["select"] == ()
    for lmap in (None, False):
        with pytest.raises(ValueError, match="heightmap: needs localmap"):
            live._check_heightmap(True, lmap)
    with pytest.raises(ValueError, match="overhead"):
        live._check_heightmap(dict(select=("floor", "overhead")))
    for bad in (3, "yes", dict(rays=4), dict(h_res=0), dict(h_res=-1.0), dict(h_res=float("nan")), dict(h_res=float("inf")),
                dict(h_res="fine"), dict(h_res=True), dict(select=("wall",)), dict(select=3), dict(min_pixels=0), dict(min_pixels=2.0),
                dict(min_pixels=True), dict(alpha=0), dict(alpha=257), dict(alpha=1.0), dict(max_step=-0.01), dict(max_step=161.0),
                dict(max_step=float("nan")), dict(robot_height=-1), dict(robot_height=1e9), dict(max_drop=-0.1), dict(max_drop=float("inf")),
                dict(max_drop=None)):
        with pytest.raises(ValueError, match="heightmap"):
            live._check_heightmap(bad)


def test_session_constructor():
    est = _WithMotion()
    for hmap in (True, dict(alpha=64)):
        with pytest.raises(ValueError, match="heightmap: needs localmap"):
            live.LiveSession(None, (8, 8), heightmap=hmap)
        with pytest.raises(ValueError, match="heightmap: needs localmap"):
            live.LiveSession(est, (8, 8), ground=True, egomotion=True, heightmap=hmap)
    with pytest.raises(ValueError, match="heightmap: unknown keys"):
        live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True, heightmap=dict(rays=4))
    with pytest.raises(ValueError, match="overhead"):
        live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True, heightmap=dict(select=("overhead",)))
    s = live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=dict(grid=(8, 12), cell=0.2, range_max=9.0),
                         heightmap=dict(select=("obstacle", "below"), alpha=64))
    assert not s._open_done and s.heightmap["alpha"] == 64
    assert s._height_par == dict(h_res=0.005, min_pixels=4, alpha=64, max_step=0.10, robot_height=1.0, max_drop=0.10,
                                 select=(1 << 1) | (1 << 3), cell=0.2, range_min=0.0, range_max=9.0)
    assert live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True).heightmap is None
    assert live.HeightMap._fields == ("top", "bot", "ceil", "top_q", "bot_q", "ceil_q", "age", "step", "flags", "integrated",
                                      "surface_pixels", "overhead_pixels", "observed", "known", "steps", "headroom", "holes", "top_max",
                                      "bot_min", "origin", "cell", "h_res")


_REF = {}


def _ref(name):
    if name not in _REF:
        c = hm.CASES[hm.NAMES[name]]
        _REF[name] = (c, hm.reference(c)[1])
    return _REF[name]


def _buffers(r):
    return [r["record"]] + [r[k] for k in hm.OUTPUTS]


def test_heightmap_from_buffers():
    c, r = _ref("overhead-only")
    m = live.heightmap_from_buffers(*_buffers(r), 0.5, 0.005)
    assert isinstance(m, live.HeightMap) and m.top_q.tobytes() == r["top_out"].tobytes() and m.ceil_q.tobytes() == r["ceil_out"].tobytes()
    assert m.top_q.dtype == np.int16 and m.age.dtype == np.uint8 and m.step.dtype == np.uint16 and m.flags.dtype == np.uint8
    assert not np.shares_memory(m.top_q, r["top_out"]) and m.top.dtype == m.bot.dtype == m.ceil.dtype == np.float32
    assert np.array_equal(np.isnan(m.top), r["top_out"] == hm.NONE) and np.array_equal(np.isnan(m.ceil), r["ceil_out"] == hm.NO_CEIL)
    known = r["top_out"] != hm.NONE
    assert known.any() and not known.all() and np.array_equal(m.top[known], r["top_out"][known].astype(f32) * f32(0.005))
    assert np.array_equal(m.bot[known], r["bot_out"][known].astype(f32) * f32(0.005))
    rec = r["record"]
    assert m.integrated is True and (m.surface_pixels, m.overhead_pixels, m.observed, m.known, m.steps, m.headroom, m.holes) == tuple(
        int(v) for v in rec[1:8])
    assert m.known == int(known.sum()) and m.top_max == rec[8] * 0.005 and m.bot_min == rec[9] * 0.005 and m.top_max == int(r["top_out"][known].max()) * 0.005
    assert m.origin == (int(rec[10]), int(rec[11])) and m.cell == 0.5 and m.h_res == 0.005
    assert np.array_equal(m.traversable(), r["flags_out"] == 0) and m.traversable().dtype == bool
    assert m.world_xz(0, 0) == ((m.origin[0] + 0.5) * 0.5, (m.origin[1] + 0.5) * 0.5)
    # a cell over which only overhead pixels were seen carries its ceil and is not known
    only = (r["ceil_out"] != hm.NO_CEIL) & ~known
    assert only.any() and (m.flags[only] == 255).all() and np.isfinite(m.ceil[only]).all()


class _Done:
    def synchronize(self):
        pass


def test_tuple_order():
    """result, ego, ground, localmap, heightmap -- and with costmap= and plan= the HeightMap still comes last, behind the Plan:
    the collection step on host buffers standing in for the downloads."""
    import torch
    c, r = _ref("forward")
    mref = lm.reference(c)
    lmap = dict(grid=(16, 24), cell=0.5)

    def session(**kw):
        s = live.LiveSession(_WithMotion(), (6, 8), ground=True, egomotion=True, localmap=lmap, heightmap=True, **kw)
        s._e_down, s._h_out = [_Done(), _Done()], [torch.zeros(6, 8)] * 2
        s._h_ground = [[torch.zeros(32, dtype=torch.float64), torch.zeros(6, 8, dtype=torch.uint8)]] * 2
        s._has_ego = [False, False]
        s._h_map = [[torch.from_numpy(mref[k].copy()) for k in ("record", "map_out", "age_out")]] * 2
        s._h_height = [[torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if v.dtype == np.uint16 else v.copy()) for v in _buffers(r)]] * 2
        s._inflight.append(0)
        return s

    s = session()
    got = s.pop()
    assert isinstance(got, tuple) and len(got) == 5 and got[1] is None and isinstance(got[2], live.Ground)
    assert isinstance(got[3], live.LocalMap) and isinstance(got[4], live.HeightMap)
    s._h_height[0][1].zero_()  # the result is the caller's: the session's slot may be reused
    assert got[4].top_q.tobytes() == r["top_out"].tobytes() and got[4].step.tobytes() == r["step_out"].tobytes()
    assert got[4].step.dtype == np.uint16 and got[4].cell == 0.5 and got[4].h_res == 0.005 and got[4].origin == got[3].origin
    s = session(costmap=True, plan=True)
    gh, gw = 16, 24
    s._h_cost = [[torch.zeros(16, dtype=torch.float64), torch.zeros(gh, gw, dtype=torch.int32), torch.zeros(gh, gw, dtype=torch.uint8),
                  torch.zeros(gh, gw, dtype=torch.uint8)]] * 2
    s._h_plan = [[torch.zeros(16, dtype=torch.float64), torch.zeros(gh, gw, dtype=torch.int32), torch.full((1024,), -1, dtype=torch.int32)]] * 2
    got = s.pop()
    assert len(got) == 7 and [type(v).__name__ for v in got[3:]] == ["LocalMap", "CostMap", "Plan", "HeightMap"]
    assert got[4].origin == got[5].origin == got[3].origin == got[6].origin


def test_entries_are_bound():
    from codd_amd import _abi
    _abi.load()
    assert not _abi.MISSING and _abi.load().codd_abi_version() == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_hip.h")).read()
    for name in ("codd_height_map_scratch", "codd_height_map"):
        assert name in _abi.SIGNATURES and f" {name}(" in header
    assert len(_abi.SIGNATURES["codd_height_map"][1]) == 39
    for name, v in (("STEP", ops.HEIGHT_STEP), ("HEADROOM", ops.HEIGHT_HEADROOM), ("HOLE", ops.HEIGHT_HOLE)):
        assert f"#define CODD_HEIGHT_{name} {v}\n" in header
    assert (ops.HEIGHT_NONE, ops.HEIGHT_NO_CEIL, ops.HEIGHT_Q_MAX, ops.HEIGHT_UNKNOWN) == (hm.NONE, hm.NO_CEIL, hm.Q_MAX, hm.UNKNOWN)


def test_entry_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    import ctypes as C
    from codd_amd import _abi
    lib = _abi.load()
    scr = lib.codd_height_map_scratch
    assert scr(0, 4) == -1 and scr(4, 0) == -1 and scr(4097, 4) == -1 and scr(4, 4097) == -1 and scr(4096, 2048) == -1
    assert scr(1, 1) == 100 and scr(16, 24) == 80 + 20 * 16 * 24 and scr(4096, 1024) == scr(2048, 2048) == 80 + 20 * 2 ** 22
    need = scr(16, 24)
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    base = buf.ctypes.data + (-buf.ctypes.data) % 8
    p, odd2, odd8 = C.c_void_p(base), C.c_void_p(base + 1), C.c_void_p(base + 4)
    nan, inf = float("nan"), float("inf")
    pointers = ("disp", "labels", "record", "state", "top", "bot", "ceil", "hage", "scratch", "top_out", "bot_out", "ceil_out", "hage_out",
                "step_out", "flags_out", "rec")

    def call(H=64, W=64, h=24, w=40, fx=40.0, fy=40.0, cx=20.0, cy=8.0, calib=20.0, gh=16, gw=24, cell=0.5, range_min=0.0,
             range_max=12.8, h_res=0.005, select=hm.SURFACES, min_pixels=4, alpha=128, max_step_q=20, robot_height_q=200, max_drop_q=20,
             nbytes=need, **ptr):
        assert set(ptr) <= set(pointers)
        a = {k: ptr.get(k, p) for k in pointers}
        return lib.codd_height_map(a["disp"], H, W, h, w, fx, fy, cx, cy, calib, a["labels"], a["record"], a["state"], gh, gw, cell,
                                   range_min, range_max, h_res, select, min_pixels, alpha, max_step_q, robot_height_q, max_drop_q,
                                   a["top"], a["bot"], a["ceil"], a["hage"], a["scratch"], nbytes, a["top_out"], a["bot_out"],
                                   a["ceil_out"], a["hage_out"], a["step_out"], a["flags_out"], a["rec"], None)

    for name in pointers:
        assert call(**{name: None}) == -1, name
    for name in ("top", "bot", "ceil", "top_out", "bot_out", "ceil_out", "step_out"):  # int16 planes on an odd address
        assert call(**{name: odd2}) == -1, name
    for name in ("record", "state", "rec"):  # doubles off their alignment
        assert call(**{name: odd8}) == -1 and call(**{name: odd2}) == -1, name
    for bad in (dict(h=0), dict(w=0), dict(H=0), dict(W=-3), dict(h=65), dict(w=65), dict(H=65536, W=32768, h=65536, w=32768),
                dict(gh=0), dict(gw=0), dict(gh=4097), dict(gw=4097), dict(gh=4096, gw=2048, nbytes=1 << 40), dict(cell=0.0),
                dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(range_max=0.0), dict(range_max=nan), dict(range_max=inf),
                dict(range_min=-0.5), dict(range_min=nan), dict(range_min=12.8), dict(range_min=13.0), dict(fx=0.0), dict(fy=nan),
                dict(calib=inf), dict(cx=nan), dict(cy=inf), dict(h_res=0.0), dict(h_res=-0.005), dict(h_res=nan), dict(h_res=inf),
                dict(select=1 << hm.OVERHEAD), dict(select=hm.SURFACES | (1 << hm.OVERHEAD)), dict(select=0xFFFFFFFF), dict(min_pixels=0),
                dict(min_pixels=-5), dict(alpha=0), dict(alpha=257), dict(alpha=-128), dict(max_step_q=-1), dict(max_step_q=32001),
                dict(robot_height_q=-1), dict(robot_height_q=32001), dict(max_drop_q=-1), dict(max_drop_q=32001),
                dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**bad) == -1, bad


def test_cli_heightmap_arguments():
    from codd_amd import inference
    base = ["--img-dir", "x", "--r-img-dir", "y"]
    for argv in (["--heightmap"], ["--live", "--heightmap"], ["--live", "--ground", "--ego", "--heightmap"],
                 ["--live", "--ground", "--heightmap"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)
    assert inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap", "--heightmap"]).heightmap
    assert inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap", "--costmap", "--plan", "--heightmap"]).heightmap
    assert not inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap"]).heightmap
