"""LiveSession local map on the CPU: the restatement of tests/live_localmap_ref.py itself -- planted camera poses over a
plane recover the planted planar increments within a bound derived from the fp32 rounding of the ego record; a map
integrated through the scrolling toroidal window equals, cell for cell, the crop of a map kept in one large fixed array
indexed by world cell; the order and the saturation of the update rule; a LOST frame under both policies and the carried
floor frame; what the planted cases are built to show -- and _check_localmap, the LiveSession constructor,
localmap_from_buffers, the tuple order, the bindings, the entry's argument checks (no launch) and the command line's
arguments.  Nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_localmap_ref as lm  # noqa: E402
import live_scan_ref as ls  # noqa: E402
from codd_amd import live, ops  # noqa: E402

f32 = np.float32
_REF = {}


def _ref(name):
    if name not in _REF:
        c = lm.CASES[lm.NAMES[name]]
        _REF[name] = (c, lm.reference(c))
    return _REF[name]


# ---- launch 1: planted poses ----------------------------------------------------------------------------------------------
# (x, z, height, yaw, pitch, roll) of a camera walking a curve while it pitches and rolls
WALK = [(0.0, 0.0, 1.20, 0.00, 0.15, 0.03), (0.1, 0.6, 1.22, 0.10, 0.11, -0.02), (0.35, 1.3, 1.18, 0.25, 0.20, 0.05),
        (0.8, 1.9, 1.21, 0.45, 0.13, 0.00), (1.5, 2.3, 1.19, 0.70, 0.17, -0.04), (2.2, 2.4, 1.20, 1.00, 0.09, 0.02),
        (2.9, 2.1, 1.23, 1.40, 0.15, 0.06), (3.3, 1.4, 1.20, 1.90, 0.18, -0.03)]


def _walk(drop_floor=()):
    """The states of the restatement's launch 1 along WALK, and what was planted: per frame the foot point and the heading
    in the first frame's floor axes, and the fp32 ego records."""
    par = dict(lm.DEFAULTS)
    cams = [(lm.camera_to_world(yaw, pitch, roll), np.array([x, h, z])) for x, z, h, yaw, pitch, roll in WALK]
    up = np.array([0.0, 1.0, 0.0])
    fw = []
    for C, o in cams:
        rec = lm.floor_record(C, o[1])
        fw.append((C @ rec[22:25], C @ np.cross(rec[22:25], rec[8:11])))  # the floor-forward and floor-right axes in the world
        assert abs(fw[-1][0] @ up) < 1e-14 and abs(fw[-1][1] @ up) < 1e-14
    f0, r0 = fw[0]
    st = lm.empty_state()
    states, want, egos = [], [], []
    for i, (C, o) in enumerate(cams):
        rec = lm.floor_record(C, o[1])
        if i in drop_floor:
            rec[3] = 0.0
        ego = None if i == 0 else lm.ego_between(*cams[i - 1], C, o)
        st = lm.pose(st, ego, rec, i == 0, par)
        states.append(st)
        egos.append(ego)
        want.append((np.array([(o - cams[0][1]) @ r0, (o - cams[0][1]) @ f0]), np.array([fw[i][0] @ r0, fw[i][0] @ f0])))
    return states, want, egos, cams


def test_planted_poses_recover_the_planar_increments():
    """The bound.  In exact arithmetic the step is exact: c = C_prev^T (o_cur - o_prev), r_p and f_p are horizontal, so dx and
    dz are the horizontal displacement in the previous floor axes whatever pitch and roll did.  What is not exact is the ego
    record, fp32: each component of t carries at most 2^-24 |t_i|, so |dt| <= sqrt(3) 2^-24 max|t_i|; each component of the
    unit q at most 2^-25, so |dq| <= 2^-24 and the rotation is off by at most an angle of 2 |dq| = 2^-23, which moves c = -R^T t
    by at most 2^-23 |t| and the heading by at most 2^-23 per step.  A heading that is off by k 2^-23 after k steps
    misplaces the next step by k 2^-23 |step|.  The fp64 operations add less than 1e-13."""
    states, want, egos, cams = _walk()
    pos_bound, head_bound = 1e-13, 1e-13
    for i in range(1, len(states)):
        st = states[i]
        assert st[lm.LINKED] == 1 and st[lm.INTEGRATED] == 1 and st[lm.RESTARTS] == 1 and st[lm.FRAMES] == i
        t = egos[i][0:3].astype(np.float64)
        tn = np.sqrt(t @ t)
        pos_bound += np.sqrt(3.0) * 2.0 ** -24 * np.abs(t).max() + 2.0 ** -23 * tn + (i - 1) * 2.0 ** -23 * tn
        head_bound += 2.0 ** -23
        p, h = np.array([st[lm.PX], st[lm.PZ]]), np.array([st[lm.HX], st[lm.HZ]])
        perr, herr = np.abs(p - want[i][0]).max(), np.abs(h - want[i][1]).max()
        print(f"frame {i}: p {p.tolist()} planted {want[i][0].tolist()}: off by {perr:.3e} (bound {pos_bound:.3e}); heading off by "
              f"{herr:.3e} (bound {head_bound:.3e})")
        assert perr <= pos_bound and herr <= head_bound
        assert abs(np.hypot(*h) - 1.0) < 2e-15
        # the step itself, in the previous frame's floor axes
        d = cams[i][1] - cams[i - 1][1]
        C = cams[i - 1][0]
        rec = lm.floor_record(C, 1.0)
        fwd, right = C @ rec[22:25], C @ np.cross(rec[22:25], rec[8:11])
        step_bound = (np.sqrt(3.0) * 2.0 ** -24 * np.abs(t).max() + 2.0 ** -23 * tn) + 1e-13
        assert abs(st[lm.DX] - d @ right) <= step_bound and abs(st[lm.DZ] - d @ fwd) <= step_bound
    assert np.abs(want[-1][0]).max() > 1.0 and abs(want[-1][1][1]) < 0.5  # the walk went somewhere and turned


def test_a_frame_without_a_floor_carries_the_stored_one():
    """Ground ok = 0 in frames 3 and 4: the floor frame stored is the last one carried through G -- the true normal and
    height of those frames within the fp32 rounding of the ego record (2^-23 per step on n, sqrt(3) 2^-24 max|t_i| + 2^-23 |t| on
    Hc) -- nothing is integrated, and the pose goes on within the bound of the test above."""
    states, want, egos, cams = _walk(drop_floor=(3, 4))
    full = _walk()[0]
    nb = hb = 1e-13
    for i in (3, 4):
        st = states[i]
        C, o = cams[i]
        t = egos[i][0:3].astype(np.float64)
        nb += 2.0 ** -23
        hb += np.sqrt(3.0) * 2.0 ** -24 * np.abs(t).max() + 2.0 ** -22 * np.sqrt(t @ t)
        true = lm.floor_record(C, o[1])
        assert st[lm.LINKED] == 1 and st[lm.INTEGRATED] == 0 and st[lm.EXISTS] == 1
        assert np.abs(st[lm.N:lm.N + 3] - true[8:11]).max() <= nb and abs(st[lm.HC] - o[1]) <= hb
        assert np.abs(st[lm.F:lm.F + 3] - true[22:25]).max() <= 4 * nb
        # (a normal off by 2^-22 tilts the axes the step is read in by as much: far below 1e-5 of a step of length 1)
        assert abs(st[lm.PX] - full[i][lm.PX]) < 1e-5 and abs(st[lm.PZ] - full[i][lm.PZ]) < 1e-5
    assert states[5][lm.INTEGRATED] == 1 and states[5][lm.N:lm.N + 3].tolist() == lm.floor_record(*[cams[5][0], cams[5][1][1]])[8:11].tolist()


def test_lost_frames_under_both_policies():
    par = dict(lm.DEFAULTS)
    rec = ls.flat_record()
    none = np.where(np.arange(32) == 3, 0.0, rec)
    st = lm.planted_state(par, p=(0.3, 0.7), h=(0.6, 0.8))
    fwd = lm.ego_record(t=(0.0, 0.0, -1.25))
    bad = lm.ego_record(t=(0.0, 0.0, -1.25), ok=0.0)
    zero_q = lm.ego_record(t=(0.0, 0.0, -1.25), q=(0, 0, 0, 0))
    ok = lm.pose(st, fwd, rec, False, par)
    assert ok[lm.LINKED] == 1 and (ok[lm.DX], ok[lm.DZ]) == (0.0, 1.25) and ok[lm.RESTARTS] == 1 and ok[lm.FRAMES] == 4
    assert np.allclose([ok[lm.PX], ok[lm.PZ]], [0.3 + 1.25 * 0.6, 0.7 + 1.25 * 0.8], atol=1e-15) and np.allclose([ok[lm.HX], ok[lm.HZ]], [0.6, 0.8], atol=1e-15)
    assert (ok[lm.PIX0], ok[lm.PIZ0]) == (st[lm.IX0], st[lm.IZ0]) and ok[lm.CLEARED] == 0
    for ego in (None, bad, zero_q):
        r = lm.pose(st, ego, rec, False, dict(par, lost=lm.RESET))
        assert r[lm.CLEARED] == 1 and r[lm.LINKED] == 0 and r[lm.EXISTS] == 1 and r[lm.INTEGRATED] == 1
        assert (r[lm.PX], r[lm.PZ], r[lm.HX], r[lm.HZ]) == (0, 0, 0, 1) and r[lm.RESTARTS] == 2 and r[lm.FRAMES] == 0
        assert (r[lm.IX0], r[lm.IZ0]) == (-12, -8)
        h = lm.pose(st, ego, rec, False, dict(par, lost=lm.HOLD))
        assert h[lm.CLEARED] == 0 and h[lm.LINKED] == 0 and h[lm.INTEGRATED] == 1 and h[lm.RESTARTS] == 1 and h[lm.FRAMES] == 4
        assert h[1:7].tolist() == st[1:7].tolist() and (h[lm.DX], h[lm.DZ]) == (0, 0)
        r = lm.pose(st, ego, none, False, dict(par, lost=lm.RESET))  # lost and no floor: the state is marked empty
        assert r[lm.CLEARED] == 1 and r[lm.EXISTS] == 0 and r[lm.INTEGRATED] == 0 and r[lm.RESTARTS] == 2 and not r[lm.N:lm.F + 3].any()
        again = lm.pose(r, fwd, none, False, par)  # nothing to lose: not another restart
        assert again[lm.EXISTS] == 0 and again[lm.RESTARTS] == 2 and again[lm.CLEARED] == 1
        found = lm.pose(again, fwd, rec, False, par)  # a floor again: the map starts here
        assert found[lm.EXISTS] == 1 and found[lm.INTEGRATED] == 1 and found[lm.LINKED] == 0 and found[lm.RESTARTS] == 2
        h = lm.pose(st, ego, none, False, dict(par, lost=lm.HOLD))  # held without a floor: the stored frame stays
        assert h[lm.EXISTS] == 1 and h[lm.INTEGRATED] == 0 and h[lm.N:lm.F + 3].tolist() == st[lm.N:lm.F + 3].tolist()
    for policy in (lm.RESET, lm.HOLD):  # fresh always resets
        r = lm.pose(st, fwd, rec, True, dict(par, lost=policy))
        assert r[lm.CLEARED] == 1 and r[lm.LINKED] == 0 and r[lm.RESTARTS] == 2 and (r[lm.PX], r[lm.PZ]) == (0, 0)
    first = lm.pose(lm.empty_state(), None, rec, True, par)
    assert first[lm.EXISTS] == 1 and first[lm.RESTARTS] == 1 and first[lm.FRAMES] == 0 and first[lm.INTEGRATED] == 1
    # m < 1e-6: the current forward axis stands on the previous floor (a quarter turn about the camera's x axis)
    up = lm.ego_record(q=(np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)))
    r = lm.pose(st, up, rec, False, par)
    assert r[lm.LINKED] == 0 and r[lm.CLEARED] == 1
    far = lm.pose(st, lm.ego_record(t=(0.0, 0.0, -3e9)), rec, False, par)  # beyond 2^30 cells
    assert far[lm.LINKED] == 0 and far[lm.CLEARED] == 1


# ---- the toroidal window against one large fixed array ---------------------------------------------------------------------
def test_scrolling_window_equals_the_crop_of_a_fixed_array():
    """The camera walks over the flat rig's scene by planted steps: forward, back by negative amounts, by exactly gh cells,
    and by more than the window (everything is forgotten), sideways both ways.  Next to the restatement's toroidal storage a
    plain array indexed by world cell keeps the same map: what lies outside the current window is forgotten, the window's
    cells take the update rule, written out here a second time, cell by cell.  The unrolled output equals the crop of that
    array, exactly, after every frame; so does the storage, slot by slot."""
    c0 = lm.CASES[lm.NAMES["identity"]]
    par = dict(c0["par"], gh=8, gw=5, cell=0.5, decay=1, min_pixels=3, select=(1 << lm.OBSTACLE) | (1 << lm.OVERHEAD))
    gh, gw = par["gh"], par["gw"]
    cell = 0.5
    steps = [None, (0.2, 0.3), (0, 0.5), (0, 1.0), (0, -0.5), (0, -2.0), (0.5, 0), (-1.5, 0), (0, gh * cell), (0, -gh * cell), (0, (gh + 3) * cell),
             (-(gw + 2) * cell, -1.0), (1.0, 0.5), (0, 0), (0.5, 0.5), (-0.5, -0.5)]
    BIG, OFF = 96, 48
    bigL, bigA = np.zeros((BIG, BIG), np.int64), np.full((BIG, BIG), 255, np.int64)
    st, L, age = lm.empty_state(), np.zeros((gh, gw), np.int16), np.zeros((gh, gw), np.uint8)
    scrolls = set()
    for i, stp in enumerate(steps):
        ego = None if stp is None else lm.ego_record(t=(-stp[0], 0.0, -stp[1]))
        c = dict(c0, par=par)
        r = lm.step(c, st, L, age, par, ego=ego, fresh=stp is None)
        new = r["state"]
        if i:
            scrolls.add((int(new[lm.IX0] - st[lm.IX0]), int(new[lm.IZ0] - st[lm.IZ0])))
            assert new[lm.LINKED] == 1 and new[lm.CLEARED] == 0
        st, L, age = new, r["logodds"], r["age"]
        x0, z0 = int(st[lm.IX0]) + OFF, int(st[lm.IZ0]) + OFF
        assert 0 <= x0 and x0 + gw <= BIG and 0 <= z0 and z0 + gh <= BIG
        inside = np.zeros((BIG, BIG), bool)
        inside[z0:z0 + gh, x0:x0 + gw] = True
        bigL[~inside], bigA[~inside] = 0, 255
        for j in range(gh):
            for k in range(gw):
                o, f = int(r["O"][j, k]), int(r["F"][j, k])
                v, a = int(bigL[z0 + j, x0 + k]), int(bigA[z0 + j, x0 + k])
                if o >= par["min_pixels"]:
                    v, a = min(v + par["l_occ"], par["l_max"]), 0
                elif f >= par["min_pixels"]:
                    v, a = max(v - par["l_free"], par["l_min"]), 0
                else:
                    a = a if a == 255 else min(a + 1, 254)
                    v = max(v - par["decay"], 0) if v > 0 else min(v + par["decay"], 0)
                bigL[z0 + j, x0 + k], bigA[z0 + j, x0 + k] = v, a
        assert np.array_equal(r["map_out"], bigL[z0:z0 + gh, x0:x0 + gw]), f"frame {i}: the map differs from the fixed array's crop"
        assert np.array_equal(r["age_out"], bigA[z0:z0 + gh, x0:x0 + gw]), f"frame {i}: the ages differ from the fixed array's crop"
        for j in range(gh):  # the storage: world cell (ix, iz) at row iz mod gh, column ix mod gw
            for k in range(gw):
                ix, iz = int(st[lm.IX0]) + k, int(st[lm.IZ0]) + j
                assert L[iz % gh, ix % gw] == r["map_out"][j, k] and age[iz % gh, ix % gw] == r["age_out"][j, k]
        assert r["record"][10] == r["O"].sum() + r["F"].sum() and r["record"][13] == (r["age_out"] == 255).sum()
    print(f"scrolls (cells in x, z): {sorted(scrolls)}; final map\n{r['map_out']}")
    assert (0, -gh) in scrolls and (0, gh) in scrolls and (0, gh + 3) in scrolls and any(s[0] < -gw for s in scrolls)
    assert any(s[1] < 0 and s[1] > -gh for s in scrolls) and any(s[0] < 0 and s[0] > -gw for s in scrolls) and (0, 0) in scrolls
    assert (r["map_out"] != 0).any() and int(st[lm.IX0]) < 0  # evidence survived the last scrolls; negative world cells were used


# ---- the update rule ------------------------------------------------------------------------------------------------------
def test_update_rule_order_and_saturation():
    par = dict(lm.DEFAULTS, gh=1, gw=12, min_pixels=3, l_occ=5, l_free=4, l_min=-6, l_max=7, decay=2, occ_level=5, free_level=-4)
    st = lm.planted_state(par)
    #              occ+free  occ    occ-sat  free   free-sat  below-min  decay+  decay-  decay-to-0  never  age-sat  free-beats-age
    O = np.array([[3,        9,     3,       0,     2,        2,         0,      0,      0,          0,     0,       0]], np.int32)
    F = np.array([[9,        0,     0,       3,     7,        2,         0,      0,      0,          0,     0,       3]], np.int32)
    L = np.array([[0,        1,     6,       0,     -5,       3,         5,      -5,     1,          0,     -1,      2]], np.int16)
    A = np.array([[9,        255,   3,       255,   0,        7,         0,      253,    254,        255,   254,     254]], np.uint8)
    assert st[lm.IX0] == -6 and st[lm.IZ0] == 0  # L and A above stand in WINDOW order; the storage is rolled by ix0 mod gw = 6
    s = lm.slots(st, par)
    Ls, As = np.zeros(12, np.int16), np.zeros(12, np.uint8)
    Ls[s.ravel()], As[s.ravel()] = L.ravel(), A.ravel()
    u = lm.update(st, Ls.reshape(1, 12), As.reshape(1, 12), O, F, par)
    assert u["map_out"].tolist() == [[5, 6, 7, -4, -6, 1, 3, -3, 0, 0, 0, -2]]
    assert u["age_out"].tolist() == [[0, 0, 0, 0, 0, 8, 1, 254, 254, 255, 254, 0]]
    assert u["counts"] == (int(O.sum() + F.sum()), 3, 2, 1) and s.ravel().tolist() == [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]
    assert u["logodds"].ravel()[s.ravel()].tolist() == u["map_out"].ravel().tolist()
    nodecay = lm.update(st, Ls.reshape(1, 12), As.reshape(1, 12), O, F, dict(par, decay=0))
    assert nodecay["map_out"].tolist() == [[5, 6, 7, -4, -6, 3, 5, -5, 1, 0, -1, -2]]
    wide = lm.update(st, np.full((1, 12), 32767, np.int16), As.reshape(1, 12), np.full((1, 12), 9, np.int32), F, dict(par, l_occ=32767, l_max=32767))
    assert (wide["map_out"] == 32767).all()  # no wrap at the int16 limits
    wide = lm.update(st, np.full((1, 12), -32768, np.int16), As.reshape(1, 12), O * 0, F * 0 + 9, dict(par, l_free=32767, l_min=-32768))
    assert (wide["map_out"] == -32768).all()


def test_what_the_cases_show():
    c, r = _ref("one-cell")
    assert r["F"].max() == 37 * 70 and (r["F"] > 0).sum() == 1 and r["record"][10] == 37 * 70 and r["map_out"].min() == -2
    c, r = _ref("keys64")
    a = r["assign"]
    assert a["ys"].size == 64 and len(set(zip(a["jx"].tolist(), a["jz"].tolist(), a["obst"].tolist()))) == 64
    assert a["ys"].min() == 8 and a["ys"].max() == 15 and a["xs"].min() == 56 and a["xs"].max() == 63  # one wave's block
    c, r = _ref("cell-edge")
    a = r["assign"]
    assert sorted(zip(a["ys"].tolist(), a["xs"].tolist(), a["jx"].tolist(), a["jz"].tolist())) == \
        [(5, 42, 10, 12), (6, 42, 11, 10), (15, 10, 8, 12), (16, 10, 10, 10)]  # (the pixels at gz = 4 lie on the far edge: outside)
    c, r = _ref("bad-disparity")
    assert r["record"][10] == (37 - 5) * 70 and set(r["assign"]["ys"].tolist()) == set(range(37)) - {3, 4, 5, 6, 7}
    c, r = _ref("range-edges")
    assert sorted(set(r["assign"]["ys"].tolist())) == list(range(10, 14)) + list(range(30, 34))  # range_min taken, range_max not
    c, r = _ref("range-edges-in")
    assert sorted(set(r["assign"]["ys"].tolist())) == list(range(20, 24)) + list(range(30, 34))
    for name in ("fresh", "ego-lost-reset", "ego-null-reset", "fresh-hold", "5x3-fresh"):
        c, r = _ref(name)
        assert r["state"][lm.CLEARED] == 1 and r["state"][lm.LINKED] == 0
        seen = r["age_out"] == 0
        assert seen.any() and (r["map_out"][~seen] == 0).all() and (r["age_out"][~seen] == 255).all()
    for name in ("ego-lost-hold", "ego-null-hold"):
        c, r = _ref(name)
        assert r["state"][lm.CLEARED] == 0 and r["state"][lm.LINKED] == 0
        assert r["map_out"].tobytes() == _ref("identity")[1]["map_out"].tobytes()
    c, r = _ref("window-jump")
    seen = r["age_out"] == 0
    assert r["state"][lm.CLEARED] == 0 and (r["age_out"][~seen] == 255).all() and (r["map_out"][~seen] == 0).all()
    c, r = _ref("negative-cells")
    assert r["state"][lm.IX0] == -18 and r["state"][lm.IZ0] == -12 and 0 < (r["age_out"] == 255).sum() < 16 * 24
    c, r = _ref("ground-lost")
    assert r["state"][lm.INTEGRATED] == 0 and r["state"][lm.LINKED] == 1 and not r["O"].any() and not r["F"].any() and r["record"][10] == 0
    assert (np.abs(r["map_out"]) <= np.maximum(np.abs(c["logodds"]).max() - 3, 0)).all()
    c, r = _ref("lost-and-no-floor")
    assert r["state"][lm.EXISTS] == 0 and (r["map_out"] == 0).all() and (r["age_out"] == 255).all() and r["record"][13] == 16 * 24
    c, r = _ref("two-labels")
    assert r["O"].sum() > _ref("identity")[1]["O"].sum()
    assert not _ref("floor-only")[1]["O"].any() and _ref("floor-only")[1]["F"].tobytes() == _ref("identity")[1]["F"].tobytes()
    c, r = _ref("saturate")
    assert r["map_out"].max() == 32767 and r["map_out"].min() == -32768
    c, r = _ref("turn")
    assert abs(abs(r["state"][lm.HX]) - 1) < 1e-6 and abs(r["state"][lm.HZ]) < 1e-6 and r["O"].any()
    c, r = _ref("1x1")
    assert r["map_out"].shape == (1, 1) and r["record"][10] > 0
    for c in lm.CASES:
        rec = lm.reference(c)["record"]
        assert not np.isnan(rec).any() and rec[11] + rec[12] <= c["par"]["gh"] * c["par"]["gw"]


# ---- the Python side ------------------------------------------------------------------------------------------------------
def test_check_localmap():
    assert live._check_localmap(None) is None and live._check_localmap(False) is None
    assert live._check_localmap(True) == live.LOCALMAP_DEFAULTS and live._check_localmap(True) is not live.LOCALMAP_DEFAULTS
    d = live.LOCALMAP_DEFAULTS
    assert {k: d[k] for k in ops.MAP_PARAMS if k not in ("select", "lost")} == {k: v for k, v in ops.MAP_PARAMS.items() if k not in ("select", "lost")}
    assert live.select_mask(d["select"]) == ops.MAP_PARAMS["select"] and live.LOCALMAP_LOST[d["lost"]] == ops.MAP_PARAMS["lost"]
    p = live._check_localmap(dict(grid=[4096, 1024], cell=1, range_min=1, range_max=20, select="overhead", lost="hold", l_min=-32768,
                                  l_max=32767, occ_level=1, free_level=0))
    assert p["grid"] == (4096, 1024) and p["cell"] == 1.0 and isinstance(p["cell"], float) and p["select"] == ("overhead",)
    assert p["lost"] == "hold" and p["min_pixels"] == 4
    assert live._check_localmap(dict(select=()))["select"] == ()
    for bad in (3, "yes", dict(rays=4), dict(grid=16), dict(grid=(16,)), dict(grid=(0, 4)), dict(grid=(4, 4097)), dict(grid=(4096, 2048)),
                dict(grid=(4.0, 4)), dict(grid=(True, 4)), dict(cell=0), dict(cell=-1), dict(cell=float("nan")), dict(cell=float("inf")),
                dict(cell="wide"), dict(range_max=0), dict(range_max=float("inf")), dict(range_min=-1), dict(range_min=12.8),
                dict(range_min=float("nan")), dict(min_pixels=0), dict(min_pixels=2.0), dict(l_occ=-1), dict(l_occ=32768),
                dict(l_free=-1), dict(l_min=1), dict(l_min=-32769), dict(l_max=-1), dict(l_max=32768), dict(decay=-1), dict(decay=1.5),
                dict(occ_level=-4), dict(free_level=8), dict(occ_level=40000), dict(select="floor"), dict(select=("obstacle", "floor")),
                dict(select="wall"), dict(select=3), dict(lost="forget"), dict(lost=0)):
        with pytest.raises(ValueError, match="localmap"):
            live._check_localmap(bad)
    for lmap in (True, dict(cell=0.2)):
        with pytest.raises(ValueError, match="localmap: needs ground"):
            live._check_localmap(lmap, None, dict(iters=4))
        with pytest.raises(ValueError, match="localmap: needs egomotion"):
            live._check_localmap(lmap, dict(step=2), None)


class _WithMotion:
    motion = object()


def test_session_constructor():
    est = _WithMotion()
    for lmap in (True, dict(cell=0.2)):
        with pytest.raises(ValueError, match="localmap: needs ground"):
            live.LiveSession(None, (8, 8), localmap=lmap)
        with pytest.raises(ValueError, match="localmap: needs ground"):
            live.LiveSession(est, (8, 8), egomotion=True, localmap=lmap)
        with pytest.raises(ValueError, match="localmap: needs egomotion"):
            live.LiveSession(None, (8, 8), ground=True, localmap=lmap)
        with pytest.raises(ValueError, match="localmap: needs egomotion"):
            live.LiveSession(None, (8, 8), ground=True, egomotion=False, scan=True, localmap=lmap)
    with pytest.raises(ValueError, match="localmap: unknown keys"):
        live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=dict(rays=4))
    s = live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=dict(select=("obstacle", "below"), grid=(8, 12), lost="hold"))
    assert not s._open_done and s.localmap["grid"] == (8, 12) and s._map_fresh
    assert s._map_par == dict(cell=0.1, range_min=0.0, range_max=12.8, min_pixels=4, l_occ=4, l_free=2, l_min=-32, l_max=64, decay=0,
                              occ_level=8, free_level=-4, select=(1 << 1) | (1 << 3), lost=ops.MAP_HOLD)
    assert set(s._map_par) == set(ops.MAP_PARAMS)
    assert live.LiveSession(est, (48, 64), ground=True, egomotion=True).localmap is None
    assert live.LocalMap._fields == ("logodds", "age", "pose", "origin", "cell", "integrated", "linked", "restarts", "frames", "occupied",
                                     "free", "unknown", "pixels", "step", "occ_level", "free_level")


def test_localmap_from_buffers():
    c, r = _ref("forward")
    m = live.localmap_from_buffers(r["record"], r["map_out"], r["age_out"], 0.5, 8, -4)
    assert isinstance(m, live.LocalMap) and m.logodds.tobytes() == r["map_out"].tobytes() and m.age.tobytes() == r["age_out"].tobytes()
    assert m.logodds.dtype == np.int16 and m.age.dtype == np.uint8 and not np.shares_memory(m.logodds, r["map_out"])
    assert m.pose == (r["state"][lm.PX], r["state"][lm.PZ], (0.0, 1.0)) and m.origin == (-12, -5) and m.cell == 0.5
    assert m.integrated is True and m.linked is True and m.restarts == 1 and m.frames == 4 and m.step == (0.0, 1.25)
    assert (m.pixels, m.occupied, m.free, m.unknown) == tuple(int(v) for v in r["record"][10:14])
    st = m.state()
    assert st.dtype == np.uint8 and st.shape == (16, 24)
    assert (st == live.MAP_OCCUPIED).sum() == m.occupied and (st == live.MAP_FREE).sum() == m.free
    assert ((st == live.MAP_UNKNOWN) == ((m.logodds > -4) & (m.logodds < 8))).all()
    assert m.world_xz(0, 0) == (-12 * 0.5 + 0.25, -5 * 0.5 + 0.25)
    x, z = m.world_xz(np.arange(16)[:, None], np.arange(24)[None, :])
    assert x.shape == (16, 24) and x[3, 5] == (-12 + 5.5) * 0.5 and z[3, 5] == (-5 + 3.5) * 0.5
    # the camera's own cell is the middle of the window
    assert m.origin[0] + 24 // 2 == np.floor(m.pose[0] / 0.5) and m.origin[1] + 16 // 2 == np.floor(m.pose[1] / 0.5)


class _Done:
    def synchronize(self):
        pass


def test_tuple_order():
    """result, ego, ground, localmap: the collection step on host buffers standing in for the downloads."""
    import torch
    c, r = _ref("forward")
    s = live.LiveSession(_WithMotion(), (6, 8), ground=True, egomotion=True, localmap=dict(grid=(16, 24), cell=0.5))
    s._e_down, s._h_out = [_Done(), _Done()], [torch.zeros(6, 8)] * 2
    s._h_ground = [[torch.zeros(32, dtype=torch.float64), torch.zeros(6, 8, dtype=torch.uint8)]] * 2
    s._has_ego = [False, False]
    bufs = [torch.from_numpy(r[k].copy()) for k in ("record", "map_out", "age_out")]
    s._h_map = [bufs] * 2
    s._inflight.append(0)
    got = s.pop()
    assert isinstance(got, tuple) and len(got) == 4 and got[1] is None and isinstance(got[2], live.Ground)
    m = got[3]
    bufs[1].zero_()  # the result is the caller's: the session's slot may be reused
    assert isinstance(m, live.LocalMap) and m.logodds.tobytes() == r["map_out"].tobytes() and m.cell == 0.5 and m.occ_level == 8


def test_entries_are_bound():
    from codd_amd import _abi
    _abi.load()
    assert not _abi.MISSING and _abi.load().codd_abi_version() == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_hip.h")).read()
    for name in ("codd_local_map_scratch", "codd_local_map"):
        assert name in _abi.SIGNATURES and f" {name}(" in header
    assert (ops.MAP_RESET, ops.MAP_HOLD) == (0, 1) and "#define CODD_MAP_RESET 0" in header and "#define CODD_MAP_HOLD 1" in header


def test_entry_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    import ctypes as C
    from codd_amd import _abi
    lib = _abi.load()
    scr = lib.codd_local_map_scratch
    assert scr(0, 4) == -1 and scr(4, 0) == -1 and scr(4097, 4) == -1 and scr(4, 4097) == -1 and scr(4096, 2048) == -1
    assert scr(1, 1) == 56 and scr(16, 24) == 48 + 8 * 16 * 24 and scr(4096, 1024) == scr(2048, 2048) == 48 + 8 * 2 ** 22
    need = scr(16, 24)
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = buf.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def call(disp=p, H=64, W=64, h=24, w=40, fx=40.0, fy=40.0, cx=20.0, cy=8.0, calib=20.0, labels=p, record=p, ego=None, fresh=0,
             gh=16, gw=24, cell=0.5, range_min=0.0, range_max=12.8, select=2, min_pixels=4, l_occ=4, l_free=2, l_min=-32, l_max=64,
             decay=0, occ_level=8, free_level=-4, lost=0, state=p, logodds=p, age=p, scratch=p, nbytes=need, map_out=p, age_out=p,
             rec=p):
        return lib.codd_local_map(disp, H, W, h, w, fx, fy, cx, cy, calib, labels, record, ego, fresh, gh, gw, cell, range_min,
                                  range_max, select, min_pixels, l_occ, l_free, l_min, l_max, decay, occ_level, free_level, lost,
                                  state, logodds, age, scratch, nbytes, map_out, age_out, rec, None)

    for name in ("disp", "labels", "record", "state", "logodds", "age", "scratch", "map_out", "age_out", "rec"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(h=0), dict(w=0), dict(H=0), dict(W=-3), dict(h=65), dict(w=65), dict(H=65536, W=32768, h=65536, w=32768),
                dict(gh=0), dict(gw=0), dict(gh=4097), dict(gw=4097), dict(gh=4096, gw=2048, nbytes=1 << 40), dict(cell=0.0),
                dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(select=1), dict(select=3), dict(min_pixels=0), dict(min_pixels=-5),
                dict(range_max=0.0), dict(range_max=nan), dict(range_max=inf), dict(range_min=-0.5), dict(range_min=nan),
                dict(range_min=12.8), dict(range_min=13.0), dict(l_occ=-1), dict(l_free=-1), dict(l_occ=32768), dict(l_min=1),
                dict(l_min=-32769), dict(l_max=-1), dict(l_max=32768), dict(decay=-1), dict(lost=2), dict(lost=-1), dict(fx=0.0),
                dict(fy=nan), dict(calib=inf), dict(cx=nan), dict(cy=inf), dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**bad) == -1, bad


def test_cli_localmap_arguments():
    from codd_amd import inference
    base = ["--img-dir", "x", "--r-img-dir", "y"]
    for argv in (["--localmap"], ["--live", "--localmap"], ["--live", "--ground", "--localmap"], ["--live", "--ego", "--localmap"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)
    assert inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap"]).localmap
    assert inference.parse_args(base + ["--live", "--ground", "--ego", "--scan", "--localmap"]).localmap
    assert not inference.parse_args(base + ["--live", "--ground", "--ego"]).localmap
