"""LiveSession cost map without a GPU: what every case of tests/live_costmap_ref.py is built to show, asserted on the
restatement; ops.cost_lut by hand; the Python side of ``costmap=`` (the checks, CostMap, the tuple order, the command
line); the bindings and every rejected argument of the entry (rejected before any launch, so no device is needed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_costmap_ref as cr  # noqa: E402
from codd_amd import live, ops  # noqa: E402


def _ref(name):
    return cr.CASES[cr.NAMES[name]], cr.expected(name)


def _at(r, key, j, i):
    return int(r[key][j, i])


# ---- the restatement on its cases -----------------------------------------------------------------------------------------
def test_distance_cases():
    c, r = _ref("no-occ")
    assert (r["dist2"] == cr.FAR).all() and (r["nearest"] == -1).all() and (r["cost"] == 0).all() and r["record"][0] == 0
    c, r = _ref("all-occ")
    assert (r["dist2"] == 0).all() and (r["nearest"] == np.arange(15).reshape(5, 3)).all() and (r["cost"] == cr.LETHAL).all()
    assert (r["reach"] == 0).all() and r["record"][:8].tolist() == [15, 15, 0, 0, 0, 0, 0, 7]
    c, r = _ref("corner-source")
    assert c["R"] == 5 and _at(r, "dist2", 0, 0) == 0 and _at(r, "dist2", 3, 4) == 25 and _at(r, "nearest", 3, 4) == 0
    assert _at(r, "dist2", 0, 5) == 25 and _at(r, "dist2", 5, 0) == 25 and _at(r, "dist2", 0, 6) == cr.FAR
    # exactly R R is inside, R R + 1 is far
    c, r = _ref("edge-of-R")
    assert _at(r, "dist2", 3, 4) == 25 and _at(r, "cost", 3, 4) >= 1 and _at(r, "nearest", 3, 4) == 0
    assert _at(r, "dist2", 1, 5) == cr.FAR and _at(r, "nearest", 1, 5) == -1 and _at(r, "cost", 1, 5) == 0  # 26
    # ties: the smallest raster index, in one column and across columns (and across both)
    c, r = _ref("tie-in-column")
    assert _at(r, "dist2", 5, 5) == 9 and _at(r, "nearest", 5, 5) == 2 * 24 + 5
    assert _at(r, "dist2", 5, 7) == 13 and _at(r, "nearest", 5, 7) == 2 * 24 + 5 and _at(r, "nearest", 6, 5) == 8 * 24 + 5
    c, r = _ref("tie-across-columns")
    assert _at(r, "dist2", 5, 5) == 9 and _at(r, "nearest", 5, 5) == 5 * 24 + 2 and _at(r, "nearest", 5, 6) == 5 * 24 + 8
    assert _at(r, "dist2", 5, 15) == 8 and _at(r, "nearest", 5, 15) == 3 * 24 + 17  # (3, 17) and (7, 13), both at 4 + 4
    c, r = _ref("R-exceeds-grid")
    assert c["R"] == 10 and (r["dist2"] != cr.FAR).all() and (r["nearest"] == 12).all() and _at(r, "dist2", 0, 2) == 20
    c, r = _ref("R1")
    assert c["R"] == 1 and len(c["lut"]) == 3 and sorted(np.unique(r["dist2"]).tolist()) == [0, 1, cr.FAR]
    assert (r["dist2"] == 1).sum() == 4 + 6 and _at(r, "nearest", 8, 12) == 8 * 24 + 13


def test_class_cases():
    c, r = _ref("never-seen-free-level")
    assert (c["map"] <= c["free_level"]).all() and (r["cls"][:8] == cr.UNKNOWN).all() and (r["cls"][8:] == cr.FREE).all()
    assert (r["cost"][:8] == cr.NO_INFO).all() and (r["reach"][:8] == 0).all() and (r["reach"][8] == 2).all() and (r["reach"][9:] == 1).all()
    c, r = _ref("unknown-inscribed")
    assert r["cls"][4, 5] == r["cls"][4, 7] == r["cls"][5, 5] == cr.UNKNOWN
    assert _at(r, "cost", 4, 5) == cr.INSCRIBED and _at(r, "cost", 4, 7) == cr.NO_INFO and _at(r, "cost", 5, 5) == cr.NO_INFO
    assert _at(r, "cost", 4, 4) == cr.LETHAL and _at(r, "cost", 4, 3) == cr.INSCRIBED and r["record"][2] == 2


def test_reachability_cases():
    c, r = _ref("start-occ")
    assert c["seed_r2"] == 9 and (r["reach"] == 0).all() and r["record"][3:8].tolist() == [0, 0, 0, 0, 8 * 24 + 12]
    c, r = _ref("start-unknown-seed")
    assert r["cls"][8, 12] == cr.UNKNOWN and r["record"][5] == 1 and _at(r, "reach", 8, 12) == 1
    # the seed disk (r2 = 4) is reachable, the unknown cells of the 5 x 5 patch outside it are not
    assert _at(r, "reach", 6, 12) == 2 and _at(r, "reach", 6, 10) == 0 and (r["reach"] != 0).sum() == 384 - 25 + 13
    c, r = _ref("seed0-unknown-start")
    assert (r["reach"] == 1).all() and _at(r, "cost", 8, 12) == cr.NO_INFO
    c, r = _ref("seed0-free-start")
    assert _at(r, "reach", 8, 12) == 1 and _at(r, "reach", 8, 13) == 0 and _at(r, "cost", 8, 13) == cr.INSCRIBED
    # a wall with a gap: two cells are both inscribed (closed), of three the middle one is not (open)
    c, r = _ref("gap-closed")
    assert (r["cost"][6, 10:12] == cr.INSCRIBED).all() and (r["reach"][7:] == 0).all() and (r["reach"][:5] == 1).all()
    c, r = _ref("gap-open")
    assert _at(r, "cost", 6, 11) < cr.INSCRIBED and _at(r, "reach", 6, 11) == 1 and (r["reach"][8:] == 1).all()
    assert _at(r, "reach", 6, 10) == 0 and _at(r, "reach", 6, 12) == 0
    c, r = _ref("through-unknown-off")
    assert (r["reach"][:4] == 1).all() and (r["reach"][4] == 2).all() and (r["reach"][5:] == 0).all() and r["record"][4] == 24
    assert r["record"][8:10].tolist() == [4 * 24 + 12, 4]
    c, r = _ref("through-unknown-on")
    assert (r["reach"] == 1).all() and r["record"][4] == 0 and r["record"][8:10].tolist() == [-1, -1]


def test_serpentine_cases():
    """Every free cell is reachable only through the whole corridor, which crosses at least three tiles each way with the
    last one partial, on either side of the single-workgroup threshold."""
    th, tw = cr.TILE
    assert cr.SMALL[0] * cr.SMALL[1] <= 16384 < cr.LARGE[0] * cr.LARGE[1]
    for gh, gw in (cr.SMALL, cr.LARGE):
        assert gh % th and gw % tw and gh % 4 and gw % 4 and (gh + th - 1) // th >= 3 and (gw + tw - 1) // tw >= 3
    for name in ("serpentine-small", "serpentine-small-vertical", "serpentine-large", "serpentine-large-vertical"):
        c, r = _ref(name)
        gh, gw = c["map"].shape
        assert ((r["reach"] == 1) == (r["cls"] == cr.FREE)).all() and _at(r, "reach", gh - 1, gw - 1) == 1
        cut = dict(c, map=c["map"].copy())
        wall = np.argwhere(r["cls"] == cr.OCC)
        a = cut["map"].T if "vertical" in name else cut["map"]
        a[wall[0][0] if "vertical" not in name else wall[0][1], :] = cr.OCC_V  # the first wall's gap closed
        assert cr.cost_map(cut)["record"][3] == 3 * (gw if "vertical" not in name else gh)


def test_frontier_cases():
    c, r = _ref("frontier-not-at-window-edge")
    assert (r["reach"][4:12, 0] == [2, 1, 1, 1, 1, 1, 1, 2]).all()  # the window's edge is no frontier, the corners' other side is
    assert (r["reach"][4, :12] == 2).all() and (r["reach"][4:12, 11] == 2).all() and r["record"][4] == 12 + 12 + 6
    c, r = _ref("frontier-tie")
    assert c["start"] == (11, 8) and r["record"][4] == 24
    for j, i in ((5, 11), (8, 8), (8, 14), (11, 11)):  # the middles of the four sides, each 3 cells from the start
        assert _at(r, "reach", j, i) == 2
    assert r["record"][8:10].tolist() == [5 * 23 + 11, 9]
    c, r = _ref("no-occ")  # nothing unknown: the window's edge alone makes no frontier
    assert r["record"][4] == 0 and r["record"][8] == -1


def test_grid_cases():
    assert cr.expected("1x1-free")["reach"].tolist() == [[1]] and cr.expected("1x1-occ")["cost"].tolist() == [[cr.LETHAL]]
    r = cr.expected("1x1-unknown")
    assert r["cost"].tolist() == [[cr.NO_INFO]] and r["reach"].tolist() == [[1]] and r["record"][:6].tolist() == [0, 0, 1, 1, 0, 1]
    shapes = {c["map"].shape for c in cr.CASES}
    assert {(1, 1), (5, 3), (16, 24), (80, 24), cr.SMALL, cr.LARGE} <= shapes
    assert max(s[0] * s[1] for s in shapes) == cr.LARGE[0] * cr.LARGE[1]
    for c in cr.CASES:
        r = cr.expected(c["name"])
        assert not np.isnan(r["record"]).any() and (r["record"][10:] == 0).all()
        assert r["record"][3] == (r["reach"] != 0).sum() and r["record"][4] == (r["reach"] == 2).sum()
        assert ((r["nearest"] >= 0) == (r["dist2"] != cr.FAR)).all() and len(c["lut"]) == c["R"] ** 2 + 2
        ok = r["nearest"] >= 0
        assert (r["cls"].ravel()[r["nearest"][ok]] == cr.OCC).all()


# ---- ops.cost_lut ------------------------------------------------------------------------------------------------------------
def test_cost_lut_by_hand():
    R, lut = ops.cost_lut(0.1, 0.3, 1.0, 3.0)
    assert R == 10 and lut.dtype == np.uint8 and lut.shape == (102,) and lut[0] == 254 and lut[101] == 0
    dist = np.sqrt(np.arange(101)) * 0.1
    # (sqrt(9) * 0.1 is 0.30000000000000004 in float64, above 0.3: the comparison is the formula's, made in float64)
    assert (lut[1:101][dist[1:] <= 0.3] == 253).all() and lut[8] == 253 and lut[9] == int(252 * np.exp(-3.0 * (dist[9] - 0.3))) == 251
    assert (np.diff(lut[:101].astype(int)) <= 0).all()
    R, exact = ops.cost_lut(0.25, 0.75, 1.0, 2.0)  # exactly the robot's radius (3 cells of 0.25) is inscribed
    assert R == 4 and exact[:11].tolist() == [254] + [253] * 9 + [int(252 * np.exp(-2.0 * (np.sqrt(10.0) * 0.25 - 0.75)))]
    assert exact[16] == int(252 * np.exp(-0.5)) and exact[17] == 0  # exactly the inflation radius is inside
    inside = (dist > 0.3) & (dist <= 1.0)
    assert (lut[:101][inside] >= 1).all() and (lut[:101][inside] <= 252).all() and lut[100] == max(1, int(252 * np.exp(-3.0 * 0.7)))
    assert lut[16] == int(252 * np.exp(-3.0 * (0.4 - 0.3)))
    R, lut = ops.cost_lut(0.3, 0.0, 1.0, 50.0)  # R = ceil(3.33) = 4: 0 beyond the inflation radius, at least 1 inside
    assert R == 4 and lut.shape == (18,) and lut[:2].tolist() == [254, 1] and lut[11] == 1 and (lut[12:] == 0).all()
    assert ops.cost_lut(1.0, 0.0, 0.5, 1.0)[0] == 1 and ops.cost_lut(1.0, 0.0, 0.5, 1.0)[1].tolist() == [254, 0, 0]
    assert ops.cost_lut(1.0, 2.0, 2.0, 0.0)[1].tolist() == [254, 253, 253, 253, 253, 0]
    assert ops.cost_lut(0.1, 0.3, 12.8, 0.0)[0] == 128
    with pytest.raises(ValueError, match="128"):
        ops.cost_lut(0.1, 0.3, 12.9, 1.0)
    assert (ops.COST_LETHAL, ops.COST_INSCRIBED, ops.COST_NO_INFO, ops.COST_FAR, ops.COST_MAX_R) == (254, 253, 255, 0x7fffffff, 128)


# ---- the Python side ------------------------------------------------------------------------------------------------------
def test_check_costmap():
    assert live._check_costmap(None) is None and live._check_costmap(False) is None
    assert live._check_costmap(True) == live.COSTMAP_DEFAULTS and live._check_costmap(True) is not live.COSTMAP_DEFAULTS
    assert live.COSTMAP_DEFAULTS == dict(robot_radius=0.3, inflation_radius=1.0, scaling=3.0, start_radius=1.5, through_unknown=False,
                                         nearest=False)
    p = live._check_costmap(dict(robot_radius=0, inflation_radius=2, scaling=0, start_radius=0, through_unknown=True, nearest=True))
    assert p == dict(robot_radius=0.0, inflation_radius=2.0, scaling=0.0, start_radius=0.0, through_unknown=True, nearest=True)
    assert isinstance(p["inflation_radius"], float)
    assert live._check_costmap(dict(inflation_radius=12.8), live._check_localmap(True))["inflation_radius"] == 12.8
    nan, inf = float("nan"), float("inf")
    for bad in (3, "yes", dict(radius=1), dict(robot_radius=-0.1), dict(robot_radius=1.5), dict(robot_radius=nan), dict(robot_radius="wide"),
                dict(robot_radius=True), dict(inflation_radius=0), dict(inflation_radius=-1), dict(inflation_radius=inf),
                dict(inflation_radius=nan), dict(inflation_radius=0.2), dict(scaling=-1), dict(scaling=nan), dict(scaling=inf),
                dict(start_radius=-1), dict(start_radius=nan), dict(start_radius=inf), dict(through_unknown=1), dict(through_unknown="no"),
                dict(nearest=0), dict(nearest=None), dict(inflation_radius=12.9)):
        with pytest.raises(ValueError, match="costmap"):
            live._check_costmap(bad, live._check_localmap(True))
    with pytest.raises(ValueError, match="costmap"):  # 1.0 / 0.005 = 200 cells
        live._check_costmap(True, live._check_localmap(dict(cell=0.005)))
    assert live._check_costmap(True, live._check_localmap(dict(cell=0.01))) == live.COSTMAP_DEFAULTS
    for cmap in (True, dict(scaling=1.0)):
        with pytest.raises(ValueError, match="costmap: needs localmap"):
            live._check_costmap(cmap, None)


class _WithMotion:
    motion = object()


def test_session_constructor():
    est = _WithMotion()
    for cmap in (True, dict(scaling=1.0)):
        with pytest.raises(ValueError, match="costmap: needs localmap"):
            live.LiveSession(None, (8, 8), costmap=cmap)
        with pytest.raises(ValueError, match="costmap: needs localmap"):
            live.LiveSession(est, (8, 8), ground=True, egomotion=True, costmap=cmap)
    with pytest.raises(ValueError, match="costmap: unknown keys"):
        live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True, costmap=dict(radius=1))
    s = live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=dict(grid=(8, 12), cell=0.25, occ_level=6, free_level=-2),
                         costmap=dict(inflation_radius=0.6, start_radius=0.6, through_unknown=True))
    assert not s._open_done and s._cost_R == 3 and s._cost_start == (6, 4)
    assert s._cost_lut_host.tobytes() == ops.cost_lut(0.25, 0.3, 0.6, 3.0)[1].tobytes()
    assert s._cost_par == dict(occ_level=6, free_level=-2, seed_r2=5, through_unknown=True)  # floor(2.4^2)
    s = live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True, costmap=True)
    assert s._cost_R == 10 and s._cost_start == (64, 64) and s._cost_par["seed_r2"] == int(np.floor((1.5 / 0.1) ** 2))
    assert live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True).costmap is None
    assert live.CostMap._fields == ("cost", "dist2", "nearest", "reach", "origin", "cell", "start", "occupied", "inscribed", "unknown",
                                    "reachable", "frontiers", "start_ok", "start_dist2", "frontier_cell", "frontier_dist2")


def test_costmap_from_buffers():
    c, r = _ref("5x3")
    m = live.costmap_from_buffers(r["record"], r["dist2"], r["cost"], r["reach"], r["nearest"], (-7, 4), 0.5, c["start"])
    assert isinstance(m, live.CostMap) and all(getattr(m, k).tobytes() == r[k].tobytes() for k in ("cost", "dist2", "nearest", "reach"))
    assert m.cost.dtype == m.reach.dtype == np.uint8 and m.dist2.dtype == m.nearest.dtype == np.int32
    assert not np.shares_memory(m.cost, r["cost"]) and m.cost.flags["OWNDATA"] and m.dist2.flags["WRITEABLE"]
    assert m.origin == (-7, 4) and m.cell == 0.5 and m.start == (1, 2)
    assert (m.occupied, m.inscribed, m.unknown, m.reachable, m.frontiers) == (1, 3, 2, 10, 3)
    assert m.start_ok is True and m.start_dist2 == 5 and m.frontier_cell == (3, 1) and m.frontier_dist2 == 1
    # clearance: sqrt(dist2) * cell in fp32, +inf where far
    cl = m.clearance()
    assert cl.dtype == np.float32 and cl.shape == (5, 3) and cl[0, 2] == 0 and cl[2, 1] == np.float32(np.sqrt(5.0) * 0.5)
    assert (np.isinf(cl) == (m.dist2 == ops.COST_FAR)).all() and np.isinf(cl).any() and not np.isnan(cl).any()
    # world_xz is LocalMap's; frontier_xz the centre of frontier_cell
    lmap = live.LocalMap(*([None] * 3), (-7, 4), 0.5, *([None] * 11))
    assert m.world_xz(3, 1) == lmap.world_xz(3, 1) == ((-7 + 1.5) * 0.5, (4 + 3.5) * 0.5) and m.frontier_xz() == m.world_xz(3, 1)
    x, z = m.world_xz(np.arange(5)[:, None], np.arange(3)[None, :])
    assert x.shape == (5, 3) and x[3, 1] == -2.75 and z[3, 1] == 3.75
    c, r = _ref("start-occ")
    m = live.costmap_from_buffers(r["record"], r["dist2"], r["cost"], r["reach"], None, (0, 0), 0.1, c["start"])
    assert m.nearest is None and m.frontier_cell is None and m.frontier_xz() is None and m.frontier_dist2 == -1
    assert m.start_ok is False and m.start_dist2 == 0 and m.reachable == 0
    assert live.costmap_from_buffers(cr.expected("no-occ")["record"], *(r[k] for k in ("dist2", "cost", "reach")), None, (0, 0), 0.1,
                                     (12, 8)).start_dist2 == -1


class _Done:
    def synchronize(self):
        pass


def test_tuple_order():
    """result, ego, ground, localmap, costmap: the collection step on host buffers standing in for the downloads."""
    import torch
    c, r = _ref("16x24-scatter")
    s = live.LiveSession(_WithMotion(), (6, 8), ground=True, egomotion=True, localmap=dict(grid=(16, 24), cell=0.5),
                         costmap=dict(nearest=True, inflation_radius=1.5))
    s._e_down, s._h_out = [_Done(), _Done()], [torch.zeros(6, 8)] * 2
    s._h_ground = [[torch.zeros(32, dtype=torch.float64), torch.zeros(6, 8, dtype=torch.uint8)]] * 2
    s._has_ego = [False, False]
    rec = torch.zeros(16, dtype=torch.float64)
    rec[8], rec[9] = -12, -5
    s._h_map = [[rec, torch.zeros(16, 24, dtype=torch.int16), torch.zeros(16, 24, dtype=torch.uint8)]] * 2
    bufs = [torch.from_numpy(r[k].copy()) for k in ("record", "dist2", "cost", "reach", "nearest")]
    s._h_cost = [bufs] * 2
    s._inflight.append(0)
    got = s.pop()
    assert isinstance(got, tuple) and len(got) == 5 and got[1] is None and isinstance(got[2], live.Ground)
    assert isinstance(got[3], live.LocalMap) and isinstance(got[4], live.CostMap)
    m = got[4]
    bufs[2].zero_()  # the result is the caller's: the session's slot may be reused
    assert m.cost.tobytes() == r["cost"].tobytes() and m.nearest.tobytes() == r["nearest"].tobytes() and m.origin == (-12, -5)
    assert m.cell == 0.5 and m.start == (12, 8) and m.reachable == int(r["record"][3])


def test_entries_are_bound():
    from codd_amd import _abi
    _abi.load()
    assert not _abi.MISSING and _abi.load().codd_abi_version() == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_hip.h")).read()
    for name in ("codd_cost_map_scratch", "codd_cost_map"):
        assert name in _abi.SIGNATURES and f" {name}(" in header
    for name, v in (("LETHAL", "254"), ("INSCRIBED", "253"), ("NO_INFO", "255"), ("FAR", "0x7fffffff"), ("MAX_R", "128")):
        assert f"#define CODD_COST_{name} {v}" in header and getattr(ops, "COST_" + name) == int(v, 0)


def test_entry_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    import ctypes as C
    from codd_amd import _abi
    lib = _abi.load()
    scr = lib.codd_cost_map_scratch
    for bad in ((0, 4, 3), (4, 0, 3), (4097, 4, 3), (4, 4097, 3), (4096, 2048, 3), (4, 4, 0), (4, 4, 129), (4, 4, -1)):
        assert scr(*bad) == -1, bad
    assert scr(1, 1, 1) == 16 + 16 + 16 + 16 + 64 and scr(16, 24, 128) == 80 + 7 * 384 and scr(2048, 2048, 1) == 80 + 7 * 2 ** 22
    need = scr(16, 24, 3)
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = buf.ctypes.data_as(C.c_void_p)

    def call(map=p, age=p, gh=16, gw=24, occ_level=8, free_level=-4, R=3, lut=p, start_i=12, start_j=8, seed_r2=4, through_unknown=0,
             scratch=p, nbytes=need, dist2=p, nearest=p, cost=p, reach=p, rec=p):
        return lib.codd_cost_map(map, age, gh, gw, occ_level, free_level, R, lut, start_i, start_j, seed_r2, through_unknown, scratch,
                                 nbytes, dist2, nearest, cost, reach, rec, None)

    for name in ("map", "age", "lut", "scratch", "dist2", "cost", "reach", "rec"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(gh=0), dict(gw=0), dict(gh=-1), dict(gh=4097), dict(gw=4097), dict(gh=4096, gw=2048, nbytes=1 << 40), dict(R=0),
                dict(R=129), dict(R=-3), dict(free_level=8), dict(free_level=9), dict(occ_level=-4), dict(start_i=-1), dict(start_i=24),
                dict(start_j=-1), dict(start_j=16), dict(seed_r2=-1), dict(nbytes=need - 1), dict(nbytes=0),
                dict(nearest=None, nbytes=need - 1)):
        assert call(**bad) == -1, bad


def test_cli_costmap_arguments():
    from codd_amd import inference
    base = ["--img-dir", "x", "--r-img-dir", "y"]
    for argv in (["--costmap"], ["--live", "--costmap"], ["--live", "--ground", "--ego", "--costmap"],
                 ["--live", "--ground", "--ego", "--scan", "--costmap"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)
    args = inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap", "--costmap"])
    assert args.costmap and args.localmap
    assert not inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap"]).costmap
