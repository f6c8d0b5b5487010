"""LiveSession plan without a GPU: the restatement of tests/live_plan_ref.py against the header's equations, cell by cell
with plain loops (a derivation independent of its Dijkstra); what every case is built to show; the path; the Python side
of ``plan=`` (the checks, Plan, lookahead, set_goal, the tuple order, the command line); the bindings and every rejected
argument of the entry (rejected before any launch, so no device is needed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_plan_ref as pr  # noqa: E402
from codd_amd import live, ops  # noqa: E402

IDS = [pr.case_id(c) for c in pr.CASES]


def _ref(name):
    return pr.CASES[pr.NAMES[name]], pr.expected(name)


def _cells(r, key="full_path"):
    gw = r["D"].shape[1]
    return [(int(k) // gw, int(k) % gw) for k in r[key]]


# ---- the restatement against the equations -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_potential_solves_the_equations(name):
    """P = 0 on G; elsewhere in D the minimum over the allowed moves of len w(q) + P(q); UNREACHED outside D and everywhere
    when G is empty.  dir is the smallest k that attains it.  Written out again here, with no helper of the restatement."""
    c, r = _ref(name)
    P, D, G, w, dirs = r["potential"].astype(np.int64), r["D"], r["G"], r["w"], r["dir"]
    gh, gw = D.shape
    assert (G <= D).all() and w.min() >= 1 and w.max() <= 1271
    for j in range(gh):
        for i in range(gw):
            if not D[j, i] or not G.any():
                assert P[j, i] == pr.UNREACHED and dirs[j, i] == 255
                continue
            if G[j, i]:
                assert P[j, i] == 0 and dirs[j, i] == 8
                continue
            best, best_k = None, None
            for k, (di, dj) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))):
                y, x = j + dj, i + di
                if not (0 <= y < gh and 0 <= x < gw and D[y, x]):
                    continue
                if k >= 4 and not (D[j, x] and D[y, i]):
                    continue
                v = (5 if k < 4 else 7) * int(w[y, x]) + int(P[y, x])
                if best is None or v < best:
                    best, best_k = v, k
            assert best is not None and P[j, i] == best and dirs[j, i] == best_k, (name, j, i)
    assert ((P != pr.UNREACHED) == (D & G.any())).all()  # D is 4-connected: finite exactly on D


@pytest.mark.parametrize("name", IDS)
def test_path_and_record(name):
    c, r = _ref(name)
    P, w, rec = r["potential"].astype(np.int64), r["w"], r["record"]
    gh, gw = r["D"].shape
    cells = _cells(r)
    assert not np.isnan(rec).any() and (rec[13:] == 0).all()
    assert rec[2] == len(cells) and rec[3] == min(len(cells), c["max_path"]) and rec[7] == r["G"].sum()
    assert (r["path"][:int(rec[3])] == r["full_path"][:int(rec[3])]).all() and (r["path"][int(rec[3]):] == -1).all()
    assert rec[9] == (P != pr.UNREACHED).sum() and rec[10] == (P[P != pr.UNREACHED].max() if rec[9] else -1)
    si, sj = c["start"]
    if not rec[0]:
        assert P[sj, si] == pr.UNREACHED and not cells and rec[1] == -1 and rec[8] == -1 and rec[11] == -1 and rec[12] == 0
        return
    assert cells[0] == (sj, si) and rec[1] == P[sj, si] and r["G"][cells[-1]] and rec[8] == cells[-1][0] * gw + cells[-1][1]
    assert not any(r["G"][at] for at in cells[:-1])  # it ends at the FIRST cell of G
    units = 0
    for (j, i), (y, x) in zip(cells[:-1], cells[1:]):  # P decreases by exactly len w of the cell entered
        step = abs(y - j) + abs(x - i)
        assert step in (1, 2) and max(abs(y - j), abs(x - i)) == 1
        length = 5 if step == 1 else 7
        assert P[j, i] - P[y, x] == length * w[y, x]
        units += length
    assert rec[12] == units
    on = [int(c["cost"][at]) for at in cells if c["cost"][at] != 255]
    assert rec[11] == (max(on) if on else -1)


# ---- what each case is built to show ------------------------------------------------------------------------------------
def test_small_cases():
    c, r = _ref("1x1")
    assert r["potential"].tolist() == [[0]] and r["dir"].tolist() == [[8]] and r["path"].tolist() == [0]
    assert r["record"][:13].tolist() == [1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 0]
    c, r = _ref("1x9-corridor")  # 8 straight steps: seven into cost 0 (w 50), one into cost 100 (w 50 + 80)
    assert r["potential"][0, 0] == 5 * (7 * 50 + 130) and r["path"].tolist() == list(range(9)) and r["record"][11] == 100
    c, r = _ref("9x1-corridor")  # the unknown cell counts as unknown_cost 128: w = 50 + 102
    assert r["potential"][8, 0] == 5 * (7 * 50 + 152) and r["path"].tolist() == list(range(8, -1, -1)) and r["record"][11] == 0
    c, r = _ref("start-in-goal")
    assert r["record"][:4].tolist() == [1, 0, 1, 1] and r["record"][12] == 0 and r["path"][0] == 3 * 6 + 2 and (r["path"][1:] == -1).all()
    # no corner is cut: the diagonal past the blocked cell is refused and the path goes round
    c, r = _ref("2x2-corner")
    assert r["path"].tolist() == [0, 2, 3, -1] and r["potential"][0, 0] == 500 and r["dir"].tolist() == [[2, 255], [0, 8]]
    c, r = _ref("3x3-corner")
    assert r["potential"][0, 0] == 4 * 5 * 50 and len(_cells(r)) == 5 and (1, 1) not in _cells(r) and r["record"][12] == 20
    assert r["dir"][0, 1] == 0 and r["dir"][1, 0] == 2  # beside the blocked centre only straight moves are left


def test_open_field_ties():
    """Uniform costs: P is the octile distance times 50, and almost every cell has several best moves."""
    c, r = _ref("open-17x19")
    gj, gi = 9, 15
    jj, ii = np.mgrid[:17, :19]
    dx, dy = np.abs(ii - gi), np.abs(jj - gj)
    assert (r["potential"] == 50 * (7 * np.minimum(dx, dy) + 5 * np.abs(dx - dy))).all()
    assert r["dir"][gj, 0] == 0 and r["dir"][0, gi] == 2 and r["dir"][16, gi] == 3 and r["dir"][gj, 18] == 1
    assert r["dir"][gj - 1, 0] == 0 and r["dir"][gj + 1, 0] == 0  # k = 0 ties with the diagonals 4 and 6: the smallest
    assert r["dir"][0, 0] == 0 and r["dir"][0, gi - 9] == 4 and r["dir"][16, gi - 7] == 6
    assert _cells(r)[1] == (2, 2) and r["record"][2] == 15  # from (2, 1): k = 0 first (7 straight and 7 diagonal steps in all)


def test_cost_decides_the_route():
    for name, through in (("corridor-factor0", True), ("detour-factor1024", False)):
        c, r = _ref(name)
        assert ((3, 4) in _cells(r)) == through, name
    assert pr.expected("corridor-factor0")["record"][11] == 200 and pr.expected("detour-factor1024")["record"][11] == 0
    assert pr.expected("corridor-factor0")["record"][2] == 5 and pr.expected("detour-factor1024")["record"][2] == 11
    free, dear = pr.expected("unknown-cost0"), pr.expected("unknown-cost254")
    assert free["record"][1] == 8 * 5 * 50 and all(i == 2 for _, i in _cells(free))  # straight through the unknown band
    assert dear["record"][1] > free["record"][1] and dear["w"][4, 2] == 50 + (205 * 254) // 256
    c, r = _ref("seed-disk-253-255")
    assert r["D"][5, 5] and c["cost"][5, 5] == 253 and c["cost"][3, 3] == 255 and r["record"][11] == 253
    assert r["w"][5, 5] == 50 + (205 * 253) // 256 and r["w"][3, 3] == 50 + (205 * 128) // 256


def test_goal_cases():
    c, r = _ref("snap-other-component")  # the goal (1, 9) lies behind the wall at column 6: the nearest cell of D is (1, 5)
    assert not r["D"][1, 9] and r["record"][4:9].tolist() == [1 * 12 + 9, 0, 1, 1, 1 * 12 + 5]
    c, r = _ref("snap-tie")  # (1, 3), (3, 1), (3, 5), (5, 3) are all 4 away from (3, 3): the smallest raster index
    assert r["D"].sum() == 16 and r["record"][6] == 1 and r["record"][8] == 1 * 7 + 3 and r["G"].sum() == 1
    c, r = _ref("goal-r2-5")
    assert r["record"][7] == r["G"].sum() == 19 and r["record"][6] == 0 and r["G"][2, 6] and not r["G"][2, 8] and r["record"][8] == 3 * 12 + 6
    c, r = _ref("world-inside")  # floor(-1.13 / 0.25) = -5, less ix0 = -9: column 4; floor(-0.62 / 0.25) = -3, less -5: row 2
    assert r["record"][4:7].tolist() == [2 * 12 + 4, 0, 0] and c["map_record"][8] < 0 and c["map_record"][9] < 0
    c, r = _ref("world-outside")  # x far to the right: clamped to column 11, which lies behind the wall: snapped to column 5
    assert r["record"][4:9].tolist() == [0 * 12 + 11, 1, 1, 1, 0 * 12 + 5]
    c, r = _ref("frontier-valid")
    assert r["record"][4] == 89 and r["record"][0] == 1 and r["record"][6] == 0
    for name in ("frontier-none", "start-not-traversable"):
        c, r = _ref(name)
        assert (r["potential"] == pr.UNREACHED).all() and (r["dir"] == 255).all() and (r["path"] == -1).all()
        assert r["record"][:4].tolist() == [0, -1, 0, 0] and r["record"][7:13].tolist() == [0, -1, 0, -1, -1, 0]
    assert pr.expected("frontier-none")["record"][4] == -1 and pr.expected("frontier-none")["D"].any()
    assert pr.expected("start-not-traversable")["record"][4] == 2 * 12 + 2 and not pr.expected("start-not-traversable")["D"].any()


def test_truncation_and_large_cases():
    full = pr.expected("open-17x19")
    for name, n in (("max-path-1", 1), ("max-path-short", 14)):
        c, r = _ref(name)
        assert r["record"][2:4].tolist() == [15, n] and r["path"].shape == (n,) and (r["path"] == full["path"][:n]).all()
        assert r["record"][8] == full["record"][8] and r["record"][12] == full["record"][12]  # of the full path
    c, r = _ref("serpentine-33x31")  # one corridor through every row: 17 rows of 31 cells less the 14 skipped next to the gaps
    assert r["record"][2] == 513 and r["record"][9] == r["D"].sum() == 17 * 31 + 16
    c, r = _ref("1x25600")
    assert r["record"][2:4].tolist() == [12800, 1024] and r["path"].tolist() == list(range(12800, 12800 + 1024))
    shapes = {c["cost"].shape for c in pr.CASES}
    assert {(1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (17, 19), (33, 31), (127, 129), (160, 160), (1, 25600)} <= shapes
    assert max(s[0] * s[1] for s in shapes) == pr.MAX_CELLS == ops.PLAN_MAX_CELLS
    for name in ("rooms-127x129", "rooms-160x160", "chained-16x24", "chained-127x129", "chained-frontier-tie"):
        assert pr.expected(name)["record"][0] == 1, name
    c, r = _ref("chained-16x24")  # the goal is the costmap restatement's own nearest frontier
    assert c["cost_record"][8] >= 0 and r["record"][4] == c["cost_record"][8] and (c["reach"] == 2).any()


# ---- the Python side ------------------------------------------------------------------------------------------------------
def test_check_plan():
    lm, cm = live._check_localmap(True), live._check_costmap(True)
    assert live._check_plan(None) is None and live._check_plan(False) is None
    assert live._check_plan(True, cm, lm) == live.PLAN_DEFAULTS and live._check_plan(True, cm, lm) is not live.PLAN_DEFAULTS
    assert live.PLAN_DEFAULTS == dict(goal="frontier", goal_radius=0.0, neutral=50, factor=205, unknown_cost=128, max_path=1024, dir=False)
    p = live._check_plan(dict(goal=(1, -2.5), goal_radius=1, neutral=1, factor=1024, unknown_cost=0, max_path=7, dir=True), cm, lm)
    assert p == dict(goal=(1.0, -2.5), goal_radius=1.0, neutral=1, factor=1024, unknown_cost=0, max_path=7, dir=True)
    nan, inf = float("nan"), float("inf")
    for bad in (3, "yes", dict(radius=1), dict(goal="home"), dict(goal=(1, 2, 3)), dict(goal=(nan, 0)), dict(goal=(0, inf)), dict(goal=None),
                dict(goal=(True, 1)), dict(goal_radius=-1), dict(goal_radius=nan), dict(goal_radius="wide"), dict(goal_radius=True),
                dict(neutral=0), dict(neutral=256), dict(neutral=1.5), dict(neutral=True), dict(factor=-1), dict(factor=1025),
                dict(unknown_cost=-1), dict(unknown_cost=255), dict(max_path=0), dict(max_path=2 ** 31), dict(dir=1), dict(dir=None)):
        with pytest.raises(ValueError, match="plan"):
            live._check_plan(bad, cm, lm)
    for plan in (True, dict(neutral=60)):
        with pytest.raises(ValueError, match="plan: needs costmap"):
            live._check_plan(plan, None, lm)
    assert live._check_plan(True, cm, live._check_localmap(dict(grid=(160, 160)))) == live.PLAN_DEFAULTS
    with pytest.raises(ValueError, match="25600"):
        live._check_plan(True, cm, live._check_localmap(dict(grid=(160, 161))))


class _WithMotion:
    motion = object()


def test_session_constructor_and_set_goal():
    est = _WithMotion()
    for plan in (True, dict(neutral=60)):
        with pytest.raises(ValueError, match="plan: needs costmap"):
            live.LiveSession(None, (8, 8), plan=plan)
        with pytest.raises(ValueError, match="plan: needs costmap"):
            live.LiveSession(est, (8, 8), ground=True, egomotion=True, localmap=True, plan=plan)
    with pytest.raises(ValueError, match="plan: unknown keys"):
        live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True, costmap=True, plan=dict(radius=1))
    with pytest.raises(ValueError, match="25600"):
        live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=dict(grid=(256, 128)), costmap=True, plan=True)
    s = live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=dict(grid=(8, 12), cell=0.25), costmap=True,
                         plan=dict(goal=(1.5, -2), goal_radius=0.6, neutral=60, dir=True))
    assert not s._open_done and s._plan_goal == (1.5, -2.0)
    assert s._plan_par == dict(goal_r2=5, neutral=60, factor=205, unknown_cost=128)  # floor(2.4^2)
    s.set_goal("frontier")
    assert s._plan_goal == "frontier" and not s._open_done  # no device call
    s.set_goal((0, 3))
    assert s._plan_goal == (0.0, 3.0)
    for bad in ("home", (1,), (float("nan"), 0), None):
        with pytest.raises(ValueError, match="plan"):
            s.set_goal(bad)
    assert s._plan_goal == (0.0, 3.0)
    assert live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True, costmap=True).plan is None
    with pytest.raises(ValueError, match="set_goal"):
        live.LiveSession(est, (48, 64), ground=True, egomotion=True, localmap=True, costmap=True).set_goal("frontier")
    assert live.Plan._fields == ("potential", "dir", "path", "found", "cost", "length_cells", "truncated", "goal_cell", "clamped",
                                 "snapped", "end_cell", "reached", "max_cost_on_path", "length", "origin", "cell", "start")


def test_plan_from_buffers_and_lookahead():
    c, r = _ref("3x3-corner")
    p = live.plan_from_buffers(r["record"], r["potential"].view(np.int32), r["dir"], r["path"], (-7, 4), 0.5, c["start"])
    assert isinstance(p, live.Plan) and p.potential.dtype == np.uint32 and p.potential.tobytes() == r["potential"].tobytes()
    assert p.dir.tobytes() == r["dir"].tobytes() and p.potential.flags["OWNDATA"] and not np.shares_memory(p.dir, r["dir"])
    assert p.path.dtype == np.int32 and p.path.tolist() == [[0, 0], [0, 1], [0, 2], [1, 2], [2, 2]]
    assert (p.found, p.cost, p.length_cells, p.truncated, p.goal_cell, p.clamped, p.snapped, p.end_cell, p.reached,
            p.max_cost_on_path) == (True, 1000, 5, False, (2, 2), False, False, (2, 2), 8, 0)
    assert p.length == 20 * 0.5 / 5 and p.origin == (-7, 4) and p.cell == 0.5 and p.start == (0, 0)
    lmap = live.LocalMap(*([None] * 3), (-7, 4), 0.5, *([None] * 11))
    assert p.world_xz(2, 1) == lmap.world_xz(2, 1) == ((-7 + 1.5) * 0.5, (4 + 2.5) * 0.5)
    xz = p.path_xz()
    assert xz.shape == (5, 2) and xz.dtype == np.float64 and tuple(xz[3]) == p.world_xz(1, 2)
    # four straight steps of 0.5: 0, 0.5, 1.0, 1.5, 2.0 along the path
    assert p.lookahead(0) == p.world_xz(0, 0) and p.lookahead(0.5) == p.world_xz(0, 1) and p.lookahead(0.6) == p.world_xz(0, 2)
    assert p.lookahead(2.0) == p.world_xz(2, 2) and p.lookahead(9.0) == p.world_xz(2, 2)
    c, r = _ref("open-17x19")  # seven straight steps from (2, 1), then seven diagonal ones of 7 / 5 cells each
    p = live.plan_from_buffers(r["record"], r["potential"], None, r["path"], (0, 0), 1.0, c["start"])
    assert p.dir is None and p.length == 84 / 5 and p.lookahead(7.0) == p.world_xz(2, 8) and p.lookahead(7.1) == p.world_xz(3, 9)
    assert p.lookahead(8.3) == p.world_xz(3, 9) and p.lookahead(8.5) == p.world_xz(4, 10)
    c, r = _ref("max-path-short")
    p = live.plan_from_buffers(r["record"], r["potential"], None, r["path"], (0, 0), 1.0, c["start"])
    assert p.truncated and p.length_cells == 15 and len(p.path) == 14 and p.end_cell == (9, 15) and p.lookahead(99) == p.world_xz(*p.path[-1])
    c, r = _ref("frontier-none")
    p = live.plan_from_buffers(r["record"], r["potential"], r["dir"], r["path"], (0, 0), 0.1, c["start"])
    assert not p.found and p.cost == -1 and p.goal_cell is None and p.end_cell is None and p.path.shape == (0, 2)
    assert p.lookahead(1.0) is None and p.path_xz().shape == (0, 2) and p.length == 0 and p.max_cost_on_path == -1 and p.reached == 0
    c, r = _ref("world-outside")
    p = live.plan_from_buffers(r["record"], r["potential"], None, r["path"], (-6, -4), 0.1, c["start"])
    assert p.clamped and p.snapped and p.goal_cell == (0, 11) and p.end_cell == (0, 5)


class _Done:
    def synchronize(self):
        pass


def test_tuple_order():
    """result, ego, ground, localmap, costmap, plan: the collection step on host buffers standing in for the downloads."""
    import live_costmap_ref as cr
    import torch
    c, r = _ref("chained-16x24")
    cm = cr.expected("16x24-scatter-b")
    s = live.LiveSession(_WithMotion(), (6, 8), ground=True, egomotion=True, localmap=dict(grid=(16, 24), cell=0.5),
                         costmap=dict(inflation_radius=1.5), plan=dict(dir=True, max_path=c["max_path"]))
    s._e_down, s._h_out = [_Done(), _Done()], [torch.zeros(6, 8)] * 2
    s._h_ground = [[torch.zeros(32, dtype=torch.float64), torch.zeros(6, 8, dtype=torch.uint8)]] * 2
    s._has_ego = [False, False]
    rec = torch.zeros(16, dtype=torch.float64)
    rec[8], rec[9] = -12, -5
    s._h_map = [[rec, torch.zeros(16, 24, dtype=torch.int16), torch.zeros(16, 24, dtype=torch.uint8)]] * 2
    s._h_cost = [[torch.from_numpy(cm[k].copy()) for k in ("record", "dist2", "cost", "reach")]] * 2
    bufs = [torch.from_numpy(r["record"].copy()), torch.from_numpy(r["potential"].view(np.int32).copy()),
            torch.from_numpy(r["path"].copy()), torch.from_numpy(r["dir"].copy())]
    s._h_plan = [bufs] * 2
    s._inflight.append(0)
    got = s.pop()
    assert isinstance(got, tuple) and len(got) == 6 and isinstance(got[4], live.CostMap) and isinstance(got[5], live.Plan)
    p = got[5]
    bufs[1].zero_()  # the result is the caller's: the session's slot may be reused
    assert p.potential.tobytes() == r["potential"].tobytes() and p.dir.tobytes() == r["dir"].tobytes() and p.origin == (-12, -5)
    assert p.cell == 0.5 and p.start == (12, 8) and p.found and p.cost == int(r["record"][1]) and len(p.path) == int(r["record"][3])


def test_entries_are_bound():
    from codd_amd import _abi
    _abi.load()
    assert not _abi.MISSING and _abi.load().codd_abi_version() == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_hip.h")).read()
    for name in ("codd_plan_scratch", "codd_plan"):
        assert name in _abi.SIGNATURES and f" {name}(" in header
    for name, v in (("MAX_CELLS", "25600"), ("UNREACHED", "0xffffffffu"), ("GOAL_CELL", "0"), ("GOAL_WORLD", "1"), ("GOAL_FRONTIER", "2")):
        assert f"#define CODD_PLAN_{name} {v}" in header and getattr(ops, "PLAN_" + name) == int(v.rstrip("u"), 0)
    assert (pr.CELL, pr.WORLD, pr.FRONTIER, pr.UNREACHED) == (ops.PLAN_GOAL_CELL, ops.PLAN_GOAL_WORLD, ops.PLAN_GOAL_FRONTIER, ops.PLAN_UNREACHED)
    assert live.PLAN_MOVES == pr.MOVES


def test_entry_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    import ctypes as C
    from codd_amd import _abi
    lib = _abi.load()
    scr = lib.codd_plan_scratch
    for bad in ((0, 4), (4, 0), (-1, 4), (4, -1), (4097, 7), (160, 161), (25601, 1), (1, 25601), (1 << 16, 1 << 16)):
        assert scr(*bad) == -1, bad
    assert scr(1, 1) == scr(160, 160) == scr(1, 25600) == scr(25600, 1) == 80
    buf = np.zeros(128, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = buf.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def call(cost=p, reach=p, crec=p, mrec=p, gh=16, gw=24, start_i=12, start_j=8, mode=0, goal_i=3, goal_j=4, goal_x=1.0, goal_z=2.0,
             cell=0.1, goal_r2=0, neutral=50, factor=205, unknown_cost=128, max_path=64, scratch=p, nbytes=80, pot=p, dirs=p, path=p, rec=p):
        return lib.codd_plan(cost, reach, crec, mrec, gh, gw, start_i, start_j, mode, goal_i, goal_j, goal_x, goal_z, cell, goal_r2,
                             neutral, factor, unknown_cost, max_path, scratch, nbytes, pot, dirs, path, rec, None)

    for name in ("cost", "reach", "pot", "path", "rec", "scratch"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(gh=0), dict(gw=0), dict(gh=-1), dict(gh=4097, gw=7), dict(gh=160, gw=161), dict(start_i=-1), dict(start_i=24),
                dict(start_j=-1), dict(start_j=16), dict(mode=3), dict(mode=-1), dict(goal_i=-1), dict(goal_i=24), dict(goal_j=-1),
                dict(goal_j=16), dict(goal_r2=-1), dict(max_path=0), dict(max_path=-5), dict(neutral=0), dict(neutral=256),
                dict(factor=-1), dict(factor=1025), dict(unknown_cost=-1), dict(unknown_cost=255), dict(nbytes=79), dict(nbytes=0),
                dict(mode=1, mrec=None), dict(mode=2, crec=None), dict(mode=1, cell=0.0), dict(mode=1, cell=-0.1), dict(mode=1, cell=nan),
                dict(mode=1, cell=inf), dict(mode=1, goal_x=nan), dict(mode=1, goal_z=inf), dict(mode=1, goal_x=-inf),
                dict(mode=1, goal_x=0.1 * 2 ** 30 * 1.01), dict(mode=1, goal_z=-0.1 * 2 ** 30 * 1.01), dict(dirs=None, nbytes=79)):
        assert call(**bad) == -1, bad


def test_ops_plan_rejects_bad_arguments():
    """ValueError before any device call: host tensors never get as far as the check that they are on a device."""
    import torch
    gh, gw = 16, 24
    cost, reach = torch.zeros(gh, gw, dtype=torch.uint8), torch.zeros(gh, gw, dtype=torch.uint8)
    pot, path, rec = torch.zeros(gh, gw, dtype=torch.int32), torch.zeros(64, dtype=torch.int32), torch.zeros(16, dtype=torch.float64)

    def call(cost=cost, start=(12, 8), path=path, **kw):
        kw.setdefault("goal", ("cell", 3, 4))
        return ops.plan(cost, reach, start, pot, path, rec, **kw)

    nan, inf = float("nan"), float("inf")
    for bad in (dict(start=(-1, 8)), dict(start=(24, 8)), dict(start=(12, 16)), dict(goal="home"), dict(goal=("cell", 24, 0)),
                dict(goal=("cell", 0, -1)), dict(goal=("cell", 1.5, 2)), dict(goal=("cell", 1)), dict(goal=("polar", 1, 2)), dict(goal=None),
                dict(goal="frontier"), dict(goal=("world", 1.0, 2.0)), dict(goal=("world", 1.0, 2.0), map_record=rec),
                dict(goal=("world", 1.0, 2.0), map_record=rec, cell=0.0), dict(goal=("world", 1.0, 2.0), map_record=rec, cell=nan),
                dict(goal=("world", nan, 2.0), map_record=rec, cell=0.1), dict(goal=("world", 1.0, inf), map_record=rec, cell=0.1),
                dict(goal=("world", 2.0 ** 30, 0.0), map_record=rec, cell=1.0), dict(goal_r2=-1), dict(neutral=0), dict(neutral=256),
                dict(factor=-1), dict(factor=1025), dict(unknown_cost=-1), dict(unknown_cost=255), dict(path=path[:0]),
                dict(cost=torch.zeros(160, 161, dtype=torch.uint8)), dict(cost=torch.zeros(gh * gw, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="plan"):
            call(**bad)
    for bad in ((0, 4), (4, 0), (4097, 7), (160, 161)):
        with pytest.raises(ValueError, match="plan_scratch"):
            ops.plan_scratch(*bad)
    assert ops.plan_scratch(160, 160) == 80
    assert ops.plan_goal("frontier")[0] == ops.PLAN_GOAL_FRONTIER and ops.plan_goal(("cell", 3, 4)) == (0, 3, 4, 0.0, 0.0)
    assert ops.plan_goal(("world", 1, -2.5)) == (1, 0, 0, 1.0, -2.5)


def test_cli_plan_arguments():
    from codd_amd import inference
    base = ["--img-dir", "x", "--r-img-dir", "y"]
    for argv in (["--plan"], ["--live", "--plan"], ["--live", "--ground", "--ego", "--localmap", "--plan"],
                 ["--live", "--ground", "--ego", "--localmap", "--costmap", "--plan", "--plan-goal", "home"],
                 ["--live", "--ground", "--ego", "--localmap", "--costmap", "--plan", "--plan-goal", "1,2,3"],
                 ["--live", "--ground", "--ego", "--localmap", "--costmap", "--plan", "--plan-goal", "1,nan"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)
    args = inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap", "--costmap", "--plan"])
    assert args.plan and args.plan_goal == "frontier"
    args = inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap", "--costmap", "--plan", "--plan-goal=-1.5,2"])
    assert args.plan_goal == (-1.5, 2.0)
    assert not inference.parse_args(base + ["--live", "--ground", "--ego", "--localmap", "--costmap"]).plan
