"""Restatement of codd_plan (include/codd_hip.h) shared by the CPU and the GPU tests, in plain Python and numpy, straight from
the definitions of the header, and the cases.

``goal_cell`` and ``goal_set`` are the goal rules, ``potential`` a heap Dijkstra from the goal set over the allowed moves
(the kernel relaxes blocks of cells in registers until nothing changes: nothing of that is here), ``direction`` the tie rule
of ``dir``, ``walk`` the path, ``plan`` chains them and writes the record.  tests/test_live_plan.py checks the potential of
every case against the header's equations cell by cell, which is a derivation independent of Dijkstra.

A case is a dict: ``cost`` and ``reach`` uint8 [gh,gw], ``start`` = (i, j), ``mode``, ``goal_i``, ``goal_j``, ``goal_x``,
``goal_z``, ``cell``, ``goal_r2``, ``neutral``, ``factor``, ``unknown_cost``, ``max_path``, ``cost_record`` and ``map_record``
(float64 [16] or None), ``with_dir``.  ``reach`` is built the way codd_cost_map defines it: the 4-connected component of the
start cell among the traversable cells (1, or 2 on some cells, as for frontiers).  The kernel takes 4 x 4 blocks of cells,
1024 at a time: 17 x 19, 33 x 31 and 127 x 129 divide by nothing, 127 x 129 and 160 x 160 have more blocks than threads.
"""
import functools
import heapq
import math
import os
import sys
from collections import deque

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_costmap_ref as cr  # noqa: E402  (the chained cases: a cost map made by the costmap restatement)

UNREACHED, NO_INFO, MAX_CELLS = 0xffffffff, 255, 25600
CELL, WORLD, FRONTIER = 0, 1, 2
MOVES = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))  # (di, dj) of k
LEN = (5, 5, 5, 5, 7, 7, 7, 7)


def weights(c):
    cc = np.where(c["cost"] == NO_INFO, c["unknown_cost"], c["cost"]).astype(np.int64)
    return c["neutral"] + (c["factor"] * cc) // 256


def allowed(D, j, i, k):
    """The target (y, x) of move k from the cell (j, i) of D if the move is allowed, else None."""
    gh, gw = D.shape
    di, dj = MOVES[k]
    y, x = j + dj, i + di
    if not (0 <= y < gh and 0 <= x < gw) or not D[y, x]:
        return None
    if k >= 4 and not (D[j, x] and D[y, i]):
        return None  # the corner would be cut
    return y, x


def goal_cell(c):
    """(gj, gi, clamped), or None without a goal cell."""
    gh, gw = c["cost"].shape
    if c["mode"] == CELL:
        return c["goal_j"], c["goal_i"], 0
    if c["mode"] == WORLD:
        cell = float(np.float32(c["cell"]))
        gi = int(math.floor(c["goal_x"] / cell)) - int(c["map_record"][8])
        gj = int(math.floor(c["goal_z"] / cell)) - int(c["map_record"][9])
        ci, cj = min(max(gi, 0), gw - 1), min(max(gj, 0), gh - 1)
        return cj, ci, int((ci, cj) != (gi, gj))
    r = int(c["cost_record"][8])
    return None if r < 0 else (r // gw, r % gw, 0)


def goal_set(D, goal, goal_r2):
    """(G bool [gh,gw], snapped)."""
    gh, gw = D.shape
    if goal is None or not D.any():
        return np.zeros((gh, gw), bool), 0
    jj, ii = np.mgrid[:gh, :gw]
    d2 = (ii - goal[1]) ** 2 + (jj - goal[0]) ** 2
    G = D & (d2 <= goal_r2)
    if G.any():
        return G, 0
    k = int(np.lexsort(((jj * gw + ii)[D], d2[D]))[0])  # the squared distance, then the raster index
    G = np.zeros((gh, gw), bool)
    G[jj[D][k], ii[D][k]] = True
    return G, 1


def potential(D, w, G):
    """int64 [gh,gw], -1 for no path: Dijkstra from G; entering q from p costs LEN w(q) (the moves are allowed both ways)."""
    gh, gw = D.shape
    P = np.full((gh, gw), -1, np.int64)
    heap = [(0, int(j), int(i)) for j, i in np.argwhere(G)]
    done = np.zeros((gh, gw), bool)
    while heap:
        p, j, i = heapq.heappop(heap)
        if done[j, i]:
            continue
        done[j, i], P[j, i] = True, p
        for k in range(8):  # the cells from which (j, i) is entered: the same eight, the rule is symmetric
            at = allowed(D, j, i, k)
            if at is not None and not done[at]:
                heapq.heappush(heap, (p + LEN[k] * int(w[j, i]), at[0], at[1]))
    return P


def direction(D, w, P, G):
    gh, gw = D.shape
    out = np.full((gh, gw), 255, np.uint8)
    for j, i in np.argwhere(P >= 0):
        if G[j, i]:
            out[j, i] = 8
            continue
        for k in range(8):
            at = allowed(D, j, i, k)
            if at is not None and P[at] >= 0 and LEN[k] * int(w[at]) + P[at] == P[j, i]:
                out[j, i] = k
                break
    return out


def walk(dirs, start):
    """The full path as raster indices and its length in units of 5 and 7."""
    gh, gw = dirs.shape
    j, i = start[1], start[0]
    if dirs[j, i] == 255:
        return [], 0
    cells, units = [j * gw + i], 0
    while dirs[j, i] != 8:
        k = int(dirs[j, i])
        j, i, units = j + MOVES[k][1], i + MOVES[k][0], units + LEN[k]
        cells.append(j * gw + i)
        assert len(cells) <= gh * gw
    return cells, units


def plan(c):
    """The outputs of the entry on the case ``c``: potential, dir, path, record (and D, G, w, full_path for the tests)."""
    gh, gw = c["cost"].shape
    si, sj = c["start"]
    D = c["reach"] != 0
    w = weights(c)
    goal = goal_cell(c)
    G, snapped = goal_set(D, goal, c["goal_r2"])
    P = potential(D, w, G)
    dirs = direction(D, w, P, G)
    cells, units = walk(dirs, c["start"])
    path = np.full(c["max_path"], -1, np.int32)
    n = min(len(cells), c["max_path"])
    path[:n] = cells[:n]
    rec = np.zeros(16, np.float64)
    found = P[sj, si] >= 0
    rec[0], rec[1], rec[2], rec[3] = float(found), float(P[sj, si]), len(cells), n
    rec[4] = -1.0 if goal is None else float(goal[0] * gw + goal[1])
    rec[5], rec[6], rec[7] = (0 if goal is None else goal[2]), snapped, G.sum()
    rec[8] = cells[-1] if found else -1.0
    rec[9], rec[10] = (P >= 0).sum(), P.max()  # (-1 when nothing is finite)
    on = [int(c["cost"].ravel()[k]) for k in cells if c["cost"].ravel()[k] != NO_INFO]
    rec[11], rec[12] = (max(on) if on else -1.0), units
    return dict(potential=np.where(P < 0, UNREACHED, P).astype(np.uint32), dir=dirs, path=path, record=rec, D=D, G=G,
                w=w, full_path=np.array(cells, np.int64))


# ---- the cases ----------------------------------------------------------------------------------------------------------
def flood(trav, start):
    """reach uint8 [gh,gw] as codd_cost_map defines it: 1 on the 4-connected component of the start cell, else 0."""
    gh, gw = trav.shape
    seen = np.zeros((gh, gw), np.uint8)
    if not trav[start[1], start[0]]:
        return seen
    seen[start[1], start[0]] = 1
    todo = deque([(start[1], start[0])])
    while todo:
        j, i = todo.popleft()
        for y, x in ((j - 1, i), (j + 1, i), (j, i - 1), (j, i + 1)):
            if 0 <= y < gh and 0 <= x < gw and trav[y, x] and not seen[y, x]:
                seen[y, x] = 1
                todo.append((y, x))
    return seen


def make(name, gh, gw, start, build=None, blocked=(), cost=(), mode=CELL, goal=(0, 0), goal_xz=(0.0, 0.0), cell=0.0, goal_r2=0,
         neutral=50, factor=205, unknown_cost=128, max_path=None, cost_record=None, origin=None, with_dir=True, reach=None):
    """A window of cost 0, all traversable; ``blocked``: cells or slices (j, i) that are not (cost 254); ``cost``: (cells,
    value) pairs; ``build(cost, trav)`` last.  ``goal`` = (i, j) in CELL mode.  ``reach`` is the flood from ``start`` unless
    given; every seventh reachable cell gets 2, as a frontier would."""
    cst, trav = np.zeros((gh, gw), np.uint8), np.ones((gh, gw), bool)
    for at in blocked:
        trav[at], cst[at] = False, 254
    for at, v in cost:
        cst[at] = v
    if build is not None:
        build(cst, trav)
    if reach is None:
        reach = flood(trav, start)
        flat = reach.ravel()
        flat[np.flatnonzero(flat)[::7]] = 2
    rec = None
    if cost_record is not None:
        rec = np.zeros(16, np.float64)
        rec[8] = cost_record
    mrec = None
    if origin is not None:
        mrec = np.zeros(16, np.float64)
        mrec[8], mrec[9] = origin
    return dict(name=name, cost=cst, reach=reach.astype(np.uint8), start=start, mode=mode, goal_i=goal[0], goal_j=goal[1],
                goal_x=float(goal_xz[0]), goal_z=float(goal_xz[1]), cell=float(cell), goal_r2=goal_r2, neutral=neutral, factor=factor,
                unknown_cost=unknown_cost, max_path=gh * gw if max_path is None else max_path, cost_record=rec, map_record=mrec,
                with_dir=with_dir)


def _wall_with_corridor(cst, trav):  # 7 x 9: a wall across row 3, one corridor of cost 200 through it at column 4
    trav[3, 1:8], cst[3, 1:8] = False, 254
    trav[3, 4] = True
    cst[2:5, 4] = 200


def _unknown_band(cst, trav):  # 9 x 11: unknown cells (cost 255, traversable: through_unknown) across rows 3 .. 5, a free lane
    cst[3:6, :] = 255
    cst[3:6, 10] = 0


def _seed_disk(cst, trav):  # the cells around the start carry 253 (inscribed) and 255 (never seen) and are traversable
    cst[3:8, 3:8] = 255
    cst[4:7, 4:7] = 253
    trav[0:2, :], cst[0:2, :] = False, 254


def _two_rooms(cst, trav):  # 9 x 12: a closed wall at column 6; the start's side is columns 0 .. 5
    trav[:, 6], cst[:, 6] = False, 254


def _snap_tie(cst, trav):  # 7 x 7: only the ring at Chebyshev distance 2 around (3, 3) is traversable
    trav[...], cst[...] = False, 254
    trav[1:6, 1:6], cst[1:6, 1:6] = True, 0
    trav[2:5, 2:5], cst[2:5, 2:5] = False, 254


def serpentine(cst, trav):
    """Walls on every odd row with a gap of one cell at alternating ends: one corridor through every row."""
    for n, r in enumerate(range(1, trav.shape[0], 2)):
        trav[r, :], cst[r, :] = False, 254
        gap = -1 if n % 2 == 0 else 0
        trav[r, gap], cst[r, gap] = True, 60


def rooms(seed, side=16):
    """Rooms of ``side`` cells with one doorway of two cells per wall segment, costs rising towards the walls, a few
    unknown cells that stay traversable."""
    def build(cst, trav):
        rng = np.random.default_rng(seed)
        gh, gw = trav.shape
        cst[...] = rng.integers(0, 40, (gh, gw))
        for r in range(side - 1, gh - 1, side):
            trav[r, :] = False
            for c0 in range(0, gw, side):
                d = c0 + int(rng.integers(1, side - 3))
                trav[r, d:d + 2] = True
        for q in range(side - 1, gw - 1, side):
            trav[:, q] = False
            for r0 in range(0, gh, side):
                d = r0 + int(rng.integers(1, side - 3))
                trav[d:d + 2, q] = True
        near = np.pad(~trav, 1)
        near = near[:-2, 1:-1] | near[2:, 1:-1] | near[1:-1, :-2] | near[1:-1, 2:]
        cst[near & trav] = 180
        cst[rng.random((gh, gw)) < 0.02] = 255
        cst[~trav] = 254
    return build


def scatter(seed, p_blocked=0.25):
    def build(cst, trav):
        rng = np.random.default_rng(seed)
        gh, gw = trav.shape
        cst[...] = rng.integers(0, 253, (gh, gw))
        cst[rng.random((gh, gw)) < 0.1] = 255
        trav[...] = rng.random((gh, gw)) >= p_blocked
        cst[~trav] = 254
    return build


def chained(name, costmap_case, **kw):
    """codd_plan behind codd_cost_map: cost, reach and the record of the costmap restatement on one of its own cases."""
    c, r = cr.CASES[cr.NAMES[costmap_case]], cr.expected(costmap_case)
    gh, gw = r["cost"].shape
    out = make(name, gh, gw, c["start"], mode=FRONTIER, cost_record=0, reach=r["reach"].copy(), **kw)
    out["cost"], out["cost_record"] = r["cost"].copy(), r["record"].copy()
    return out


CASES = [
    make("1x1", 1, 1, (0, 0)),
    make("1x9-corridor", 1, 9, (0, 0), goal=(8, 0), cost=[((0, 4), 100)]),
    make("9x1-corridor", 9, 1, (0, 8), goal=(0, 0), cost=[((2, 0), 255)]),
    make("start-in-goal", 5, 6, (2, 3), goal=(2, 3)),
    make("2x2-corner", 2, 2, (0, 0), goal=(1, 1), blocked=[(0, 1)]),
    make("3x3-corner", 3, 3, (0, 0), goal=(2, 2), blocked=[(1, 1)]),
    make("open-17x19", 17, 19, (1, 2), goal=(15, 9)),
    make("corridor-factor0", 7, 9, (4, 1), goal=(4, 5), factor=0, build=_wall_with_corridor),
    make("detour-factor1024", 7, 9, (4, 1), goal=(4, 5), factor=1024, build=_wall_with_corridor),
    make("unknown-cost0", 9, 11, (2, 0), goal=(2, 8), unknown_cost=0, build=_unknown_band),
    make("unknown-cost254", 9, 11, (2, 0), goal=(2, 8), unknown_cost=254, build=_unknown_band),
    make("seed-disk-253-255", 11, 11, (5, 5), goal=(10, 10), build=_seed_disk),
    make("snap-other-component", 9, 12, (2, 4), goal=(9, 1), build=_two_rooms),
    make("snap-tie", 7, 7, (1, 1), goal=(3, 3), build=_snap_tie),
    make("goal-r2-5", 9, 12, (1, 7), goal=(8, 2), goal_r2=5, blocked=[(2, 8), (3, 7)]),
    make("world-inside", 9, 12, (6, 4), mode=WORLD, goal_xz=(-1.13, -0.62), cell=0.25, origin=(-9, -5), blocked=[(4, 5), (3, 5)]),
    make("world-outside", 9, 12, (2, 4), mode=WORLD, goal_xz=(40.0, -3.0), cell=0.1, origin=(-6, -4), build=_two_rooms),
    make("frontier-valid", 9, 12, (2, 4), mode=FRONTIER, cost_record=7 * 12 + 5, build=_two_rooms),
    make("frontier-none", 9, 12, (2, 4), mode=FRONTIER, cost_record=-1, build=_two_rooms),
    make("start-not-traversable", 9, 12, (6, 4), goal=(2, 2), build=_two_rooms),
    make("max-path-1", 17, 19, (1, 2), goal=(15, 9), max_path=1),
    make("max-path-short", 17, 19, (1, 2), goal=(15, 9), max_path=14),
    make("dir-null", 17, 19, (3, 12), goal=(16, 1), with_dir=False, build=scatter(11, 0.15)),
    make("scatter-17x19", 17, 19, (9, 8), goal=(0, 0), goal_r2=2, build=scatter(12)),
    make("serpentine-33x31", 33, 31, (0, 0), goal=(0, 32), build=serpentine),
    make("scatter-33x31", 33, 31, (15, 16), goal=(30, 0), build=scatter(13, 0.2)),
    make("rooms-127x129", 127, 129, (66, 66), goal=(2, 2), build=rooms(1)),
    make("scatter-127x129", 127, 129, (64, 63), goal=(120, 120), goal_r2=9, build=scatter(14, 0.2)),
    make("rooms-160x160", 160, 160, (80, 80), goal=(157, 3), build=rooms(2)),
    make("open-160x160", 160, 160, (80, 80), mode=FRONTIER, cost_record=159 * 160 + 159),
    make("1x25600", 1, 25600, (12800, 0), goal=(25599, 0), max_path=1024, cost=[((0, slice(100, 25600, 100)), 90)]),
    chained("chained-16x24", "16x24-scatter-b"),
    chained("chained-frontier-tie", "frontier-tie", goal_r2=2),
    chained("chained-127x129", "small-scatter-b", max_path=64),
]
NAMES = {c["name"]: k for k, c in enumerate(CASES)}
assert len(NAMES) == len(CASES)


def case_id(c):
    return c["name"]


@functools.lru_cache(None)
def expected(name):
    """The restatement's outputs for the case ``name``, computed once a process and left unchanged (read-only arrays)."""
    out = plan(CASES[NAMES[name]])
    for v in out.values():
        v.setflags(write=False)
    return out
