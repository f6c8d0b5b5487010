"""Restatement of codd_cost_map (include/codd_hip.h) shared by the CPU and the GPU tests, in numpy only, by brute force and
straight from the definitions of the header, and the cases.

``distance`` visits every pair of a cell and an OCC cell (the sources in raster order, a strictly smaller distance wins: the
smallest raster index among ties), ``flood`` is a plain breadth-first fill from the start cell, ``frontiers`` the rule of the
header, ``cost_map`` chains them and writes the record.  Nothing here is separable, tiled or a union-find: what the kernel
does in two passes and five launches is one loop each here.  ``ops.cost_lut`` enters only through the bytes of the table it
returns.

A case is a dict: ``map`` int16 and ``age`` uint8 [gh,gw], ``R``, ``lut`` uint8 [R R + 2], ``start`` = (i, j), ``seed_r2``,
``through_unknown``, ``occ_level``, ``free_level``.  Cells are planted with ``OCC_V`` (occupied), ``FREE_V`` with age 0 (free)
and 0 with age 0 (unknown: between the levels).  The union-find tile of the kernel is 16 rows x 64 columns, and the
single-workgroup variant that was measured against it takes windows of at most 16384 cells: 127 x 129 (16383 cells) lies
below and 161 x 137 (11 x 3 tiles, the last of each partial) above that threshold, and neither side divides by a tile side.
"""
import functools
import os
import sys
from collections import deque

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codd_amd import ops  # noqa: E402  (cost_lut: host only)

FREE, OCC, UNKNOWN = 0, 1, 2
LETHAL, INSCRIBED, NO_INFO, FAR = 254, 253, 255, 0x7fffffff
OCC_LEVEL, FREE_LEVEL = 8, -4
OCC_V, FREE_V, UNKNOWN_V = 16, -8, 0
TILE = (16, 64)  # the kernel's union-find tile (rows, columns)
SMALL, LARGE = (127, 129), (161, 137)  # either side of 16384 cells, the threshold of the single-workgroup variant


def classes(c):
    m, age = c["map"].astype(np.int64), c["age"]
    return np.where(m >= c["occ_level"], OCC, np.where((age != 255) & (m <= c["free_level"]), FREE, UNKNOWN)).astype(np.uint8)


def distance(cls, R):
    """(dist2, nearest) int32 [gh,gw]: every cell against every OCC cell."""
    gh, gw = cls.shape
    jj, ii = np.mgrid[:gh, :gw]
    best = np.full((gh, gw), np.iinfo(np.int64).max, np.int64)
    near = np.full((gh, gw), -1, np.int64)
    for j, i in np.argwhere(cls == OCC):  # (raster order)
        d = (ii - i) ** 2 + (jj - j) ** 2
        take = d < best
        best[take], near[take] = d[take], j * gw + i
    far = best > R * R
    return np.where(far, FAR, best).astype(np.int32), np.where(far, -1, near).astype(np.int32)


def costs(cls, dist2, lut, R):
    """(c, cost): the table's value per cell and the cost (NO_INFO on an UNKNOWN cell that is not inscribed)."""
    c = lut[np.where(dist2 <= R * R, dist2, R * R + 1)].astype(np.int64)
    return c, np.where((cls == UNKNOWN) & (c < INSCRIBED), NO_INFO, c).astype(np.uint8)


def traversable(cls, c, start, seed_r2, through_unknown):
    gh, gw = cls.shape
    jj, ii = np.mgrid[:gh, :gw]
    seed = (ii - start[0]) ** 2 + (jj - start[1]) ** 2 <= seed_r2
    other = (c < INSCRIBED) & ((cls == FREE) | ((cls == UNKNOWN) & bool(through_unknown)))
    return np.where(seed, cls != OCC, other)


def flood(trav, start):
    """bool [gh,gw]: the cells joined to the start cell by 4-neighbour steps over traversable cells."""
    gh, gw = trav.shape
    seen = np.zeros((gh, gw), bool)
    if not trav[start[1], start[0]]:
        return seen
    seen[start[1], start[0]] = True
    todo = deque([(start[1], start[0])])
    while todo:
        j, i = todo.popleft()
        for y, x in ((j - 1, i), (j + 1, i), (j, i - 1), (j, i + 1)):
            if 0 <= y < gh and 0 <= x < gw and trav[y, x] and not seen[y, x]:
                seen[y, x] = True
                todo.append((y, x))
    return seen


def frontiers(cls, reached):
    """bool [gh,gw]: reachable cells with a 4-neighbour inside the window that is UNKNOWN and not reachable."""
    edge = np.pad((cls == UNKNOWN) & ~reached, 1)  # (outside the window: no neighbour)
    return reached & (edge[:-2, 1:-1] | edge[2:, 1:-1] | edge[1:-1, :-2] | edge[1:-1, 2:])


def cost_map(c):
    """The outputs of the entry on the case ``c``: dist2, nearest, cost, reach, record (and cls, trav for the tests)."""
    cls = classes(c)
    gh, gw = cls.shape
    si, sj = c["start"]
    dist2, nearest = distance(cls, c["R"])
    cv, cost = costs(cls, dist2, c["lut"], c["R"])
    trav = traversable(cls, cv, c["start"], c["seed_r2"], c["through_unknown"])
    reached = flood(trav, c["start"])
    front = frontiers(cls, reached)
    reach = (reached.astype(np.uint8) + front.astype(np.uint8)).astype(np.uint8)
    rec = np.zeros(16, np.float64)
    rec[0], rec[1], rec[2] = (cls == OCC).sum(), ((cost == INSCRIBED) | (cost == LETHAL)).sum(), (cost == NO_INFO).sum()
    rec[3], rec[4], rec[5] = reached.sum(), front.sum(), float(trav[sj, si])
    rec[6] = -1.0 if dist2[sj, si] == FAR else float(dist2[sj, si])
    rec[7] = float(nearest[sj, si])
    rec[8], rec[9] = -1.0, -1.0
    fj, fi = np.nonzero(front)
    if fj.size:
        d = (fi - si) ** 2 + (fj - sj) ** 2
        k = int(np.lexsort((fj * gw + fi, d))[0])  # the squared distance, then the raster index
        rec[8], rec[9] = float(fj[k] * gw + fi[k]), float(d[k])
    return dict(dist2=dist2, nearest=nearest, cost=cost, reach=reach, record=rec, cls=cls, trav=trav)


# ---- the cases ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def lut(cell, robot_radius, inflation_radius, scaling):
    R, table = ops.cost_lut(cell, robot_radius, inflation_radius, scaling)
    return R, np.frombuffer(table.tobytes(), np.uint8)  # (its bytes)


THIN = (1.0, 0.0, 1.0, 1.0)   # R = 1: only an OCC cell itself blocks
ROBOT1 = (1.0, 1.0, 3.0, 1.0)  # R = 3, inscribed radius 1 cell: the 4-neighbours of an OCC cell cost 253
WIDE = (1.0, 1.5, 5.0, 0.5)    # R = 5


def make(name, gh, gw, table=ROBOT1, fill=FREE_V, start=None, seed_r2=0, through_unknown=False, occ=(), unknown=(), free=(),
         never=(), build=None):
    """A window filled with ``fill`` (age 0), then ``occ``, ``unknown``, ``free`` cells or slices planted ((j, i) or (slice,
    slice)), ``never``: age 255 with the value left; ``build(map, age)`` last."""
    m, age = np.full((gh, gw), fill, np.int16), np.zeros((gh, gw), np.uint8)
    for cells, v in ((unknown, UNKNOWN_V), (free, FREE_V), (occ, OCC_V)):
        for at in cells:
            m[at] = v
    for at in never:
        age[at] = 255
    if build is not None:
        build(m, age)
    R, table = lut(*table)
    return dict(name=name, map=m, age=age, R=R, lut=table, start=(gw // 2, gh // 2) if start is None else start,
                seed_r2=seed_r2, through_unknown=through_unknown, occ_level=OCC_LEVEL, free_level=FREE_LEVEL)


def serpentine(vertical):
    """Walls every fourth row (column) with a gap of three cells at alternating ends: one corridor that crosses every tile
    border of the union-find many times, both ways.  The start is at one end, the far end is reached only through all of it."""
    def build(m, age):
        a = m.T if vertical else m
        for n, r in enumerate(range(3, a.shape[0] - 1, 4)):
            a[r, :] = OCC_V
            if n % 2:
                a[r, :3] = FREE_V
            else:
                a[r, -3:] = FREE_V
    return build


def scatter(seed, p_occ=0.03):
    """A seeded scene: free and unknown patches, never-seen cells, scattered obstacles and a few walls."""
    def build(m, age):
        rng = np.random.default_rng(seed)
        gh, gw = m.shape
        m[...] = rng.integers(-10, 8, (gh, gw))  # below occ_level; <= free_level on about a third
        m[rng.random((gh, gw)) < 0.55] = FREE_V
        m[rng.random((gh, gw)) < p_occ] = OCC_V
        age[...] = rng.choice(np.array([0, 3, 254, 255], np.uint8), (gh, gw), p=(0.5, 0.3, 0.1, 0.1))
        for _ in range(max(1, gh // 16)):
            j, i, n = rng.integers(0, gh), rng.integers(0, gw), rng.integers(1, max(2, gw // 3))
            m[j, i:i + n] = OCC_V
    return build


def _wall_with_gap(width):
    def build(m, age):
        m[6, :] = OCC_V
        m[6, 10:10 + width] = FREE_V
    return build


def _band(m, age):  # an unknown band between the start and the free cells beyond it
    m[5:8, :] = UNKNOWN_V


def _island(m, age):  # free cells around the start inside unknown ones, up to the window's left edge
    m[...] = UNKNOWN_V
    m[4:12, 0:12] = FREE_V


def _ring(m, age):  # a free square around the start in unknown cells: its four sides are frontiers at equal distances
    m[...] = UNKNOWN_V
    m[5:12, 8:15] = FREE_V


CASES = [
    # distances
    make("no-occ", 16, 24),
    make("all-occ", 5, 3, fill=OCC_V, table=WIDE),
    make("corner-source", 16, 24, table=WIDE, occ=[(0, 0)], start=(20, 12)),
    make("tie-in-column", 16, 24, table=WIDE, occ=[(2, 5), (8, 5)], start=(20, 12)),
    make("tie-across-columns", 16, 24, table=WIDE, occ=[(5, 2), (5, 8), (3, 17), (7, 13)], start=(20, 12)),
    make("edge-of-R", 16, 24, table=WIDE, occ=[(0, 0)], start=(20, 12)),  # (3, 4): 25 = R R; (1, 5): 26
    make("R-exceeds-grid", 5, 3, table=(1.0, 1.0, 10.0, 0.3), occ=[(4, 0)], start=(2, 0)),
    make("R1", 16, 24, table=THIN, occ=[(3, 3), (8, 13), (8, 14)]),
    # classes
    make("never-seen-free-level", 16, 24, never=[(slice(0, 8), slice(None))], seed_r2=0),
    make("unknown-inscribed", 16, 24, occ=[(4, 4)], unknown=[(4, 5), (4, 7), (5, 5)]),
    # reachability
    make("start-occ", 16, 24, occ=[(8, 12)], seed_r2=9),
    make("start-unknown-seed", 16, 24, unknown=[(slice(6, 11), slice(10, 15))], seed_r2=4),
    make("seed0-unknown-start", 16, 24, unknown=[(8, 12)], seed_r2=0),
    make("seed0-free-start", 16, 24, seed_r2=0, occ=[(8, 14)]),
    make("gap-closed", 16, 24, start=(11, 2), build=_wall_with_gap(2)),
    make("gap-open", 16, 24, start=(11, 2), build=_wall_with_gap(3)),
    make("serpentine-small", *SMALL, table=THIN, start=(0, 0), build=serpentine(False)),
    make("serpentine-small-vertical", *SMALL, table=THIN, start=(0, 0), build=serpentine(True)),
    make("serpentine-large", *LARGE, table=THIN, start=(0, 0), build=serpentine(False)),
    make("serpentine-large-vertical", *LARGE, table=THIN, start=(0, 0), build=serpentine(True)),
    make("through-unknown-off", 16, 24, start=(12, 2), build=_band),
    make("through-unknown-on", 16, 24, start=(12, 2), through_unknown=True, build=_band),
    make("frontier-not-at-window-edge", 16, 24, start=(5, 8), build=_island),
    make("frontier-tie", 17, 23, start=(11, 8), build=_ring),
    # grids
    make("1x1-free", 1, 1),
    make("1x1-occ", 1, 1, fill=OCC_V),
    make("1x1-unknown", 1, 1, fill=UNKNOWN_V, seed_r2=3),
    make("5x3", 5, 3, occ=[(0, 2)], unknown=[(4, 0), (4, 1)], start=(1, 2)),
    make("16x24-scatter", 16, 24, seed_r2=2, build=scatter(1, 0.05)),
    make("16x24-scatter-b", 16, 24, table=WIDE, seed_r2=2, through_unknown=True, build=scatter(2, 0.02)),
    make("80x24-scatter", 80, 24, table=WIDE, seed_r2=5, build=scatter(3)),
    make("small-scatter", *SMALL, table=WIDE, seed_r2=30, build=scatter(4, 0.01)),
    make("small-scatter-b", *SMALL, table=ROBOT1, seed_r2=30, through_unknown=True, build=scatter(5, 0.02)),
    make("large-scatter", *LARGE, table=WIDE, seed_r2=30, build=scatter(6, 0.01)),
    make("large-scatter-b", *LARGE, table=ROBOT1, seed_r2=30, through_unknown=True, build=scatter(7, 0.02)),
    make("large-R40", *LARGE, table=(0.1, 0.3, 4.0, 3.0), seed_r2=100, build=scatter(8, 0.002)),
]
NAMES = {c["name"]: k for k, c in enumerate(CASES)}
assert len(NAMES) == len(CASES)


def case_id(c):
    return c["name"]


@functools.lru_cache(None)
def expected(name):
    """The restatement's outputs for the case ``name``, computed once a process and left unchanged (read-only arrays)."""
    out = cost_map(CASES[NAMES[name]])
    for v in out.values():
        v.setflags(write=False)
    return out
