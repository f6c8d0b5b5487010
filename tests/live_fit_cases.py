"""The launches of the three fitted LiveSession stages whose output bits tests/golden/live_fit_bits.json records (sha256
of the bytes of ONE output tensor each), shared by the generator tools/parent_bits.py --cases live_fit and by
tests/test_gpu_live_fit_bits.py.  The recorded bits are those of the library BEFORE the fixed-order sums, the Cholesky
solve, the ticket and the scratch layout of ego.hip, epipolar.hip and ground.hip moved into fit_sums.h.  Inputs are the
scenes the stages' own GPU tests use, at their sizes; every output is pre-filled with a fixed pattern, so bytes the entry
leaves alone are part of the digest, and the scratch holds a pattern too (its contents must not matter).

* ``ego/<case>/<record|moving|residual>``: ops.ego_motion on live_ego_ref.scene for every (shape, mover) of
  test_gpu_live_ego.CASES, and on the three live_ego_ref.degenerate kinds.
* ``epipolar/<case>/<map|nomap>/<record|dy_map>``: ops.epipolar_check on every live_epi_ref.CASES entry, once with the
  map requested and once without (the record only).
* ``ground/<case>/<record|labels|height|grid_count|grid_height>``: ops.ground_plane on every live_ground_ref.CASES entry
  with the heights and, where the case has a grid, the grid: heavy-unseeded and none (ok = 0), few-inliers (the outputs
  taken back) and two-trips (260 x 256: the stride loops take two trips) among them."""
import numpy as np
import torch

import live_ego_ref as lego
import live_epi_ref as lepi
import live_ground_ref as lg
import test_gpu_live_ego as gle
from parent_bits import DEV, digest

NAME = "live_fit"
# the sources of the three entries, in the tree of the fixture's commit and in this one
SOURCES = ("codd_amd/csrc/ego.hip", "codd_amd/csrc/epipolar.hip", "codd_amd/csrc/ground.hip", "codd_amd/csrc/fit_sums.h")
DEGENERATE = ("all_invalid", "few_valid", "one_ray")
EGO_OUT = ("record", "moving", "residual")
FILL, FILL_U8, FILL_SCRATCH = -7.0, 0x5A, 0xAB


def _full(shape, dtype, fill=FILL):
    return torch.full(tuple(shape), fill, dtype=dtype, device=DEV)


def _scratch(nbytes):
    return _full((nbytes,), torch.uint8, FILL_SCRATCH)


# ------------------------------------------------------------------------------------------------ ego
def ego_cases():
    """[(case id, function -> scene, scale)]"""
    out = [(i, (lambda s=shape, m=mover: lego.scene(s, m)), lego.SCALE) for i, (shape, mover) in zip(gle.ids, gle.CASES)]
    return out + [("degenerate-" + k, (lambda k=k: lego.degenerate(k)), 1.0) for k in DEGENERATE]


def ego_keys():
    return ["ego/%s/%s" % (i, o) for i, _, _ in ego_cases() for o in EGO_OUT]


def ego_digests():
    from codd_amd import ops
    out = {}
    for i, make, scale in ego_cases():
        s = make()
        h, w = s["crop"]
        rec, mov, res = _full((16,), torch.float32), _full((h, w), torch.uint8, FILL_U8), _full((h, w), torch.float32)
        ops.ego_motion(s["T"].to(DEV), s["depth"][0].to(DEV), s["K"], (h, w), rec, mov, res, scale=scale,
                       scratch=_scratch(ops.ego_motion_scratch(h, w)))
        for o, t in zip(EGO_OUT, (rec, mov, res)):
            out["ego/%s/%s" % (i, o)] = digest(t)
    return out


# ------------------------------------------------------------------------------------------------ epipolar
def epi_keys():
    return ["epipolar/%s/%s" % (lepi.case_id(s), k) for s in lepi.CASES for k in ("map/record", "map/dy_map", "nomap/record")]


def epi_digests():
    from codd_amd import ops
    out = {}
    for spec in lepi.CASES:
        c = lepi.case(spec)
        h, w = c["crop"]
        disp, left, right = (torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("disp", "left", "right"))
        for with_map in (True, False):
            rec, dy = _full((32,), torch.float64), _full((h, w), torch.float32)
            ops.epipolar_check(disp, left, right, c["K"], (h, w), rec, dy if with_map else None,
                               scratch=_scratch(ops.epipolar_scratch(h, w)), **c["par"])
            key = "epipolar/%s/%s/" % (lepi.case_id(spec), "map" if with_map else "nomap")
            out[key + "record"] = digest(rec)
            if with_map:
                out[key + "dy_map"] = digest(dy)
    return out


# ------------------------------------------------------------------------------------------------ ground
def _ground_out(spec):
    return ("record", "labels", "height") + (("grid_count", "grid_height") if spec["grid"] is not None else ())


def ground_keys():
    return ["ground/%s/%s" % (lg.case_id(s), o) for s in lg.CASES for o in _ground_out(s)]


def ground_digests():
    from codd_amd import ops
    out = {}
    for spec in lg.CASES:
        c = lg.case(spec)
        h, w = c["crop"]
        grid = None if c["grid"] is None else c["grid"][0]
        rec, lab, hgt = _full((32,), torch.float64), _full((h, w), torch.uint8, FILL_U8), _full((h, w), torch.float32)
        cnt = None if grid is None else _full((2,) + grid, torch.int32, -7)
        gh = None if grid is None else _full(grid, torch.float32)
        par = {k: v for k, v in c["par"].items() if grid is not None or k != "cell"}
        ops.ground_plane(torch.from_numpy(c["disp"]).to(DEV), c["K"], c["calib"], (h, w), rec, lab, hgt, cnt, gh,
                         scratch=_scratch(ops.ground_scratch(h, w, grid)), seed=c["seed"], up=lg.UP, **par)
        for o, t in zip(_ground_out(spec), (rec, lab, hgt, cnt, gh)):
            out["ground/%s/%s" % (lg.case_id(spec), o)] = digest(t)
    return out


# ------------------------------------------------------------------------------------------------ all of it
def groups():
    """[(group id, keys, function -> {key: digest})] in the fixture's order: one group per stage."""
    return [("ego", ego_keys(), ego_digests), ("epipolar", epi_keys(), epi_digests), ("ground", ground_keys(), ground_digests)]
