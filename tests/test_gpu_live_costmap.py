"""LiveSession cost map on the GPU: codd_cost_map against the brute-force restatement of tests/live_costmap_ref.py.

Everything the entry computes is an integer, so every comparison is BIT FOR BIT: dist2, nearest, cost, reach and the 16
doubles of the record, with no excluded cell and no tolerance (what each case is built to show is asserted on the
restatement in tests/test_live_costmap.py).  The grids reach from 1 x 1 to 127 x 129 and 161 x 137, either side of the threshold of
the single-workgroup variant (which is not in the library), each case compared with the restatement.  Then nearest =
NULL, determinism, dirty buffers and scratch with guard elements, rejected arguments, a three-frame session against the
entry called by hand, and the command line.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_costmap_ref as cr  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every buffer the entry writes
IDS = [cr.case_id(c) for c in cr.CASES]
OUT = ("dist2", "nearest", "cost", "reach", "record")


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


class Run:
    """One call of ops.cost_map on the case ``c``: everything the entry writes lies between guard elements, and the outputs
    and the scratch start out as garbage (0xFF bytes: NaN as a double, -1 as an integer)."""
    FILLS = dict(dist2=-7, nearest=-7, cost=7, reach=7, record=-7.0, scratch=0x5A)

    def __init__(self, c, nearest=True):
        from codd_amd import ops
        gh, gw = c["map"].shape
        self.shape, self.with_nearest = (gh, gw), nearest
        self.map = torch.zeros(gh, gw, dtype=torch.int16, device=DEV)
        self.age = torch.zeros(gh, gw, dtype=torch.uint8, device=DEV)
        self.bufs = {}
        for name, n, dt in (("dist2", gh * gw, torch.int32), ("nearest", gh * gw, torch.int32), ("cost", gh * gw, torch.uint8),
                            ("reach", gh * gw, torch.uint8), ("record", 16, torch.float64),
                            ("scratch", ops.cost_map_scratch(gh, gw, c["R"]), torch.uint8)):  # (the same for every R)
            self.bufs[name] = _guarded(n, dt, self.FILLS[name])
            self.bufs[name][1].view(torch.uint8).fill_(0xFF)
        self.launch(c)

    def view(self, name):
        v = self.bufs[name][1]
        return v.view(*self.shape) if name in ("dist2", "nearest", "cost", "reach") else v

    def launch(self, c, **over):
        """(again, with another case of the same shape: into the outputs and the scratch as the last call left them)"""
        from codd_amd import ops
        assert c["map"].shape == self.shape
        self.map.copy_(torch.from_numpy(c["map"]))
        self.age.copy_(torch.from_numpy(c["age"]))
        self.lut = torch.from_numpy(c["lut"].copy()).to(DEV)
        self.inputs = tuple(t.clone() for t in (self.map, self.age, self.lut))
        args = dict(start=c["start"], occ_level=c["occ_level"], free_level=c["free_level"], seed_r2=c["seed_r2"],
                    through_unknown=c["through_unknown"], scratch=self.view("scratch"))
        args.update(over)
        ops.cost_map(self.map, self.age, self.lut, c["R"], args.pop("start"), self.view("dist2"),
                     self.view("nearest") if self.with_nearest else None, self.view("cost"), self.view("reach"), self.view("record"),
                     **args)
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        for name, (buf, view) in self.bufs.items():
            fill, n = self.FILLS[name], view.numel()
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), f"{what}: {name} guard overwritten"
        assert all(torch.equal(a, b) for a, b in zip((self.map, self.age, self.lut), self.inputs)), f"{what}: an input was modified"
        if not self.with_nearest:
            assert bool((self.view("nearest") == -1).all()), f"{what}: nearest = NULL was written"

    def outputs(self):
        return {k: self.view(k).cpu().numpy() for k in OUT if k != "nearest" or self.with_nearest}

    def same_bytes(self, other):
        a, b = self.outputs(), other.outputs()
        return all(a[k].tobytes() == b[k].tobytes() for k in a if k in b)


def _assert_equal(out, name, what=None):
    ref = cr.expected(name)
    what = what or name
    print(f"{what}: record {out['record'].tolist()}")
    for k in out:
        if k == "record":
            continue
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (what, k)
        bad = np.argwhere(out[k] != ref[k])
        assert bad.size == 0, (f"{what}: {k} differs in {len(bad)} cells, first at {bad[:8].tolist()}: {out[k][tuple(bad[0])]} vs "
                               f"{ref[k][tuple(bad[0])]}")
    assert not np.isnan(out["record"]).any(), f"{what}: NaN in the record"
    assert out["record"].tobytes() == ref["record"].tobytes(), f"{what}: record {out['record'].tolist()} vs {ref['record'].tolist()}"


@pytest.mark.parametrize("name", IDS)
def test_cost_map_against_reference(name):
    c = cr.CASES[cr.NAMES[name]]
    a = Run(c)
    a.check_guards(name)
    _assert_equal(a.outputs(), name)
    b = Run(c)  # determinism: a second run gives equal bytes
    assert a.same_bytes(b)
    n = Run(c, nearest=False)  # nearest = NULL: the other outputs keep their bytes, record [7] included
    n.check_guards(name + " without nearest")
    _assert_equal(n.outputs(), name, name + " without nearest")
    assert a.same_bytes(n)


@pytest.mark.parametrize("order", (("no-occ", "corner-source", "start-occ", "gap-open", "through-unknown-on", "16x24-scatter", "R1",
                                    "unknown-inscribed", "start-unknown-seed", "never-seen-free-level"),
                                   ("small-scatter", "serpentine-small", "small-scatter-b", "serpentine-small-vertical"),
                                   ("large-scatter", "serpentine-large", "large-scatter-b", "serpentine-large-vertical", "large-R40")),
                         ids=("16x24", "127x129", "161x137"))
def test_dirty_buffers_and_scratch_give_the_same_bytes(order):
    """A call into outputs and a scratch that still hold another case's results: its parents, its counters, its record."""
    r = Run(cr.CASES[cr.NAMES[order[0]]])
    for name in order:  # (the first case twice)
        c = cr.CASES[cr.NAMES[name]]
        r.launch(c)
        r.check_guards(name)
        _assert_equal(r.outputs(), name, name + " into used buffers")
        assert Run(c).same_bytes(r), f"{name}: used buffers changed a byte"


def test_ops_reject_bad_arguments():
    from codd_amd import _abi, ops
    for bad in ((0, 4, 3), (4, 0, 3), (4097, 1, 3), (1, 4097, 3), (4096, 2048, 3), (4, 4, 0), (4, 4, 129)):
        with pytest.raises(ValueError):
            ops.cost_map_scratch(*bad)
    assert ops.cost_map_scratch(2048, 2048, 128) > 0
    c = cr.CASES[cr.NAMES["16x24-scatter"]]
    a = Run(c)
    want = a.outputs()
    before = {k: buf.clone() for k, (buf, _) in a.bufs.items()}
    scr = a.view("scratch")
    for bad in (dict(start=(-1, 8)), dict(start=(24, 8)), dict(start=(12, -1)), dict(start=(12, 16)), dict(seed_r2=-1),
                dict(free_level=c["occ_level"]), dict(free_level=c["occ_level"] + 1), dict(occ_level=c["free_level"]),
                dict(scratch=scr[:-1])):
        with pytest.raises(_abi.CoddHipError):
            a.launch(c, **bad)
    with pytest.raises(_abi.CoddHipError):  # R outside [1, 128]: the table would have 129^2 + 2 entries
        ops.cost_map(a.map, a.age, torch.zeros(129 * 129 + 2, dtype=torch.uint8, device=DEV), 129, c["start"], a.view("dist2"), None,
                     a.view("cost"), a.view("reach"), a.view("record"), scratch=scr)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k].view(torch.uint8), buf.view(torch.uint8)) for k, (buf, _) in a.bufs.items()), \
        "a rejected call wrote something"
    with pytest.raises(AssertionError):  # the outputs have the map's shape
        ops.cost_map(a.map, a.age, a.lut, c["R"], c["start"], a.view("dist2")[:-1], None, a.view("cost"), a.view("reach"),
                     a.view("record"), scratch=scr)
    with pytest.raises(AssertionError):  # the table has R R + 2 entries
        ops.cost_map(a.map, a.age, a.lut[:-1], c["R"], c["start"], a.view("dist2"), None, a.view("cost"), a.view("reach"),
                     a.view("record"), scratch=scr)
    got = a.outputs()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


# ---- the session against the entry called by hand -------------------------------------------------------------------------
LOCALMAP = dict(grid=(16, 24), cell=0.25, range_max=25.6, min_pixels=4, select=("obstacle", "overhead"), decay=1)
COSTMAP = dict(robot_radius=0.25, inflation_radius=1.0, scaling=2.0, start_radius=0.8, nearest=True)
NFRAMES = 3


def test_session_costmap_against_the_entry_by_hand():
    import test_gpu_live_ground as glg
    import test_gpu_live_localmap as gll
    import test_gpu_live_objects as glo
    from codd_amd import live, ops
    plain = glm._plain_results()
    frames = glm._frames()[:NFRAMES]
    s = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP, costmap=COSTMAP)
    base = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP)  # without costmap=: the parent's tuple and bytes
    thru = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP, costmap=dict(COSTMAP, through_unknown=True, nearest=False))
    gh, gw = LOCALMAP["grid"]
    R, lut = ops.cost_lut(0.25, 0.25, 1.0, 2.0)
    assert R == 4 and s._cost_R == 4
    lut = torch.from_numpy(lut).to(DEV)
    d2, near = torch.empty(gh, gw, dtype=torch.int32, device=DEV), torch.empty(gh, gw, dtype=torch.int32, device=DEV)
    cost, reach = torch.empty(gh, gw, dtype=torch.uint8, device=DEV), torch.empty(gh, gw, dtype=torch.uint8, device=DEV)
    rec = torch.empty(16, dtype=torch.float64, device=DEV)
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 5
        res, e, g, m, cm = got
        got1 = base.step(left, right)
        assert len(got1) == 4
        res1, e1, g1, m1 = got1
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i]), f"frame {i}: the depth result changed"
        assert glg._same_ground(g, g1), f"frame {i}: Ground changed with costmap= on"
        assert (e is None) == (e1 is None) and (e is None or (e.pose.tobytes() == e1.pose.tobytes() and e.moving.tobytes() == e1.moving.tobytes()))
        assert gll._same_map(m, m1), f"frame {i}: LocalMap changed with costmap= on"
        assert isinstance(cm, live.CostMap) and cm.cost.shape == (gh, gw) and cm.cost.flags["OWNDATA"]
        assert cm.origin == m.origin and cm.cell == 0.25 and cm.start == (gw // 2, gh // 2)
        # by hand, on this frame's LocalMap arrays
        for through, nr, have in ((False, near, cm), (True, None, thru.step(left, right)[-1])):
            ops.cost_map(torch.from_numpy(m.logodds).to(DEV), torch.from_numpy(m.age).to(DEV), lut, R, (gw // 2, gh // 2), d2, nr, cost,
                         reach, rec, occ_level=m.occ_level, free_level=m.free_level, seed_r2=int(np.floor((0.8 / 0.25) ** 2)),
                         through_unknown=through)
            torch.cuda.synchronize()
            want = live.costmap_from_buffers(rec.cpu().numpy(), d2.cpu().numpy(), cost.cpu().numpy(), reach.cpu().numpy(),
                                             None if nr is None else nr.cpu().numpy(), m.origin, 0.25, (gw // 2, gh // 2))
            for k in ("cost", "dist2", "reach"):
                assert getattr(have, k).tobytes() == getattr(want, k).tobytes(), f"frame {i}: CostMap.{k} differs from the entry by hand"
            assert (have.nearest is None) == (nr is None) and (nr is None or have.nearest.tobytes() == want.nearest.tobytes())
            assert tuple(have[4:]) == tuple(want[4:]), f"frame {i}: {tuple(have[4:])} vs {tuple(want[4:])}"
        print(f"frame {i}: {cm.occupied} occupied, {cm.inscribed} inscribed, {cm.unknown} unknown, {cm.reachable} reachable, "
              f"{cm.frontiers} frontiers, start ok {cm.start_ok}, nearest frontier {cm.frontier_cell} at {cm.frontier_dist2}")
        assert cm.occupied == m.occupied and cm.reachable == int((cm.reach != 0).sum()) and cm.frontiers == int((cm.reach == 2).sum())
        assert cm.start_ok == (m.logodds[gh // 2, gw // 2] < m.occ_level) and np.isfinite(cm.clearance()).sum() == (cm.dist2 != ops.COST_FAR).sum()
    for t in (base, thru, s):
        t.reset()
        t.close()
    assert s._d_cost is None and s._h_cost is None and s._cost_lut is None and s._cost_scratch is None


def test_cli_live_costmap(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 3
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    inference.main(["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
                    "--live", "--ground", "--ego", "--localmap", "--costmap", "--show-dir", str(tmp_path / "out")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "costmap:" in ln]
    assert len(lines) == 1 and f"of {n} frames" in lines[0]
    assert {"left.costmap.pred.npz", "left.localmap.pred.npz"} <= set(os.listdir(tmp_path / "out"))
    z = np.load(tmp_path / "out" / "left.costmap.pred.npz")
    counts = ("occupied", "inscribed", "unknown", "reachable", "frontiers", "start_ok", "start_dist2", "frontier_dist2")
    assert sorted(z.files) == sorted(counts + ("cost", "dist2", "reach", "frontier_cell", "start", "cell", "robot_radius", "inflation_radius"))
    assert z["cost"].shape == z["dist2"].shape == z["reach"].shape == (1, n, 128, 128)
    assert z["cost"].dtype == z["reach"].dtype == np.uint8 and z["dist2"].dtype == np.int32
    assert all(z[k].shape == (1, n) and z[k].dtype == np.int32 for k in counts) and z["frontier_cell"].shape == (1, n, 2)
    assert tuple(z["start"]) == (64, 64) and float(z["cell"]) == 0.1 and float(z["robot_radius"]) == 0.3 and float(z["inflation_radius"]) == 1.0
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, ground=True, egomotion=True, localmap=True, costmap=True)
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        cm = s.step(left, right)[-1]
        assert all(getattr(cm, k).tobytes() == z[k][0, i].tobytes() for k in ("cost", "dist2", "reach"))
        assert all(int(getattr(cm, k)) == z[k][0, i] for k in counts)
        assert (cm.frontier_cell or (-1, -1)) == tuple(z["frontier_cell"][0, i])
    s.reset()
    s.close()
