"""LiveSession plan on the GPU: codd_plan against the restatement of tests/live_plan_ref.py.

Everything the entry computes is an integer and its result is defined independently of the algorithm, so every comparison
is BIT FOR BIT: potential, dir, path and the 16 doubles of the record, with no excluded cell and no tolerance (what each case
is built to show is asserted on the restatement in tests/test_live_plan.py).  The windows reach from 1 x 1 to 160 x 160 and
1 x 25600, the limit.  Then dir = NULL, determinism, dirty buffers and scratch with guard elements, rejected arguments, a
three-frame session against the entries called by hand with a ``set_goal`` between frames, and the command line.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_plan_ref as pr  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every buffer the entry writes
IDS = [pr.case_id(c) for c in pr.CASES]
OUT = ("potential", "dir", "path", "record")
GOALS = {pr.CELL: lambda c: ("cell", c["goal_i"], c["goal_j"]), pr.WORLD: lambda c: ("world", c["goal_x"], c["goal_z"]),
         pr.FRONTIER: lambda c: "frontier"}


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


class Run:
    """One call of ops.plan on the case ``c``: everything the entry writes lies between guard elements, and the outputs and
    the scratch start out as garbage (0xFF bytes: NaN as a double, -1 as an integer)."""
    FILLS = dict(potential=-7, dir=7, path=-7, record=-7.0, scratch=0x5A)

    def __init__(self, c, with_dir=None):
        from codd_amd import ops
        gh, gw = c["cost"].shape
        self.shape, self.max_path = (gh, gw), c["max_path"]
        self.with_dir = c["with_dir"] if with_dir is None else with_dir
        self.cost = torch.zeros(gh, gw, dtype=torch.uint8, device=DEV)
        self.reach = torch.zeros(gh, gw, dtype=torch.uint8, device=DEV)
        self.crec = torch.zeros(16, dtype=torch.float64, device=DEV)
        self.mrec = torch.zeros(16, dtype=torch.float64, device=DEV)
        self.bufs = {}
        for name, n, dt in (("potential", gh * gw, torch.int32), ("dir", gh * gw, torch.uint8), ("path", c["max_path"], torch.int32),
                            ("record", 16, torch.float64), ("scratch", ops.plan_scratch(gh, gw), torch.uint8)):
            self.bufs[name] = _guarded(n, dt, self.FILLS[name])
            self.bufs[name][1].view(torch.uint8).fill_(0xFF)
        self.launch(c)

    def view(self, name):
        v = self.bufs[name][1]
        return v.view(*self.shape) if name in ("potential", "dir") else v

    def launch(self, c, **over):
        """(again, with another case of the same shape: into the outputs and the scratch as the last call left them)"""
        from codd_amd import ops
        assert c["cost"].shape == self.shape and c["max_path"] == self.max_path
        self.cost.copy_(torch.from_numpy(c["cost"]))
        self.reach.copy_(torch.from_numpy(c["reach"]))
        self.crec.copy_(torch.from_numpy(c["cost_record"] if c["cost_record"] is not None else np.full(16, np.nan)))
        self.mrec.copy_(torch.from_numpy(c["map_record"] if c["map_record"] is not None else np.full(16, np.nan)))
        self.inputs = tuple(t.clone() for t in (self.cost, self.reach, self.crec, self.mrec))
        args = dict(start=c["start"], goal=GOALS[c["mode"]](c), cost_record=self.crec if c["mode"] == pr.FRONTIER else None,
                    map_record=self.mrec if c["mode"] == pr.WORLD else None, cell=c["cell"] if c["mode"] == pr.WORLD else None,
                    goal_r2=c["goal_r2"], neutral=c["neutral"], factor=c["factor"], unknown_cost=c["unknown_cost"],
                    scratch=self.view("scratch"), path=self.view("path"))
        args.update(over)
        ops.plan(self.cost, self.reach, args.pop("start"), self.view("potential"), args.pop("path"), self.view("record"),
                 dir=self.view("dir") if self.with_dir else None, **args)
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        for name, (buf, view) in self.bufs.items():
            fill, n = self.FILLS[name], view.numel()
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), f"{what}: {name} guard overwritten"
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in
                   zip((self.cost, self.reach, self.crec, self.mrec), self.inputs)), f"{what}: an input was modified"
        if not self.with_dir:
            assert bool((self.view("dir") == 0xFF).all()), f"{what}: dir = NULL was written"

    def outputs(self):
        out = {k: self.view(k).cpu().numpy() for k in OUT if k != "dir" or self.with_dir}
        out["potential"] = out["potential"].view(np.uint32)
        return out

    def same_bytes(self, other):
        a, b = self.outputs(), other.outputs()
        return all(a[k].tobytes() == b[k].tobytes() for k in a if k in b)


def _assert_equal(out, name, what=None):
    ref = pr.expected(name)
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
def test_plan_against_reference(name):
    c = pr.CASES[pr.NAMES[name]]
    a = Run(c)
    a.check_guards(name)
    _assert_equal(a.outputs(), name)
    b = Run(c)  # determinism: a second run gives equal bytes
    assert a.same_bytes(b)
    n = Run(c, with_dir=not a.with_dir)  # dir = NULL (or not): the other outputs keep their bytes
    n.check_guards(name + " with dir the other way")
    _assert_equal(n.outputs(), name, name + " with dir the other way")
    assert a.same_bytes(n)


@pytest.mark.parametrize("order", (("snap-other-component", "frontier-none", "world-outside", "goal-r2-5", "start-not-traversable",
                                    "frontier-valid", "world-inside"),
                                   ("open-17x19", "scatter-17x19", "dir-null"), ("corridor-factor0", "detour-factor1024"),
                                   ("serpentine-33x31", "scatter-33x31"), ("rooms-127x129", "scatter-127x129"),
                                   ("rooms-160x160", "open-160x160")),
                         ids=("9x12", "17x19", "7x9", "33x31", "127x129", "160x160"))
def test_dirty_buffers_and_scratch_give_the_same_bytes(order):
    """A call into outputs and a scratch that still hold another case's results: its potential, its path, its record."""
    r = Run(pr.CASES[pr.NAMES[order[0]]], with_dir=True)
    for name in order + order[:1]:  # (the first case twice, and once more at the end)
        c = pr.CASES[pr.NAMES[name]]
        r.launch(c)
        r.check_guards(name)
        _assert_equal(r.outputs(), name, name + " into used buffers")


def test_rejected_arguments_write_nothing():
    from codd_amd import _abi, ops
    c = pr.CASES[pr.NAMES["world-inside"]]
    a = Run(c, with_dir=True)
    want = a.outputs()
    before = {k: buf.clone() for k, (buf, _) in a.bufs.items()}
    lib = _abi.load()
    ptr = {k: C.c_void_p(a.view(k).data_ptr()) for k in a.bufs}
    cost, reach, crec, mrec = (C.c_void_p(t.data_ptr()) for t in (a.cost, a.reach, a.crec, a.mrec))
    nan, inf = float("nan"), float("inf")

    def call(cost=cost, reach=reach, crec=crec, mrec=mrec, gh=9, gw=12, start_i=6, start_j=4, mode=1, goal_i=3, goal_j=4, goal_x=-1.13,
             goal_z=-0.62, cell=0.25, goal_r2=0, neutral=50, factor=205, unknown_cost=128, max_path=c["max_path"], scratch=ptr["scratch"],
             nbytes=80, pot=ptr["potential"], dirs=ptr["dir"], path=ptr["path"], rec=ptr["record"]):
        return lib.codd_plan(cost, reach, crec, mrec, gh, gw, start_i, start_j, mode, goal_i, goal_j, goal_x, goal_z, cell, goal_r2,
                             neutral, factor, unknown_cost, max_path, scratch, nbytes, pot, dirs, path, rec,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))

    for name in ("cost", "reach", "pot", "path", "rec", "scratch", "mrec"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(gh=0), dict(gw=0), dict(gh=160, gw=161), dict(start_i=-1), dict(start_i=12), dict(start_j=-1), dict(start_j=9),
                dict(mode=3), dict(mode=-1), dict(mode=0, goal_i=-1), dict(mode=0, goal_i=12), dict(mode=0, goal_j=-1), dict(mode=0, goal_j=9),
                dict(mode=2, crec=None), dict(goal_r2=-1), dict(max_path=0), dict(neutral=0), dict(neutral=256), dict(factor=-1),
                dict(factor=1025), dict(unknown_cost=-1), dict(unknown_cost=255), dict(cell=0.0), dict(cell=-1.0), dict(cell=nan),
                dict(cell=inf), dict(goal_x=nan), dict(goal_z=inf), dict(goal_x=0.25 * 2 ** 30), dict(goal_z=-0.25 * 2 ** 30),
                dict(nbytes=79)):
        assert call(**bad) == -1, bad
    with pytest.raises(_abi.CoddHipError):  # the same through ops: a scratch that is too small
        a.launch(c, scratch=a.view("scratch")[:-1])
    for bad in (dict(start=(12, 4)), dict(goal=("cell", 12, 0)), dict(goal="frontier", cost_record=None), dict(map_record=None),
                dict(neutral=0), dict(factor=1025), dict(unknown_cost=255), dict(goal_r2=-1), dict(cell=0.0), dict(path=a.view("path")[:0])):
        with pytest.raises(ValueError, match="plan"):
            a.launch(c, **bad)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k].view(torch.uint8), buf.view(torch.uint8)) for k, (buf, _) in a.bufs.items()), \
        "a rejected call wrote something"
    assert call() == 0  # (the defaults above are the case itself: the call the rejected ones were variations of)
    torch.cuda.synchronize()
    got = a.outputs()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    with pytest.raises(AssertionError):  # the outputs have the window's shape
        ops.plan(a.cost, a.reach, c["start"], a.view("potential")[:-1], a.view("path"), a.view("record"), goal=("cell", 0, 0))


# ---- the session against the entries called by hand -----------------------------------------------------------------------
LOCALMAP = dict(grid=(16, 24), cell=0.25, range_max=25.6, min_pixels=4, select=("obstacle", "overhead"), decay=1)
COSTMAP = dict(robot_radius=0.25, inflation_radius=1.0, scaling=2.0, start_radius=0.8, through_unknown=True)
PLAN = dict(goal_radius=0.3, neutral=40, factor=300, unknown_cost=60, max_path=48, dir=True)
NFRAMES = 3
WORLD_GOAL = (1.9, 2.6)


def _same_costmap(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("cost", "dist2", "reach")) and tuple(a[4:]) == tuple(b[4:])


def _same_plan(a, b):
    return (a.potential.tobytes() == b.potential.tobytes() and a.path.tobytes() == b.path.tobytes() and tuple(a[3:]) == tuple(b[3:])
            and (a.dir is None) == (b.dir is None) and (a.dir is None or a.dir.tobytes() == b.dir.tobytes()))


def test_session_plan_against_the_entries_by_hand(monkeypatch):
    import test_gpu_live_ground as glg
    import test_gpu_live_localmap as gll
    import test_gpu_live_objects as glo
    from codd_amd import live, ops
    calls, entry = [], ops.plan
    monkeypatch.setattr(ops, "plan", lambda *a, **k: (calls.append(1), entry(*a, **k))[1])  # (the sessions call ops.plan)
    plain = glm._plain_results()
    frames = glm._frames()[:NFRAMES]
    s = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP, costmap=COSTMAP, plan=PLAN)
    base = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP, costmap=COSTMAP)  # without plan=: the parent's tuple
    nodir = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP, costmap=COSTMAP, plan=dict(PLAN, dir=False, goal=WORLD_GOAL))
    gh, gw = LOCALMAP["grid"]
    start = (gw // 2, gh // 2)
    pot, dirs = torch.empty(gh, gw, dtype=torch.int32, device=DEV), torch.empty(gh, gw, dtype=torch.uint8, device=DEV)
    path, rec = torch.empty(PLAN["max_path"], dtype=torch.int32, device=DEV), torch.empty(16, dtype=torch.float64, device=DEV)
    goals = ["frontier", WORLD_GOAL, "frontier"]  # frame 1 is planned to a point of the map frame
    assert s._plan_par == dict(goal_r2=1, neutral=40, factor=300, unknown_cost=60)  # floor(1.2^2)
    for i, (left, right) in enumerate(frames):
        s.set_goal(goals[i])
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 6 and len(calls) == 1
        res, e, g, m, cm, pl = got
        got1 = base.step(left, right)
        assert len(got1) == 5 and len(calls) == 1, "a session without plan= called the entry"
        calls.clear()
        res1, e1, g1, m1, cm1 = got1
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i]), f"frame {i}: the depth result changed"
        assert glg._same_ground(g, g1), f"frame {i}: Ground changed with plan= on"
        assert (e is None) == (e1 is None) and (e is None or (e.pose.tobytes() == e1.pose.tobytes() and e.moving.tobytes() == e1.moving.tobytes()))
        assert gll._same_map(m, m1), f"frame {i}: LocalMap changed with plan= on"
        assert _same_costmap(cm, cm1), f"frame {i}: CostMap changed with plan= on"
        assert isinstance(pl, live.Plan) and pl.potential.shape == (gh, gw) and pl.potential.dtype == np.uint32 and pl.potential.flags["OWNDATA"]
        assert pl.origin == m.origin and pl.cell == 0.25 and pl.start == start
        # by hand, on this frame's CostMap arrays and records
        crec, mrec = np.zeros(16), np.zeros(16)
        crec[8] = -1 if cm.frontier_cell is None else cm.frontier_cell[0] * gw + cm.frontier_cell[1]
        mrec[8], mrec[9] = m.origin
        for goal, dr, have in ((goals[i], dirs, pl), (WORLD_GOAL, None, nodir.step(left, right)[-1])):
            ops.plan(torch.from_numpy(cm.cost).to(DEV), torch.from_numpy(cm.reach).to(DEV), start, pot, path, rec, dir=dr,
                     goal=goal if goal == "frontier" else ("world",) + goal, cost_record=torch.from_numpy(crec).to(DEV),
                     map_record=torch.from_numpy(mrec).to(DEV), cell=0.25, goal_r2=1, neutral=40, factor=300, unknown_cost=60)
            torch.cuda.synchronize()
            calls.clear()
            want = live.plan_from_buffers(rec.cpu().numpy(), pot.cpu().numpy(), None if dr is None else dr.cpu().numpy(),
                                          path.cpu().numpy(), m.origin, 0.25, start)
            assert _same_plan(have, want), f"frame {i}, goal {goal}: Plan differs from the entry by hand: {tuple(have[3:])} vs {tuple(want[3:])}"
        print(f"frame {i}: goal {goals[i]}: found {pl.found}, cost {pl.cost}, {pl.length_cells} cells, goal cell {pl.goal_cell}, "
              f"clamped {pl.clamped}, snapped {pl.snapped}, end {pl.end_cell}, {pl.reached} reached, lookahead {pl.lookahead(0.5)}")
        assert pl.reached == int((pl.potential != ops.PLAN_UNREACHED).sum()) == (cm.reachable if pl.goal_cell is not None else 0)
        assert ((pl.dir == 255) == (pl.potential == ops.PLAN_UNREACHED)).all() and len(pl.path) == min(pl.length_cells, PLAN["max_path"])
        if goals[i] == "frontier":
            assert pl.goal_cell == cm.frontier_cell and not pl.clamped
        if pl.found:
            assert tuple(pl.path[0]) == (start[1], start[0]) and pl.potential[tuple(pl.path[-1])] == 0 and pl.cost == pl.potential[start[1], start[0]]
    for t in (base, nodir, s):
        t.reset()
        t.close()
    assert s._d_plan is None and s._h_plan is None and s._plan_scratch is None and getattr(base, "_plan_goal", None) is None


def test_cli_live_plan(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 3
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    inference.main(["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
                    "--live", "--ground", "--ego", "--localmap", "--costmap", "--plan", "--plan-goal", "0.55,3.05", "--show-dir",
                    str(tmp_path / "out")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "plan:" in ln]
    assert len(lines) == 1 and f"of {n} frames" in lines[0]
    assert {"left.plan.pred.npz", "left.costmap.pred.npz", "left.localmap.pred.npz"} <= set(os.listdir(tmp_path / "out"))
    z = np.load(tmp_path / "out" / "left.plan.pred.npz")
    counts = ("found", "cost", "length_cells", "truncated", "clamped", "snapped", "reached", "max_cost_on_path")
    assert sorted(z.files) == sorted(counts + ("potential", "path", "goal_cell", "end_cell", "length", "start", "cell"))
    assert z["potential"].shape == (1, n, 128, 128) and z["potential"].dtype == np.uint32
    assert z["path"].shape == (1, n, 1024, 2) and z["path"].dtype == np.int32 and z["length"].shape == (1, n)
    assert all(z[k].shape == (1, n) and z[k].dtype == np.int32 for k in counts) and z["goal_cell"].shape == z["end_cell"].shape == (1, n, 2)
    assert tuple(z["start"]) == (64, 64) and float(z["cell"]) == 0.1
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, ground=True, egomotion=True, localmap=True, costmap=True, plan=dict(goal=(0.55, 3.05)))
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        pl = s.step(left, right)[-1]
        assert pl.potential.tobytes() == z["potential"][0, i].tobytes() and pl.length == z["length"][0, i]
        assert (z["path"][0, i, :len(pl.path)] == pl.path).all() and (z["path"][0, i, len(pl.path):] == -1).all()
        assert all(int(getattr(pl, k)) == z[k][0, i] for k in counts)
        assert (pl.goal_cell or (-1, -1)) == tuple(z["goal_cell"][0, i]) and (pl.end_cell or (-1, -1)) == tuple(z["end_cell"][0, i])
    s.reset()
    s.close()
