"""LiveSession elevation layer on the GPU: codd_height_map against the restatement of tests/live_heightmap_ref.py.

Every case runs codd_local_map first, as the entry's precondition asks, and then codd_height_map on the state that call left
on the device.  The four persistent layers, the six outputs, the five tables in the scratch and the record are compared BIT
FOR BIT with the restatement run from the device's own state, with no excluded cell and no tolerance (what the rule is meant
to do is asserted on the restatement in tests/test_live_heightmap.py).  Then determinism, a scratch and outputs of 0xFF
bytes or of another case's results, guard elements around everything written, untouched inputs and state, four frames
carried on the device, rejected arguments, a three-frame session against the entry called by hand, and the command line.  The crop of the
cases is 37 x 70 in 64 x 128: five tile rows and three tile columns of 32 x 8 pixels, the last of each partial; the grids are
16 x 24, 80 x 24, 1 x 1 and 5 x 3.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_heightmap_ref as hm  # noqa: E402
import live_localmap_ref as lm  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every buffer the entry writes
IDS = [hm.case_id(c) for c in hm.CASES]
MAP_KEYS = tuple(k for k in lm.DEFAULTS if k not in ("gh", "gw"))
I16, U8, U16 = torch.int16, torch.uint8, torch.uint16
DTYPES = dict(top=I16, bot=I16, ceil=I16, hage=U8, top_out=I16, bot_out=I16, ceil_out=I16, hage_out=U8, step_out=U16, flags_out=U8)


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _call(r, c, scratch=None, **over):
    """ops.height_map on the buffers of the Run ``r`` with the parameters of the case ``c``: the thresholds go through the
    host's quantisation, as units of h_res times h_res."""
    from codd_amd import ops
    hp = dict(c["hpar"], **over)
    res = float(hp["h_res"])
    par = dict(h_res=res, select=hp["select"], min_pixels=hp["min_pixels"], alpha=hp["alpha"], max_step=hp["max_step_q"] * res,
               robot_height=hp["robot_height_q"] * res, max_drop=hp["max_drop_q"] * res)
    if all(k in hp and 0 <= hp[k] <= hm.Q_MAX for k in ("max_step_q", "robot_height_q", "max_drop_q")) and np.isfinite(res) and res > 0:
        assert ops.height_thresholds(res, par["max_step"], par["robot_height"], par["max_drop"]) == (
            hp["max_step_q"], hp["robot_height_q"], hp["max_drop_q"])
    return ops.height_map(r.disp, c["K"], c["calib"], c["crop"], r.lab, r.rec, r.state, *(r.view(k) for k in hm.LAYERS),
                          *(r.view(k) for k in hm.OUTPUTS), r.view("record"), cell=c["par"]["cell"], range_min=c["par"]["range_min"],
                          range_max=c["par"]["range_max"], scratch=r.view("scratch") if scratch is None else scratch, **par)


class Run:
    """codd_local_map, then one call of ops.height_map on the case ``c``: everything the entry writes lies between guard
    elements, and the outputs and the scratch start out as garbage (0xFF bytes: NaN as a double, -1 as an integer)."""
    FILL = 7

    def __init__(self, c):
        from codd_amd import ops
        h, w = c["crop"]
        H, W = c["padded"]
        gh, gw = c["par"]["gh"], c["par"]["gw"]
        self.shape = (h, w, gh, gw)
        self.disp = torch.zeros(H, W, device=DEV)
        self.lab = torch.zeros(h, w, dtype=torch.uint8, device=DEV)
        self.rec = torch.zeros(32, dtype=torch.float64, device=DEV)
        self.ego = torch.zeros(16, device=DEV)
        self.state = torch.zeros(32, dtype=torch.float64, device=DEV)
        self.map = [torch.zeros(gh, gw, dtype=I16, device=DEV), torch.zeros(gh, gw, dtype=U8, device=DEV),
                    torch.zeros(gh, gw, dtype=I16, device=DEV), torch.zeros(gh, gw, dtype=U8, device=DEV),
                    torch.zeros(16, dtype=torch.float64, device=DEV)]  # logodds, age, map_out, age_out, record
        self.bufs = {k: _guarded(gh * gw, dt, self.FILL) for k, dt in DTYPES.items()}
        self.bufs["record"] = _guarded(16, torch.float64, float(self.FILL))
        self.bufs["scratch"] = _guarded(ops.height_map_scratch(gh, gw), U8, self.FILL)
        for name in hm.OUTPUTS + ("scratch", "record"):
            self.bufs[name][1].view(U8).fill_(0xFF)
        self.launch(c)

    def view(self, name):
        gh, gw = self.shape[2:]
        v = self.bufs[name][1]
        return v.view(gh, gw) if name in DTYPES else v

    def launch(self, c, layers=None, state=None):
        """(again, with another case of the same shapes: into the outputs and the scratch as the last call left them)"""
        from codd_amd import ops
        assert (c["crop"] + (c["par"]["gh"], c["par"]["gw"])) == self.shape
        self.c = c
        self.disp.copy_(torch.from_numpy(c["disp"]))
        self.lab.copy_(torch.from_numpy(c["labels"]))
        self.rec.copy_(torch.from_numpy(c["rec"]))
        if c["ego"] is not None:
            self.ego.copy_(torch.from_numpy(c["ego"]))
        if state is None:  # the case's planted state and map; otherwise what the last call left on the device
            self.state.copy_(torch.from_numpy(c["state"]))
            self.map[0].copy_(torch.from_numpy(c["logodds"]))
            self.map[1].copy_(torch.from_numpy(c["age"]))
        self.planted = {k: np.array(c["layers"][k]) for k in hm.LAYERS} if layers is None else layers
        if layers is None:
            for k in hm.LAYERS:
                self.view(k).copy_(torch.from_numpy(self.planted[k]))
        ops.local_map(self.disp, c["K"], c["calib"], c["crop"], self.lab, self.rec, None if c["ego"] is None else self.ego,
                      self.state, *self.map, fresh=c["fresh"], **{k: c["par"][k] for k in MAP_KEYS})
        self.inputs = tuple(t.clone() for t in (self.disp, self.lab, self.rec, self.state))
        _call(self, c)
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        for name, (buf, view) in self.bufs.items():
            n = view.numel()
            assert bool((buf[:GUARD] == self.FILL).all()) and bool((buf[GUARD + n:] == self.FILL).all()), f"{what}: {name} guard overwritten"
        now = (glm._bits(self.disp), self.lab, self.rec.view(torch.int64), self.state.view(torch.int64))
        was = (glm._bits(self.inputs[0]), self.inputs[1], self.inputs[2].view(torch.int64), self.inputs[3].view(torch.int64))
        assert all(torch.equal(a, b) for a, b in zip(now, was)), f"{what}: an input or the state was modified"

    def outputs(self):
        gh, gw = self.shape[2:]
        out = {k: self.view(k).cpu().numpy() for k in tuple(DTYPES) + ("record",)}
        out["state"] = self.state.cpu().numpy()
        scr = self.view("scratch")
        off = (-scr.data_ptr()) % 16  # the entry aligns its tables itself
        tables = scr[off:off + 20 * gh * gw].cpu().numpy().view(np.int32).reshape(5, gh, gw)
        out.update({k: tables[i] for i, k in enumerate(hm.TABLES)})
        return out

    def same_bytes(self, other):
        a, b = self.outputs(), other.outputs()
        return all(a[k].tobytes() == b[k].tobytes() for k in a)


def _assert_equal(out, c, layers, name):
    """All four launches, from the state the device's codd_local_map left: bytes, not values."""
    ref = hm.after_map(c, out["state"], layers, c["par"], c["hpar"])
    print(f"{name}: record {out['record'].tolist()}")
    for k in hm.TABLES + hm.LAYERS + hm.OUTPUTS:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (name, k, out[k].dtype, ref[k].dtype)
        bad = np.argwhere(out[k] != ref[k])
        assert bad.size == 0, f"{name}: {k} differs at {bad[:8].tolist()}: {out[k][tuple(bad[0])]} vs {ref[k][tuple(bad[0])]}"
    assert not np.isnan(out["record"]).any()
    assert out["record"].tobytes() == ref["record"].tobytes(), f"{name}: record {out['record'].tolist()} vs {ref['record'].tolist()}"
    return ref


@pytest.mark.parametrize("name", IDS)
def test_height_map_against_reference(name):
    c = hm.CASES[hm.NAMES[name]]
    a = Run(c)
    a.check_guards(name)
    out = a.outputs()
    _assert_equal(out, c, a.planted, name)
    assert (out["bot"].astype(np.int64) <= out["top"]).all()
    b = Run(c)  # determinism: a second run gives equal bytes
    assert a.same_bytes(b)


def test_first_call_needs_no_initialised_layers():
    """The header's promise: the first codd_local_map call on a zeroed state is CLEARED, so layers of any content -- zeros, which
    are not a valid start, or 0xFF bytes -- give the bytes of layers that held the sentinels."""
    base = hm.CASES[hm.NAMES["first-from-zeros"]]
    gh, gw = base["par"]["gh"], base["par"]["gw"]
    runs = []
    for top, ceil, hage in ((hm.NONE, hm.NO_CEIL, 255), (0, 0, 0), (-1, -1, 255)):  # the sentinels, zeros, 0xFF bytes
        lay = dict(top=np.full((gh, gw), top, np.int16), bot=np.full((gh, gw), top, np.int16),
                   ceil=np.full((gh, gw), ceil, np.int16), hage=np.full((gh, gw), hage, np.uint8))
        r = Run(dict(base, layers=lay))
        assert r.outputs()["state"][lm.CLEARED] == 1
        runs.append(r)
    assert runs[0].same_bytes(runs[1]) and runs[0].same_bytes(runs[2])
    assert (runs[0].outputs()["top"] != hm.NONE).any()


@pytest.mark.parametrize("order", (("identity", "window-jump", "ground-lost", "fresh", "turn", "lost-and-no-floor", "overhead-only",
                                    "non-finite-height", "negative-cells", "bad-disparity", "cell-edge", "no-surface-label"),
                                   ("5x3", "5x3-fresh", "5x3")), ids=("16x24", "5x3"))
def test_dirty_buffers_and_scratch_give_the_same_bytes(order):
    """A call into outputs and a scratch that still hold another case's results: its tables, its counters, its record."""
    r = Run(hm.CASES[hm.NAMES[order[0]]])
    for name in order[1:]:
        c = hm.CASES[hm.NAMES[name]]
        r.launch(c)
        r.check_guards(name)
        _assert_equal(r.outputs(), c, r.planted, name + " into used buffers")
        assert Run(c).same_bytes(r), f"{name}: used buffers changed a byte"


def test_frames_carried_on_the_device():
    """Four frames with the state, both maps' storage and the outputs left on the device between the calls, against the
    restatement carried the same way: a walk forward, a turn, a frame without a floor, a step back."""
    names = ("fresh", "forward", "turn", "ground-lost", "negative-cells")
    c0 = hm.CASES[hm.NAMES[names[0]]]
    r = Run(c0)
    seen = {r.outputs()["top"].tobytes()}
    for name in names[1:]:
        before = r.outputs()
        layers = {k: before[k] for k in hm.LAYERS}
        c = dict(hm.CASES[hm.NAMES[name]], par=c0["par"], hpar=c0["hpar"])
        r.launch(c, layers=layers, state="carried")
        r.check_guards(name)
        out = r.outputs()
        _assert_equal(out, c, layers, "carried " + name)
        if name == "ground-lost":  # nothing integrated: the values stay, every observed cell ages
            assert out["record"][0] == 0 and out["record"][3] == 0
        seen.add(out["top"].tobytes())
    assert len(seen) > 2


def test_ops_reject_bad_arguments():
    from codd_amd import _abi, ops
    c = hm.CASES[hm.NAMES["identity"]]
    for bad in ((0, 4), (4, 0), (4097, 1), (1, 4097), (4096, 2048)):
        with pytest.raises(ValueError):
            ops.height_map_scratch(*bad)
    assert ops.height_map_scratch(2048, 2048) == 16 + 20 * 2 ** 22 + 64
    a = Run(c)
    want = a.outputs()
    before = {k: buf.clone() for k, (buf, _) in a.bufs.items()}
    state = a.state.clone()
    with pytest.raises(TypeError):
        ops.height_map(a.disp, c["K"], c["calib"], c["crop"], a.lab, a.rec, a.state, *(a.view(k) for k in hm.LAYERS),
                       *(a.view(k) for k in hm.OUTPUTS), a.view("record"), speed=3)
    for bad in (dict(select=1 << hm.OVERHEAD), dict(select=hm.SURFACES | (1 << hm.OVERHEAD)), dict(min_pixels=0), dict(alpha=0),
                dict(alpha=257), dict(alpha=-1)):
        with pytest.raises(_abi.CoddHipError):
            _call(a, c, **bad)
    for bad in (dict(h_res=0.0), dict(h_res=float("nan")), dict(h_res=float("inf")), dict(h_res=-0.005), dict(max_step_q=-1),
                dict(max_step_q=hm.Q_MAX + 1), dict(robot_height_q=hm.Q_MAX + 1), dict(max_drop_q=-1), dict(select=2 ** 32),
                dict(select=-1)):
        with pytest.raises(ValueError):
            _call(a, c, **bad)
    with pytest.raises(_abi.CoddHipError):  # scratch too small
        _call(a, c, scratch=a.view("scratch")[:-1])
    for cell, rmin, rmax in ((0.0, 0.0, 12.8), (float("nan"), 0.0, 12.8), (0.5, -1.0, 12.8), (0.5, 12.8, 12.8), (0.5, 0.0, float("inf"))):
        with pytest.raises(_abi.CoddHipError):
            _call(a, dict(c, par=dict(c["par"], cell=cell, range_min=rmin, range_max=rmax)))
    for K, calib in (((0.0,) + tuple(c["K"][1:]), c["calib"]), (c["K"][:2] + (float("nan"),) + c["K"][3:], c["calib"]),
                     (c["K"], float("inf"))):
        with pytest.raises(_abi.CoddHipError):
            _call(a, dict(c, K=K, calib=calib))
    torch.cuda.synchronize()
    assert all(torch.equal(before[k].view(U8), buf.view(U8)) for k, (buf, _) in a.bufs.items()), "a rejected call wrote something"
    assert torch.equal(state.view(torch.int64), a.state.view(torch.int64))
    got = a.outputs()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


# ---- the session against the entry called by hand -------------------------------------------------------------------------
LOCALMAP = dict(grid=(16, 24), cell=0.25, range_max=25.6, min_pixels=4, select=("obstacle", "overhead"), decay=1)
HEIGHTMAP = dict(h_res=0.01, min_pixels=2, alpha=96, max_step=0.2, robot_height=1.5, max_drop=0.15)
NFRAMES = 3
PLANES = ("top_q", "bot_q", "ceil_q", "age", "step", "flags")


def _same_height(a, b):
    return (all(getattr(a, k).dtype == getattr(b, k).dtype and getattr(a, k).tobytes() == getattr(b, k).tobytes()
                for k in PLANES + ("top", "bot", "ceil")) and tuple(a[9:]) == tuple(b[9:]))


def test_session_heightmap_against_the_entry_by_hand():
    import test_gpu_live_ground as glg
    import test_gpu_live_localmap as gll
    import test_gpu_live_objects as glo
    from codd_amd import live, ops
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()[:NFRAMES]
    s = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP, heightmap=HEIGHTMAP)
    base = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP)  # without heightmap=: the parent's tuple and bytes
    p, hp = live._check_localmap(LOCALMAP), live._check_heightmap(HEIGHTMAP)
    gh, gw = p["grid"]
    par = dict({k: hp[k] for k in ops.HEIGHT_PARAMS if k != "select"}, select=live.select_mask(hp["select"]), cell=p["cell"],
               range_min=p["range_min"], range_max=p["range_max"])
    lay = [torch.zeros(gh, gw, dtype=dt, device=DEV) for dt in (I16, I16, I16, U8)]
    outs = [torch.empty(gh, gw, dtype=dt, device=DEV) for dt in (I16, I16, I16, U8, U16, U8)]
    rec = torch.empty(16, dtype=torch.float64, device=DEV)
    first = []
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 5
        res, e, g, m, hgt = got
        got1 = base.step(left, right)
        assert isinstance(got1, tuple) and len(got1) == 4
        res1, e1, g1, m1 = got1
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i]), f"frame {i}: the depth result changed"
        assert glg._same_ground(g, g1), f"frame {i}: Ground changed with heightmap= on"
        assert gll._same_map(m, m1), f"frame {i}: LocalMap changed with heightmap= on"
        assert (e is None) == (e1 is None) and (e is None or (e.pose.tobytes() == e1.pose.tobytes() and e.moving.tobytes() == e1.moving.tobytes()))
        assert isinstance(hgt, live.HeightMap) and hgt.top_q.shape == (gh, gw) and hgt.top.dtype == np.float32 and hgt.step.dtype == np.uint16
        assert hgt.top_q.flags["OWNDATA"] and hgt.cell == 0.25 and hgt.h_res == 0.01 and hgt.origin == m.origin
        assert hgt.integrated == m.integrated
        # by hand, on the session's own device records, labels and map state (this frame's: the session was stepped)
        ops.height_map(parent[i][0], glm.INTRINSICS, glm.CALIB, (glm.H0, glm.W0), s._d_ground[1], s._d_ground[0], s._map_state[0],
                       *lay, *outs, rec, **par)
        torch.cuda.synchronize()
        want = live.heightmap_from_buffers(rec.cpu().numpy(), *(t.cpu().numpy() for t in outs), p["cell"], hp["h_res"])
        print(f"frame {i}: floor {g.ok}; integrated {hgt.integrated}, {hgt.surface_pixels} surface and {hgt.overhead_pixels} overhead "
              f"pixels, {hgt.observed} observed, {hgt.known} known, {hgt.steps} steps, {hgt.headroom} headroom, {hgt.holes} holes, top "
              f"up to {hgt.top_max:.3f}, bot down to {hgt.bot_min:.3f}")
        assert _same_height(hgt, want), f"frame {i}: HeightMap differs from the entry called by hand"
        assert int((hgt.flags != 255).sum()) == hgt.known and int((hgt.age == 0).sum()) == hgt.observed
        assert np.array_equal(hgt.traversable(), hgt.flags == 0) and np.array_equal(np.isnan(hgt.top), hgt.top_q == ops.HEIGHT_NONE)
        first.append(hgt)
    assert any(hgt.known for hgt in first), "no frame put a surface into the layer"
    kept = [tuple(getattr(hgt, k).copy() for k in PLANES) + (tuple(hgt[9:]),) for hgt in first]
    for hgt in first:  # the results are the caller's: scribbling on them changes no later frame
        hgt.top_q[...] = -1
    base.reset()
    base.close()
    s.reset()
    second = []
    for left, right in frames:  # a new sequence, pipelined: push, push, pop, pop -- reset() restarts the layers with the map
        s.push(left.copy(), right.copy())
        if s.pending() == 2:
            second.append(s.pop())
    while s.pending():
        second.append(s.pop())
    assert len(second) == NFRAMES
    for i in range(NFRAMES):
        hgt = second[i][-1]
        assert np.array_equal(second[i][0], plain[i]), f"pipelined frame {i}: the result differs"
        assert all(getattr(hgt, k).tobytes() == kept[i][j].tobytes() for j, k in enumerate(PLANES)), f"pipelined frame {i}"
        assert tuple(hgt[9:]) == kept[i][-1], f"pipelined frame {i}"
    s.reset()
    s.close()
    assert s._d_height is None and s._h_height is None and s._height_state is None and s._height_scratch is None


def test_cli_live_heightmap(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 3
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    inference.main(["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
                    "--live", "--ground", "--ego", "--localmap", "--heightmap", "--show-dir", str(tmp_path / "out")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "heightmap:" in ln]
    assert len(lines) == 1 and f"in {n} frames" in lines[0]
    assert {"left.heightmap.pred.npz", "left.localmap.pred.npz"} <= set(os.listdir(tmp_path / "out"))
    z = np.load(tmp_path / "out" / "left.heightmap.pred.npz")
    counts = ("integrated", "surface_pixels", "overhead_pixels", "observed", "known", "steps", "headroom", "holes")
    assert sorted(z.files) == sorted(("top", "bot", "ceil", "age", "step", "flags", "origin", "cell", "h_res") + counts)
    assert all(z[k].shape == (1, n, 128, 128) and z[k].dtype == np.int16 for k in ("top", "bot", "ceil"))
    assert z["age"].dtype == z["flags"].dtype == np.uint8 and z["step"].dtype == np.uint16 and z["step"].shape == (1, n, 128, 128)
    assert z["origin"].shape == (1, n, 2) and float(z["cell"]) == 0.1 and float(z["h_res"]) == 0.005
    assert all(z[k].shape == (1, n) and z[k].dtype == np.int32 for k in counts)
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, ground=True, egomotion=True, localmap=True, heightmap=True)
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        m = s.step(left, right)[-1]
        assert all(getattr(m, k + "_q").tobytes() == z[k][0, i].tobytes() for k in ("top", "bot", "ceil"))
        assert m.flags.tobytes() == z["flags"][0, i].tobytes() and m.step.tobytes() == z["step"][0, i].tobytes()
        assert m.origin == tuple(z["origin"][0, i]) and (m.known, m.steps, m.holes) == (z["known"][0, i], z["steps"][0, i], z["holes"][0, i])
    s.reset()
    s.close()
