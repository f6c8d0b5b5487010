"""LiveSession local map on the GPU: codd_local_map against the restatement of tests/live_localmap_ref.py.

Launch 1 (the pose, fp64) is compared with the restatement within 1e-12 * max(1, |value|): fewer than 40 fp64 operations
stand behind every entry, so the margin over 40 * 2^-53 is above 200 x; the window origin and the flags are compared
exactly (every planted pose lies at least 1e-6 cells off a cell edge, or exactly on one by exact arithmetic).  Launches 2
to 4 are compared BIT FOR BIT with the restatement run from the state the device's launch 1 left: the storage, both
outputs, the tables O and F in the scratch and the record in full, with no excluded pixel and no tolerance (what each case
is built to show is asserted on the restatement in tests/test_live_localmap.py).  Then determinism, dirty buffers and
scratch with guard elements, rejected arguments, a three-frame session against the entry called by hand, and the command
line.  The crop of the cases is 37 x 70 in 64 x 128: five tile rows and three tile columns of 32 x 8 pixels, the last of each
partial; the grids are 16 x 24, 80 x 24, 1 x 1 and 5 x 3.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_localmap_ref as lm  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every buffer the entry writes
IDS = [lm.case_id(c) for c in lm.CASES]
PAR_KEYS = tuple(k for k in lm.DEFAULTS if k not in ("gh", "gw"))


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _par(c):
    return {k: c["par"][k] for k in PAR_KEYS}


class Run:
    """One call of ops.local_map on the case ``c``: everything the entry writes lies between guard elements, and the outputs
    and the scratch start out as garbage (0xFF bytes: NaN as a double, -1 as an integer)."""
    FILLS = dict(state=-7.0, logodds=-7, age=7, map_out=-7, age_out=7, record=-7.0, scratch=0xFF)

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
        self.bufs = {}
        for name, n, dt in (("state", 32, torch.float64), ("logodds", gh * gw, torch.int16), ("age", gh * gw, torch.uint8),
                            ("map_out", gh * gw, torch.int16), ("age_out", gh * gw, torch.uint8), ("record", 16, torch.float64),
                            ("scratch", ops.local_map_scratch(gh, gw), torch.uint8)):
            self.bufs[name] = _guarded(n, dt, self.FILLS[name])
        for name in ("map_out", "age_out", "scratch"):
            self.bufs[name][1].view(torch.uint8).fill_(0xFF)
        self.bufs["record"][1].fill_(float("nan"))
        self.launch(c)

    def view(self, name):
        gh, gw = self.shape[2:]
        v = self.bufs[name][1]
        return v.view(gh, gw) if name in ("logodds", "age", "map_out", "age_out") else v

    def launch(self, c, **over):
        """(again, with another case of the same shapes: into the outputs and the scratch as the last call left them)"""
        from codd_amd import ops
        assert (c["crop"] + (c["par"]["gh"], c["par"]["gw"])) == self.shape
        self.c = c
        self.disp.copy_(torch.from_numpy(c["disp"]))
        self.lab.copy_(torch.from_numpy(c["labels"]))
        self.rec.copy_(torch.from_numpy(c["rec"]))
        if c["ego"] is not None:
            self.ego.copy_(torch.from_numpy(c["ego"]))
        self.view("state").copy_(torch.from_numpy(c["state"]))
        self.view("logodds").copy_(torch.from_numpy(c["logodds"]))
        self.view("age").copy_(torch.from_numpy(c["age"]))
        self.inputs = tuple(t.clone() for t in (self.disp, self.lab, self.rec, self.ego))
        ops.local_map(self.disp, c["K"], c["calib"], c["crop"], self.lab, self.rec, None if c["ego"] is None else self.ego,
                      self.view("state"), self.view("logodds"), self.view("age"), self.view("map_out"), self.view("age_out"),
                      self.view("record"), fresh=c["fresh"], scratch=self.view("scratch"), **dict(_par(c), **over))
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        for name, (buf, view) in self.bufs.items():
            fill, n = self.FILLS[name], view.numel()
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), f"{what}: {name} guard overwritten"
        now = (glm._bits(self.disp), self.lab, self.rec.view(torch.int64), glm._bits(self.ego))
        was = (glm._bits(self.inputs[0]), self.inputs[1], self.inputs[2].view(torch.int64), glm._bits(self.inputs[3]))
        assert all(torch.equal(a, b) for a, b in zip(now, was)), f"{what}: an input was modified"

    def outputs(self):
        gh, gw = self.shape[2:]
        out = {k: self.view(k).cpu().numpy() for k in ("state", "logodds", "age", "map_out", "age_out", "record")}
        scr = self.view("scratch")
        off = (-scr.data_ptr()) % 16  # the entry aligns its tables itself
        tables = scr[off:off + 8 * gh * gw].cpu().numpy().view(np.int32)
        out["O"], out["F"] = tables[:gh * gw].reshape(gh, gw), tables[gh * gw:].reshape(gh, gw)
        return out

    def same_bytes(self, other):
        a, b = self.outputs(), other.outputs()
        return all(a[k].tobytes() == b[k].tobytes() for k in a)


def _assert_pose(state, c, name):
    """Launch 1 against the fp64 restatement."""
    want = lm.pose(c["state"], c["ego"], c["rec"], c["fresh"], c["par"])
    exact = (lm.EXISTS, lm.IX0, lm.IZ0, lm.FRAMES, lm.RESTARTS, lm.PIX0, lm.PIZ0, lm.CLEARED, lm.INTEGRATED, lm.LINKED)
    assert not np.isnan(state).any(), f"{name}: NaN in the state"
    for k in exact:
        assert state[k] == want[k], f"{name}: state[{k}] = {state[k]} (restatement {want[k]})"
    err = np.abs(state - want) / np.maximum(1.0, np.abs(want))
    print(f"{name}: pose ({state[lm.PX]:.6f}, {state[lm.PZ]:.6f}) heading ({state[lm.HX]:.6f}, {state[lm.HZ]:.6f}); largest "
          f"deviation from the restatement {err.max():.3e}")
    assert err.max() <= 1e-12, f"{name}: state differs from the fp64 restatement by {err.max():.3e} at {int(err.argmax())}"
    assert np.all(state[23:] == 0)


def _assert_equal(out, c, name):
    """Launches 2 to 4, from the state the device's launch 1 left: bytes, not values."""
    ref = lm.after_pose(c, out["state"], c["logodds"], c["age"], c["par"])
    print(f"{name}: record {out['record'].tolist()}")
    for k in ("O", "F", "logodds", "age", "map_out", "age_out"):
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (name, k)
        bad = np.argwhere(out[k] != ref[k])
        assert bad.size == 0, f"{name}: {k} differs at {bad[:8].tolist()}: {out[k][tuple(bad[0])]} vs {ref[k][tuple(bad[0])]}"
    assert out["record"].tobytes() == ref["record"].tobytes(), f"{name}: record {out['record'].tolist()} vs {ref['record'].tolist()}"


@pytest.mark.parametrize("name", IDS)
def test_local_map_against_reference(name):
    c = lm.CASES[lm.NAMES[name]]
    a = Run(c)
    a.check_guards(name)
    out = a.outputs()
    _assert_pose(out["state"], c, name)
    _assert_equal(out, c, name)
    b = Run(c)  # determinism: a second run gives equal bytes
    assert a.same_bytes(b)


@pytest.mark.parametrize("order", (("identity", "window-jump", "ground-lost", "fresh", "turn", "lost-and-no-floor", "saturate",
                                    "ego-null-hold", "negative-cells", "bad-disparity", "cell-edge"),
                                   ("5x3", "5x3-fresh", "5x3")), ids=("16x24", "5x3"))
def test_dirty_buffers_and_scratch_give_the_same_bytes(order):
    """A call into outputs and a scratch that still hold another case's results: its tables, its counters, its record."""
    r = Run(lm.CASES[lm.NAMES[order[0]]])
    for name in order[1:]:
        c = lm.CASES[lm.NAMES[name]]
        r.launch(c)
        r.check_guards(name)
        out = r.outputs()
        _assert_pose(out["state"], c, name + " into used buffers")
        _assert_equal(out, c, name + " into used buffers")
        assert Run(c).same_bytes(r), f"{name}: used buffers changed a byte"


def test_frames_carried_on_the_device():
    """Four frames with the state, the storage and the outputs left on the device between the calls, against the
    restatement carried the same way from the device's state after each launch 1: a walk forward, a turn, a frame without a
    floor, a step back."""
    names = ("fresh", "forward", "turn", "ground-lost", "negative-cells")
    c0 = lm.CASES[lm.NAMES[names[0]]]
    r = Run(c0)
    L, age = r.outputs()["logodds"], r.outputs()["age"]
    for name in names[1:]:
        base = lm.CASES[lm.NAMES[name]]
        before = r.outputs()
        c = dict(base, state=before["state"], logodds=before["logodds"], age=before["age"], par=dict(c0["par"], decay=1))
        r.launch(c)
        r.check_guards(name)
        out = r.outputs()
        _assert_pose(out["state"], c, "carried " + name)
        _assert_equal(out, c, "carried " + name)
        assert out["logodds"].tobytes() != L.tobytes() or out["age"].tobytes() != age.tobytes()
        L, age = out["logodds"], out["age"]


def test_ops_reject_bad_arguments():
    from codd_amd import _abi, ops
    c = lm.CASES[lm.NAMES["identity"]]
    for bad in ((0, 4), (4, 0), (4097, 1), (1, 4097), (4096, 2048)):
        with pytest.raises(ValueError):
            ops.local_map_scratch(*bad)
    assert ops.local_map_scratch(2048, 2048) > 0
    a = Run(c)
    want = a.outputs()
    st, L, ag, mo, ao, rec, scr = (a.view(k) for k in ("state", "logodds", "age", "map_out", "age_out", "record", "scratch"))
    args = (a.disp, c["K"], c["calib"], c["crop"], a.lab, a.rec, a.ego, st, L, ag, mo, ao, rec)
    with pytest.raises(TypeError):
        ops.local_map(*args, scratch=scr, speed=3)
    before = {k: buf.clone() for k, (buf, _) in a.bufs.items()}
    par = _par(c)
    for bad in (dict(select=1), dict(select=3), dict(min_pixels=0), dict(cell=0.0), dict(cell=float("nan")), dict(cell=float("inf")),
                dict(range_max=0.0), dict(range_max=float("inf")), dict(range_max=float("nan")), dict(range_min=-1.0),
                dict(range_min=float("nan")), dict(range_min=par["range_max"]), dict(l_occ=-1), dict(l_free=-1), dict(l_min=1),
                dict(l_min=-32769), dict(l_max=-1), dict(l_max=32768), dict(decay=-1), dict(lost=2), dict(lost=-1)):
        with pytest.raises(_abi.CoddHipError):
            ops.local_map(*args, scratch=scr, **dict(par, **bad))
    for K, calib in (((0.0,) + tuple(c["K"][1:]), c["calib"]), (c["K"][:2] + (float("nan"),) + c["K"][3:], c["calib"]),
                     (c["K"], float("inf"))):
        with pytest.raises(_abi.CoddHipError):
            ops.local_map(a.disp, K, calib, *args[3:], scratch=scr, **par)
    with pytest.raises(_abi.CoddHipError):  # scratch too small
        ops.local_map(*args, scratch=scr[:-1], **par)
    with pytest.raises(_abi.CoddHipError):  # the crop does not fit the padded map
        ops.local_map(a.disp, c["K"], c["calib"], (c["padded"][0] + 1, c["crop"][1]),
                      torch.zeros(c["padded"][0] + 1, c["crop"][1], dtype=torch.uint8, device=DEV), *args[5:], scratch=scr, **par)
    with pytest.raises(_abi.CoddHipError):  # w > W
        ops.local_map(a.disp, c["K"], c["calib"], (c["crop"][0], c["padded"][1] + 1),
                      torch.zeros(c["crop"][0], c["padded"][1] + 1, dtype=torch.uint8, device=DEV), *args[5:], scratch=scr, **par)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k].view(torch.uint8), buf.view(torch.uint8)) for k, (buf, _) in a.bufs.items()), \
        "a rejected call wrote something"
    with pytest.raises(AssertionError):  # the outputs have the storage's shape
        ops.local_map(*args[:10], mo[:-1], *args[11:], scratch=scr, **par)
    got = a.outputs()
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


# ---- the session against the entry called by hand -------------------------------------------------------------------------
LOCALMAP = dict(grid=(16, 24), cell=0.25, range_max=25.6, min_pixels=4, select=("obstacle", "overhead"), decay=1)
NFRAMES = 3


def _same_map(a, b):
    return (a.logodds.dtype == b.logodds.dtype and a.logodds.tobytes() == b.logodds.tobytes() and a.age.tobytes() == b.age.tobytes()
            and tuple(a[2:]) == tuple(b[2:]))


def test_session_localmap_against_the_entry_by_hand():
    import test_gpu_live_ground as glg
    import test_gpu_live_objects as glo
    from codd_amd import live, ops
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()[:NFRAMES]
    s = glm._session(ground=glo.GROUND, egomotion=True, localmap=LOCALMAP)
    base = glm._session(ground=glo.GROUND, egomotion=True)  # without localmap=: the parent's tuple and bytes
    held = glm._session(ground=glo.GROUND, egomotion=True, localmap=dict(LOCALMAP, lost="hold"))
    p = live._check_localmap(LOCALMAP)
    gh, gw = p["grid"]
    par = dict({k: p[k] for k in ops.MAP_PARAMS if k not in ("select", "lost")}, select=live.select_mask(p["select"]),
               lost=ops.MAP_RESET)
    state = torch.zeros(32, dtype=torch.float64, device=DEV)
    L, age = torch.zeros(gh, gw, dtype=torch.int16, device=DEV), torch.zeros(gh, gw, dtype=torch.uint8, device=DEV)
    mo, ao = torch.empty(gh, gw, dtype=torch.int16, device=DEV), torch.empty(gh, gw, dtype=torch.uint8, device=DEV)
    rec = torch.empty(16, dtype=torch.float64, device=DEV)
    first = []
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 4
        res, e, g, m = got
        res1, e1, g1 = base.step(left, right)
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i]), f"frame {i}: the depth result changed"
        assert glg._same_ground(g, g1), f"frame {i}: Ground changed with localmap= on"
        assert (e is None) == (e1 is None) and (e is None or (e.pose.tobytes() == e1.pose.tobytes() and e.moving.tobytes() == e1.moving.tobytes()))
        assert isinstance(m, live.LocalMap) and m.logodds.shape == (gh, gw) and m.logodds.dtype == np.int16 and m.age.dtype == np.uint8
        assert m.logodds.flags["OWNDATA"] and m.cell == 0.25 and (not m.linked or (i > 0 and e is not None and e.ok))
        assert (i > 0 or (m.restarts == 1 and m.frames == 0)) and m.integrated == bool(g.ok)
        # by hand, on the session's own device records and labels, with the state carried here
        ops.local_map(parent[i][0], glm.INTRINSICS, glm.CALIB, (glm.H0, glm.W0), s._d_ground[1], s._d_ground[0],
                      s._d_ego[0] if e is not None else None, state, L, age, mo, ao, rec, fresh=i == 0, **par)
        torch.cuda.synchronize()
        want = live.localmap_from_buffers(rec.cpu().numpy(), mo.cpu().numpy(), ao.cpu().numpy(), p["cell"], p["occ_level"], p["free_level"])
        print(f"frame {i}: floor {g.ok}; integrated {m.integrated}, linked {m.linked}, restarts {m.restarts}, frames {m.frames}, pose "
              f"{m.pose}, origin {m.origin}, step {m.step}; {m.pixels} pixels, {m.occupied} occupied, {m.free} free, {m.unknown} unknown")
        assert _same_map(m, want), f"frame {i}: LocalMap differs from the entry called by hand"
        st = m.state()
        assert st.dtype == np.uint8 and int((st == live.MAP_OCCUPIED).sum()) == m.occupied
        assert int((st == live.MAP_FREE).sum()) == m.free and int((m.age == 255).sum()) == m.unknown
        x, z = m.world_xz(0, 0)
        assert x == (m.origin[0] + 0.5) * 0.25 and z == (m.origin[1] + 0.5) * 0.25
        m2 = held.step(left, right)[-1]
        if m.linked or i == 0:  # nothing was lost: the policy changes no byte
            assert _same_map(m2, m), f"frame {i}: lost='hold' changed a frame that was not lost"
        first.append(m)
    kept = [(m.logodds.copy(), m.age.copy(), tuple(m[2:])) for m in first]
    for m in first:  # the results are the caller's: scribbling on them changes no later frame
        m.logodds[...] = -1
    for t in (base, held):
        t.reset()
        t.close()
    s.reset()
    second = []
    for left, right in frames:  # a new sequence, pipelined: push, push, pop, pop -- reset() starts a new map
        s.push(left.copy(), right.copy())
        if s.pending() == 2:
            second.append(s.pop())
    while s.pending():
        second.append(s.pop())
    assert len(second) == NFRAMES
    for i in range(NFRAMES):
        m = second[i][-1]
        assert np.array_equal(second[i][0], plain[i]), f"pipelined frame {i}: the result differs"
        assert m.logodds.tobytes() == kept[i][0].tobytes() and m.age.tobytes() == kept[i][1].tobytes(), f"pipelined frame {i}"
        # (the state is the session's, not the sequence's: the restarts go on counting)
        assert tuple(m[2:])[:5] == kept[i][2][:5] and tuple(m[2:])[6:] == kept[i][2][6:]
        assert m.restarts - second[0][-1].restarts == kept[i][2][5] - kept[0][2][5] and second[0][-1].restarts > kept[0][2][5]
    s.reset()
    s.close()
    assert s._d_map is None and s._h_map is None and s._map_state is None and s._map_scratch is None


def test_cli_live_localmap(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 3
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    inference.main(["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
                    "--live", "--ground", "--ego", "--localmap", "--show-dir", str(tmp_path / "out")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "localmap:" in ln]
    assert len(lines) == 1 and f"in {n} frames" in lines[0] and "128 x 128 cells" in lines[0]
    assert "left.localmap.pred.npz" in os.listdir(tmp_path / "out")
    z = np.load(tmp_path / "out" / "left.localmap.pred.npz")
    assert sorted(z.files) == ["age", "cell", "free", "free_level", "integrated", "linked", "logodds", "occ_level", "occupied", "origin",
                               "pose", "restarts", "unknown"]
    assert z["logodds"].shape == z["age"].shape == (1, n, 128, 128) and z["logodds"].dtype == np.int16 and z["age"].dtype == np.uint8
    assert z["pose"].shape == (1, n, 4) and z["origin"].shape == (1, n, 2) and float(z["cell"]) == 0.1
    assert all(z[k].shape == (1, n) and z[k].dtype == np.int32 for k in ("integrated", "linked", "restarts", "occupied", "free", "unknown"))
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, ground=True, egomotion=True, localmap=True)
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        m = s.step(left, right)[-1]
        assert m.logodds.tobytes() == z["logodds"][0, i].tobytes() and m.age.tobytes() == z["age"][0, i].tobytes()
        assert m.pose[:2] + m.pose[2] == tuple(z["pose"][0, i]) and m.origin == tuple(z["origin"][0, i])
        assert (m.occupied, m.free, m.unknown) == (z["occupied"][0, i], z["free"][0, i], z["unknown"][0, i])
    s.reset()
    s.close()
