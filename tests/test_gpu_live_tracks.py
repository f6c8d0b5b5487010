"""LiveSession object tracks on the GPU: codd_track_objects against the restatement of tests/live_tracks_ref.py, bit for bit
on trk_count, both tables in full (zero rows included) and the rolled state, frame after frame, with no excluded pixel and
no tolerance (what the cases are built to show is asserted on the restatement in tests/test_live_tracks.py); guard
regions around every output, the state and the scratch, dirty buffers, unaligned pointers, determinism, untouched
inputs, the CODD_EINVAL list; LiveSession(ground=..., objects=..., egomotion=True, tracks=True) against the entry called
by hand on the session's own device buffers, stepwise and pipelined; and the --live --ground --objects --tracks command
line.  The id maps and fields of the cases are synthetic: no ground or objects launch is needed.  The crop of the cases
is 70 x 150 in 128 x 192: 10500 pixels are 11 workgroups of 16 waves in the per-pixel launch, the last partial, and a row
of 150 pixels puts object borders inside waves and several objects into one workgroup.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_tracks_ref as lt  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every output
_CACHE = {}
IDS = [c["name"] for c in lt.CASES]


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _case(name):
    """(inputs, the reference of every frame), computed once and never modified."""
    if name not in _CACHE:
        c = lt.CASES[lt.NAMES[name]]
        _CACHE[name] = (c, lt.reference(c))
    return _CACHE[name]


def _guarded(n, dtype, fill, off):
    buf = torch.full((n + 2 * GUARD + 4,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD + off:GUARD + off + n]


class Run:
    """The buffers of one sequence of ops.track_objects calls at the shapes of the case ``c``: every output, the state and
    the scratch between guard regions; ``off`` shifts every fp32 / int32 / uint16 pointer by that many elements off a
    16-byte boundary and the byte buffers (moving, state, scratch) by as many bytes."""
    FILLS = dict(trk_count=-7, trk_i=-7, trk_f=-7.0, state=0x5A, scratch=0x5A)

    def __init__(self, c, off=0):
        from codd_amd import ops
        h, w = c["crop"]
        H, W = c["padded"]
        m = c["par"]["max_objects"]
        self.c, self.off, self.h, self.w, self.m = c, off, h, w, m
        self.T = torch.zeros(H * W * 7 + 4, device=DEV)[off:off + H * W * 7].view(1, H, W, 7)
        self.depth = torch.zeros(H * W + 4, device=DEV)[off:off + H * W].view(H, W)
        self.ids = torch.zeros(h * w + 4, dtype=torch.int16, device=DEV)[off:off + h * w].view(h, w)  # (uint16 bits)
        self.count = torch.zeros(8, dtype=torch.int32, device=DEV)[off:off + 4]
        self.ego = torch.zeros(20, device=DEV)[off:off + 16]
        self.moving = torch.zeros(h * w + 4, dtype=torch.uint8, device=DEV)[off:off + h * w].view(h, w)
        self.bcnt, self.cnt = _guarded(4, torch.int32, -7, off)
        self.bti, self.ti = _guarded(m * 8, torch.int32, -7, off)
        self.btf, self.tf = _guarded(m * 8, torch.float32, -7.0, off)
        self.bst, self.st = _guarded(ops.track_state_bytes(h, w, m), torch.uint8, 0x5A, off)
        self.bscr, self.scr = _guarded(ops.track_scratch(h, w, m), torch.uint8, 0x5A, off)
        self.ti, self.tf = self.ti.view(m, 8), self.tf.view(m, 8)
        self.base = (-self.st.data_ptr()) % 16  # the state's layout starts at the first 16-byte boundary
        self.nstate = 32 + 8 * m + 2 * h * w
        assert self.btf.data_ptr() % 16 == 0 and self.tf.data_ptr() % 16 == 4 * off and self.st.data_ptr() % 16 == off

    def seed(self, st):
        raw = np.frombuffer(lt.state_bytes(st), np.uint8).copy()
        self.st[self.base:self.base + self.nstate].copy_(torch.from_numpy(raw))

    def launch(self, c, f):
        """One frame ``f`` of the case ``c`` (of this Run's shapes), into the buffers as the last call left them."""
        from codd_amd import ops
        assert c["crop"] == (self.h, self.w) and c["par"]["max_objects"] == self.m
        self.ids.copy_(torch.from_numpy(f["ids"].view(np.int16)))
        self.count.copy_(torch.from_numpy(f["count"]))
        self.inputs = [self.ids.clone(), self.count.clone()]
        kw = {}
        if f["T"] is not None:
            self.T.copy_(torch.from_numpy(f["T"])[None])
            self.depth.copy_(torch.from_numpy(f["depth"]))
            self.inputs += [glm._bits(self.T).clone(), glm._bits(self.depth).clone()]
        if f["ego"] is not None:
            self.ego.copy_(torch.from_numpy(f["ego"]))
            kw["ego_record"] = self.ego
        if f["moving"] is not None:
            self.moving.copy_(torch.from_numpy(f["moving"]))
            kw["moving"] = self.moving
        with_T = f["T"] is not None
        ops.track_objects(self.T if with_T else None, self.depth if with_T else None, c["K"], c["crop"],
                          self.ids.view(torch.uint16), self.count, self.st, self.cnt, self.ti, self.tf, scratch=self.scr,
                          scale=c["scale"], fresh=f["fresh"], **c["par"], **kw)
        torch.cuda.synchronize()
        now = [self.ids, self.count] + ([glm._bits(self.T), glm._bits(self.depth)] if with_T else [])
        assert all(torch.equal(a, b) for a, b in zip(self.inputs, now)), "an input was modified"

    def check_guards(self, what=""):
        lo_ = GUARD + self.off
        for name, buf, view in (("trk_count", self.bcnt, self.cnt), ("trk_i", self.bti, self.ti), ("trk_f", self.btf, self.tf),
                                ("state", self.bst, self.st), ("scratch", self.bscr, self.scr)):
            fill, n = self.FILLS[name], view.numel()
            assert bool((buf[:lo_] == fill).all()) and bool((buf[lo_ + n:] == fill).all()), f"{what}: {name} guard overwritten"
        assert bool((self.st[:self.base] == 0x5A).all()) and bool((self.st[self.base + self.nstate:] == 0x5A).all()), \
            f"{what}: the state's slack bytes were written"

    def outputs(self):
        return dict(count=self.cnt.cpu().numpy(), trk_i=self.ti.cpu().numpy(), trk_f=self.tf.cpu().numpy(),
                    state=self.st[self.base:self.base + self.nstate].cpu().numpy().tobytes())


def _assert_equal(out, ref, name):
    """trk_count, both tables in full and the state against the restatement: bytes, not values."""
    print(f"{name}: count {out['count'].tolist()} (restatement {ref['count'].tolist()})")
    assert out["count"].tolist() == ref["count"].tolist(), name
    bad = np.argwhere(out["trk_i"] != ref["trk_i"])
    assert bad.size == 0, f"{name}: trk_i differs at {bad[:8].tolist()}: {out['trk_i'][bad[0][0]].tolist()} vs {ref['trk_i'][bad[0][0]].tolist()}"
    a, b = out["trk_f"].view(np.uint32), ref["trk_f"].view(np.uint32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{name}: trk_f differs at {bad[:8].tolist()}: {out['trk_f'][bad[0][0]].tolist()} vs {ref['trk_f'][bad[0][0]].tolist()}"
    want = lt.state_bytes(ref["state"])
    if out["state"] != want:
        g, r = np.frombuffer(out["state"], np.uint8), np.frombuffer(want, np.uint8)
        raise AssertionError(f"{name}: the rolled state differs at bytes {np.flatnonzero(g != r)[:8].tolist()}")


def _sequence(c, refs, name, off=0, run=None):
    run = Run(c, off) if run is None else run
    if c["seed"] is not None:
        run.seed(c["seed"])
    outs = []
    for i, (f, ref) in enumerate(zip(c["frames"], refs)):
        run.launch(c, f)
        run.check_guards(f"{name} frame {i}")
        outs.append(run.outputs())
        _assert_equal(outs[-1], ref, f"{name} frame {i}")
    return run, outs


@pytest.mark.parametrize("name", IDS)
def test_tracks_against_reference(name):
    c, refs = _case(name)
    _, a = _sequence(c, refs, name)
    _, b = _sequence(c, refs, name)  # determinism: a second run gives equal bytes
    for x, y in zip(a, b):
        assert x["state"] == y["state"] and all(x[k].tobytes() == y[k].tobytes() for k in ("count", "trk_i", "trk_f"))


def test_dirty_buffers_and_scratch_give_the_same_bytes():
    """Six sequences in a row into the same outputs, state and scratch, each starting fresh on what the one before left:
    the vote matrix, the sums, the maxima and the cleared rows of the earlier case.  All 70 x 150 with 256 rows."""
    order = ["whole-crop", "split-merge-tie", "n-cur-0", "invalid", "leaving", "ego-moving"]
    run = Run(_case(order[0])[0])
    for name in order:
        c, refs = _case(name)
        _sequence(c, refs, name + " into used buffers", run=run)


@pytest.mark.parametrize("name", ("ego-moving", "invalid", "crop-5x7"))
def test_tracks_unaligned_views(name):
    """Every fp32 / int32 pointer 4, 8, 12 bytes off a 16-byte boundary (ids 2, 4, 6; moving, state and scratch 1, 2, 3
    bytes): the bytes of the restatement, nothing written outside the views."""
    c, refs = _case(name)
    for off in (1, 2, 3):
        run, _ = _sequence(c, refs, f"{name} offset {off}", off=off)
        assert run.T.data_ptr() % 16 == 4 * off and run.ids.data_ptr() % 16 == 2 * off and run.scr.data_ptr() % 16 == off


def test_entry_rejects_bad_arguments():
    """The CODD_EINVAL list of include/codd_hip.h, on the entry itself: -1 before any launch, nothing written."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    c, _ = _case("crop-5x7")
    run = Run(c)
    f = c["frames"][1]
    run.launch(c, c["frames"][0])
    before = run.outputs()
    h, w = c["crop"]
    H, W = c["padded"]
    run.T.copy_(torch.from_numpy(f["T"])[None])
    run.depth.copy_(torch.from_numpy(f["depth"]))
    good = dict(T=run.T.data_ptr(), depth=run.depth.data_ptr(), H=H, W=W, h=h, w=w, fx=100.0, fy=100.0, cx=74.5, cy=20.25, scale=1.0,
                ids=run.ids.data_ptr(), count=run.count.data_ptr(), ego=None, moving=None, min_votes=1, m=run.m, fresh=0,
                state=run.st.data_ptr(), state_bytes=run.st.numel(), scratch=run.scr.data_ptr(), scratch_bytes=run.scr.numel(),
                trk_count=run.cnt.data_ptr(), trk_i=run.ti.data_ptr(), trk_f=run.tf.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.codd_track_objects(a["T"], a["depth"], a["H"], a["W"], a["h"], a["w"], a["fx"], a["fy"], a["cx"], a["cy"], a["scale"],
                                    a["ids"], a["count"], a["ego"], a["moving"], a["min_votes"], a["m"], a["fresh"], a["state"],
                                    a["state_bytes"], a["scratch"], a["scratch_bytes"], a["trk_count"], a["trk_i"], a["trk_f"],
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    nan, inf = float("nan"), float("inf")
    bad = [dict(ids=None), dict(count=None), dict(state=None), dict(scratch=None), dict(trk_count=None), dict(trk_i=None),
           dict(trk_f=None), dict(depth=None), dict(h=0), dict(w=0), dict(H=0), dict(W=-1), dict(h=H + 1), dict(w=W + 1),
           dict(h=65536, w=32768, H=65536, W=32768), dict(m=0), dict(m=1025), dict(min_votes=0), dict(fx=0.0), dict(fx=nan),
           dict(fy=-1.0), dict(fy=inf), dict(scale=0.0), dict(scale=inf), dict(scale=nan), dict(cx=nan), dict(cy=inf),
           dict(state_bytes=ops.track_state_bytes(h, w, run.m) - 1), dict(scratch_bytes=ops.track_scratch(h, w, run.m) - 1)]
    for kw in bad:
        assert call(**kw) == -1, f"{kw} was not rejected"
        now = run.outputs()
        assert now["state"] == before["state"] and all(now[k].tobytes() == before[k].tobytes() for k in ("count", "trk_i", "trk_f")), kw
    assert lib.codd_track_state_bytes(0, 5, 4) == -1 and lib.codd_track_scratch(5, 5, 1025) == -1
    assert lib.codd_track_state_bytes(65536, 32768, 4) == -1 and lib.codd_track_scratch(5, 0, 4) == -1
    assert lib.codd_track_state_bytes(5, 7, 8) == 16 + 32 + 64 + 70
    assert call() == 0  # the same arguments unchanged are accepted (T given, depth given, no ego, no moving)
    assert call(T=None, depth=None) == 0  # T is not a required pointer
    with pytest.raises(ValueError):
        ops.track_objects(None, None, c["K"], c["crop"], run.ids.view(torch.uint16), run.count, run.st, run.cnt, run.ti, run.tf,
                          scratch=run.scr, min_votes=0, max_objects=run.m)
    with pytest.raises(_abi.CoddHipError):  # a state that is too small reaches the entry and is rejected there
        ops.track_objects(None, None, c["K"], c["crop"], run.ids.view(torch.uint16), run.count, run.st[:-1], run.cnt, run.ti,
                          run.tf, scratch=run.scr, max_objects=run.m)


# ---- the session against the entry on the session's own device buffers ------------------------------------------------
FIELDS = ("track", "age", "prev", "votes", "pixels", "moving", "own_pixels", "motion", "own")


def _same_tracks(a, b):
    return (tuple(a[:4]) == tuple(b[:4])
            and all(getattr(a, k).dtype == getattr(b, k).dtype and getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in FIELDS))


def test_session_tracks_against_the_entries_by_hand():
    import live_ego_ref as le
    import test_gpu_live_ego as gle
    import test_gpu_live_ground as glg
    import test_gpu_live_objects as glo
    from codd_amd import live, ops
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()
    h, w = glm.H0, glm.W0
    bf = le.lm.bf_of(glm.INTRINSICS[0])
    K = [float(np.float32(v)) for v in glm.INTRINSICS]
    objects = dict(glo.OBJECTS, map=True)
    m = objects["max_objects"]
    s = glm._session(ground=glo.GROUND, objects=objects, egomotion=True, tracks=dict(min_votes=4))
    base = glm._session(ground=glo.GROUND, objects=objects, egomotion=True)
    state = torch.zeros(ops.track_state_bytes(h, w, m), dtype=torch.uint8, device=DEV)
    cnt = torch.empty(4, dtype=torch.int32, device=DEV)
    ti, tf = torch.empty(m, 8, dtype=torch.int32, device=DEV), torch.empty(m, 8, device=DEV)
    first = []
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 5
        res, ego, g, ob, tr = got
        res1, ego1, g1, ob1 = base.step(left, right)
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i]), f"frame {i}: the depth result changed"
        assert gle._same_ego(ego, ego1), f"frame {i}: Ego changed with tracks= on"
        assert glg._same_ground(g, g1), f"frame {i}: Ground changed with tracks= on"
        assert glo._same_objects(ob, ob1), f"frame {i}: Objects changed with tracks= on"
        assert isinstance(tr, live.Tracks) and tr.n == ob.n and tr.continued + tr.started == tr.n
        assert tr.track.shape == (tr.n,) and tr.motion.shape == tr.own.shape == (tr.n, 3) and tr.track.flags["OWNDATA"]
        # the entry called by hand on the session's device buffers of this frame (step() has synchronised) and on the
        # previous depth map of the route a user had to write
        Ts = parent[i][1]
        depth_prev = None if Ts is None else ops.disp_to_depth(parent[i - 1][0], bf)[0, 0].contiguous()
        ops.track_objects(Ts, depth_prev, K, (h, w), s._d_objects[3], s._d_objects[0], state, cnt, ti, tf,
                          ego_record=None if Ts is None else s._d_ego[0], moving=None if Ts is None else s._d_ego[1],
                          scale=glm.CALIB / bf, fresh=i == 0, min_votes=4, max_objects=m)
        want = live.tracks_from_buffers(cnt.cpu().numpy(), ti.cpu().numpy(), tf.cpu().numpy())
        print(f"frame {i}: {tr.n} objects: {tr.continued} continued, {tr.started} started, {tr.ended} ended; tracks "
              f"{tr.track.tolist()[:8]} ages {tr.age.tolist()[:8]} votes {tr.votes.tolist()[:8]}")
        assert _same_tracks(tr, want), f"frame {i}: Tracks differ from the entry called by hand"
        if i == 0:
            assert tr.started == tr.n and tr.ended == 0 and tr.track.tolist() == list(range(1, tr.n + 1))
        first.append(tr)
    kept = [tuple(getattr(tr, k).copy() for k in FIELDS) for tr in first]
    for tr in first:  # the results are the caller's: scribbling on them changes no later frame
        tr.track[...] = -1
    s.reset()
    base.reset()
    base.close()
    second = []
    for left, right in frames:  # a new sequence, pipelined: push, push, pop, pop; the ids restart at 1
        s.push(left.copy(), right.copy())
        if s.pending() == 2:
            second.append(s.pop())
    while s.pending():
        second.append(s.pop())
    assert len(second) == glm.FRAMES
    for i in range(glm.FRAMES):
        assert np.array_equal(second[i][0], plain[i]), f"pipelined frame {i}: the result differs"
        tr = second[i][4]
        assert tuple(tr[:4]) == tuple(first[i][:4])
        assert all(getattr(tr, k).tobytes() == v.tobytes() for k, v in zip(FIELDS, kept[i])), f"pipelined frame {i}: Tracks differ from step()'s"
    s.reset()
    s.close()
    assert s._d_tracks is None and s._h_tracks is None and s._track_state is None and s._track_scratch is None
    # without objects=dict(map=True) the id map stays on the device: the same Tracks, no ids in Objects
    t = glm._session(ground=glo.GROUND, objects=dict(objects, map=False), tracks=dict(min_votes=4))
    for i, (left, right) in enumerate(frames[:3]):
        res, g, ob, tr = t.step(left, right)
        assert ob.ids is None and tuple(tr[:4]) == tuple(first[i][:4])
        assert all(getattr(tr, k).tobytes() == v.tobytes() for k, v in zip(FIELDS[:5], kept[i][:5])), f"frame {i} without the map"
    t.reset()
    t.close()


def test_cli_live_tracks(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    h, w, n = 100, 200, 4
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    inference.main(["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
                    "--live", "--ground", "--objects", "--tracks", "--show-dir", str(tmp_path / "out")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "tracks:" in ln]
    assert len(lines) == 1 and f"in {n} frames" in lines[0]
    assert sorted(os.listdir(tmp_path / "out")) == ["left.objects.pred.npz", "left.tracks.pred.npz"]
    z, o = np.load(tmp_path / "out" / "left.tracks.pred.npz"), np.load(tmp_path / "out" / "left.objects.pred.npz")
    assert sorted(z.files) == ["age", "continued", "ended", "motion", "moving", "n", "own", "own_pixels", "pixels", "prev",
                               "started", "track", "votes"]
    m = 256
    assert all(z[k].shape == (1, n) and z[k].dtype == np.int32 for k in ("n", "continued", "started", "ended"))
    assert all(z[k].shape == (1, n, m) and z[k].dtype == np.int32 for k in ("track", "age", "prev", "votes", "pixels", "moving", "own_pixels"))
    assert z["motion"].shape == z["own"].shape == (1, n, m, 3) and z["motion"].dtype == np.float32
    assert np.array_equal(z["n"], o["n"]) and np.array_equal(z["continued"] + z["started"], z["n"])
    n0 = int(z["n"][0, 0])
    assert z["started"][0, 0] == n0 and z["track"][0, 0, :n0].tolist() == list(range(1, n0 + 1)) and not z["track"][0, 0, n0:].any()
