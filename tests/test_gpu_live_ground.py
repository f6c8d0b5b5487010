"""LiveSession ground plane on the GPU: codd_ground_plane against the restatement of tests/live_ground_ref.py (labels exact
outside the undecided pixels; coefficients, normal, camera height and heights within K_DEV x the deviation of the fp32
restatement from the fp64 reference; the grid's counts within the undecided pixels that can reach a cell; the record's sums
against the host fit of the same inputs; determinism, dirty buffers, padding, guard regions, unaligned pointers, the calls
without heights and without a grid), LiveSession(ground=...) against the kernel called directly on the disparity of the
route a user had to write, and the --live --ground command line.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ground_ref as lg  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every output
K_DEV = 5.0  # x the restatement's own deviation (finding 85)
REL = 1e-9  # the record against the host fit of the same inputs: sums in another order only
_CACHE = {}
IDS = [lg.case_id(s) for s in lg.CASES]
NAMES = {n: i for i, n in enumerate(IDS)}


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _case(i):
    """(inputs, reference), computed once and never modified."""
    if i not in _CACHE:
        c = lg.case(lg.CASES[i])
        _CACHE[i] = (c, lg.reference(c))
    return _CACHE[i]


def _guarded(n, dtype, fill, off):
    buf = torch.full((n + 2 * GUARD + 4,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD + off:GUARD + off + n]


class Run:
    """One call of ops.ground_plane on the case ``c``: every output and the scratch between guard regions; ``off`` shifts
    every fp32 / int32 pointer by that many elements off a 16-byte boundary and the byte buffers by as many bytes.  The grid
    buffers exist whether the case asks for a grid or not (``grid`` False: the call gets None and must leave them)."""

    def __init__(self, c, with_height=True, with_grid=True, off=0, disp=None):
        from codd_amd import ops
        h, w = c["crop"]
        self.c, self.off, self.h, self.w = c, off, h, w
        src = torch.from_numpy(np.ascontiguousarray(c["disp"] if disp is None else disp))
        buf = torch.zeros(src.numel() + 4, device=DEV)
        self.disp = buf[off:off + src.numel()].view(src.shape)
        self.disp.copy_(src)
        self.gshape = c["grid"][0] if c["grid"] is not None else (4, 4)
        self.with_height, self.with_grid = with_height, with_grid and c["grid"] is not None
        cells = self.gshape[0] * self.gshape[1]
        self.brec, self.rec = _guarded(32, torch.float64, -7.0, 0)
        self.blab, self.lab = _guarded(h * w, torch.uint8, 0x5A, off)
        self.bhgt, self.hgt = _guarded(h * w, torch.float32, -7.0, off)
        self.bcnt, self.cnt = _guarded(2 * cells, torch.int32, -7, off)
        self.bgh, self.gh = _guarded(cells, torch.float32, -7.0, off)
        n = ops.ground_scratch(h, w, self.gshape if self.with_grid else None)
        self.bscr, self.scr = _guarded(n, torch.uint8, 0x5A, off)
        self.lab, self.hgt = self.lab.view(h, w), self.hgt.view(h, w)
        self.cnt, self.gh = self.cnt.view((2,) + self.gshape), self.gh.view(self.gshape)
        assert self.bhgt.data_ptr() % 16 == 0 and self.disp.data_ptr() % 16 == 4 * off
        self.launch(c)

    def launch(self, c, disp=None):
        """(again, with another case of the same shapes: into the buffers and the scratch as the last call left them)"""
        from codd_amd import ops
        if disp is not None:
            self.disp.copy_(torch.from_numpy(np.ascontiguousarray(disp)))
        self.disp0 = self.disp.clone()
        par = {k: v for k, v in c["par"].items() if self.with_grid or k != "cell"}
        ops.ground_plane(self.disp, c["K"], c["calib"], c["crop"], self.rec, self.lab, self.hgt if self.with_height else None,
                         self.cnt if self.with_grid else None, self.gh if self.with_grid else None, scratch=self.scr,
                         seed=c["seed"], up=lg.UP, **par)
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        lo = GUARD + self.off
        for name, buf, view, fill, used in (("record", self.brec, self.rec, -7.0, True), ("labels", self.blab, self.lab, 0x5A, True),
                                            ("height", self.bhgt, self.hgt, -7.0, self.with_height),
                                            ("grid_count", self.bcnt, self.cnt, -7, self.with_grid),
                                            ("grid_height", self.bgh, self.gh, -7.0, self.with_grid),
                                            ("scratch", self.bscr, self.scr, 0x5A, True)):
            n, first = view.numel(), GUARD if name == "record" else lo
            if used:
                assert bool((buf[:first] == fill).all()) and bool((buf[first + n:] == fill).all()), f"{what}: {name} guard overwritten"
            else:
                assert bool((buf == fill).all()), f"{what}: no {name} asked for and its buffer was written"
        assert torch.equal(glm._bits(self.disp), glm._bits(self.disp0)), f"{what}: the input was modified"

    def outputs(self):
        return dict(rec=self.rec.cpu().numpy().copy(), labels=self.lab.cpu().numpy(), height=self.hgt.cpu().numpy(),
                    grid_count=self.cnt.cpu().numpy(), grid_height=self.gh.cpu().numpy())

    def same_bytes(self, other):
        ok = torch.equal(self.rec.view(torch.int64), other.rec.view(torch.int64)) and torch.equal(self.lab, other.lab)
        if self.with_height and other.with_height:
            ok = ok and torch.equal(glm._bits(self.hgt), glm._bits(other.hgt))
        if self.with_grid and other.with_grid:
            ok = ok and torch.equal(self.cnt, other.cnt) and torch.equal(glm._bits(self.gh), glm._bits(other.gh))
        return ok


@pytest.mark.parametrize("i", range(len(lg.CASES)), ids=IDS)
def test_ground_against_reference(i):
    from codd_amd import live
    c, ref = _case(i)
    name = IDS[i]
    a = Run(c)
    a.check_guards(name)
    out = a.outputs()
    rec = out["rec"]
    assert np.isfinite(rec).all() and not rec[25:].any()
    got = live.ground_from_record(rec, out["labels"], out["height"])
    r64, r32 = ref["r64"], ref["r32"]
    f64, m64, p64 = r64["fit"], r64["plane"], r64["pix"]
    und = ref["undecided"]
    print(f"{name}: record {rec[:13].tolist()}; undecided {int(und.sum())} of {int(ref['valid'].sum())} valid; dev coef "
          f"{ref['dev_coef']:.3e}, normal {ref['dev_normal']:.3e}, Hc {ref['dev_Hc']:.3e}, height {ref['dev_h']:.3e}")
    assert got.ok == m64["ok"] and got.valid == f64["n"] and got.steps == f64["steps"]
    if c["name"] == "none":  # nothing valid: ok = 0, a finite zero record, labels all 255
        assert not rec.any()
    # ---- the record against the header's fit (fp32 terms, fp64 sums) of the SAME inputs on the host: only the order of
    # the sums differs
    own = r32["fit"]
    A = np.zeros((3, 3))
    A[np.triu_indices(3)] = rec[13:19]
    A = A + np.triu(A, 1).T
    scale = max(np.abs(own["coef"]).max(), 1e-300)
    print(f"  record vs host fit: coef {np.abs(got.coef - own['coef']).max() / scale:.3e} relative; vs fp64 reference "
          f"{np.abs(got.coef - f64['coef']).max():.3e} (bound {K_DEV * ref['dev_coef']:.3e})")
    assert np.abs(got.coef - own["coef"]).max() <= REL * scale
    assert np.abs(A - own["A"]).max() <= REL * max(np.abs(own["A"]).max(), 1e-300)
    assert np.abs(rec[19:22] - own["b"]).max() <= REL * max(np.abs(own["b"]).max(), 1e-300)
    # inliers: exact unless a fit pixel's |e| sits within the restatement's error of delta_px
    ys, xs = own["idx"]
    _, _, _, e = lg.residual(c, own["coef"], np.float32, ys, xs)
    near = int((np.abs(np.abs(e.astype(np.float64)) - c["par"]["delta_px"]) <= 2 * max(ref["dev_e"], 1e-6)).sum())
    assert abs(got.inliers - own["inliers"]) <= near
    if near == 0:
        assert abs(got.rms_px - own["rms"]) <= REL * max(own["rms"], 1e-12)
    # ---- against the fp64 reference, by the k x rule
    assert np.abs(got.coef - f64["coef"]).max() <= K_DEV * ref["dev_coef"]
    if f64["alive"] and m64["Hc"] > 0:  # (reported for a plane that fails the tilt rule too)
        r32m = r32["plane"]
        assert np.abs(got.normal - m64["normal"]).max() <= K_DEV * ref["dev_normal"]
        assert abs(got.camera_height - m64["Hc"]) <= K_DEV * ref["dev_Hc"]
        assert abs(got.tilt_deg - m64["tilt"]) <= K_DEV * max(abs(r32m["tilt"] - m64["tilt"]), 1e-12)
        assert np.abs(got.forward - m64["forward"]).max() <= K_DEV * max(np.abs(r32m["forward"] - m64["forward"]).max(), 1e-15)
    # ---- labels: exact outside the undecided pixels; heights by the k x rule
    lab, hgt = out["labels"], out["height"]
    assert np.array_equal(lab[~und], p64["labels"][~und]), f"{name}: labels differ at {np.argwhere((lab != p64['labels']) & ~und)[:8].tolist()}"
    assert np.array_equal(np.isnan(hgt), np.isnan(p64["height"]))
    if m64["ok"]:
        ok_px = ~np.isnan(hgt)
        err = float(np.abs(hgt.astype(np.float64) - p64["height"])[ok_px].max())
        same32 = np.array_equal(hgt, r32["pix"]["height"], equal_nan=True) and np.array_equal(lab, r32["pix"]["labels"])
        print(f"  max |height - fp64 reference| {err:.3e} (bound {K_DEV * ref['dev_h']:.3e}); labels and heights equal to the "
              f"fp32 restatement bit for bit: {same32}")
        assert err <= K_DEV * ref["dev_h"]
    else:
        assert (lab == lg.INVALID).all() and np.isnan(hgt).all()
    # ---- the grid: counts within the undecided pixels that can reach a cell; heights where no such pixel can
    if c["grid"] is not None:
        cnt, gh = out["grid_count"], out["grid_height"]
        if not m64["ok"]:
            assert not cnt.any() and not gh.any()
        else:
            reach = ref["reach"]
            diff = np.abs(cnt.astype(np.int64) - p64["grid_count"])
            print(f"  grid: {int(cnt[0].sum())} floor and {int(cnt[1].sum())} obstacle pixels in {int((cnt.sum(0) > 0).sum())} cells; "
                  f"cells that differ from the reference {int((diff > 0).sum())}, cells an undecided pixel can reach {int((reach > 0).sum())}")
            assert (diff <= reach[None]).all()
            clean = reach == 0
            assert np.abs(gh.astype(np.float64) - p64["grid_height"])[clean].max() <= K_DEV * ref["dev_h"]
            assert ((gh > 0) == (cnt[1] > 0)).all() and (cnt >= 0).all()
    # ---- determinism: a second run gives equal bytes
    assert a.same_bytes(Run(c))


def test_dirty_buffers_and_scratch_give_the_same_bytes():
    """A call into buffers and a scratch that still hold another case's results: the grid clear, the ticket reset and, for
    the scene that fails, the labels and grid taken back.  easy -> heavy-unseeded (ok = 0) -> wall, all 96 x 160 with a
    32 x 32 grid."""
    order = [NAMES["easy"], NAMES["heavy-unseeded"], NAMES["wall"], NAMES["heavy-seeded"]]
    r = Run(_case(order[0])[0])
    for i in order[1:]:
        c, ref = _case(i)
        r.launch(c, c["disp"])
        r.check_guards(IDS[i])
        fresh = Run(c)
        assert r.same_bytes(fresh), f"{IDS[i]} into used buffers differs from a run into fresh ones"
        if not ref["r64"]["plane"]["ok"]:
            assert bool((r.lab == 255).all()) and not bool(r.cnt.any()) and not bool(r.gh.any()) and bool(torch.isnan(r.hgt).all())


@pytest.mark.parametrize("name", ("easy", "plain", "odd-s1", "none"))
def test_padding_influences_no_output_byte(name):
    c, _ = _case(NAMES[name])
    h, w = c["crop"]
    a = Run(c)
    for fill in (float("nan"), -777.0, 0.5):
        t = c["disp"].copy()
        t[h:, :] = fill
        t[:, w:] = fill
        b = Run(c, disp=t)
        b.check_guards("padding")
        assert a.same_bytes(b), f"padding {fill} changed an output byte"


@pytest.mark.parametrize("name", ("easy", "odd-s3", "wall-seeded"))
def test_ground_unaligned_views_and_optional_outputs(name):
    """Every fp32 / int32 pointer 4, 8, 12 bytes off a 16-byte boundary (labels and scratch 1, 2, 3 bytes): the bytes of the
    aligned run, nothing written outside the views; without heights and without a grid the other outputs have the same
    bytes and the buffers not asked for are untouched."""
    c, _ = _case(NAMES[name])
    want = Run(c)
    want.check_guards("aligned")
    for off in (1, 2, 3):
        got = Run(c, off=off)
        assert got.hgt.data_ptr() % 16 == 4 * off and got.disp.data_ptr() % 16 == 4 * off and got.cnt.data_ptr() % 16 == 4 * off
        got.check_guards(f"offset {off}")
        assert want.same_bytes(got), f"offset {off}: bytes differ from the aligned run"
    for kw in (dict(with_height=False), dict(with_grid=False), dict(with_height=False, with_grid=False, off=1)):
        part = Run(c, **kw)
        part.check_guards(str(kw))
        assert part.same_bytes(want), f"{kw}: the remaining outputs differ"


def test_ops_reject_bad_arguments():
    from codd_amd import _abi, ops
    c, _ = _case(NAMES["plain"])
    with pytest.raises(ValueError):
        ops.ground_scratch(0, 5)
    with pytest.raises(ValueError):
        ops.ground_scratch(4, 5, (0, 3))
    a = Run(c)
    with pytest.raises(TypeError):
        ops.ground_plane(a.disp, c["K"], c["calib"], c["crop"], a.rec, a.lab, scratch=a.scr, speed=3)
    for bad in (dict(step=0), dict(iters=33), dict(delta_px=0.0), dict(asym=0.5), dict(clearance=0.01), dict(tol_px=float("nan"))):
        before = a.rec.clone()
        with pytest.raises(_abi.CoddHipError):
            ops.ground_plane(a.disp, c["K"], c["calib"], c["crop"], a.rec, a.lab, scratch=a.scr, **dict(c["par"], **bad))
        assert torch.equal(before, a.rec)
    with pytest.raises(_abi.CoddHipError):  # scratch too small
        ops.ground_plane(a.disp, c["K"], c["calib"], c["crop"], a.rec, a.lab, scratch=a.scr[:-1])


# ---- the session against the kernel on the tensors of the existing route ----------------------------------------
FIELDS = ("coef", "normal", "forward")


def _same_ground(a, b):
    return (all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in FIELDS)
            and (a.ok, a.camera_height, a.tilt_deg, a.valid, a.inliers, a.rms_px, a.steps) ==
            (b.ok, b.camera_height, b.tilt_deg, b.valid, b.inliers, b.rms_px, b.steps)
            and np.array_equal(a.labels, b.labels) and glm._equal_nan(a.height, b.height)
            and glm._equal_nan(a.grid_count, b.grid_count) and glm._equal_nan(a.grid_height, b.grid_height))


GROUND = dict(height=0.5, pitch_deg=12.0, map=True, grid=(16, 24), cell=0.05, min_valid=64, max_tilt_deg=90.0)


def _direct(disp):
    """ops.ground_plane as a user calls it on the route's (padded) disparity, with the session's parameters."""
    from codd_amd import live, ops
    h, w = glm.H0, glm.W0
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    lab, hgt = torch.empty(h, w, dtype=torch.uint8, device=DEV), torch.empty(h, w, device=DEV)
    cnt, gh = torch.empty((2,) + GROUND["grid"], dtype=torch.int32, device=DEV), torch.empty(GROUND["grid"], device=DEV)
    par = {k: GROUND.get(k, live.GROUND_DEFAULTS[k]) for k in ops.GROUND_PARAMS}
    ops.ground_plane(disp, glm.INTRINSICS, glm.CALIB, (h, w), rec, lab, hgt, cnt, gh,
                     seed=live.ground_seed(GROUND["height"], glm.INTRINSICS, glm.CALIB, pitch_deg=GROUND["pitch_deg"]),
                     up=live._unit_up((0, -1, 0), GROUND["pitch_deg"]), **par)
    return live.ground_from_record(rec.cpu().numpy(), lab.cpu().numpy(), hgt.cpu().numpy(), cnt.cpu().numpy(), gh.cpu().numpy())


def test_session_ground_against_the_existing_route():
    from codd_amd import live
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()
    s = glm._session(ground=GROUND)
    marks, first = {}, []
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 2
        torch.cuda.synchronize()
        marks[i + 1] = torch.cuda.memory_allocated()
        first.append(got[1])
        assert isinstance(plain[i], np.ndarray) and np.array_equal(got[0], plain[i]), f"frame {i}: the depth result changed"
    print("memory_allocated per frame:", marks)
    assert marks[3] == marks[6]  # nothing is allocated per frame
    graph = s.runner.graph
    assert graph is not None
    for i in range(glm.FRAMES):  # frame 0 included: no motion stage is needed
        g = first[i]
        assert isinstance(g, live.Ground) and g.coef.dtype == np.float64 and g.coef.shape == (3,)
        assert g.labels.dtype == np.uint8 and g.labels.shape == (glm.H0, glm.W0) and g.labels.flags["OWNDATA"]
        assert g.height.dtype == np.float32 and g.height.shape == (glm.H0, glm.W0)
        assert g.grid_count.dtype == np.int32 and g.grid_count.shape == (2, 16, 24) and g.grid_height.shape == (16, 24)
        want = _direct(parent[i][0])
        assert _same_ground(g, want), f"frame {i}: Ground differs from the direct call"
        print(f"frame {i}: ok {g.ok}, fit pixels {g.valid}, inliers {g.inliers}, camera height {g.camera_height:.4f}, tilt "
              f"{g.tilt_deg:.2f}, labels {np.bincount(g.labels.ravel(), minlength=256)[[0, 1, 2, 3, 255]].tolist()}, grid "
              f"{g.grid_count.sum(axis=(1, 2)).tolist()}")
    # a new sequence, pipelined: the same bytes as step()
    s.reset()
    second = []
    for left, right in frames:
        s.push(left.copy(), right.copy())
        if s.pending() == 2:
            second.append(s.pop())
    while s.pending():
        second.append(s.pop())
    assert len(second) == glm.FRAMES
    for i in range(glm.FRAMES):
        assert np.array_equal(second[i][0], plain[i]), f"pipelined frame {i}: the result differs"
        assert _same_ground(second[i][1], first[i]), f"pipelined frame {i} after reset(): Ground differs from step()'s"
    assert s.runner.graph is graph  # no re-capture
    s.reset()
    s.close()
    assert s._d_ground is None and s._h_ground is None and s._ground_scratch is None


def test_session_ground_with_every_other_output():
    """(result, motion, ego, confidence, aligned, epipolar, ground): the first six with the bits of a session without
    ground=; no map and no grid asked for: labels only."""
    from codd_amd import calibration, live
    import test_gpu_live_ego as gle
    plain, frames = glm._plain_results(), glm._frames()
    alone = glm._session(ground=dict(GROUND, map=False, grid=None, cell=0.1))
    want = [alone.step(left, right)[1] for left, right in frames]
    alone.reset()
    alone.close()
    target = calibration.AlignTarget(calibration.CameraModel((100, 150), (500.0, 500.0, 75.0, 50.0)), np.eye(3), [0.01, 0.0, 0.0])
    kw = dict(motion="sceneflow", egomotion=True, confidence=True, align_to=target, epipolar=True)
    both, only = glm._session(ground=dict(GROUND, map=False, grid=None, cell=0.1), **kw), glm._session(**kw)
    for i, (left, right) in enumerate(frames):
        got = both.step(left, right)
        assert isinstance(got, tuple) and len(got) == 7
        res, motion, ego, conf, al, epi, g = got
        res1, motion1, ego1, conf1, al1, epi1 = only.step(left, right)
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i])
        assert glm._equal_nan(motion, motion1), f"frame {i}: the motion output changed"
        assert gle._same_ego(ego, ego1), f"frame {i}: the ego output changed"
        assert np.array_equal(conf.flags, conf1.flags) and np.array_equal(conf.residual, conf1.residual, equal_nan=True)
        assert np.array_equal(al.depth, al1.depth)
        assert epi.coef.tobytes() == epi1.coef.tobytes() and epi.A.tobytes() == epi1.A.tobytes() and epi.valid == epi1.valid
        assert isinstance(g, live.Ground) and g.height is None and g.grid_count is None and g.grid_height is None
        assert _same_ground(g, want[i]), f"frame {i}: Ground differs with every option set"
    for t in (both, only):
        t.reset()
        t.close()


def test_cli_live_ground(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 6
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    common = ["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
              "--show", "--live"]
    inference.main(common + ["--show-dir", str(tmp_path / "plain")])
    assert "ground:" not in capsys.readouterr().out
    inference.main(common + ["--show-dir", str(tmp_path / "ground"), "--ground", "--ground-grid", "32x32"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "ground:" in ln]
    assert len(lines) == 1 and f"of {n} frames" in lines[0]
    assert sorted(os.listdir(tmp_path / "plain")) == ["left.disp.pred.npz"]  # no such file without the flag
    assert sorted(os.listdir(tmp_path / "ground")) == ["left.disp.pred.npz", "left.ground.pred.npz"]
    a = np.load(tmp_path / "plain" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "ground" / "left.disp.pred.npz")["disp"]
    assert a.shape == b.shape == (1, n, h, w) and np.array_equal(a, b)  # the disparity file is unchanged
    z = np.load(tmp_path / "ground" / "left.ground.pred.npz")
    assert sorted(z.files) == ["camera_height", "coef", "grid_count", "grid_height", "labels", "normal", "ok"]
    assert z["coef"].shape == (1, n, 3) and z["ok"].shape == (1, n) and z["normal"].shape == (1, n, 3)
    assert z["camera_height"].shape == (1, n) and z["labels"].shape == (1, n, h, w) and z["labels"].dtype == np.uint8
    assert z["grid_count"].shape == (1, n, 2, 32, 32) and z["grid_count"].dtype == np.int32
    assert z["grid_height"].shape == (1, n, 32, 32) and z["grid_height"].dtype == np.float32
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, ground=dict(grid=(32, 32)))
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        res, g = s.step(left, right)
        assert np.array_equal(res, a[0, i])
        assert np.array_equal(g.coef, z["coef"][0, i]) and bool(z["ok"][0, i]) == g.ok and np.array_equal(g.normal, z["normal"][0, i])
        assert z["camera_height"][0, i] == g.camera_height and np.array_equal(g.labels, z["labels"][0, i])
        assert np.array_equal(g.grid_count, z["grid_count"][0, i]) and np.array_equal(g.grid_height, z["grid_height"][0, i])
    s.reset()
    s.close()
