"""Depth registered to another camera on the GPU: codd_align_depth on exact plants (bits), against the brute-force fp64
reference of tests/live_align_ref.py (depth inside the counted bound outside the ambiguous pixels, uv inside DELTA / 2),
skipped pixels and guard regions, determinism and padding, LiveSession(align_to=...) against the kernel called directly on
the disparity the session returns, and the --live --align command line.  Autotune is off in every test.

DELTA and DEPTH_C are derived in tests/live_align_ref.py and checked on the CPU by tests/test_live_align.py: the fp32
restatement's position deviates from fp64 by at most 1.23e-5 px over the general cases (MEASURED_DEV = 1.3e-5), 8 times that
is below the floor, so DELTA = 2^-10 px and uv is held to 2^-11 px; DEPTH_C = 8 is counted from the operation order.
test_general_cases_against_the_reference prints each case's figures before it asserts; on the MI355X run these tests were
written on: depth error at most 0.48 of the bound, uv error at most 1.23e-5 px, ambiguous pixels 0 in the 2 x 2 and 4 x 6
cases and 12 .. 32 (0.7 .. 1.9 % of the covered pixels, cap 2 %) at 37 x 53, and outside them no pixel that differs from the
reference in being reached."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_align_ref as la  # noqa: E402
import live_calib_ref as cr  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames and estimator, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # canary floats on either side of every output
CANARY = -7.0
shape_id = lambda s: "%dx%d" % s[0]  # noqa: E731
_CACHE = {}


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _struct(t):
    from codd_amd import _abi, ops
    s = _abi.AlignView()
    s.R[:] = [float(x) for x in np.asarray(t["R"], np.float64).reshape(-1)]
    s.T[:] = [float(x) for x in t["T"]]
    s.K[:] = [float(x) for x in t["K"]]
    s.dist[:] = [float(x) for x in t["dist"]]
    s.r2_max, s.model = float(t["r2_max"]), ops.CALIB_MODELS[t["model"]]
    return s


def _general(spec):
    """(case, reference), computed once and never modified."""
    if spec not in _CACHE:
        c = la.general_case(spec)
        _CACHE[spec] = (c, la.reference(c))
    return _CACHE[spec]


class Run:
    """One call of ops.align_depth on the case ``c``: both outputs between canaries; ``off`` shifts each output by that
    many floats off a 16-byte boundary; ``uv`` False passes no uv_out; ``disp`` / ``padded`` override the input."""

    def __init__(self, c, off=0, uv=True, disp=None):
        from codd_amd import ops
        (h, w), (ht, wt) = c["crop"], c["target"]["size"]
        src = torch.from_numpy(np.ascontiguousarray(c["disp"] if disp is None else disp))
        self.disp = src.to(DEV)
        self.disp0 = self.disp.clone()
        self.off, self.nd, self.nuv = off, ht * wt, h * w * 2
        self.bdepth = torch.full((self.nd + 2 * GUARD + 4,), CANARY, device=DEV)
        self.buv = torch.full((self.nuv + 2 * GUARD + 4,), CANARY, device=DEV)
        self.depth = self.bdepth[GUARD + off:GUARD + off + self.nd].view(ht, wt)
        self.uv = self.buv[GUARD + off:GUARD + off + self.nuv].view(h, w, 2) if uv else None
        assert self.bdepth.data_ptr() % 16 == 0 and self.depth.data_ptr() % 16 == 4 * off
        ops.align_depth(self.disp, (h, w), (c["f"], c["f"], c["cx"], c["cy"]), c["calib"], _struct(c["target"]), (ht, wt),
                        c["k"], self.depth, self.uv)
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        lo = GUARD + self.off
        assert bool((self.bdepth[:lo] == CANARY).all()) and bool((self.bdepth[lo + self.nd:] == CANARY).all()), f"{what}: depth canary overwritten"
        if self.uv is None:
            assert bool((self.buv == CANARY).all()), f"{what}: no uv asked for and its buffer was written"
        else:
            assert bool((self.buv[:lo] == CANARY).all()) and bool((self.buv[lo + self.nuv:] == CANARY).all()), f"{what}: uv canary overwritten"
        assert torch.equal(glm._bits(self.disp), glm._bits(self.disp0)), f"{what}: the disparity was modified"

    def outputs(self):
        return self.depth.cpu().numpy(), None if self.uv is None else self.uv.cpu().numpy()

    def same_bytes(self, other, uv=True):
        same = torch.equal(glm._bits(self.depth), glm._bits(other.depth))
        if uv and self.uv is not None and other.uv is not None:
            same = same and torch.equal(glm._bits(self.uv), glm._bits(other.uv))
        return same


# ---- 1. exact plants: every bit, no excluded pixel ------------------------------------------------------------------
@pytest.mark.parametrize("which", ("a", "b"))
@pytest.mark.parametrize("shape", la.SHAPES, ids=shape_id)
def test_exact_plants(shape, which):
    c, want, (by0, by1, bx0, bx1) = la.plant_case(shape, which)
    r = Run(c)
    r.check_guards(f"plant {which}")
    depth, uv = r.outputs()
    assert depth.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    (h, w) = c["crop"]
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    Z = np.float32(c["calib"]) / c["disp"][:h, :w]
    shift = (5.0, -2.0) if which == "a" else (16.0 / Z, 0.0)
    assert np.array_equal(uv[..., 0], uu + shift[0]) and np.array_equal(uv[..., 1], vv + shift[1])  # exact positions
    if which == "b" and shape[0] == (37, 53):
        assert (depth[by0:by1, bx0 + 8:bx1 + 8] == 2).all() and np.isinf(depth[by0:by1, bx0 + 2:bx0 + 8]).all()


# ---- 2. general cases against the fp64 reference --------------------------------------------------------------------
@pytest.mark.parametrize("spec", la.GENERAL, ids=la.case_id)
def test_general_cases_against_the_reference(spec):
    c, ref = _general(spec)
    name = la.case_id(spec)
    r = Run(c)
    r.check_guards(name)
    depth, uv = r.outputs()
    amb = la.ambiguous(ref["pos"], c["k"], c["target"]["size"], la.DELTA)
    covered = int(np.isfinite(ref["depth"]).sum())
    keep = ~amb & np.isfinite(ref["depth"]) & np.isfinite(depth)
    ok = ref["pos"]["ok"]
    with np.errstate(invalid="ignore"):  # (inf - inf where nothing landed: masked by ``keep``)
        derr = np.abs(depth.astype(np.float64) - ref["depth"])
    print(name, "ambiguous / covered:", int(amb.sum()), "/", covered,
          "depth error / bound:", float((derr[keep] / ref["bound"][keep]).max()) if keep.any() else 0.0,
          "uv error px:", float(np.nanmax(np.abs(uv.astype(np.float64) - ref["uv"])[ok])) if ok.any() else 0.0,
          "pixels off the reference in being reached:", int((np.isposinf(depth) != np.isinf(ref["depth"]))[~amb].sum()))
    assert int(amb.sum()) <= la.CAP * covered
    la.check_depth(depth, ref, amb, name)
    la.check_uv(uv, ref, la.DELTA / 2, name)


# ---- 3. skipped pixels and bounds -----------------------------------------------------------------------------------
BIG = la.SHAPES[2]
AWKWARD = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))


def _awkward_case():
    c, _ = _general((BIG, "brown", 1.5, 2))
    disp = c["disp"].copy()
    (h, w) = c["crop"]
    spots = [(0, 0), (h - 1, w - 1), (h // 2, w // 2), (3, w - 2), (h - 2, 5), (h // 2, 1), (7, 7), (20, 40), (11, 30), (30, 11)]
    for i, (y, x) in enumerate(spots):
        disp[y, x] = AWKWARD[i % len(AWKWARD)]
    return dict(c, disp=disp), spots


def test_unusable_disparities_are_skipped():
    c, spots = _awkward_case()
    ref = la.reference(c)
    r = Run(c)
    r.check_guards("awkward")
    depth, uv = r.outputs()
    for y, x in spots:
        assert not ref["pos"]["ok"][y, x] and np.isnan(uv[y, x]).all()
    assert int((~ref["pos"]["ok"]).sum()) == len(spots)
    amb = la.ambiguous(ref["pos"], c["k"], c["target"]["size"], la.DELTA)
    la.check_depth(depth, ref, amb, "awkward")
    la.check_uv(uv, ref, la.DELTA / 2, "awkward")


def test_points_behind_the_target_are_skipped():
    c, _ = _general((BIG, "fisheye", 0.75, 1))
    t = dict(c["target"], R=np.diag([-1.0, 1.0, -1.0]) @ c["target"]["R"])  # the target looks the other way
    c = dict(c, target=t)
    ref = la.reference(c)
    assert not ref["pos"]["ok"].any()
    r = Run(c)
    r.check_guards("behind")
    depth, uv = r.outputs()
    assert np.isposinf(depth).all() and np.isnan(uv).all()


def _fold_case():
    """A wide rectified camera (f = 16: x up to 2.3) in front of a Brown lens with k1 = -0.3, which folds back at r^2 =
    1.11: the pixels beyond it would land inside the image again.  One of them is the nearest point of the scene."""
    (h, w), (H, W) = BIG
    dist = (-0.3,) + (0.0,) * 7
    t = la.make_target("brown", (40, 56), 24.0, om=(0.0, 0.0, 0.0), T3=(0.0, 0.0, 0.0), dist=dist)
    disp = np.full((H, W), 2.0, np.float32)
    plant = (2, 3)
    disp[plant] = 16.0  # eight times nearer than everything else
    c = dict(disp=disp, crop=(h, w), f=16.0, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, calib=4.0, target=t, k=1)
    return c, plant


def test_points_beyond_r2_max_do_not_fold_back():
    c, plant = _fold_case()
    ref = la.reference(c)
    (h, w), t = c["crop"], c["target"]
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    r2 = ((uu - c["cx"]) / c["f"]) ** 2 + ((vv - c["cy"]) / c["f"]) ** 2
    assert np.abs(r2 - t["r2_max"]).min() > 1e-4  # no pixel sits on the threshold: fp32 and fp64 decide alike
    assert r2[plant] > t["r2_max"] and not ref["pos"]["ok"][plant] and 100 < int((~ref["pos"]["ok"]).sum()) < h * w - 100
    # without the guard the plant lands inside the target and, being nearest, wins its pixel
    loose = la.reference(dict(c, target=dict(t, r2_max=1e6)))
    sx, sy = loose["uv"][plant]
    ht, wt = t["size"]
    assert 0 <= np.rint(sx) < wt and 0 <= np.rint(sy) < ht and loose["depth"].min() == 0.25
    r = Run(c)
    r.check_guards("fold")
    depth, uv = r.outputs()
    assert np.isnan(uv[plant]).all() and depth.min() == 2.0  # the plant did not land: nothing is nearer than the wall
    amb = la.ambiguous(ref["pos"], 1, t["size"], la.DELTA)
    la.check_depth(depth, ref, amb, "fold")
    la.check_uv(uv, ref, la.DELTA / 2, "fold")


def test_positions_outside_the_target_are_reported_and_not_written():
    c, ref = _general((BIG, "fisheye", 0.75, 1))
    ht, wt = c["target"]["size"]
    t = dict(c["target"], K=(c["target"]["K"][0], c["target"]["K"][1], -3.0, ht + 2.0))  # the principal point off the image
    c = dict(c, target=t)
    ref = la.reference(c)
    r = Run(c)
    r.check_guards("outside")
    depth, uv = r.outputs()
    outside = (uv[..., 0] < -0.5) | (uv[..., 1] > ht - 0.5)
    assert np.isfinite(uv).all() and int(outside.sum()) > 0.5 * outside.size and 0 < int(np.isfinite(depth).sum())
    la.check_depth(depth, ref, la.ambiguous(ref["pos"], 1, (ht, wt), la.DELTA), "outside")
    la.check_uv(uv, ref, la.DELTA / 2, "outside")


@pytest.mark.parametrize("spec", ((la.SHAPES[0], "brown", 1.5, 2), (la.SHAPES[1], "fisheye", 1.4, 3), (BIG, "brown", 1.6, 3)),
                         ids=la.case_id)
def test_unaligned_outputs_and_no_uv(spec):
    """depth_out and uv_out 4, 8 and 12 bytes off a 16-byte boundary (uv_out then off an 8-byte one too): the bytes of the
    aligned run, the canaries untouched; and without uv_out the same depth and an untouched uv buffer."""
    c, _ = _general(spec)
    want = Run(c)
    want.check_guards("aligned")
    for off in (1, 2, 3):
        got = Run(c, off=off)
        assert got.depth.data_ptr() % 16 == 4 * off and got.uv.data_ptr() % 16 == 4 * off
        got.check_guards(f"offset {off}")
        assert want.same_bytes(got), f"offset {off}: bytes differ from the aligned run"
    for off in (0, 1):
        got = Run(c, off=off, uv=False)
        got.check_guards(f"uv_out = NULL, offset {off}")
        assert want.same_bytes(got, uv=False)


# ---- 4. determinism and padding -------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ((la.SHAPES[0], "fisheye", 0.75, 1), (la.SHAPES[1], "brown", 1.5, 2), (BIG, "brown", 1.5, 2),
                                  (BIG, "fisheye", 1.4, 3)), ids=la.case_id)
def test_determinism_and_padding(spec):
    c, _ = _general(spec)
    (h, w) = c["crop"]
    a, b = Run(c), Run(c)
    assert a.same_bytes(b)
    junk = c["disp"].copy()
    junk[h:, :], junk[:, w:] = np.float32(0.37), np.float32("nan")
    assert not np.array_equal(junk, c["disp"], equal_nan=True)
    p = Run(c, disp=junk)
    p.check_guards("padding")
    assert a.same_bytes(p), "the padding influenced an output byte"
    crop = Run(c, disp=np.ascontiguousarray(c["disp"][:h, :w]))  # H = h, W = w
    crop.check_guards("crop")
    assert a.same_bytes(crop), "[h,w] crop passed with H = h, W = w gives other bytes than the padded [H,W] input"


# ---- 5. the session -------------------------------------------------------------------------------------------------
SH, SW, SN = 100, 200, 6
S_INTRINSICS, S_CALIB = (210.0, 210.0, 99.5, 49.5), 21.0


def _colour_target():
    from codd_amd import calibration
    t = la.make_target("brown", (90, 160), 150.0)
    return calibration.AlignTarget(la.as_camera(t), t["R"], t["T"])


def _session(**kw):
    from codd_amd.live import LiveSession
    return LiveSession(glm._estimator(iters=4), (SH, SW), intrinsics=S_INTRINSICS, calib=S_CALIB, output="disp", bgr=False, **kw)


def _direct(disp_hw, view, size, k, uv, intrinsics=S_INTRINSICS, calib=S_CALIB):
    """ops.align_depth on a disparity the session returned ([h,w], passed with H = h, W = w)."""
    from codd_amd import ops
    h, w = disp_hw.shape
    d = torch.from_numpy(disp_hw).to(DEV)
    depth = torch.empty(size, device=DEV)
    pos = torch.empty(h, w, 2, device=DEV) if uv else None
    ops.align_depth(d, (h, w), intrinsics, calib, view, size, k, depth, pos)
    return depth.cpu().numpy(), None if pos is None else pos.cpu().numpy()


def _same_aligned(a, b):
    return np.array_equal(a.depth, b.depth) and ((a.uv is None and b.uv is None) or np.array_equal(a.uv, b.uv, equal_nan=True))


def test_session_aligned_depth():
    from codd_amd import live, ops
    frames = glm._frames(SH, SW, SN)
    plain = _session()
    want = [plain.step(left, right) for left, right in frames]
    plain.reset()
    plain.close()
    target = _colour_target()
    s = _session(align_to=target, align=dict(uv=True))
    assert s.align["footprint"] == 1  # (150 / 210: the target shrinks)
    view = ops.align_view(target)
    first, marks = [], {}
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 2 and isinstance(got[1], live.Aligned)
        torch.cuda.synchronize()
        marks[i + 1] = torch.cuda.memory_allocated()
        assert isinstance(want[i], np.ndarray) and got[0].tobytes() == want[i].tobytes(), f"frame {i}: the disparity changed"
        al = got[1]
        assert al.depth.dtype == np.float32 and al.depth.shape == (90, 160) and al.depth.flags["OWNDATA"]
        assert al.uv.dtype == np.float32 and al.uv.shape == (SH, SW, 2) and al.uv.flags["OWNDATA"]
        depth, uv = _direct(got[0], view, (90, 160), 1, True)
        assert al.depth.tobytes() == depth.tobytes(), f"frame {i}: Aligned.depth differs from ops.align_depth on the returned disparity"
        assert np.array_equal(al.uv, uv, equal_nan=True)
        assert np.isfinite(al.depth).mean() > 0.25
        first.append(al)
    print("memory_allocated per frame:", marks)
    assert marks[3] == marks[6]  # nothing is allocated per frame
    graph = s.runner.graph
    s.reset()
    second = []
    for left, right in frames:  # a new sequence, pipelined
        s.push(left.copy(), right.copy())
        if s.pending() == 2:
            second.append(s.pop())
    while s.pending():
        second.append(s.pop())
    assert len(second) == SN and s.runner.graph is graph
    for i in range(SN):
        assert second[i][0].tobytes() == want[i].tobytes(), f"pipelined frame {i}: the disparity differs"
        assert _same_aligned(second[i][1], first[i]), f"pipelined frame {i}: Aligned differs from step()'s"
    s.reset()
    s.close()
    assert s._d_align is None and s._h_align is None
    # without uv, next to confidence: (result, confidence, aligned), footprint given
    both = _session(align_to=target, align=dict(footprint=2), confidence=True)
    for i, (left, right) in enumerate(frames[:2]):
        res, conf, al = both.step(left, right)
        assert res.tobytes() == want[i].tobytes() and isinstance(conf, live.Confidence) and al.uv is None
        assert al.depth.tobytes() == _direct(res, view, (90, 160), 2, False)[0].tobytes()
    both.reset()
    both.close()


def test_session_aligns_to_the_rigs_own_left_camera():
    """calibration= with align_to="left": the depth map on the grid of the distorted left frames the caller owns."""
    from codd_amd import calibration, ops
    from codd_amd.live import LiveSession
    (Kl, dl), (Kr, dr), R, T = cr.make_rig("brown", (SH, SW))
    sc = calibration.StereoCalibration(calibration.CameraModel((SH, SW), Kl, "brown", dl), calibration.CameraModel((SH, SW), Kr, "brown", dr), R, T)
    s = LiveSession(glm._estimator(iters=4), (SH, SW), calibration=sc, output="disp", align_to="left")
    view = ops.align_view(calibration.AlignTarget.of_rig(s.rect, "left"))
    for left, right in glm._frames(SH, SW, SN)[:3]:
        disp, al = s.step(left, right)
        assert al.depth.shape == (SH, SW) and al.uv is None and np.isfinite(al.depth).mean() > 0.25
        depth, _ = _direct(disp, view, (SH, SW), s.align["footprint"], False, s.rect.intrinsics, s.rect.calib)
        assert al.depth.tobytes() == depth.tobytes()
    s.reset()
    s.close()


def test_cli_live_align(tmp_path):
    from PIL import Image
    from codd_amd import calibration, inference
    (Kl, dl), (Kr, dr), R, T = cr.make_rig("brown", (SH, SW))
    sc = calibration.StereoCalibration(calibration.CameraModel((SH, SW), Kl, "brown", dl), calibration.CameraModel((SH, SW), Kr, "brown", dr), R, T)
    sc.save(tmp_path / "rig.json")
    n = 3
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(SH, SW, SN)[:n]):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    common = ["--stereo-only", "--no-autotune", "--show", "--live", "--img-dir", str(tmp_path / "left"), "--r-img-dir",
              str(tmp_path / "right"), "--calibration", str(tmp_path / "rig.json")]
    inference.main(common + ["--show-dir", str(tmp_path / "plain")])
    inference.main(common + ["--show-dir", str(tmp_path / "al"), "--align", "right", "--align-footprint", "2"])
    assert sorted(os.listdir(tmp_path / "plain")) == ["left.disp.pred.npz"]  # no such file without the flag
    assert sorted(os.listdir(tmp_path / "al")) == ["left.aligned.pred.npz", "left.disp.pred.npz"]
    a = np.load(tmp_path / "plain" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "al" / "left.disp.pred.npz")["disp"]
    assert a.shape == (1, n, SH, SW) and a.tobytes() == b.tobytes()  # the disparity file is unchanged
    z = np.load(tmp_path / "al" / "left.aligned.pred.npz")
    assert z.files == ["depth"]
    depth = z["depth"]
    assert depth.shape == (1, n, SH, SW) and depth.dtype == np.float32
    from codd_amd import ops
    rect = sc.rectify((SH, SW))
    view = ops.align_view(calibration.AlignTarget.of_rig(rect, "right"))
    for i in range(n):
        want, _ = _direct(np.ascontiguousarray(a[0, i]), view, (SH, SW), 2, False, rect.intrinsics, rect.calib)
        assert depth[0, i].tobytes() == want.tobytes()
