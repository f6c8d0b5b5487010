"""LiveSession motion output on the GPU: codd_export_motion against the fp64 restatement of tests/live_motion_ref.py
(three modes, validity, the depth roll, unaligned pointers, determinism), LiveSession(motion=...) against the route a
user had to write before it existed (FrameRunner.step, runner.last["Ts"], ops.disp_to_depth of the previous disparity),
and the --live --motion command line.  Autotune is off in every test, so launch configurations are the deterministic
heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_motion_ref as lm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.0
_CACHE = {}
case_id = lambda s: "%dx%d" % s[0]  # noqa: E731


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case(H, W):
    """Inputs and the fp64 reference of one padded shape, computed once and never modified."""
    if (H, W) not in _CACHE:
        c = lm.case(H, W)
        c["ref"] = lm.reference(c["T"], c["depth"], c["K"], c["bf"], lm.SCALE)
        c["disp"] = lm.disparity(H, W)
        _CACHE[(H, W)] = c
    return _CACHE[(H, W)]


def _depth_prev(c, h, w):
    """The case's depth inside the crop, SENTINEL outside it."""
    d = torch.full_like(c["depth"][0], SENTINEL)
    d[:h, :w] = c["depth"][0, :h, :w]
    return d.to(DEV)


def _run(c, h, w, mode, with_field=True):
    from codd_amd import ops
    dp = _depth_prev(c, h, w)
    out = torch.full((h, w, lm.CHANNELS[mode]), SENTINEL, device=DEV)
    ops.export_motion(c["T"].to(DEV) if with_field else None, c["disp"].to(DEV), dp, out, mode, c["K"], c["bf"], scale=lm.SCALE)
    torch.cuda.synchronize()
    return out, dp


def _check_roll(c, dp, h, w):
    from codd_amd import ops
    want = ops.disp_to_depth(c["disp"].to(DEV), c["bf"])[0, 0]
    assert torch.equal(dp[:h, :w], want[:h, :w]), "the rolled depth is not disp_to_depth of the current disparity"
    outside = torch.ones_like(dp, dtype=torch.bool)
    outside[:h, :w] = False
    assert bool((dp[outside] == SENTINEL).all()), "depth_prev was written outside the crop"
    # the awkward disparities: 0 -> the cap, negative -> 0, NaN -> 0, +inf -> 0
    assert dp[1, 2] == 210.0 and dp[3, 5] == 0.0 and dp[7, 11] == 0.0 and dp[13, 17] == 0.0


@pytest.mark.parametrize("mode", lm.MODES)
@pytest.mark.parametrize("shape", lm.CASES, ids=case_id)
def test_export_motion_against_fp64_reference(shape, mode):
    (h, w), (H, W) = shape
    c = _case(H, W)
    out, dp = _run(c, h, w, mode)
    res = lm.compare(out.cpu(), c["ref"], mode, h, w, f"kernel {h}x{w} in {H}x{W}", c["regime"])
    lm.within(res, 1.0, f"{mode} {h}x{w}")
    assert int(c["ref"]["invalid"][:h, :w].sum()) >= 8  # validity is exercised
    _check_roll(c, dp, h, w)
    # determinism: a second run gives equal bits
    out2, dp2 = _run(c, h, w, mode)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(dp), _bits(dp2))


@pytest.mark.parametrize("shape", lm.CASES, ids=case_id)
def test_export_motion_without_a_field_only_rolls(shape):
    (h, w), (H, W) = shape
    c = _case(H, W)
    for mode in lm.MODES:
        out, dp = _run(c, h, w, mode, with_field=False)
        assert bool((out == SENTINEL).all()), "out was written although the frame has no field"
        _check_roll(c, dp, h, w)
    # out may be NULL then
    from codd_amd import _abi
    dp = _depth_prev(c, h, w)
    disp = c["disp"].to(DEV)
    rc = _abi.load().codd_export_motion(None, disp.data_ptr(), dp.data_ptr(), H, W, h, w, 2, *[float(v) for v in c["K"]],
                                        c["bf"], 1.0, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    _check_roll(c, dp, h, w)


@pytest.mark.parametrize("mode", lm.MODES)
def test_export_motion_unaligned_views(mode):
    """Every pointer 4, 8 or 12 bytes off a 16-byte boundary: the scalar heads and tails give the bits of the aligned
    run and nothing is written outside the views."""
    from codd_amd import ops
    (h, w), (H, W) = lm.CASES[0]
    c = _case(H, W)
    ch = lm.CHANNELS[mode]
    want, want_dp = _run(c, h, w, mode)
    for off in (1, 2, 3):
        bT, bd, bp, bo = (torch.zeros(n + 8, device=DEV) for n in (H * W * 7, H * W, H * W, h * w * ch))
        T = bT[off:off + H * W * 7].view(1, H, W, 7)
        disp = bd[off:off + H * W].view(1, 1, H, W)
        dp = bp[off:off + H * W].view(H, W)
        out = bo[off:off + h * w * ch].view(h, w, ch)
        T.copy_(c["T"])
        disp.copy_(c["disp"])
        dp.copy_(_depth_prev(c, h, w))
        assert T.data_ptr() % 16 == 4 * off and out.data_ptr() % 16 == 4 * off
        ops.export_motion(T, disp, dp, out, mode, c["K"], c["bf"], scale=lm.SCALE)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want)), f"offset {off}: output differs from the aligned run"
        assert torch.equal(_bits(dp), _bits(want_dp)), f"offset {off}: rolled depth differs from the aligned run"
        for buf, n in ((bo, h * w * ch), (bp, H * W)):
            assert bool((buf[:off] == 0).all()) and bool((buf[off + n:] == 0).all()), f"offset {off}: guard overwritten"
        assert torch.equal(T, c["T"].to(DEV)) and torch.equal(_bits(disp), _bits(c["disp"].to(DEV)))  # inputs untouched


# ---- the session against the route a user had to write ----------------------------------------------------------
H0, W0, FRAMES = 200, 300, 6  # in 256 x 320: the smallest padded height the network admits is 128
INTRINSICS, CALIB = (1050.0, 1050.0, 150.0, 100.0), 210.0


def _frames(h=H0, w=W0, n=FRAMES):
    """``n`` frames of synth.stereo_sequence quantised to uint8 HWC (RGB)."""
    if ("frames", h, w, n) not in _CACHE:
        from codd_amd import synth
        img, r_img, _ = synth.stereo_sequence(h, w, n)

        def u8(t):
            return np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())

        _CACHE[("frames", h, w, n)] = [(u8(img[0, i]), u8(r_img[0, i])) for i in range(n)]
    return _CACHE[("frames", h, w, n)]


def _estimator(iters=16):
    if ("est", iters) not in _CACHE:
        import codd_amd  # noqa: F401
        from codd_amd import configs, synth
        from codd_amd.registry import build_estimator
        est = build_estimator(configs.codd(iters=iters) if iters != 16 else configs.codd()).eval()
        synth.load_synthetic_weights(est, gain=1.4)
        _CACHE[("est", iters)] = est.to(DEV)
    return _CACHE[("est", iters)]


def _parent_route():
    """What a user wrote before: ops.preprocess, FrameRunner.step, and after every frame a clone of runner.last["Ts"] and
    of the returned (padded) disparity -> [(disp [1,1,H,W], Ts [1,H,W,7] or None)], device tensors."""
    if "parent" not in _CACHE:
        from codd_amd import ops, synth
        from codd_amd.runtime import FrameRunner
        est = _estimator()
        H, W = -(-H0 // 64) * 64, -(-W0 // 64) * 64
        metas = synth.default_metas(H, W, img_shape=(H0, W0, 3), intrinsics=INTRINSICS)[0]
        metas[0]["calib"] = CALIB
        runner = FrameRunner(est, metas, use_graph=True)
        outs = []
        with torch.no_grad():
            for left, right in _frames():
                dl = ops.preprocess(torch.from_numpy(left).to(DEV), bgr=False)
                dr = ops.preprocess(torch.from_numpy(right).to(DEV), bgr=False)
                disp = runner.step(dl, dr).clone()
                Ts = runner.last.get("Ts")
                outs.append((disp, None if Ts is None else Ts.clone()))
        torch.cuda.synchronize()
        est.reset_inference_state()
        _CACHE["parent"] = outs
    return _CACHE["parent"]


def _session(**kw):
    from codd_amd.live import LiveSession
    return LiveSession(_estimator(), (H0, W0), intrinsics=INTRINSICS, calib=CALIB, output="depth", bgr=False, **kw)


def _plain_results():
    """The results of a motion=None session on the same frames."""
    if "plain" not in _CACHE:
        s = _session()
        _CACHE["plain"] = [s.step(left, right) for left, right in _frames()]
        s.reset()
        s.close()
    return _CACHE["plain"]


def _equal_nan(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b, equal_nan=True))


@pytest.mark.parametrize("mode", lm.MODES)
def test_session_motion_against_the_existing_route(mode):
    from codd_amd import ops
    parent, plain = _parent_route(), _plain_results()
    bf = lm.bf_of(INTRINSICS[0])
    K = [float(np.float32(v)) for v in INTRINSICS]
    s = _session(motion=mode)
    marks, first = {}, []
    for i, (left, right) in enumerate(_frames()):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 2
        res, motion = got
        torch.cuda.synchronize()
        marks[i + 1] = torch.cuda.memory_allocated()
        first.append(motion)
        assert isinstance(plain[i], np.ndarray) and np.array_equal(res, plain[i]), f"frame {i}: the result changed"
        if i == 0:
            assert motion is None and parent[0][1] is None
            continue
        assert isinstance(motion, np.ndarray) and motion.dtype == np.float32 and motion.flags["OWNDATA"]
        assert motion.shape == (H0, W0, lm.CHANNELS[mode])
        Ts = parent[i][1]
        depth_prev = ops.disp_to_depth(parent[i - 1][0], bf)[:, 0].cpu()  # (no device tensor of the test's stays alive)
        ref = lm.reference(Ts.cpu(), depth_prev, K, bf, CALIB / bf)
        r = lm.compare(torch.from_numpy(motion), ref, mode, H0, W0, f"session frame {i}")
        lm.within(r, 1.0, f"{mode} frame {i}")
    print("memory_allocated per frame:", marks)
    assert marks[3] == marks[6]  # nothing is allocated per frame
    graph = s.runner.graph
    assert graph is not None
    # a new sequence, pipelined: the first frame has no field again, the others repeat the first run's bits
    s.reset()
    second = []
    for left, right in _frames():
        s.push(left.copy(), right.copy())
        if s.pending() == 2:
            second.append(s.pop())
    while s.pending():
        second.append(s.pop())
    assert len(second) == FRAMES and second[0][1] is None
    for i in range(FRAMES):
        assert np.array_equal(second[i][0], plain[i]), f"pipelined frame {i}: the result differs"
        assert _equal_nan(second[i][1], first[i]), f"pipelined frame {i} after reset(): motion differs from step()'s"
    assert s.runner.graph is graph  # no re-capture
    s.reset()
    s.close()


def test_cli_live_motion(tmp_path):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 6
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(_frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    common = ["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
              "--show", "--live"]
    inference.main(common + ["--show-dir", str(tmp_path / "plain")])
    inference.main(common + ["--show-dir", str(tmp_path / "motion"), "--motion", "sceneflow"])
    assert not os.path.exists(tmp_path / "plain" / "left.motion.pred.npz")
    a = np.load(tmp_path / "plain" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "motion" / "left.disp.pred.npz")["disp"]
    assert a.shape == b.shape == (1, n, h, w) and np.array_equal(a, b)  # the disparity file is unchanged
    z = np.load(tmp_path / "motion" / "left.motion.pred.npz")
    assert z.files == ["motion"]
    m = z["motion"]
    assert m.shape == (1, n, h, w, 3) and m.dtype == np.float32
    assert bool(np.isnan(m[0, 0]).all())  # a frame without a field
    s = LiveSession(_estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, motion="sceneflow")
    for i, (left, right) in enumerate(_frames(h, w, n)):
        res, motion = s.step(left, right)
        assert np.array_equal(res, a[0, i])
        if i:
            assert np.array_equal(motion, m[0, i], equal_nan=True) and bool(np.isfinite(motion).any())
        else:
            assert motion is None
    s.reset()
    s.close()
