"""LiveSession stereo confidence on the GPU: codd_export_confidence against the restatement of tests/live_conf_ref.py
(exact flag bits, the residual within its bound, the MISMATCH rule; determinism, padding, guard regions, unaligned
pointers, the image-free call, the longest supported row), LiveSession(confidence=...) against the kernel called directly
on the disparity and images of the route a user had to write, and the --live --confidence command line.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_conf_ref as lc  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every output
_CACHE = {}
case_id = lambda s: "%dx%d" % s[0]  # noqa: E731


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _case(shape):
    """(inputs, reference with images, reference without), computed once and never modified."""
    if shape not in _CACHE:
        c = lc.case(shape)
        _CACHE[shape] = (c, lc.reference(c), lc.reference(c, images=False))
    return _CACHE[shape]


class Run:
    """One call of ops.export_confidence on the case ``c``: both outputs between guard regions; ``off`` shifts the flags
    by that many bytes and every fp32 pointer by that many floats off a 16-byte boundary."""

    def __init__(self, c, images=True, residual=True, off=0, **over):
        from codd_amd import ops
        (h, w), (H, W) = c["crop"], c["padded"]
        src = {k: torch.from_numpy(np.ascontiguousarray(over.get(k, c[k]))) for k in ("disp", "left", "right")}
        self.off, self.h, self.w = off, h, w
        self.inp, self.inp0 = {}, {}
        for k, t in src.items():
            buf = torch.zeros(t.numel() + 4, device=DEV)
            self.inp[k] = buf[off:off + t.numel()].view(t.shape)
            self.inp[k].copy_(t)
            self.inp0[k] = self.inp[k].clone()
        self.bflags = torch.full((h * w + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        self.bres = torch.full((h * w + 2 * GUARD,), -7.0, device=DEV)
        self.flags = self.bflags[GUARD + off:GUARD + off + h * w].view(h, w)
        self.res = self.bres[GUARD + off:GUARD + off + h * w].view(h, w) if residual and images else None
        assert self.bflags.data_ptr() % 16 == 0 and self.bres.data_ptr() % 16 == 0 and self.inp["disp"].data_ptr() % 16 == 4 * off
        ops.export_confidence(self.inp["disp"], self.flags, self.res, self.inp["left"] if images else None,
                              self.inp["right"] if images else None, occ_px=lc.OCC_PX, tau=lc.TAU)
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        n, lo = self.h * self.w, GUARD + self.off
        assert bool((self.bflags[:lo] == 0x5A).all()) and bool((self.bflags[lo + n:] == 0x5A).all()), f"{what}: flags guard overwritten"
        if self.res is None:
            assert bool((self.bres == -7.0).all()), f"{what}: no residual asked for and its buffer was written"
        else:
            assert bool((self.bres[:lo] == -7.0).all()) and bool((self.bres[lo + n:] == -7.0).all()), f"{what}: residual guard overwritten"
        for k in self.inp:
            assert torch.equal(glm._bits(self.inp[k]), glm._bits(self.inp0[k])), f"{what}: input {k} was modified"

    def outputs(self):
        return self.flags.cpu().numpy(), None if self.res is None else self.res.cpu().numpy()

    def same_bytes(self, other):
        return torch.equal(self.flags, other.flags) and (self.res is None or other.res is None or
                                                         torch.equal(glm._bits(self.res), glm._bits(other.res)))


@pytest.mark.parametrize("shape", lc.CASES, ids=case_id)
def test_confidence_against_reference(shape):
    c, ref, _ = _case(shape)
    name = case_id(shape)
    a = Run(c)
    a.check_guards(name)
    flags, res = a.outputs()
    print(name, "pixels per flag (1, 2, 4, 128):", [int(((flags & b) != 0).sum()) for b in (1, 2, 4, 128)],
          "undecided:", int((~ref["decided"]).sum()))
    lc.check_outputs(flags, res, ref, name=name)
    if shape[0][1] >= 32:  # (the 5x3 and 3x1 crops have fewer than 3 x 8 pixels: tests/test_live_conf.py)
        for b in (lc.OUT_OF_VIEW, lc.OCCLUDED, lc.MISMATCH, lc.INVALID):
            assert int(((flags & b) != 0).sum()) >= 8, f"{name}: fewer than 8 pixels with flag {b}"
    # determinism: a second run gives equal bytes
    b = Run(c)
    assert a.same_bytes(b) and b.res is not None


@pytest.mark.parametrize("shape", lc.CASES[:4], ids=case_id)
def test_padding_influences_no_output_byte(shape):
    c, _, _ = _case(shape)
    h, w = c["crop"]
    over = {}
    for k, fill in (("disp", 99.0), ("left", float("nan")), ("right", -777.0)):
        t = c[k].copy()
        t[..., h:, :] = fill
        t[..., :, w:] = fill
        over[k] = t
    a, b = Run(c), Run(c, **over)
    assert not torch.equal(glm._bits(a.inp["disp"]), glm._bits(b.inp["disp"]))
    b.check_guards("padding")
    assert a.same_bytes(b)


@pytest.mark.parametrize("shape", (lc.CASES[0], lc.CASES[1], lc.CASES[3]), ids=case_id)
def test_confidence_unaligned_views(shape):
    """flags 1, 2, 3 bytes and every fp32 pointer 4, 8, 12 bytes off a 16-byte boundary: the bytes of the aligned run,
    and nothing is written outside the views."""
    c, _, _ = _case(shape)
    want = Run(c)
    for off in (1, 2, 3):
        got = Run(c, off=off)
        assert got.flags.data_ptr() % 4 == off and got.res.data_ptr() % 16 == 4 * off
        assert all(got.inp[k].data_ptr() % 16 == 4 * off for k in got.inp)
        got.check_guards(f"offset {off}")
        assert want.same_bytes(got), f"offset {off}: bytes differ from the aligned run"


@pytest.mark.parametrize("shape", lc.CASES, ids=case_id)
def test_confidence_without_images(shape):
    c, ref, ref_noimg = _case(shape)
    a = Run(c, images=False)
    a.check_guards("no images")
    flags, res = a.outputs()
    assert res is None
    lc.check_outputs(flags, None, ref_noimg, name="no images")  # bits 1, 2, 128 exact, bit 4 never
    assert np.array_equal(flags, ref["flags124"])
    # with images but without the residual map: the flags of the full call, the map's buffer untouched
    b, full = Run(c, residual=False), Run(c)
    b.check_guards("residual=None")
    assert torch.equal(b.flags, full.flags)


def test_longest_supported_row():
    """w = CODD_CONF_MAX_W = 8192: the whole 64 KiB of LDS a workgroup may use."""
    h, w = 2, 8192
    rng = np.random.default_rng(5)
    disp = (np.round(4 * rng.uniform(0.25, 40.0, (h, w))) / 4).astype(np.float32)
    disp[0, 4000:4100] = 90.0
    img = rng.uniform(-2, 2, (2, 3, h, w)).astype(np.float32)
    c = dict(disp=disp, left=img[0], right=img[1], crop=(h, w), padded=(h, w))
    ref = lc.reference(c)
    a = Run(c)
    a.check_guards("w=8192")
    lc.check_outputs(*a.outputs(), ref, name="w=8192")
    assert int((ref["flags124"] & lc.OCCLUDED != 0).sum()) >= 8


# ---- the session against the kernel on the tensors of the existing route ----------------------------------------
def _same_conf(a, b):
    return np.array_equal(a.flags, b.flags) and np.array_equal(a.residual, b.residual, equal_nan=True)


def test_session_confidence_against_the_existing_route():
    from codd_amd import live, ops
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()
    s = glm._session(confidence=True)
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
    for i, (left, right) in enumerate(frames):  # frame 0 included: no motion stage is needed
        c = first[i]
        assert isinstance(c, live.Confidence)
        assert c.flags.dtype == np.uint8 and c.flags.shape == (glm.H0, glm.W0) and c.flags.flags["OWNDATA"]
        assert c.residual.dtype == np.float32 and c.residual.shape == (glm.H0, glm.W0) and c.residual.flags["OWNDATA"]
        # the kernel called directly on the cloned disparity and the images ops.preprocess makes: equal bytes
        dl = ops.preprocess(torch.from_numpy(left).to(DEV), bgr=False)
        dr = ops.preprocess(torch.from_numpy(right).to(DEV), bgr=False)
        flags = torch.empty(glm.H0, glm.W0, dtype=torch.uint8, device=DEV)
        res = torch.empty(glm.H0, glm.W0, device=DEV)
        ops.export_confidence(parent[i][0], flags, res, dl, dr)
        assert np.array_equal(c.flags, flags.cpu().numpy()), f"frame {i}: flags differ from the direct call"
        assert np.array_equal(c.residual, res.cpu().numpy(), equal_nan=True), f"frame {i}: residual differs"
        assert bool((np.isnan(c.residual) == ((c.flags & 0x81) != 0)).all())
        print(f"frame {i}: pixels per flag (1, 2, 4, 128):", [int(((c.flags & b) != 0).sum()) for b in (1, 2, 4, 128)])
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
        assert _same_conf(second[i][1], first[i]), f"pipelined frame {i} after reset(): confidence differs from step()'s"
    assert s.runner.graph is graph  # no re-capture
    s.reset()
    s.close()
    # with motion= and egomotion= as well: (result, motion, ego, confidence), the first three with the bits of a session
    # without the option
    import test_gpu_live_ego as gle
    both = glm._session(motion="sceneflow", egomotion=True, confidence=dict(occ_px=1.0, tau=24.0))
    only = glm._session(motion="sceneflow", egomotion=True)
    for i, (left, right) in enumerate(frames):
        got = both.step(left, right)
        assert isinstance(got, tuple) and len(got) == 4
        res, motion, ego, conf = got
        res1, motion1, ego1 = only.step(left, right)
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i])
        assert glm._equal_nan(motion, motion1), f"frame {i}: the motion output changed"
        assert gle._same_ego(ego, ego1), f"frame {i}: the ego output changed"
        assert _same_conf(conf, first[i]), f"frame {i}: confidence differs with motion= and egomotion= set"
    for t in (both, only):
        t.reset()
        t.close()


def test_cli_live_confidence(tmp_path):
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
    inference.main(common + ["--show-dir", str(tmp_path / "conf"), "--confidence"])
    assert sorted(os.listdir(tmp_path / "plain")) == ["left.disp.pred.npz"]  # no such file without the flag
    assert sorted(os.listdir(tmp_path / "conf")) == ["left.conf.pred.npz", "left.disp.pred.npz"]
    a = np.load(tmp_path / "plain" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "conf" / "left.disp.pred.npz")["disp"]
    assert a.shape == b.shape == (1, n, h, w) and np.array_equal(a, b)  # the disparity file is unchanged
    z = np.load(tmp_path / "conf" / "left.conf.pred.npz")
    assert sorted(z.files) == ["flags", "residual"]
    flags, residual = z["flags"], z["residual"]
    assert flags.shape == (1, n, h, w) and flags.dtype == np.uint8
    assert residual.shape == (1, n, h, w) and residual.dtype == np.float32
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, confidence=True)
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        res, conf = s.step(left, right)
        assert np.array_equal(res, a[0, i])
        assert np.array_equal(conf.flags, flags[0, i]) and np.array_equal(conf.residual, residual[0, i], equal_nan=True)
    s.reset()
    s.close()
