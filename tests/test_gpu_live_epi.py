"""LiveSession rectification health check on the GPU: codd_epipolar_check against the restatement of tests/live_epi_ref.py
(the measurable mask exact outside the undecided pixels, dy and the coefficients within K_DEV x the deviation of the fp32
restatement from the fp64 reference, the record against the fit of the kernel's own map; determinism, padding, guard
regions, unaligned pointers, the call without a map), LiveSession(epipolar=...) against the kernel called directly on the
disparity and images of the route a user had to write, and the --live --epipolar command line.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_epi_ref as le  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every output
K_DEV = 5.0  # x the restatement's own deviation (finding 85)
REL = 1e-9  # the record against the fit of the kernel's own map: sums in another order only
_CACHE = {}
IDS = [le.case_id(s) for s in le.CASES]


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _case(i):
    """(inputs, reference), computed once and never modified."""
    if i not in _CACHE:
        c = le.case(le.CASES[i])
        _CACHE[i] = (c, le.reference(c))
    return _CACHE[i]


class Run:
    """One call of ops.epipolar_check on the case ``c``: record, map and scratch between guard regions; ``off`` shifts every
    fp32 pointer by that many floats off a 16-byte boundary and the scratch by as many bytes."""

    def __init__(self, c, with_map=True, off=0, **over):
        from codd_amd import ops
        h, w = c["crop"]
        src = {k: torch.from_numpy(np.ascontiguousarray(over.get(k, c[k]))) for k in ("disp", "left", "right")}
        self.off, self.h, self.w = off, h, w
        self.inp, self.inp0 = {}, {}
        for k, t in src.items():
            buf = torch.zeros(t.numel() + 4, device=DEV)
            self.inp[k] = buf[off:off + t.numel()].view(t.shape)
            self.inp[k].copy_(t)
            self.inp0[k] = self.inp[k].clone()
        self.brec = torch.full((32 + 2 * GUARD,), -7.0, dtype=torch.float64, device=DEV)
        self.bmap = torch.full((h * w + 2 * GUARD,), -7.0, device=DEV)
        n = ops.epipolar_scratch(h, w)
        self.bscr = torch.full((n + 2 * GUARD + 4,), 0x5A, dtype=torch.uint8, device=DEV)
        self.rec = self.brec[GUARD:GUARD + 32]
        self.map = self.bmap[GUARD + off:GUARD + off + h * w].view(h, w) if with_map else None
        self.scr = self.bscr[GUARD + off:GUARD + off + n]
        assert self.bmap.data_ptr() % 16 == 0 and self.inp["disp"].data_ptr() % 16 == 4 * off
        ops.epipolar_check(self.inp["disp"], self.inp["left"], self.inp["right"], c["K"], (h, w), self.rec, self.map,
                           scratch=self.scr, **c["par"])
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        n, lo = self.h * self.w, GUARD + self.off
        assert bool((self.brec[:GUARD] == -7.0).all()) and bool((self.brec[GUARD + 32:] == -7.0).all()), f"{what}: record guard overwritten"
        if self.map is None:
            assert bool((self.bmap == -7.0).all()), f"{what}: no map asked for and its buffer was written"
        else:
            assert bool((self.bmap[:lo] == -7.0).all()) and bool((self.bmap[lo + n:] == -7.0).all()), f"{what}: map guard overwritten"
        ns = self.scr.numel()
        assert bool((self.bscr[:lo] == 0x5A).all()) and bool((self.bscr[lo + ns:] == 0x5A).all()), f"{what}: scratch guard overwritten"
        for k in self.inp:
            assert torch.equal(glm._bits(self.inp[k]), glm._bits(self.inp0[k])), f"{what}: input {k} was modified"

    def outputs(self):
        return self.rec.cpu().numpy().copy(), None if self.map is None else self.map.cpu().numpy()

    def same_bytes(self, other):
        return torch.equal(self.rec.view(torch.int64), other.rec.view(torch.int64)) and (
            self.map is None or other.map is None or torch.equal(glm._bits(self.map), glm._bits(other.map)))


@pytest.mark.parametrize("i", range(len(le.CASES)), ids=IDS)
def test_epipolar_against_reference(i):
    from codd_amd import live
    c, ref = _case(i)
    name = IDS[i]
    a = Run(c)
    a.check_guards(name)
    rec, dy = a.outputs()
    assert np.isfinite(rec).all() and not rec[24:].any()
    got = live.epipolar_from_record(rec)
    und, m64 = ref["undecided"], ref["measurable64"]
    meas = ~np.isnan(dy)
    print(f"{name}: measurable gpu {int(meas.sum())} / fp64 {int(m64.sum())}, undecided {int(und.sum())}; dev dy {ref['dev_dy']:.3e}, "
          f"dev coef {ref['dev_coef']:.3e}; record {rec[:10].tolist()}")
    # the measurable mask: exact outside the undecided pixels; the counts with it
    assert np.array_equal(meas[~und], m64[~und]), f"{name}: measurable mask differs at {np.argwhere((meas != m64) & ~und)[:8].tolist()}"
    assert abs(got.valid - int(m64.sum())) <= int(und.sum()) and got.valid == int(meas.sum())
    if c["crop"] == (5, 3):  # nothing measurable: ok = 0, a finite zero record, an all-NaN map
        assert not meas.any() and not got.ok and not rec.any()
        return
    both = meas & m64 & ~und
    err = float(np.abs(dy.astype(np.float64) - ref["m64"]["dy"])[both].max())
    same32 = np.array_equal(dy, ref["m32"]["dy"], equal_nan=True)
    print(f"  max |dy - fp64 reference| {err:.3e} (bound {K_DEV * ref['dev_dy']:.3e}); equal to the fp32 restatement bit for bit: {same32}")
    assert err <= K_DEV * ref["dev_dy"]
    # the record against the header's fit (fp32 terms, fp64 sums) of the kernel's OWN map: only the order of the sums differs
    own = le.fit(c, dy, np.float32)
    scale = np.abs(own["coef"]).max()
    print(f"  record vs fit of its own map: coef {np.abs(got.coef - own['coef']).max() / scale:.3e} relative; "
          f"vs fp64 reference {np.abs(got.coef - ref['f64']['coef']).max():.3e} (bound {K_DEV * ref['dev_coef']:.3e})")
    assert got.ok == own["ok"] == ref["f64"]["ok"] and rec[9] == own["steps"]
    assert np.abs(got.coef - own["coef"]).max() <= REL * scale
    assert np.abs(got.A - own["A"]).max() <= REL * np.abs(own["A"]).max() and np.abs(got.b - own["b"]).max() <= REL * np.abs(own["b"]).max()
    assert abs(got.rms_px - own["rms"]) <= REL * own["rms"]
    # inliers: exact unless a pixel's |e| sits within the coefficient tolerance of delta
    _, _, _, p, e = le.terms(c, dy, own["coef"], np.float32)
    near = int((np.abs(np.abs(e) - c["par"]["delta_px"]) <= 1e-6).sum())
    assert abs(got.inliers - own["inliers"]) <= near
    if near == 0:
        assert abs(got.rms_fit_px - own["rms_fit"]) <= REL * max(own["rms_fit"], 1e-12)
    # and against the fp64 reference's coefficients, by the same k x rule
    assert np.abs(got.coef - ref["f64"]["coef"]).max() <= K_DEV * ref["dev_coef"]
    # determinism: a second run gives equal bytes
    assert a.same_bytes(Run(c))


@pytest.mark.parametrize("i", (0, 1, 4, 5), ids=[IDS[k] for k in (0, 1, 4, 5)])
def test_padding_influences_no_output_byte(i):
    c, _ = _case(i)
    h, w = c["crop"]
    a = Run(c)
    for fills in ((99.0, float("nan"), -777.0), (float("nan"), -777.0, 99.0), (-777.0, 99.0, float("nan"))):
        over = {}
        for k, fill in zip(("disp", "left", "right"), fills):
            t = c[k].copy()
            t[..., h:, :] = fill
            t[..., :, w:] = fill
            over[k] = t
        b = Run(c, **over)
        b.check_guards("padding")
        assert a.same_bytes(b), f"padding {fills} changed an output byte"


@pytest.mark.parametrize("i", (0, 2, 3), ids=[IDS[k] for k in (0, 2, 3)])
def test_epipolar_unaligned_views_and_no_map(i):
    """Every fp32 pointer 4, 8, 12 bytes off a 16-byte boundary: the bytes of the aligned run, nothing written outside the
    views; without a map the record has the same bytes and the map's buffer is untouched."""
    c, _ = _case(i)
    want = Run(c)
    want.check_guards("aligned")
    for off in (1, 2, 3):
        got = Run(c, off=off)
        assert got.map.data_ptr() % 16 == 4 * off and all(got.inp[k].data_ptr() % 16 == 4 * off for k in got.inp)
        got.check_guards(f"offset {off}")
        assert want.same_bytes(got), f"offset {off}: bytes differ from the aligned run"
    nomap = Run(c, with_map=False, off=1)
    nomap.check_guards("dy_map=None")
    assert nomap.same_bytes(want)


def test_ops_reject_bad_arguments():
    from codd_amd import _abi, ops
    c, _ = _case(0)
    with pytest.raises(ValueError):
        ops.epipolar_scratch(0, 5)
    a = Run(c)
    for bad in (dict(range_px=5), dict(step=0), dict(iters=33), dict(delta_px=0.0), dict(tau=float("nan"))):
        before = a.rec.clone()
        with pytest.raises(_abi.CoddHipError):
            ops.epipolar_check(a.inp["disp"], a.inp["left"], a.inp["right"], c["K"], c["crop"], a.rec, None, scratch=a.scr,
                               **dict(c["par"], **bad))
        assert torch.equal(before, a.rec)
    with pytest.raises(_abi.CoddHipError):  # scratch too small
        ops.epipolar_check(a.inp["disp"], a.inp["left"], a.inp["right"], c["K"], c["crop"], a.rec, None, scratch=a.scr[:-1],
                           **c["par"])


# ---- the session against the kernel on the tensors of the existing route ----------------------------------------
def _same_epi(a, b):
    return (a.coef.tobytes() == b.coef.tobytes() and a.ok == b.ok and (a.valid, a.inliers) == (b.valid, b.inliers)
            and (a.rms_px, a.rms_fit_px) == (b.rms_px, b.rms_fit_px) and a.A.tobytes() == b.A.tobytes()
            and a.b.tobytes() == b.b.tobytes() and glm._equal_nan(a.dy, b.dy))


def test_session_epipolar_against_the_existing_route():
    from codd_amd import calibration, live, ops
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()
    s = glm._session(epipolar=dict(map=True))
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
        e = first[i]
        assert isinstance(e, live.Epipolar) and e.coef.dtype == np.float64 and e.coef.shape == (4,)
        assert e.A.shape == (4, 4) and np.array_equal(e.A, e.A.T) and e.b.shape == (4,)
        assert e.dy.dtype == np.float32 and e.dy.shape == (glm.H0, glm.W0) and e.dy.flags["OWNDATA"]
        # the kernel called directly on the cloned disparity and the images ops.preprocess makes: equal bytes
        dl = ops.preprocess(torch.from_numpy(left).to(DEV), bgr=False)
        dr = ops.preprocess(torch.from_numpy(right).to(DEV), bgr=False)
        rec = torch.zeros(32, dtype=torch.float64, device=DEV)
        dy = torch.empty(glm.H0, glm.W0, device=DEV)
        ops.epipolar_check(parent[i][0], dl, dr, glm.INTRINSICS, (glm.H0, glm.W0), rec, dy)
        want = live.epipolar_from_record(rec.cpu().numpy(), dy.cpu().numpy())
        assert _same_epi(e, want), f"frame {i}: Epipolar differs from the direct call"
        assert e.valid == int((~np.isnan(e.dy)).sum())
        print(f"frame {i}: measurable {e.valid}, inliers {e.inliers}, ok {e.ok}, rms {e.rms_px:.3f} px, coef {e.coef.tolist()}")
    coef, ok = live.combine_epipolar(first)
    print("combined:", coef.tolist(), ok)
    assert coef.shape == (4,) and np.isfinite(coef).all()
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
        assert _same_epi(second[i][1], first[i]), f"pipelined frame {i} after reset(): Epipolar differs from step()'s"
    assert s.runner.graph is graph  # no re-capture
    s.reset()
    s.close()
    assert s._d_epi is None and s._h_epi is None and s._epi_scratch is None
    # with every other option as well: (result, motion, ego, confidence, aligned, epipolar), the first five with the bits
    # of a session without the option; no map asked for: dy is None
    import test_gpu_live_ego as gle
    target = calibration.AlignTarget(calibration.CameraModel((100, 150), (500.0, 500.0, 75.0, 50.0)), np.eye(3), [0.01, 0.0, 0.0])
    kw = dict(motion="sceneflow", egomotion=True, confidence=True, align_to=target)
    both, only = glm._session(epipolar=True, **kw), glm._session(**kw)
    for i, (left, right) in enumerate(frames):
        got = both.step(left, right)
        assert isinstance(got, tuple) and len(got) == 6
        res, motion, ego, conf, al, epi = got
        res1, motion1, ego1, conf1, al1 = only.step(left, right)
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i])
        assert glm._equal_nan(motion, motion1), f"frame {i}: the motion output changed"
        assert gle._same_ego(ego, ego1), f"frame {i}: the ego output changed"
        assert np.array_equal(conf.flags, conf1.flags) and np.array_equal(conf.residual, conf1.residual, equal_nan=True)
        assert np.array_equal(al.depth, al1.depth) and al.uv is None and al1.uv is None
        assert isinstance(epi, live.Epipolar) and epi.dy is None
        assert _same_epi(epi._replace(dy=first[i].dy), first[i]), f"frame {i}: Epipolar differs with every option set"
    for t in (both, only):
        t.reset()
        t.close()


def test_cli_live_epipolar(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference, live
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 6
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    common = ["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
              "--show", "--live"]
    inference.main(common + ["--show-dir", str(tmp_path / "plain")])
    assert "epipolar:" not in capsys.readouterr().out
    inference.main(common + ["--show-dir", str(tmp_path / "epi"), "--epipolar"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "epipolar:" in ln]
    assert len(lines) == 1 and "millidegrees" in lines[0] and "vertical disparity" in lines[0]
    assert sorted(os.listdir(tmp_path / "plain")) == ["left.disp.pred.npz"]  # no such file without the flag
    assert sorted(os.listdir(tmp_path / "epi")) == ["left.disp.pred.npz", "left.epi.pred.npz"]
    a = np.load(tmp_path / "plain" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "epi" / "left.disp.pred.npz")["disp"]
    assert a.shape == b.shape == (1, n, h, w) and np.array_equal(a, b)  # the disparity file is unchanged
    z = np.load(tmp_path / "epi" / "left.epi.pred.npz")
    assert sorted(z.files) == ["A", "b", "coef", "combined", "combined_ok", "stats"]
    assert z["coef"].shape == (1, n, 4) and z["stats"].shape == (1, n, 5) and z["A"].shape == (1, n, 4, 4) and z["b"].shape == (1, n, 4)
    assert z["combined"].shape == (4,) and z["combined_ok"].shape == ()
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, epipolar=True)
    epis = []
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        res, e = s.step(left, right)
        epis.append(e)
        assert np.array_equal(res, a[0, i])
        assert np.array_equal(e.coef, z["coef"][0, i]) and np.array_equal(e.A, z["A"][0, i]) and np.array_equal(e.b, z["b"][0, i])
        assert z["stats"][0, i].tolist() == [e.ok, e.valid, e.inliers, e.rms_px, e.rms_fit_px]
    coef, ok = live.combine_epipolar(epis)
    assert np.array_equal(coef, z["combined"]) and bool(z["combined_ok"]) == ok
    s.reset()
    s.close()
