"""Live stereo session on the GPU: the ingest and export kernels against ops.preprocess / torch / the fp64 restatements
of tests/live_ref.py, and LiveSession against the route a user had to write before it existed
(torch.from_numpy(...).to(dev) -> ops.preprocess -> FrameRunner(use_graph=True).step -> crop).  Autotune is off in
every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [((540, 960), (576, 960)), ((375, 1242), (384, 1280)), ((37, 53), (64, 64))]
# Tolerance of the rectified ingest, derived (not measured): the bilinear blend is at most eight roundings of values
# <= 255, each <= 255 * 2^-24 -> 1.2e-4 in pixel units, divided by std >= 57 -> 2.2e-6, plus the normalisation's own two
# roundings on |v| < 2.7 (2 * 2.7 * 2^-24 = 3.2e-7): 1e-5 absolute in normalised units covers it with margin.
RECT_TOL = 1e-5


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _images(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _ingest(left, right, H, W, bgr, maps=None):
    from codd_amd import ops
    ol, orr = (torch.full((1, 3, H, W), float("nan"), device=DEV) for _ in range(2))
    dm = None
    if maps is not None:
        dm = tuple(None if p is None else tuple(torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in p) for p in maps)
    ops.ingest_pair(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), ol, orr, bgr=bgr, maps=dm)
    torch.cuda.synchronize()
    return ol, orr


def _q64(a):
    """Round to multiples of 1/64 (exact in fp32 at these magnitudes): the fp64 restatement sees the kernel's weights."""
    return (np.round(np.asarray(a, np.float64) * 64.0) / 64.0).astype(np.float32)


def _maps(kind, h, w):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if kind == "identity":
        return xx.astype(np.float32), yy.astype(np.float32)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    if kind == "radial":  # smooth barrel distortion, up to ~4 px at the corners
        r2 = ((xx - cx) ** 2 + (yy - cy) ** 2) / (cx * cx + cy * cy)
        return _q64(xx + 4.0 * r2 * (xx - cx) / max(cx, 1.0)), _q64(yy + 4.0 * r2 * (yy - cy) / max(cy, 1.0))
    assert kind == "leaving"  # 1.25x zoom-out about the centre plus a shift: leaves the source on all four sides
    mx, my = _q64(cx + 1.25 * (xx - cx) + 0.375), _q64(cy + 1.25 * (yy - cy) - 0.640625)
    assert mx.min() < -1 and mx.max() > w and my.min() < -1 and my.max() > h
    mx[h // 2, w // 3], my[h // 3, w // 2], mx[1, 1] = np.nan, np.inf, -np.inf  # non-finite entries give 0
    return mx, my


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_ingest_pair_is_bit_identical_to_preprocess(shape, bgr):
    from codd_amd import ops
    (h, w), (H, W) = shape
    left, right = _images(h, w, 1)
    ol, orr = _ingest(left, right, H, W, bgr)
    assert torch.equal(ol, ops.preprocess(torch.from_numpy(left).to(DEV), bgr=bgr))
    assert torch.equal(orr, ops.preprocess(torch.from_numpy(right).to(DEV), bgr=bgr))


def test_ingest_pair_unaligned_views():
    """Source pointers that are not dword-aligned and an output that is not 16-byte aligned take the scalar paths and
    give the same bits."""
    from codd_amd import ops
    (h, w), (H, W) = SHAPES[2]
    left, right = _images(h, w, 2)
    bufl, bufr = (torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device=DEV) for _ in range(2))
    dl, dr = bufl[1:1 + h * w * 3].view(h, w, 3), bufr[3:3 + h * w * 3].view(h, w, 3)
    dl.copy_(torch.from_numpy(left))
    dr.copy_(torch.from_numpy(right))
    obuf = torch.zeros(2 * 3 * H * W + 8, device=DEV)
    ol, orr = obuf[1:1 + 3 * H * W].view(1, 3, H, W), obuf[3 * H * W + 2:2 * 3 * H * W + 2].view(1, 3, H, W)
    ops.ingest_pair(dl, dr, ol, orr, bgr=False)
    assert torch.equal(ol, ops.preprocess(torch.from_numpy(left).to(DEV), bgr=False))
    assert torch.equal(orr, ops.preprocess(torch.from_numpy(right).to(DEV), bgr=False))
    assert obuf[0] == 0 and obuf[3 * H * W + 1] == 0 and bool((obuf[2 * 3 * H * W + 2:] == 0).all())  # nothing written outside


@pytest.mark.parametrize("kind", ["identity", "radial", "leaving"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_ingest_pair_rectified_matches_fp64_restatement(shape, kind):
    (h, w), (H, W) = shape
    left, right = _images(h, w, 3)
    lm = _maps(kind, h, w)
    rm = tuple(np.ascontiguousarray(m[::-1, ::-1]) for m in lm) if kind != "identity" else lm  # another map for the right view
    for bgr in (True, False):
        ol, orr = _ingest(left, right, H, W, bgr, maps=(lm, rm))
        worst = 0.0
        for got, img, m in ((ol, left, lm), (orr, right, rm)):
            ref = live_ref.ingest(img, H, W, bgr, maps=m)
            worst = max(worst, float(np.abs(got[0].cpu().numpy().astype(np.float64) - ref).max()))
        print(f"rectified ingest {h}x{w} {kind} bgr={bgr}: max |delta| = {worst:.3e} (bound {RECT_TOL:g})")
        assert worst <= RECT_TOL
        if kind == "identity":  # the identity map gives the bits of the map-free path
            pl, pr = _ingest(left, right, H, W, bgr)
            assert torch.equal(ol, pl) and torch.equal(orr, pr)
    # maps for one view only: the other view takes the map-free path
    ol, orr = _ingest(left, right, H, W, False, maps=(None, rm))
    pl, _ = _ingest(left, right, H, W, False)
    assert torch.equal(ol, pl)
    assert float(np.abs(orr[0].cpu().numpy().astype(np.float64) - live_ref.ingest(right, H, W, False, maps=rm)).max()) <= RECT_TOL


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_export_depth_modes(shape):
    from codd_amd import ops
    (h, w), (H, W) = shape
    g = torch.Generator().manual_seed(4)
    disp = (torch.rand(1, 1, H, W, generator=g) * 300.0 + 0.01).to(DEV)
    # mode 0: the crop
    out = torch.full((h, w), float("nan"), device=DEV)
    ops.export_depth(disp, out, "disp")
    assert torch.equal(out, disp[0, 0, :h, :w])
    # mode 1: within 1 ulp of torch's `calib / disp`.  Seen on the MI355X: EQUAL at all three shapes -- torch evaluates a Python
    # scalar over a tensor as reciprocal() * scalar and the kernel rounds twice the same way (a single correctly rounded
    # division differed by 1 ulp in 27 % of the values)
    calib = 210.0
    ops.export_depth(disp, out, "depth", calib=calib)
    ref = calib / disp[0, 0, :h, :w]
    ulps = (out.view(torch.int32).long() - ref.contiguous().view(torch.int32).long()).abs()
    print(f"export depth {h}x{w}: {int((ulps > 0).sum())} of {h * w} values differ from torch's calib / disp, max {int(ulps.max())} ulp")
    assert int(ulps.max()) <= 1
    # mode 2: uint16 disp * 256 on a map with the awkward values
    special = torch.tensor([0.0, 255.998, 300.0, float("inf"), float("nan"), -3.0, float("-inf"), 0.5 / 256, 1.5 / 256,
                            2.5 / 256, 100.5 / 256, 101.5 / 256, 65535.5 / 256, 65534.5 / 256, 1e30], device=DEV)
    d2 = disp.clone()
    d2[0, 0, 0, :special.numel()] = special
    d2[0, 0, h - 1, w - special.numel():w] = special
    q = torch.zeros(h, w, dtype=torch.int16, device=DEV)
    ops.export_depth(d2, q, "disp_u16")
    got = q.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, live_ref.export(d2[0, 0].cpu().numpy(), h, w, "disp_u16"))
    assert got[0, :special.numel()].tolist() == [0, 65535, 65535, 0, 0, 0, 0, 0, 2, 2, 100, 102, 65535, 65534, 65535]


# ---- the session against the route it replaces -----------------------------------------------------------------
H0, W0, FRAMES = 540, 960, 8
_CACHE = {}


def _frames(h=H0, w=W0, n=FRAMES):
    """``n`` frames of synth.stereo_sequence quantised to uint8 HWC (RGB)."""
    if (h, w, n) not in _CACHE:
        from codd_amd import synth
        img, r_img, _ = synth.stereo_sequence(h, w, n)

        def u8(t):
            return np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())

        _CACHE[(h, w, n)] = [(u8(img[0, i]), u8(r_img[0, i])) for i in range(n)]
    return _CACHE[(h, w, n)]


def _estimator(stereo_only):
    key = ("est", stereo_only)
    if key not in _CACHE:
        import codd_amd  # noqa: F401
        from codd_amd import configs, synth
        from codd_amd.registry import build_estimator
        est = build_estimator(configs.stereo_only() if stereo_only else configs.codd()).eval()
        synth.load_synthetic_weights(est, gain=1.4)
        _CACHE[key] = est.to(DEV)
    return _CACHE[key]


def _parent_route(stereo_only):
    """What a user wrote before LiveSession: blocking uploads, one preprocess per view, FrameRunner.step, crop."""
    key = ("parent", stereo_only)
    if key not in _CACHE:
        from codd_amd import ops, synth
        from codd_amd.runtime import FrameRunner
        est = _estimator(stereo_only)
        H, W = -(-H0 // 64) * 64, -(-W0 // 64) * 64
        runner = FrameRunner(est, synth.default_metas(H, W, img_shape=(H0, W0, 3))[0], use_graph=True)
        outs = []
        with torch.no_grad():
            for left, right in _frames():
                dl = ops.preprocess(torch.from_numpy(left).to(DEV), bgr=False)
                dr = ops.preprocess(torch.from_numpy(right).to(DEV), bgr=False)
                outs.append(runner.step(dl, dr)[0, 0, :H0, :W0].clone())
        torch.cuda.synchronize()
        _CACHE[key] = outs
    return _CACHE[key]


def _session(stereo_only, **kw):
    from codd_amd.live import LiveSession
    return LiveSession(_estimator(stereo_only), (H0, W0), output="disp", bgr=False, **kw)


@pytest.mark.parametrize("stereo_only", [False, True], ids=["codd", "stereo_only"])
def test_session_step_equals_the_existing_path(stereo_only):
    ref = _parent_route(stereo_only)
    s = _session(stereo_only)
    for i, (left, right) in enumerate(_frames()):
        got = s.step(left, right)
        assert isinstance(got, np.ndarray) and got.shape == (H0, W0) and got.dtype == np.float32 and got.flags["OWNDATA"]
        assert torch.equal(torch.from_numpy(got), ref[i].cpu()), f"frame {i} differs from the existing path"
    s.close()


def test_session_pipelined_reset_and_allocation():
    ref = [r.cpu().numpy() for r in _parent_route(False)]
    s = _session(False)
    rng = np.random.default_rng(5)

    def run_pipelined():
        outs = []
        for left, right in _frames():
            a, b = left.copy(), right.copy()
            s.push(a, b)
            a[...] = rng.integers(0, 256, a.shape, dtype=np.uint8)  # the caller's arrays are its own again
            b[...] = 0
            if s.pending() == 2:
                outs.append(s.pop())
        while s.pending():
            outs.append(s.pop())
        with pytest.raises(IndexError):
            s.pop()
        return outs

    first = run_pipelined()
    assert len(first) == FRAMES
    for i in range(FRAMES):
        assert np.array_equal(first[i], ref[i]), f"pipelined frame {i} differs from the existing path"
    graph = s.runner.graph
    assert graph is not None
    s.reset()
    second = run_pipelined()
    for i in range(FRAMES):
        assert np.array_equal(second[i], first[i]), f"frame {i} after reset() differs from the first run"
    assert s.runner.graph is graph  # no re-capture for the second sequence
    # three pushes without a pop: the third parks the oldest result, order is kept
    s.reset()
    for left, right in _frames()[:3]:
        s.push(left, right)
    assert s.pending() == 3
    for i in range(3):
        assert np.array_equal(s.pop(), ref[i])
    # no per-frame allocation: device memory after frame 3 equals device memory after frame 8
    s.reset()
    marks = {}
    for i, (left, right) in enumerate(_frames()):
        s.step(left, right)
        torch.cuda.synchronize()
        marks[i + 1] = torch.cuda.memory_allocated()
    print("memory_allocated per frame:", marks)
    assert marks[3] == marks[8]
    s.close()


def test_session_outputs_depth_and_u16_and_rectified():
    """The other output formats are functions of the same disparity; rectification by an identity map changes nothing."""
    ref = [r.cpu().numpy() for r in _parent_route(True)]
    from codd_amd.live import LiveSession
    est = _estimator(True)
    yy, xx = np.meshgrid(np.arange(H0, dtype=np.float32), np.arange(W0, dtype=np.float32), indexing="ij")
    for output, kw in (("depth", {}), ("disp_u16", {}), ("disp", dict(rectify=((xx, yy), (xx, yy))))):
        s = LiveSession(est, (H0, W0), output=output, calib=210.0, **kw)
        for i, (left, right) in enumerate(_frames()[:3]):
            got = s.step(left, right)
            if output == "depth":
                want = (torch.tensor(210.0) / torch.from_numpy(ref[i]).to(DEV)).cpu().numpy()
                ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
                assert got.dtype == np.float32 and int(ulps.max()) <= 1
            elif output == "disp_u16":
                assert got.dtype == np.uint16 and np.array_equal(got, live_ref.export(ref[i], H0, W0, "disp_u16"))
            else:
                assert np.array_equal(got, ref[i])
        s.close()


def test_cli_live_writes_what_the_default_path_writes(tmp_path):
    from PIL import Image
    from codd_amd import inference
    h, w, n = 100, 200, 6
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(_frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    common = ["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
              "--show"]
    inference.main(common + ["--show-dir", str(tmp_path / "default")])
    inference.main(common + ["--show-dir", str(tmp_path / "live"), "--live"])
    a = np.load(tmp_path / "default" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "live" / "left.disp.pred.npz")["disp"]
    assert a.shape == b.shape == (1, n, h, w) and a.dtype == b.dtype == np.float32
    assert np.array_equal(a, b)
    inference.main(common + ["--show-dir", str(tmp_path / "u16"), "--live", "--output", "disp_u16"])
    c = np.load(tmp_path / "u16" / "left.disp.pred.npz")["disp"]
    assert c.dtype == np.uint16 and np.array_equal(c[0, 0], live_ref.export(a[0, 0], h, w, "disp_u16"))
