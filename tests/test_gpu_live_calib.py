"""Rectification from a stereo calibration on the GPU.  ops.rectify_maps against the fp64 restatement of the map function
(tests/live_calib_ref.py); ops.ingest_calibrated -- the map function evaluated inside the ingest launch -- bit for bit
against ops.ingest_pair / ops.ingest_frames given those maps, and, with a source of another size, against the fp64
restatement of the blend; LiveSession(calibration=) against LiveSession(rectify=<the same maps>); the CLI.  Autotune is off
in every test."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_calib_ref as cr  # noqa: E402
import live_fmt_ref as fr  # noqa: E402
import live_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
RECT_TOL = 1e-5  # derived in tests/test_gpu_live_session.py; the derivation does not involve the source size
MODELS = ("brown", "fisheye")
# (fmt, bgr, yuv): rgb8 both channel orders, the eight raw formats, each YUV matrix once
FORMATS = [("rgb8", False, "bt601"), ("rgb8", True, "bt601"), ("mono8", False, "bt601"), ("yuyv", False, "bt601"),
           ("uyvy", False, "bt709"), ("nv12", False, "jpeg"), ("bayer_rggb", False, "bt601"), ("bayer_grbg", False, "bt601"),
           ("bayer_gbrg", False, "bt601"), ("bayer_bggr", False, "bt601")]
_CACHE = {}


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _rig(model, size):
    from codd_amd.calibration import CameraModel, StereoCalibration
    (Kl, dl), (Kr, dr), R, T = cr.make_rig(model, size)
    return StereoCalibration(CameraModel(size, Kl, model, dl), CameraModel(size, Kr, model, dr), R, T)


def _frames(fmt, hs, ws):
    """Two tight source frames of random bytes (every byte string is a valid frame); rgb8: [hs,ws,3]."""
    key = ("frames", fmt, hs, ws)
    if key not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(f"calib {fmt} {hs} {ws}".encode()))
        if fmt == "rgb8":
            _CACHE[key] = tuple(rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8) for _ in range(2))
        else:
            _CACHE[key] = tuple(fr.random_frame(rng, fmt, hs, ws) for _ in range(2))
    return _CACHE[key]


def _outputs(H, W):
    return tuple(torch.full((1, 3, H, W), float("nan"), device=DEV) for _ in range(2))


def _same(a, b):
    """Byte for byte (NaN-safe)."""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _dev(a, offset=None):
    """The array on the device; with ``offset``, at that byte offset into a larger allocation."""
    a = np.ascontiguousarray(a)
    if offset is None:
        return torch.from_numpy(a).to(DEV)
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device=DEV)
    t = buf[offset:offset + a.size]
    t.copy_(torch.from_numpy(a.reshape(-1)))
    assert t.data_ptr() % 4 == offset % 4
    return t.view(a.shape)


def _fused(frames, fmt, bgr, yuv, rect, src, shape, HW, pitch=None, offset=None, outs=None):
    from codd_amd import ops
    ol, orr = outs or _outputs(*HW)
    ops.ingest_calibrated(_dev(frames[0], offset), _dev(frames[1], offset), ol, orr, rect, fmt, src, shape, bgr=bgr, yuv=yuv,
                          pitch=pitch)
    torch.cuda.synchronize()
    return ol, orr


def _via_maps(frames, fmt, bgr, yuv, maps, shape, HW, pitch=None):
    """The parent's path: the existing ingest entries given map arrays."""
    from codd_amd import ops
    ol, orr = _outputs(*HW)
    if fmt == "rgb8":
        ops.ingest_pair(_dev(frames[0]), _dev(frames[1]), ol, orr, bgr=bgr, maps=maps)
    else:
        ops.ingest_frames(_dev(frames[0]), _dev(frames[1]), ol, orr, fmt, shape, yuv=yuv, pitch=pitch, maps=maps)
    torch.cuda.synchronize()
    return ol, orr


# ---- 1. the maps against fp64 ------------------------------------------------------------------------------------------
MAP_CASES = [((48, 70), (37, 53)), ((40, 64), (40, 64)), ((800, 1280), (540, 960))]


@pytest.mark.parametrize("case", MAP_CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
@pytest.mark.parametrize("model", MODELS)
def test_rectify_maps_match_fp64(model, case):
    """Bound: 5 x the worst deviation of the header's fp32 operation order, restated in numpy, from fp64 on the same case
    (the convention of finding 77) -- and that bound must itself stay below 1/32 px, the quantum of OpenCV's fixed-point
    maps.  Measured on MI355X (DESIGN.md finding 82): see the printed lines."""
    from codd_amd import ops
    size, shape = case
    rect = _rig(model, size).rectify(shape)
    maps = ops.rectify_maps(rect, shape, DEV)
    torch.cuda.synchronize()
    uu, vv = cr.grid(shape)
    for view, name in enumerate(("left", "right")):
        v = cr.as_view(rect.views[view])
        rx, ry, W = cr.map_fp64(v, uu, vv)
        assert (W > 0.05).all()
        fx_, fy_ = cr.map_fp32(v, uu, vv)
        own = max(np.abs(fx_ - rx).max(), np.abs(fy_ - ry).max())
        bound = 5.0 * own
        gx, gy = (m.cpu().numpy() for m in maps[view])
        assert gx.dtype == gy.dtype == np.float32 and gx.shape == gy.shape == tuple(shape)
        got = max(np.abs(gx - rx).max(), np.abs(gy - ry).max())
        print(f"rectify_maps {model} {size}->{shape} {name}: GPU max |delta| = {got:.3e} px; fp32 restatement {own:.3e} px; "
              f"bound {bound:.3e} px")
        assert bound < 1.0 / 32
        assert got <= bound


# ---- 2. W <= 0 ------------------------------------------------------------------------------------------------------------
def test_rays_behind_the_camera_are_nan_and_read_zero():
    """f' = 5 at w = 53 sees +-79 degrees; R_rect turned 30 degrees about y pushes one side of that past the source
    camera's image plane (W <= 0)."""
    from codd_amd import ops
    from codd_amd.calibration import RectifiedView, Rectification
    size, shape, HW = (48, 70), (37, 53), (64, 64)
    rig = _rig("brown", size)
    P = (5.0, 5.0, 26.0, 18.0)
    rect = Rectification(RectifiedView(cr.rot((0, np.pi / 6, 0)), P, rig.left), RectifiedView(cr.rot((0, -np.pi / 6, 0)), P, rig.right),
                         shape, 0.12)
    maps = ops.rectify_maps(rect, shape, DEV)
    frames = _frames("rgb8", *size)
    outs = _fused(frames, "rgb8", False, "bt601", rect, size, shape, HW)
    uu, vv = cr.grid(shape)
    mean, std = np.float32(live_ref.MEAN), np.float32(live_ref.STD)
    zero = ((np.float32(0) - mean) / std).astype(np.float32)  # (0 - mean) / std in fp32; the division is correctly rounded
    for view in (0, 1):
        W = cr.map_fp64(cr.as_view(rect.views[view]), uu, vv)[2]
        behind = W < -0.01
        assert behind.sum() > 100 and (W > 0.05).sum() > 100
        gx, gy = (m.cpu().numpy() for m in maps[view])
        assert np.isnan(gx[behind]).all() and np.isnan(gy[behind]).all()
        assert np.isfinite(gx[W > 0.05]).all() and np.isfinite(gy[W > 0.05]).all()
        o = outs[view][0, :, :shape[0], :shape[1]].cpu().numpy()
        for ch in range(3):
            assert np.array_equal(o[ch][behind], np.full(int(behind.sum()), zero[ch], np.float32))
        assert np.isfinite(outs[view].cpu().numpy()).all()


# ---- 3. fused against the maps path, bit for bit, same size ------------------------------------------------------------
SAME_SHAPES = [((38, 54), (64, 64)), ((38, 54), (40, 55))]  # (40, 55): W % 4 != 0 -> the scalar stores


@pytest.mark.parametrize("HW", [s[1] for s in SAME_SHAPES], ids=lambda s: "pad%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("fmt,bgr,yuv", FORMATS, ids=lambda v: str(v))
def test_fused_equals_the_maps_path_bit_for_bit(fmt, bgr, yuv, model, HW):
    from codd_amd import ops
    shape = SAME_SHAPES[0][0]
    rect = _rig(model, shape).rectify(shape, zoom=0.8)  # zoom 0.8: the border of the rectified image leaves the source
    maps = ops.rectify_maps(rect, shape, DEV)
    mx = maps[0][0].cpu().numpy()
    assert (~((mx > -1) & (mx < shape[1]))).any(), "the case must have taps outside the source"
    frames = _frames(fmt, *shape)
    want = _via_maps(frames, fmt, bgr, yuv, maps, shape, HW)
    got = _fused(frames, fmt, bgr, yuv, rect, shape, shape, HW)
    assert _same(got[0], want[0]), "left view differs"
    assert _same(got[1], want[1]), "right view differs"
    assert np.isfinite(got[0].cpu().numpy()).all()
    # a view passed without calibration: the map-free path of that view
    for views, m in (((rect.views[0], None), (maps[0], None)), ((None, rect.views[1]), (None, maps[1]))):
        want1 = _via_maps(frames, fmt, bgr, yuv, m, shape, HW)
        got1 = _fused(frames, fmt, bgr, yuv, views, shape, shape, HW)
        assert _same(got1[0], want1[0]) and _same(got1[1], want1[1]), f"mapped: {[v is not None for v in views]}"


@pytest.mark.parametrize("fmt,bgr,yuv", FORMATS[1:], ids=lambda v: str(v))
def test_fused_with_a_pitch(fmt, bgr, yuv):
    """A pitch larger than the row: the bits of the tight frame, whatever the padding bytes hold."""
    shape, HW = SAME_SHAPES[0]
    h, w = shape
    rect = _rig("brown", shape).rectify(shape, zoom=0.8)
    frames = _frames(fmt, h, w)
    tight = _fused(frames, fmt, bgr, yuv, rect, shape, shape, HW)
    rng = np.random.default_rng(11)
    if fmt == "rgb8":
        pitch = 3 * w + 5
        padded = []
        for f in frames:
            b = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
            b[:, :3 * w] = f.reshape(h, 3 * w)
            padded.append(b)
    else:
        pitch = fr.layout(fmt, h, w)[1] + 10
        padded = [fr.with_pitch(f, fmt, h, w, pitch, lambda s: rng.integers(0, 256, s, dtype=np.uint8)) for f in frames]
    got = _fused(padded, fmt, bgr, yuv, rect, shape, shape, HW, pitch=pitch)
    assert _same(got[0], tight[0]) and _same(got[1], tight[1])
    one = _fused(padded, fmt, bgr, yuv, (None, rect.views[1]), shape, shape, HW, pitch=pitch)  # the map-free path too
    ref = _fused(frames, fmt, bgr, yuv, (None, rect.views[1]), shape, shape, HW)
    assert _same(one[0], ref[0]) and _same(one[1], ref[1])


@pytest.mark.parametrize("fmt,bgr,yuv", [FORMATS[0], FORMATS[5], FORMATS[7]], ids=lambda v: str(v))
def test_fused_unaligned_views(fmt, bgr, yuv):
    """Source frames at odd byte offsets and outputs that are not 16-byte aligned: the same bits, and nothing written
    outside the outputs (guard words), as test_ingest_pair_unaligned_views."""
    from codd_amd import ops
    shape, (H, W) = SAME_SHAPES[0]
    rect = _rig("fisheye", shape).rectify(shape, zoom=0.8)
    frames = _frames(fmt, *shape)
    want = _fused(frames, fmt, bgr, yuv, rect, shape, shape, (H, W))
    for views in (rect, (rect.views[0], None)):
        ref = want if views is rect else _fused(frames, fmt, bgr, yuv, views, shape, shape, (H, W))
        for offset in (1, 2, 3):
            got = _fused(frames, fmt, bgr, yuv, views, shape, shape, (H, W), offset=offset)
            assert _same(got[0], ref[0]) and _same(got[1], ref[1]), f"source offset {offset}"
        n = 3 * H * W
        obuf = torch.zeros(2 * n + 8, device=DEV)
        ol, orr = obuf[1:1 + n].view(1, 3, H, W), obuf[n + 2:2 * n + 2].view(1, 3, H, W)
        _fused(frames, fmt, bgr, yuv, views, shape, shape, (H, W), outs=(ol, orr))
        assert _same(ol, ref[0]) and _same(orr, ref[1])
        assert obuf[0] == 0 and obuf[n + 1] == 0 and bool((obuf[2 * n + 2:] == 0).all())
    # the maps: an unaligned pair takes the scalar stores and writes nothing outside
    h, w = 40, 64
    rect = _rig("brown", (h, w)).rectify((h, w))
    aligned = ops.rectify_maps(rect, (h, w), DEV)
    lib, structs = ops._abi.load(), ops.calib_structs(rect)
    mbuf = torch.zeros(4 * h * w + 8, device=DEV)
    views = [mbuf[1 + i * (h * w + 1):1 + i * (h * w + 1) + h * w] for i in range(4)]
    rc = lib.codd_rectify_maps(C.byref(structs[0]), C.byref(structs[1]), h, w, *(v.data_ptr() for v in views),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for v, m in zip(views, (aligned[0][0], aligned[0][1], aligned[1][0], aligned[1][1])):
        assert _same(v.view(h, w), m)
    guards = [0] + [(i + 1) * (h * w + 1) for i in range(4)]
    assert all(mbuf[g] == 0 for g in guards) and bool((mbuf[4 * h * w + 5:] == 0).all())


# ---- 4. fused, source size != rectified size ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("fmt,yuv", [("rgb8", "bt601"), ("nv12", "bt709"), ("bayer_grbg", "bt601"), ("yuyv", "bt601")],
                         ids=lambda v: str(v))
def test_fused_from_a_source_of_another_size_matches_fp64(fmt, yuv, model):
    from codd_amd import ops
    size, shape, (H, W) = (48, 70), (37, 53), (64, 64)
    h, w = shape
    rect = _rig(model, size).rectify(shape, zoom=0.8)
    maps = ops.rectify_maps(rect, shape, DEV)
    frames = _frames(fmt, *size)
    got = _fused(frames, fmt, False, yuv, rect, size, shape, (H, W))
    worst, outside = 0.0, 0
    for view in (0, 1):
        rgb = frames[view] if fmt == "rgb8" else fr.decode(frames[view], fmt, size[0], size[1], yuv=yuv)
        mx, my = (m.cpu().numpy() for m in maps[view])
        outside += int((~((mx > 0) & (mx < size[1] - 1) & (my > 0) & (my < size[0] - 1))).sum())
        v = live_ref.remap(rgb, mx, my)  # fp64 [h,w,3] at the GPU-written maps; taps outside the 48 x 70 source are 0
        v = np.pad(v, ((0, H - h), (0, W - w), (0, 0)), mode="reflect")  # BORDER_REFLECT_101 of the RECTIFIED image
        ref = np.transpose((v - live_ref.MEAN) / live_ref.STD, (2, 0, 1))
        worst = max(worst, float(np.abs(got[view][0].cpu().numpy().astype(np.float64) - ref).max()))
    print(f"fused {fmt} {model} {size}->{shape}: max |delta| = {worst:.3e} (bound {RECT_TOL:g}); {outside} pixels with a tap outside")
    assert outside > 0
    assert worst <= RECT_TOL


# ---- 5. errors: CODD_EINVAL before any launch ----------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_launch():
    from codd_amd import _abi, ops
    lib = _abi.load()
    size, shape, (H, W) = (48, 70), (37, 53), (64, 64)
    rect = _rig("brown", size).rectify(shape)
    good = ops.calib_structs(rect)
    src = [_dev(f) for f in _frames("rgb8", 72, 70)]  # (72 rows: room for every format's 48 x 70 frame)
    outs = _outputs(H, W)
    maps = [torch.full(shape, float("nan"), device=DEV) for _ in range(4)]
    m, s = (C.c_float * 3)(1, 2, 3), (C.c_float * 3)(1, 1, 1)
    stream = torch.cuda.current_stream().cuda_stream

    def view(**kw):
        v = ops.calib_structs(rect)[0]
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(v, k)[val[0]] = val[1]
            else:
                setattr(v, k, val)
        return C.byref(v)

    L, R_ = C.byref(good[0]), C.byref(good[1])
    nan, inf = float("nan"), float("inf")
    bad_views = [view(model=2), view(f=0.0), view(f=-3.0), view(f=nan), view(f=inf), view(K=(0, 0.0)), view(K=(1, -1.0)),
                 view(K=(0, inf)), view(K=(1, nan)), view(R=(4, nan)), view(dist=(7, inf))]

    def ingest(left=src[0].data_ptr(), right=src[1].data_ptr(), fmt=0, yuv=0, hs=48, ws=70, pitch=0, l=L, r=R_, h=37, w=53,
               mean=m, std=s, H=H, W=W, ol=outs[0].data_ptr(), orr=outs[1].data_ptr()):
        return lib.codd_ingest_calibrated(left, right, fmt, 0, yuv, hs, ws, pitch, l, r, h, w, mean, std, H, W, ol, orr, stream)

    for k in ("left", "right", "mean", "std", "ol", "orr"):
        assert ingest(**{k: None}) == EINVAL, k
    calls = [dict(l=None, r=None), dict(fmt=9), dict(fmt=-1), dict(fmt=4, yuv=3), dict(fmt=2, yuv=-1), dict(fmt=2, ws=69),
             dict(fmt=4, hs=47), dict(fmt=5, hs=1), dict(hs=0), dict(pitch=209), dict(fmt=1, pitch=69), dict(fmt=2, pitch=139),
             dict(H=36), dict(W=52), dict(h=32, H=64), dict(w=32, W=64), dict(l=None), dict(r=None)]
    calls += [dict(l=b) for b in bad_views] + [dict(r=b) for b in bad_views]
    for kw in calls:
        assert ingest(**kw) == EINVAL, kw

    def rmaps(l=L, r=R_, h=37, w=53, ptrs=tuple(t.data_ptr() for t in maps)):
        return lib.codd_rectify_maps(l, r, h, w, *ptrs, stream)

    assert rmaps(l=None, r=None) == EINVAL and rmaps(h=0) == EINVAL and rmaps(w=0) == EINVAL
    for i in range(4):
        ptrs = [t.data_ptr() for t in maps]
        ptrs[i] = None
        assert rmaps(ptrs=tuple(ptrs)) == EINVAL
    for b in bad_views:
        assert rmaps(l=b) == EINVAL and rmaps(r=b) == EINVAL
    torch.cuda.synchronize()
    for t in list(outs) + maps:  # nothing was launched: every output is untouched
        assert bool(torch.isnan(t).all())
    assert ingest() == 0 and rmaps() == 0  # ... and the same calls without a fault go through
    torch.cuda.synchronize()
    for t in list(outs) + maps:
        assert bool(torch.isfinite(t).all())


# ---- 6. the session ------------------------------------------------------------------------------------------------------
SH, SW, SN = 100, 200, 3


def _rgb_frames(h=SH, w=SW):
    key = ("seq", h, w)
    if key not in _CACHE:
        from codd_amd import synth
        img, r_img, _ = synth.stereo_sequence(h, w, SN)

        def u8(t):
            return np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())

        _CACHE[key] = [(u8(img[0, i]), u8(r_img[0, i])) for i in range(SN)]
    return _CACHE[key]


def _nv12_of(rgb):
    """A raw frame that looks like the RGB image: G as luma, (B, R) halved around 128 as chroma, sub-sampled by dropping."""
    h, w = rgb.shape[:2]
    Y, U, V = rgb[..., 1], (rgb[..., 2] >> 1) + 64, (rgb[..., 0] >> 1) + 64
    uv = np.stack([U[0::2, 0::2], V[0::2, 0::2]], axis=-1)
    return np.ascontiguousarray(np.concatenate([Y, uv.reshape(h // 2, w)], axis=0))


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


def _flat(res):
    """A session result (array, tuple of arrays / namedtuples / numbers / None) as a flat list of arrays."""
    if res is None or isinstance(res, np.ndarray):
        return [res]
    if isinstance(res, (bool, int, float, np.generic)):
        return [np.asarray(res)]
    return [a for part in res for a in _flat(part)]


def _run_pipelined(s, frames):
    outs = []
    for left, right in frames:
        s.push(left, right)
        if s.pending() == 2:
            outs.append(s.pop())
    while s.pending():
        outs.append(s.pop())
    return outs


def _assert_same_results(got, want):
    assert len(got) == len(want) == SN
    for i, (g, w_) in enumerate(zip(got, want)):
        ga, wa = _flat(g), _flat(w_)
        assert len(ga) == len(wa)
        for a, b in zip(ga, wa):
            assert (a is None) == (b is None), f"frame {i}"
            if a is not None:
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"frame {i} differs"


def _host_maps(rect, shape):
    from codd_amd import ops
    return tuple(tuple(m.cpu().numpy() for m in pair) for pair in ops.rectify_maps(rect, shape, DEV))


@pytest.mark.parametrize("fmt,kw", [("rgb8", dict(motion="sceneflow", egomotion=True, confidence=True)),
                                    ("nv12", dict(confidence=True))], ids=["rgb8-sceneflow-ego-confidence", "nv12-pitch"])
def test_session_with_calibration_equals_session_with_its_maps(fmt, kw):
    """Source size == net size: the bits of LiveSession(rectify=<the GPU maps>, intrinsics=, calib= of the rectification)."""
    from codd_amd.live import LiveSession
    rig = _rig("brown", (SH, SW))
    rect = rig.rectify((SH, SW))
    est = _estimator(stereo_only="motion" not in kw)
    frames, extra = _rgb_frames(), {}
    if fmt == "nv12":
        pitch = SW + 8
        frames = [tuple(fr.with_pitch(_nv12_of(v), fmt, SH, SW, pitch, 0x5A).reshape(-1, pitch) for v in pair) for pair in frames]
        extra = dict(pixel_format=fmt, pitch=pitch, yuv="bt709")
    ref_s = LiveSession(est, (SH, SW), output="depth", rectify=_host_maps(rect, (SH, SW)), intrinsics=rect.intrinsics,
                        calib=rect.calib, **extra, **kw)
    want = _run_pipelined(ref_s, frames)
    ref_s.close()
    s = LiveSession(est, (SH, SW), output="depth", calibration=rig, **extra, **kw)
    got = _run_pipelined(s, frames)
    s.close()
    _assert_same_results(got, want)
    assert _flat(got[-1])[0].shape == (SH, SW)


def test_session_from_a_larger_source():
    from codd_amd.live import LiveSession
    src = (160, 320)
    rig = _rig("fisheye", src)
    frames = _rgb_frames(*src)
    s = LiveSession(_estimator(stereo_only=True), (SH, SW), output="depth", calibration=rig, zoom=0.9, confidence=True)
    wrong = np.zeros((SH, SW, 3), np.uint8)  # a frame of the net size is not a frame of this session
    with pytest.raises(ValueError):
        s.push(wrong, frames[0][1])
    with pytest.raises(ValueError):
        s.push(frames[0][0], wrong)
    assert not s._open_done and s.pending() == 0  # raised before the device was touched
    first = [s.step(*pair) for pair in frames]
    for depth, conf in first:
        assert depth.shape == (SH, SW) and depth.dtype == np.float32
        assert conf.flags.shape == conf.residual.shape == (SH, SW) and conf.flags.dtype == np.uint8
    assert all(tuple(t.shape) == src + (3,) for slot in s._d_in + s._h_in for t in slot)  # the slots hold SOURCE frames
    assert s.calib == pytest.approx(rig.rectify((SH, SW), zoom=0.9).calib) and s.metas[0]["calib"] == s.calib
    s.reset()
    _assert_same_results([s.step(*pair) for pair in frames], first)  # a second run after reset(): the same bits
    s.reset()
    _assert_same_results(_run_pipelined(s, frames), first)  # pipelined push / pop equals step
    s.close()


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_calibration_writes_what_the_rectify_maps_route_writes(tmp_path):
    """--stereo-only: the --rectify-maps route has no way to name the rectified camera and runs on the CLI's pseudo
    intrinsics, so with a motion stage (which reads them from the second frame on) the two routes differ by design --
    the calibrated one has the right camera.  The stereo network reads the images alone: there the files are equal."""
    from PIL import Image
    from codd_amd import inference
    rig = _rig("brown", (SH, SW))
    rig.save(tmp_path / "cal.json")
    (lx, ly), (rx, ry) = _host_maps(rig.rectify((SH, SW)), (SH, SW))
    np.savez(tmp_path / "maps.npz", left_x=lx, left_y=ly, right_x=rx, right_y=ry)
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(_rgb_frames()):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    common = ["--stereo-only", "--no-autotune", "--show", "--live", "--img-dir", str(tmp_path / "left"), "--r-img-dir",
              str(tmp_path / "right")]
    inference.main(common + ["--rectify-maps", str(tmp_path / "maps.npz"), "--show-dir", str(tmp_path / "out_maps")])
    inference.main(common + ["--calibration", str(tmp_path / "cal.json"), "--show-dir", str(tmp_path / "out_cal")])
    a = np.load(tmp_path / "out_maps" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "out_cal" / "left.disp.pred.npz")["disp"]
    assert a.shape == b.shape == (1, SN, SH, SW) and a.dtype == b.dtype == np.float32
    assert a.tobytes() == b.tobytes()
    with pytest.raises(SystemExit):
        inference.main(common + ["--calibration", str(tmp_path / "cal.json"), "--rectify-maps", str(tmp_path / "maps.npz")])
