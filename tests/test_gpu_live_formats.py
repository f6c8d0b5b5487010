"""Raw camera formats of the live session on the GPU.  The contract is "decode, then ingest": ops.ingest_frames(frame)
must give, bit for bit, what ops.ingest_pair gives on D_F(frame), the numpy integer restatement of the decoder in
tests/live_fmt_ref.py -- map-free, with rectification maps, with a row pitch, from an unaligned base -- and a LiveSession
fed raw frames must return what a LiveSession fed the decoded frames returns.  Autotune is off in every test."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_fmt_ref as fr  # noqa: E402
import live_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RECT_TOL = 1e-5  # derived in tests/test_gpu_live_session.py; the derivation does not depend on the source format
SMALL = [((2, 2), (3, 3)), ((4, 6), (6, 8)), ((38, 54), (64, 64))]
PRODUCT = ((540, 960), (576, 960))


def _shapes(fmt):
    odd = {"mono8": [((37, 53), (64, 64))], "yuyv": [((37, 54), (64, 64))], "uyvy": [((37, 54), (64, 64))], "nv12": []}
    return SMALL + odd.get(fmt, [((37, 53), (64, 64))]) + [PRODUCT]


def _yuvs(fmt):
    return tuple(fr.YUV) if fmt in fr.YUV_FORMATS else ("bt601",)


CASES = [(fmt, yuv, shape) for fmt in fr.FORMATS for yuv in _yuvs(fmt) for shape in _shapes(fmt)]
FMT_YUV = [(fmt, yuv) for fmt in fr.FORMATS for yuv in _yuvs(fmt)]


def _case_id(c):
    return "%s-%s-%dx%d" % (c[0], c[1], c[2][0][0], c[2][0][1])


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


_CACHE = {}


def _pair(fmt, h, w):
    """Two tight frames of random bytes (every byte string is a valid frame) with a few planted extremes."""
    key = ("pair", fmt, h, w)
    if key not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(f"{fmt} {h} {w}".encode()))
        pair = []
        for _ in range(2):
            f = fr.random_frame(rng, fmt, h, w)
            n = min(8, f.size // 4)
            f[:n], f[-n:] = 0, 255  # saturating corners: Y = U = V = 0 and = 255
            if f.size > 64:
                f[20:24], f[24:28] = (255, 0, 255, 0), (0, 255, 0, 255)  # extreme chroma / checkerboard mosaic
            pair.append(f)
        _CACHE[key] = tuple(pair)
    return _CACHE[key]


def _decoded(fmt, yuv, h, w):
    key = ("rgb", fmt, yuv, h, w)
    if key not in _CACHE:
        _CACHE[key] = tuple(np.ascontiguousarray(fr.decode(f, fmt, h, w, yuv=yuv)) for f in _pair(fmt, h, w))
    return _CACHE[key]


def _dev_maps(maps):
    if maps is None:
        return None
    return tuple(None if p is None else tuple(torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in p) for p in maps)


def _outputs(H, W):
    return tuple(torch.full((1, 3, H, W), float("nan"), device=DEV) for _ in range(2))


def _ingest_rgb(left, right, H, W, maps=None):
    """The existing kernel on decoded frames: the reference of every bit comparison below."""
    from codd_amd import ops
    ol, orr = _outputs(H, W)
    ops.ingest_pair(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), ol, orr, bgr=False, maps=_dev_maps(maps))
    torch.cuda.synchronize()
    return ol, orr


def _ingest_raw(left, right, fmt, yuv, h, w, H, W, pitch=None, maps=None, offset=None):
    from codd_amd import ops
    if offset is None:
        dl, dr = torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV)
    else:  # the frame at a byte offset into a larger allocation
        bl, br = (torch.zeros(left.size + 16, dtype=torch.uint8, device=DEV) for _ in range(2))
        dl, dr = bl[offset:offset + left.size], br[offset:offset + right.size]
        dl.copy_(torch.from_numpy(left))
        dr.copy_(torch.from_numpy(right))
        assert dl.data_ptr() % 4 == offset % 4
    ol, orr = _outputs(H, W)
    ops.ingest_frames(dl, dr, ol, orr, fmt, (h, w), yuv=yuv, pitch=pitch, maps=_dev_maps(maps))
    torch.cuda.synchronize()
    return ol, orr


def _same(a, b):
    """Byte for byte (NaN-safe)."""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _q64(a):
    """Round to multiples of 1/64 (exact in fp32 at these magnitudes)."""
    return (np.round(np.asarray(a, np.float64) * 64.0) / 64.0).astype(np.float32)


def _maps(kind, h, w):
    """identity / radial / leaving: as tests/test_gpu_live_session.py::_maps.  edge: a slight zoom-out whose first column
    has the tap x0 = -1 and whose last has x0 + 1 = w (and the same in y) at every size, the smallest included."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if kind == "identity":
        return xx.astype(np.float32), yy.astype(np.float32)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    if kind == "radial":  # smooth barrel distortion, up to ~4 px at the corners
        r2 = ((xx - cx) ** 2 + (yy - cy) ** 2) / (cx * cx + cy * cy)
        return _q64(xx + 4.0 * r2 * (xx - cx) / max(cx, 1.0)), _q64(yy + 4.0 * r2 * (yy - cy) / max(cy, 1.0))
    if kind == "edge":
        mx, my = _q64(xx * (w + 0.25) / (w - 1) - 0.625), _q64(yy * (h + 0.125) / (h - 1) - 0.390625)
        assert -1 < mx.min() < 0 and w - 1 < mx.max() < w and -1 < my.min() < 0 and h - 1 < my.max() < h
        return mx, my
    assert kind == "leaving"  # 1.25x zoom-out about the centre plus a shift: leaves the source on all four sides
    mx, my = _q64(cx + 1.25 * (xx - cx) + 0.375), _q64(cy + 1.25 * (yy - cy) - 0.640625)
    assert mx.min() < -1 and mx.max() > w and my.min() < -1 and my.max() > h
    mx[h // 2, w // 3], my[h // 3, w // 2], mx[1, 1] = np.nan, np.inf, -np.inf  # non-finite entries give 0
    return mx, my


# ---- 1. map-free -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_ingest_frames_equals_ingest_pair_of_the_decoded_frame(case):
    fmt, yuv, ((h, w), (H, W)) = case
    left, right = _pair(fmt, h, w)
    rl, rr = _decoded(fmt, yuv, h, w)
    wl, wr = _ingest_rgb(rl, rr, H, W)
    gl, gr = _ingest_raw(left, right, fmt, yuv, h, w, H, W)
    assert _same(gl, wl), "left view differs"
    assert _same(gr, wr), "right view differs"
    if fmt not in fr.YUV_FORMATS:  # yuv is ignored for mono and Bayer
        jl, jr = _ingest_raw(left, right, fmt, "jpeg", h, w, H, W)
        assert _same(jl, wl) and _same(jr, wr)


# ---- 2. 1/64-pixel maps: every intermediate of the blend is exact in fp32, so the bits are equal ------------------------
MAP_CASES = [(fmt, yuv, shape, kind) for fmt, yuv in FMT_YUV if yuv == "bt601" or fmt == "nv12"
             for shape in _shapes(fmt)[:-1] for kind in ("identity", "radial", "leaving", "edge")
             if kind != "leaving" or shape[0][0] >= 37]
MAP_CASES += [(fmt, "bt601", PRODUCT, "radial") for fmt in ("mono8", "yuyv", "nv12", "bayer_grbg")]


@pytest.mark.parametrize("case", MAP_CASES, ids=lambda c: _case_id(c) + "-" + c[3])
def test_ingest_frames_with_quantised_maps_equals_ingest_pair(case):
    fmt, yuv, ((h, w), (H, W)), kind = case
    left, right = _pair(fmt, h, w)
    rl, rr = _decoded(fmt, yuv, h, w)
    lm = _maps(kind, h, w)
    rm = tuple(np.ascontiguousarray(m[::-1, ::-1]) for m in lm) if kind != "identity" else lm  # another map for the right view
    for maps in ((lm, rm), (lm, None), (None, rm)):  # both views mapped; one mapped and the other not
        wl, wr = _ingest_rgb(rl, rr, H, W, maps)
        gl, gr = _ingest_raw(left, right, fmt, yuv, h, w, H, W, maps=maps)
        assert _same(gl, wl), f"left view differs ({kind}, mapped: {[m is not None for m in maps]})"
        assert _same(gr, wr), f"right view differs ({kind}, mapped: {[m is not None for m in maps]})"
    if kind == "identity":  # the identity map gives the bits of the map-free path
        pl, pr = _ingest_raw(left, right, fmt, yuv, h, w, H, W)
        il, ir = _ingest_raw(left, right, fmt, yuv, h, w, H, W, maps=(lm, rm))
        assert _same(il, pl) and _same(ir, pr)


# ---- 3. unquantised maps against the fp64 restatement -----------------------------------------------------------------
def _smooth_maps(h, w):
    """An unquantised barrel distortion per view: the weights of the blend have full fp32 mantissas."""
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    r2 = ((xx - cx) ** 2 + (yy - cy) ** 2) / (cx * cx + cy * cy)
    lm = ((xx + 3.3 * r2 * (xx - cx) / cx + 0.2137).astype(np.float32), (yy + 3.3 * r2 * (yy - cy) / cy - 0.3719).astype(np.float32))
    return lm, tuple(np.ascontiguousarray(m[::-1, ::-1]) for m in lm)


@pytest.mark.parametrize("fmt,yuv", FMT_YUV, ids=lambda v: str(v))
def test_ingest_frames_smooth_map_matches_fp64_restatement(fmt, yuv):
    (h, w), (H, W) = SMALL[2]
    left, right = _pair(fmt, h, w)
    lm, rm = _smooth_maps(h, w)
    gl, gr = _ingest_raw(left, right, fmt, yuv, h, w, H, W, maps=(lm, rm))
    worst = 0.0
    for got, rgb, m in zip((gl, gr), _decoded(fmt, yuv, h, w), (lm, rm)):
        ref = live_ref.ingest(rgb, H, W, False, maps=m)
        worst = max(worst, float(np.abs(got[0].cpu().numpy().astype(np.float64) - ref).max()))
    print(f"smooth-map ingest {fmt} {yuv} {h}x{w}: max |delta| = {worst:.3e} (bound {RECT_TOL:g})")
    assert worst <= RECT_TOL


@pytest.mark.parametrize("fmt", fr.FORMATS)
def test_ingest_frames_smooth_map_equals_ingest_pair_bit_for_bit(fmt):
    """The blend has ONE fp32 operation order (include/codd_hip.h: THE BLEND) in every instantiation of the one ingest
    kernel, so the contract "decode, then ingest_pair" holds to the bit on maps where the blend rounds, too."""
    (h, w), (H, W) = SMALL[2]
    left, right = _pair(fmt, h, w)
    rl, rr = _decoded(fmt, "bt601", h, w)
    maps = _smooth_maps(h, w)
    frac = np.modf(maps[0][0] * 64.0)[0]
    assert (frac != 0).mean() > 0.9, "the map must not be quantised"
    wl, wr = _ingest_rgb(rl, rr, H, W, maps)
    gl, gr = _ingest_raw(left, right, fmt, "bt601", h, w, H, W, maps=maps)
    assert _same(gl, wl), "left view differs"
    assert _same(gr, wr), "right view differs"


# ---- 4. pitch ------------------------------------------------------------------------------------------------------------
def _pitches(fmt, w):
    if fmt in ("yuyv", "uyvy"):
        return (2 * w + 2, 2 * w + 7)
    if fmt == "nv12":
        return (w + 10, w + 3)  # 64 at w = 54; and an odd one
    return (w + 3, w + 8)  # an odd pitch at the even widths, an even one


@pytest.mark.parametrize("shape", SMALL[1:] + [((37, 53), (64, 64))], ids=lambda s: "%dx%d" % s[0])
@pytest.mark.parametrize("fmt,yuv", [(f, "bt601") for f in fr.FORMATS], ids=lambda v: str(v))
def test_ingest_frames_pitch_and_padding_bytes(fmt, yuv, shape):
    (h, w), (H, W) = shape
    if fmt in fr.YUV_FORMATS and w % 2:
        w += 1  # (37, 54) for yuyv / uyvy
    if fmt == "nv12" and h % 2:
        h += 1
    left, right = _pair(fmt, h, w)
    rng = np.random.default_rng(7)
    maps = (_maps("radial", h, w), None)
    tight = _ingest_raw(left, right, fmt, yuv, h, w, H, W)
    tight_m = _ingest_raw(left, right, fmt, yuv, h, w, H, W, maps=maps)
    for pitch in _pitches(fmt, w):
        for fill in (0xA5, lambda s: rng.integers(0, 256, s, dtype=np.uint8)):
            pl, pr = (fr.with_pitch(f, fmt, h, w, pitch, fill) for f in (left, right))
            got = _ingest_raw(pl, pr, fmt, yuv, h, w, H, W, pitch=pitch)
            assert _same(got[0], tight[0]) and _same(got[1], tight[1]), f"pitch {pitch}"
            got = _ingest_raw(pl, pr, fmt, yuv, h, w, H, W, pitch=pitch, maps=maps)
            assert _same(got[0], tight_m[0]) and _same(got[1], tight_m[1]), f"pitch {pitch} with maps"


# ---- 5. unaligned base -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,yuv", [(f, "bt601") for f in fr.FORMATS], ids=lambda v: str(v))
def test_ingest_frames_unaligned_base(fmt, yuv):
    for (h, w), (H, W) in (SMALL[1], SMALL[2]):
        left, right = _pair(fmt, h, w)
        want = _ingest_raw(left, right, fmt, yuv, h, w, H, W)
        pitch = _pitches(fmt, w)[0]
        pl, pr = (fr.with_pitch(f, fmt, h, w, pitch, 0x3C) for f in (left, right))
        for offset in (1, 2, 3):
            got = _ingest_raw(left, right, fmt, yuv, h, w, H, W, offset=offset)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), f"offset {offset}"
            got = _ingest_raw(pl, pr, fmt, yuv, h, w, H, W, pitch=pitch, offset=offset)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), f"offset {offset}, pitch {pitch}"


def test_ingest_frames_unaligned_output():
    """An output that is not 16-byte aligned takes the scalar stores and nothing is written outside it."""
    from codd_amd import ops
    (h, w), (H, W) = SMALL[2]
    left, right = _pair("nv12", h, w)
    want = _ingest_raw(left, right, "nv12", "bt601", h, w, H, W)
    obuf = torch.zeros(2 * 3 * H * W + 8, device=DEV)
    ol, orr = obuf[1:1 + 3 * H * W].view(1, 3, H, W), obuf[3 * H * W + 2:2 * 3 * H * W + 2].view(1, 3, H, W)
    ops.ingest_frames(torch.from_numpy(left).to(DEV), torch.from_numpy(right).to(DEV), ol, orr, "nv12", (h, w))
    assert _same(ol, want[0]) and _same(orr, want[1])
    assert obuf[0] == 0 and obuf[3 * H * W + 1] == 0 and bool((obuf[2 * 3 * H * W + 2:] == 0).all())


# ---- 6. the session ----------------------------------------------------------------------------------------------------
SH, SW, SN = 100, 200, 3


def _rgb_frames():
    if "frames" not in _CACHE:
        from codd_amd import synth
        img, r_img, _ = synth.stereo_sequence(SH, SW, SN)

        def u8(t):
            return np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())

        _CACHE["frames"] = [(u8(img[0, i]), u8(r_img[0, i])) for i in range(SN)]
    return _CACHE["frames"]


def _raw_of(rgb, fmt):
    """A raw frame that looks like the RGB image (any bytes are a valid frame; the network wants an image): the mosaic a
    sensor records, or G as luma with (B, R) halved around 128 as chroma, sub-sampled by dropping."""
    h, w = rgb.shape[:2]
    if fmt.startswith("bayer_"):
        return fr.mosaic_of(rgb, fmt[len("bayer_"):])
    Y, U, V = rgb[..., 1], (rgb[..., 2] >> 1) + 64, (rgb[..., 0] >> 1) + 64
    if fmt == "nv12":
        uv = np.stack([U[0::2, 0::2], V[0::2, 0::2]], axis=-1)
        return np.ascontiguousarray(np.concatenate([Y, uv.reshape(h // 2, w)], axis=0))
    assert fmt == "yuyv"
    return np.ascontiguousarray(np.stack([Y[:, 0::2], U[:, 0::2], Y[:, 1::2], V[:, 0::2]], axis=-1).reshape(h, 2 * w))


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
    """A session result (array, tuple of arrays / namedtuples / None) as a flat list of arrays."""
    if res is None or isinstance(res, np.ndarray):
        return [res]
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


@pytest.mark.parametrize("fmt,pitch,kw", [("nv12", None, dict(confidence=True)), ("bayer_rggb", SW + 5, dict(confidence=True)),
                                          ("yuyv", None, dict(motion="flow2d", rectify="radial"))],
                         ids=["nv12-confidence", "bayer_rggb-pitch-confidence", "yuyv-rectify-flow2d"])
def test_session_on_raw_frames_equals_session_on_decoded_frames(fmt, pitch, kw):
    from codd_amd.live import LiveSession
    kw = dict(kw)
    if kw.get("rectify"):
        lm = _maps(kw["rectify"], SH, SW)
        kw["rectify"] = (lm, tuple(np.ascontiguousarray(m[::-1, ::-1]) for m in lm))
    est = _estimator(stereo_only="motion" not in kw)
    tight = [tuple(_raw_of(v, fmt) for v in pair) for pair in _rgb_frames()]
    decoded = [tuple(np.ascontiguousarray(fr.decode(v, fmt, SH, SW)) for v in pair) for pair in tight]
    rows = fr.layout(fmt, SH, SW, pitch)[0]
    raw = tight if pitch is None else [tuple(fr.with_pitch(v, fmt, SH, SW, pitch, 0x77).reshape(rows, pitch) for v in pair)
                                       for pair in tight]
    ref_s = LiveSession(est, (SH, SW), output="disp", bgr=False, **kw)
    want = _run_pipelined(ref_s, decoded)
    ref_s.close()
    s = LiveSession(est, (SH, SW), output="disp", pixel_format=fmt, pitch=pitch, **kw)
    got = _run_pipelined(s, raw)
    assert len(got) == len(want) == SN
    for i, (g, w_) in enumerate(zip(got, want)):
        ga, wa = _flat(g), _flat(w_)
        assert len(ga) == len(wa)
        for a, b in zip(ga, wa):
            assert (a is None) == (b is None), f"frame {i}"
            if a is not None:
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"frame {i} differs"
    # the slots hold the frame's bytes, and nothing is allocated per frame (the check of
    # test_session_pipelined_reset_and_allocation: device memory after frame 3 equals device memory after the last)
    nbytes = fr.layout(fmt, SH, SW, pitch)[3]
    assert all(t.numel() == nbytes for slot in s._d_in + s._h_in for t in slot)
    ptrs = [t.data_ptr() for slot in s._d_in for t in slot]
    s.reset()
    marks = {}
    for i in range(6):
        s.step(*raw[i % SN])
        torch.cuda.synchronize()
        marks[i + 1] = torch.cuda.memory_allocated()
    print("memory_allocated per frame:", marks)
    assert marks[3] == marks[6]
    assert ptrs == [t.data_ptr() for slot in s._d_in for t in slot]
    s.close()


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_live_pixel_format_writes_what_png_frames_write(tmp_path):
    from PIL import Image
    from codd_amd import inference
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / "raw" / side)
        os.makedirs(tmp_path / "png" / side)
        for i, pair in enumerate(_rgb_frames()):
            raw = _raw_of(pair[k], "nv12")
            raw.tofile(tmp_path / "raw" / side / f"{i:03d}.nv12")
            Image.fromarray(fr.decode(raw, "nv12", SH, SW, yuv="bt709")).save(tmp_path / "png" / side / f"{i:03d}.png")
    common = ["--iters", "4", "--no-autotune", "--show", "--live"]
    inference.main(common + ["--img-dir", str(tmp_path / "png" / "left"), "--r-img-dir", str(tmp_path / "png" / "right"),
                             "--show-dir", str(tmp_path / "out_png")])
    inference.main(common + ["--img-dir", str(tmp_path / "raw" / "left"), "--r-img-dir", str(tmp_path / "raw" / "right"),
                             "--img-suffix", ".nv12", "--pixel-format", "nv12", "--frame-size", f"{SH}x{SW}", "--yuv", "bt709",
                             "--show-dir", str(tmp_path / "out_raw")])
    a = np.load(tmp_path / "out_png" / "left.disp.pred.npz")["disp"]
    b = np.load(tmp_path / "out_raw" / "left.disp.pred.npz")["disp"]
    assert a.shape == b.shape == (1, SN, SH, SW) and a.dtype == b.dtype == np.float32
    assert a.tobytes() == b.tobytes()
