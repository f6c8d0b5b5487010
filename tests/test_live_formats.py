"""Raw camera formats of the live session, the parts that need no GPU: the numpy restatements of the decoders
(tests/live_fmt_ref.py) on planted frames, the argument checks of codd_ingest_frames / codd_frame_bytes (every call is
rejected before any launch), and LiveSession's validation of pixel_format / yuv / pitch and of raw frames."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_fmt_ref as fr  # noqa: E402

from codd_amd import _abi  # noqa: E402

EINVAL = -1  # CODD_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("rggb", "grbg", "gbrg", "bggr")


# ---- decoder plants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", [(2, 2), (5, 7), (6, 4)], ids=lambda s: "%dx%d" % s)
def test_flat_colour_mosaic_decodes_to_the_colour(shape, pattern):
    h, w = shape
    for colour in ((200, 30, 90), (0, 255, 1), (17, 17, 17)):
        rgb = np.broadcast_to(np.array(colour, np.uint8), (h, w, 3))
        got = fr.decode(fr.mosaic_of(rgb, pattern), "bayer_" + pattern, h, w)
        assert np.array_equal(got, rgb), (colour, pattern)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_ramp_mosaics_are_exact_in_the_interior(pattern):
    h, w = 9, 12
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for ramp in (3 * xx + 5, 7 * yy + 2, 3 * xx + 7 * yy):  # horizontal, vertical, both: every average is exact
        got = fr.decode(ramp.astype(np.uint8), "bayer_" + pattern, h, w)
        want = np.repeat(ramp[..., None], 3, axis=2)
        assert np.array_equal(got[1:-1, 1:-1], want[1:-1, 1:-1])


def test_bayer_sites_keep_their_own_byte():
    rng = np.random.default_rng(0)
    m = rng.integers(0, 256, (6, 8), dtype=np.uint8)
    for pattern in PATTERNS:
        got = fr.decode(m, "bayer_" + pattern, 6, 8)
        assert np.array_equal(fr.mosaic_of(got, pattern), m)


@pytest.mark.parametrize("yuv", list(fr.YUV))
@pytest.mark.parametrize("fmt", fr.YUV_FORMATS)
def test_grey_sweep_gives_grey(fmt, yuv):
    h, w = 2, 256
    Y = np.broadcast_to(np.arange(256, dtype=np.uint8), (h, w))
    if fmt == "nv12":
        frame = np.concatenate([Y.reshape(-1), np.full(h // 2 * w, 128, np.uint8)])
    else:
        q = np.full((h, w // 2, 4), 128, np.uint8)
        yo = 0 if fmt == "yuyv" else 1
        q[..., yo], q[..., yo + 2] = Y[:, 0::2], Y[:, 1::2]
        frame = q.reshape(-1)
    rgb = fr.decode(frame, fmt, h, w, yuv=yuv)
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
    assert np.all(np.diff(rgb[0, :, 0].astype(int)) >= 0) and rgb[0, -1, 0] == 255
    yoff = fr.YUV[yuv][0]
    assert rgb[0, yoff, 0] == 0 and (yuv != "jpeg" or np.array_equal(rgb[0, :, 0], np.arange(256)))


def test_chroma_is_nearest_and_byte_orders_differ_only_in_position():
    rng = np.random.default_rng(1)
    h, w = 4, 6
    f = fr.random_frame(rng, "yuyv", h, w)
    swapped = f.reshape(-1, 2)[:, ::-1].reshape(-1)  # Y0 U Y1 V -> U Y0 V Y1
    assert np.array_equal(fr.decode(f, "yuyv", h, w), fr.decode(swapped, "uyvy", h, w))
    # nv12 with the chroma of row pair r repeated = yuyv rows 2r, 2r+1 sharing that chroma
    q = f.reshape(h, w // 2, 4).copy()
    q[1::2, :, 1], q[1::2, :, 3] = q[0::2, :, 1], q[0::2, :, 3]
    Y = np.stack([q[..., 0], q[..., 2]], axis=-1).reshape(h, w)
    uv = np.stack([q[0::2, :, 1], q[0::2, :, 3]], axis=-1)
    nv12 = np.concatenate([Y.reshape(-1), uv.reshape(-1)])
    assert np.array_equal(fr.decode(nv12, "nv12", h, w), fr.decode(q.reshape(-1), "yuyv", h, w))


@pytest.mark.parametrize("yuv", list(fr.YUV))
def test_integer_formula_is_within_one_level_and_fits_int32(yuv):
    s = np.unique(np.concatenate([np.arange(0, 256, 5), [15, 16, 17, 127, 128, 129, 234, 235, 236, 240, 255]]))
    Y, U, V = np.meshgrid(s, s, s, indexing="ij")
    acc = []
    got = fr.yuv_to_rgb(Y, U, V, yuv, accumulators=acc).astype(np.float64)
    worst = float(np.abs(got - fr.yuv_to_rgb_real(Y, U, V, yuv)).max())
    biggest = max(int(np.abs(a).max()) for a in acc)
    print(f"{yuv}: max |integer - real| = {worst:.4f} levels, largest accumulator {biggest:.3e}")
    assert worst <= 1.0
    assert biggest < 5.8e8 < 2 ** 31 - 1


def test_bt601_integers():
    assert fr.coefficients("bt601") == (16, (1220542, 1673527, 409993, 852492, 2116026))
    assert fr.coefficients("jpeg")[1][0] == 1 << 20


def test_pitch_helper_and_layout():
    rng = np.random.default_rng(2)
    for fmt, h, w, pitch in (("mono8", 5, 7, 11), ("yuyv", 3, 6, 14), ("nv12", 4, 6, 9), ("bayer_grbg", 5, 7, 8)):
        f = fr.random_frame(rng, fmt, h, w)
        a = fr.with_pitch(f, fmt, h, w, pitch, 0)
        b = fr.with_pitch(f, fmt, h, w, pitch, lambda s: rng.integers(0, 256, s, dtype=np.uint8))
        assert a.size == fr.layout(fmt, h, w, pitch)[3]
        assert np.array_equal(fr.decode(a, fmt, h, w, pitch=pitch), fr.decode(f, fmt, h, w))
        assert np.array_equal(fr.decode(b, fmt, h, w, pitch=pitch), fr.decode(f, fmt, h, w))


# ---- the C ABI: rejected before any launch --------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_format_constants_match_the_header():
    from codd_amd import ops
    src = open(os.path.join(ROOT, "include", "codd_hip.h")).read()
    fmts = {k.lower(): int(v) for k, v in re.findall(r"#define CODD_FMT_([A-Z0-9_]+) (\d+)", src)}
    assert fmts == dict(ops.FRAME_FORMATS) and sorted(fmts.values()) == list(range(1, 9))
    assert tuple(ops.FRAME_FORMATS) == fr.FORMATS
    yuvs = {k.lower(): int(v) for k, v in re.findall(r"#define CODD_YUV_([A-Z0-9_]+) (\d+)", src)}
    assert yuvs == dict(ops.YUV_MATRICES) == dict(bt601=0, bt709=1, jpeg=2)


def test_ingest_frames_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    lib = _abi.load()
    assert "codd_ingest_frames" in _abi.SIGNATURES and lib.codd_ingest_frames is not None
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = _ptr(buf)
    m, s = (C.c_float * 3)(1, 2, 3), (C.c_float * 3)(1, 1, 1)

    def call(left=p, right=p, fmt=1, yuv=0, h=40, w=50, pitch=0, mean=m, std=s, lx=None, ly=None, rx=None, ry=None, H=64,
             W=64, ol=p, orr=p):
        return lib.codd_ingest_frames(left, right, fmt, yuv, h, w, pitch, mean, std, lx, ly, rx, ry, H, W, ol, orr, None)

    for name in ("left", "right", "mean", "std", "ol", "orr"):
        assert call(**{name: None}) == EINVAL, name
    for fmt in (0, 9, -1, 100):
        assert call(fmt=fmt) == EINVAL
    for fmt in (2, 3, 4):  # the YUV formats need a yuv row of the table
        assert call(fmt=fmt, yuv=3) == EINVAL and call(fmt=fmt, yuv=-1) == EINVAL
    # size rules of the table
    assert call(h=0) == EINVAL and call(w=0) == EINVAL and call(h=-2) == EINVAL
    assert call(fmt=2, w=49) == EINVAL and call(fmt=3, w=49) == EINVAL  # yuyv / uyvy: w even
    assert call(fmt=4, w=49) == EINVAL and call(fmt=4, h=39) == EINVAL  # nv12: w, h even
    for fmt in (5, 6, 7, 8):
        assert call(fmt=fmt, h=1, H=1) == EINVAL and call(fmt=fmt, w=1, W=1) == EINVAL  # Bayer: h, w >= 2
    # pitch: 0 or at least the row's bytes
    assert call(pitch=49) == EINVAL and call(pitch=-1) == EINVAL
    assert call(fmt=2, pitch=99) == EINVAL and call(fmt=3, pitch=50) == EINVAL  # 2w bytes per row
    assert call(fmt=4, pitch=49) == EINVAL and call(fmt=5, pitch=1) == EINVAL
    # maps: both of a view or neither
    assert call(lx=p) == EINVAL and call(ly=p) == EINVAL and call(rx=p) == EINVAL
    assert call(lx=p, ly=p, ry=p) == EINVAL
    # h <= H < 2h, w <= W < 2w
    assert call(H=39) == EINVAL and call(W=49) == EINVAL
    assert call(w=32, W=64) == EINVAL and call(h=32, H=64) == EINVAL


def test_frame_bytes():
    lib = _abi.load()
    fb = lib.codd_frame_bytes
    assert fb(4, 38, 54, 64) == 64 * 57  # nv12: Y rows + h/2 interleaved UV rows
    assert fb(4, 38, 54, 0) == 54 * 57
    assert fb(1, 37, 53, 0) == 37 * 53 and fb(1, 37, 53, 55) == 37 * 55 and fb(1, 1, 1, 0) == 1
    assert fb(2, 37, 54, 0) == 37 * 108 and fb(3, 37, 54, 110) == 37 * 110
    for fmt in (5, 6, 7, 8):
        assert fb(fmt, 2, 2, 0) == 4 and fb(fmt, 37, 53, 61) == 37 * 61
    assert fb(1, 540, 960, 0) == 518400 and fb(2, 540, 960, 0) == 2 * 518400 and fb(4, 540, 960, 0) == 777600
    assert fb(1, 70000, 70000, 0) == 70000 * 70000  # 64-bit
    for bad in ((0, 4, 4, 0), (9, 4, 4, 0), (1, 0, 4, 0), (1, 4, 0, 0), (2, 4, 5, 0), (3, 4, 5, 0), (4, 4, 5, 0), (4, 5, 4, 0),
                (5, 1, 4, 0), (8, 4, 1, 0), (1, 4, 4, 3), (2, 4, 4, 7), (1, 4, 4, -4)):
        assert fb(*bad) == -1, bad
    from codd_amd import ops
    assert ops.frame_bytes("nv12", 38, 54, 64) == 64 * 57 and ops.frame_bytes("yuyv", 4, 6) == 48
    with pytest.raises(ValueError):
        ops.frame_bytes("nv12", 38, 53)
    with pytest.raises(ValueError):
        ops.frame_bytes("rgb8", 4, 4)  # not a raw format


# ---- LiveSession -------------------------------------------------------------------------------------------------
def _cpu_session(shape=(40, 50), **kw):
    from codd_amd import configs
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.stereo_only()).eval()  # on the CPU: any device call would raise CoddHipError
    return LiveSession(est, shape, **kw)


def test_frame_layout():
    from codd_amd.live import PIXEL_FORMATS, frame_layout
    assert PIXEL_FORMATS == ("rgb8",) + fr.FORMATS
    assert frame_layout("rgb8", 40, 50) == (40, 150, 150, 6000)
    assert frame_layout("mono8", 37, 53) == (37, 53, 53, 37 * 53)
    assert frame_layout("mono8", 37, 53, 55) == (37, 53, 55, 37 * 55)
    assert frame_layout("yuyv", 37, 54) == (37, 108, 108, 37 * 108)
    assert frame_layout("uyvy", 37, 54, 110) == (37, 108, 110, 37 * 110)
    assert frame_layout("nv12", 38, 54, 64) == (57, 54, 64, 64 * 57)
    assert frame_layout("bayer_bggr", 2, 2) == (2, 2, 2, 4)
    lib = _abi.load()
    from codd_amd import ops
    for fmt in fr.FORMATS:  # the Python restatement agrees with the library and with the tests' own
        for h, w, pitch in ((38, 54, None), (38, 54, 120), (2, 2, None)):
            assert frame_layout(fmt, h, w, pitch)[3] == lib.codd_frame_bytes(ops.FRAME_FORMATS[fmt], h, w, pitch or 0)
            assert frame_layout(fmt, h, w, pitch) == fr.layout(fmt, h, w, pitch)
    for bad in (("rgb8", 4, 4, 12), ("yuv420", 4, 4, None), ("yuyv", 4, 5, None), ("nv12", 5, 4, None), ("nv12", 4, 5, None),
                ("bayer_rggb", 1, 4, None), ("mono8", 4, 4, 3), ("uyvy", 4, 4, 7), ("mono8", 0, 4, None)):
        with pytest.raises(ValueError):
            frame_layout(*bad)


def test_session_validates_pixel_format_configuration():
    for kw in (dict(pixel_format="yuv420"), dict(pixel_format="nv12", yuv="bt2020"), dict(yuv="rec709"),
               dict(pixel_format="mono8", pitch=49), dict(pixel_format="yuyv", pitch=99),
               dict(pixel_format="nv12", bgr=True), dict(pixel_format="bayer_rggb", bgr=True), dict(pitch=150),
               dict(pixel_format="rgb8", pitch=160)):
        with pytest.raises(ValueError):
            _cpu_session(**kw)
    for shape, fmt in (((40, 51), "yuyv"), ((40, 51), "uyvy"), ((40, 51), "nv12"), ((41, 50), "nv12"), ((1, 50), "bayer_gbrg")):
        with pytest.raises(ValueError):
            _cpu_session(shape=shape, pixel_format=fmt)
    s = _cpu_session(pixel_format="nv12", yuv="bt709", pitch=64)
    assert (s.pixel_format, s.yuv, s.pitch) == ("nv12", "bt709", 64) and not s._open_done
    s = _cpu_session(bgr=True)  # rgb8 keeps bgr=
    assert s.pixel_format == "rgb8" and s.bgr and s.pitch is None


def test_session_validates_raw_frames_before_touching_the_device():
    s = _cpu_session(pixel_format="nv12", pitch=64)
    good = np.zeros((60, 64), np.uint8)
    for bad in (np.zeros((40, 50, 3), np.uint8), np.zeros((60, 50), np.uint8), np.zeros((40, 64), np.uint8),
                np.zeros(60 * 64, np.uint8), good.astype(np.int8), np.zeros((60, 128), np.uint8)[:, ::2],
                torch.zeros(60, 64, dtype=torch.int16)):
        with pytest.raises(ValueError):
            s.push(good, bad)
        with pytest.raises(ValueError):
            s.push(bad, good)
    with pytest.raises(TypeError):
        s.push(good.tolist(), good)
    with pytest.raises(TypeError):
        s.step(None, good)
    assert s.pending() == 0 and not s._open_done
    # tight yuyv: (h, 2w) or (h, w, 2); with a pitch only (h, pitch)
    from codd_amd.live import check_raw_frame
    check_raw_frame(np.zeros((40, 100), np.uint8), "yuyv", (40, 50))
    check_raw_frame(torch.zeros(40, 50, 2, dtype=torch.uint8), "uyvy", (40, 50))
    check_raw_frame(np.zeros((40, 104), np.uint8), "yuyv", (40, 50), 104)
    with pytest.raises(ValueError):
        check_raw_frame(np.zeros((40, 50, 2), np.uint8), "yuyv", (40, 50), 104)
    with pytest.raises(ValueError):
        check_raw_frame(np.zeros((40, 50, 2), np.uint8), "mono8", (40, 50))
    # a valid pair gets past validation and is then refused by the device check: there is no CPU fallback
    with pytest.raises(_abi.CoddHipError):
        s.push(good, torch.from_numpy(good))


def test_cli_pixel_format_arguments():
    from codd_amd import inference
    for argv in (["--pixel-format", "nv12", "--frame-size", "38x54"],  # needs --live
                 ["--live", "--pixel-format", "nv12"],  # needs --frame-size
                 ["--live", "--frame-size", "38x54", "--pitch", "64"],  # --pitch needs --pixel-format
                 ["--live", "--pixel-format", "nv12", "--frame-size", "38"],
                 ["--live", "--pixel-format", "i420", "--frame-size", "38x54"]):
        with pytest.raises(SystemExit):
            inference.parse_args(argv)
    a = inference.parse_args(["--live", "--pixel-format", "nv12", "--frame-size", "38x54", "--pitch", "64", "--yuv", "bt709"])
    assert (a.pixel_format, a.frame_size, a.pitch, a.yuv) == ("nv12", (38, 54), 64, "bt709")


def test_raw_frame_iterator(tmp_path):
    from codd_amd import inference
    rng = np.random.default_rng(3)
    rows, _, pitch, nbytes = fr.layout("nv12", 4, 6, 8)
    frames = [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(3)]
    paths = []
    for i, f in enumerate(frames):
        paths.append(str(tmp_path / f"{i}.raw"))
        f.tofile(paths[-1])
    got = list(inference.iter_raw_frames(paths, paths[::-1], "nv12", (4, 6), 8))
    assert len(got) == 3
    for i, (left, right) in enumerate(got):
        assert left.shape == right.shape == (rows, pitch) and left.dtype == np.uint8 and left.flags["C_CONTIGUOUS"]
        assert np.array_equal(left.reshape(-1), frames[i]) and np.array_equal(right.reshape(-1), frames[2 - i])
    frames[0][:-1].tofile(paths[0])  # a truncated dump is an error, not a short frame
    with pytest.raises(ValueError):
        list(inference.iter_raw_frames(paths, paths, "nv12", (4, 6), 8))
