"""The live-ingest launches whose output bits tests/golden/ingest_bits.json records (sha256 of the bytes of one output
view), shared by the generator tools/parent_bits.py --cases ingest, by tests/test_gpu_ingest_bits.py and by
tests/test_ingest_cases.py.  The recorded bits are those of the library BEFORE the three ingest kernels became one and
the bilinear blend got a pinned operation order.  Every case here is EXACT -- no map, an identity map, or a 1/64-pixel
map, on which every intermediate of the blend is a short dyadic number -- so any correct evaluation order gives the same
bits and every output byte stays.

Sizes: an image of 38 x 54 in an output of 64 x 64 (16-byte stores) and of 40 x 55 (W % 4 != 0: the scalar stores).
Map kinds: ``free`` no maps; ``off1`` no maps, both sources at byte offset 1 of their allocation; ``identity``; ``q64`` a
1/64-pixel zoom-out that leaves the source on all four sides, with a NaN, a +inf and a -inf entry (the right view's map
is the left's turned by 180 degrees); ``left`` / ``right``: only that view has the q64 map; ``pitch`` / ``pitch_q64``: rows
3 bytes wider than the row, padding bytes random.

* ``pair/<size>/bgr<b>/<kind>/<view>``: ops.ingest_pair.
* ``frames/<size>/<fmt>-<yuv>/<kind>/<view>``: ops.ingest_frames, the eight formats under bt601 and nv12 under all three
  yuv rows.
* ``calib/<size>/<fmt>[-bgr]/<view>``: ops.ingest_calibrated with the OTHER view calibrated; <view> has no calibration,
  takes the map-free path and is the one digested (the calibrated view blends at unquantised positions: not exact).
* ``maps/<model>/<h>x<w>/<view>``: ops.rectify_maps, both maps of the view; 37 x 53 takes the scalar stores."""
import functools
import zlib

import numpy as np
import torch

import live_calib_ref as cr
import live_fmt_ref as fr
from parent_bits import DEV, digest

NAME = "ingest"
# the sources of the ingest entries, in the tree of the fixture's commit and in this one
SOURCES = ("codd_amd/csrc/live.hip", "codd_amd/csrc/ingest_decode.h", "codd_amd/csrc/ingest_formats.hip",
           "codd_amd/csrc/ingest_calib.hip", "codd_amd/csrc/ingest.hip")
IMAGE = (38, 54)
OUTPUTS = ((64, 64), (40, 55))
VIEWS = ("left", "right")
PAIR_KINDS = ("free", "off1", "identity", "q64", "left", "right")
FRAME_KINDS = PAIR_KINDS + ("pitch", "pitch_q64")
FRAME_FORMATS = tuple((f, "bt601") for f in fr.FORMATS) + (("nv12", "bt709"), ("nv12", "jpeg"))
CALIB_FORMATS = (("rgb8", False), ("rgb8", True)) + tuple((f, False) for f in fr.FORMATS)
MODELS = ("brown", "fisheye")
MAP_SHAPES = ((38, 54), (37, 53))


def size_id(HW):
    return "%dx%din%dx%d" % (IMAGE + tuple(HW))


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def source(fmt):
    """Two tight frames of random bytes with planted extremes; rgb8: [h,w,3], a raw format: flat."""
    h, w = IMAGE
    rng = np.random.default_rng(zlib.crc32(("ingest bits " + fmt).encode()))
    out = []
    for _ in range(2):
        f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if fmt == "rgb8" else fr.random_frame(rng, fmt, h, w)
        flat = f.reshape(-1)
        flat[:8], flat[-8:] = 0, 255
        flat[20:24], flat[24:28] = (255, 0, 255, 0), (0, 255, 0, 255)
        out.append(f)
    return tuple(out)


def row_bytes(fmt):
    return 3 * IMAGE[1] if fmt == "rgb8" else fr.layout(fmt, *IMAGE)[1]


@functools.lru_cache(maxsize=None)
def padded(fmt):
    """source(fmt) with rows of row_bytes + 3 bytes, the padding random -> (pitch, frames)."""
    pitch = row_bytes(fmt) + 3
    rng = np.random.default_rng(17)
    out = []
    for f in source(fmt):
        rows = f.size // row_bytes(fmt)
        b = rng.integers(0, 256, (rows, pitch), dtype=np.uint8)
        b[:, :row_bytes(fmt)] = f.reshape(rows, row_bytes(fmt))
        out.append(b.reshape(-1))
    return pitch, tuple(out)


def _q64(a):
    return (np.round(np.asarray(a, np.float64) * 64.0) / 64.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_maps(kind):
    """((lmx, lmy), (rmx, rmy)) of fp32 [h,w] arrays, a pair None where the view has no map."""
    h, w = IMAGE
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if kind in ("free", "off1", "pitch"):
        return None, None
    if kind == "identity":
        m = (xx.astype(np.float32), yy.astype(np.float32))
        return m, m
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    mx, my = _q64(cx + 1.25 * (xx - cx) + 0.375), _q64(cy + 1.25 * (yy - cy) - 0.640625)
    assert mx.min() < -1 and mx.max() > w and my.min() < -1 and my.max() > h
    mx[h // 2, w // 3], my[h // 3, w // 2], mx[1, 1] = np.nan, np.inf, -np.inf
    lm = (mx, my)
    rm = tuple(np.ascontiguousarray(m[::-1, ::-1]) for m in lm)
    return (None if kind == "right" else lm), (None if kind == "left" else rm)


def _dev(a, offset=None):
    a = np.ascontiguousarray(a)
    if offset is None:
        return torch.from_numpy(a).to(DEV)
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device=DEV)
    t = buf[offset:offset + a.size]
    t.copy_(torch.from_numpy(a.reshape(-1)))
    assert t.data_ptr() % 4 == offset % 4
    return t.view(a.shape)


def _dev_maps(kind):
    return tuple(None if p is None else tuple(_dev(m) for m in p) for p in host_maps(kind))


def _outputs(HW):
    return tuple(torch.full((1, 3) + tuple(HW), float("nan"), device=DEV) for _ in range(2))


@functools.lru_cache(maxsize=None)
def rectification(model, shape):
    from codd_amd.calibration import CameraModel, StereoCalibration
    (Kl, dl), (Kr, dr), R, T = cr.make_rig(model, shape)
    rig = StereoCalibration(CameraModel(shape, Kl, model, dl), CameraModel(shape, Kr, model, dr), R, T)
    return rig.rectify(shape, zoom=0.8)


# ------------------------------------------------------------------------------------------------ groups
def pair_keys(HW):
    return ["pair/%s/bgr%d/%s/%s" % (size_id(HW), b, k, v) for b in (0, 1) for k in PAIR_KINDS for v in VIEWS]


def pair_digests(HW):
    from codd_amd import ops
    out = {}
    for b in (0, 1):
        for kind in PAIR_KINDS:
            src = [_dev(f, 1 if kind == "off1" else None) for f in source("rgb8")]
            o = _outputs(HW)
            ops.ingest_pair(src[0], src[1], o[0], o[1], bgr=bool(b), maps=_dev_maps(kind))
            for v, t in zip(VIEWS, o):
                out["pair/%s/bgr%d/%s/%s" % (size_id(HW), b, kind, v)] = digest(t)
    return out


def frames_keys(HW):
    return ["frames/%s/%s-%s/%s/%s" % (size_id(HW), f, y, k, v) for (f, y) in FRAME_FORMATS for k in FRAME_KINDS for v in VIEWS]


def frames_digests(HW):
    from codd_amd import ops
    out = {}
    for fmt, yuv in FRAME_FORMATS:
        for kind in FRAME_KINDS:
            pitch, frames = padded(fmt) if kind.startswith("pitch") else (None, source(fmt))
            src = [_dev(f, 1 if kind == "off1" else None) for f in frames]
            o = _outputs(HW)
            ops.ingest_frames(src[0], src[1], o[0], o[1], fmt, IMAGE, yuv=yuv, pitch=pitch,
                              maps=_dev_maps("q64" if kind == "pitch_q64" else kind))
            for v, t in zip(VIEWS, o):
                out["frames/%s/%s-%s/%s/%s" % (size_id(HW), fmt, yuv, kind, v)] = digest(t)
    return out


def calib_keys(HW):
    return ["calib/%s/%s%s/%s" % (size_id(HW), f, "-bgr" if b else "", v) for (f, b) in CALIB_FORMATS for v in VIEWS]


def calib_digests(HW):
    from codd_amd import ops
    out = {}
    for fmt, bgr in CALIB_FORMATS:
        for i, v in enumerate(VIEWS):  # view i has no calibration; the other one has (brown for one, fisheye for the other)
            views = list(rectification(MODELS[i], IMAGE).views)
            views[i] = None
            src = [_dev(f) for f in source(fmt)]
            o = _outputs(HW)
            ops.ingest_calibrated(src[0], src[1], o[0], o[1], tuple(views), fmt, IMAGE, IMAGE, bgr=bgr)
            out["calib/%s/%s%s/%s" % (size_id(HW), fmt, "-bgr" if bgr else "", v)] = digest(o[i])
    return out


def maps_keys(model):
    return ["maps/%s/%dx%d/%s" % ((model,) + s + (v,)) for s in MAP_SHAPES for v in VIEWS]


def maps_digests(model):
    from codd_amd import ops
    out = {}
    for s in MAP_SHAPES:
        maps = ops.rectify_maps(rectification(model, s), s, DEV)
        for v, (mx, my) in zip(VIEWS, maps):
            out["maps/%s/%dx%d/%s" % ((model,) + s + (v,))] = digest(torch.stack([mx, my]))
    return out


# ------------------------------------------------------------------------------------------------ all of it
def groups():
    """[(group id, keys, function -> {key: digest})] in the fixture's order."""
    out = []
    for HW in OUTPUTS:
        out += [("pair/" + size_id(HW), pair_keys(HW), functools.partial(pair_digests, HW)),
                ("frames/" + size_id(HW), frames_keys(HW), functools.partial(frames_digests, HW)),
                ("calib/" + size_id(HW), calib_keys(HW), functools.partial(calib_digests, HW))]
    return out + [("maps/" + m, maps_keys(m), functools.partial(maps_digests, m)) for m in MODELS]
