"""numpy integer restatements of the raw-frame decoders D_F of codd_ingest_frames (include/codd_hip.h), written from the
stated contract, not from the kernel: D_F(frame bytes) -> uint8 [h,w,3] RGB.  Every byte string of the right length is a
valid frame, so the tests feed random bytes and need no encoder."""
import numpy as np

FORMATS = ("mono8", "yuyv", "uyvy", "nv12", "bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr")
YUV_FORMATS = ("yuyv", "uyvy", "nv12")
# yuv row -> yoff, (CY, CVR, CUG, CVG, CUB) as real numbers; the integers are the nearest to c * 2^20
YUV = dict(bt601=(16, (1.164, 1.596, 0.391, 0.813, 2.018)),
           bt709=(16, (1.164, 1.793, 0.213, 0.533, 2.112)),
           jpeg=(0, (1.000, 1.402, 0.344, 0.714, 1.772)))
SHIFT = 20


def coefficients(yuv):
    yoff, real = YUV[yuv]
    return yoff, tuple(int(np.floor(c * (1 << SHIFT) + 0.5)) for c in real)


def layout(fmt, h, w, pitch=None):
    """(rows, row_bytes, pitch, nbytes) of one view."""
    row_bytes = 2 * w if fmt in ("yuyv", "uyvy") else w
    rows = h + h // 2 if fmt == "nv12" else h
    p = row_bytes if pitch is None else pitch
    assert p >= row_bytes
    return rows, row_bytes, p, rows * p


def yuv_to_rgb(Y, U, V, yuv, accumulators=None):
    """Integer arrays (any shape) -> uint8 [..., 3].  ``accumulators``: a list that receives every pre-shift sum."""
    yoff, (cy, cvr, cug, cvg, cub) = coefficients(yuv)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    yy = np.maximum(Y - yoff, 0) * cy
    half = 1 << (SHIFT - 1)
    acc = (yy + half + cvr * (V - 128), yy + half - cug * (U - 128) - cvg * (V - 128), yy + half + cub * (U - 128))
    if accumulators is not None:
        accumulators.extend([yy, cvr * (V - 128), cug * (U - 128), cvg * (V - 128), cub * (U - 128), *acc])
    return np.stack([np.clip(a >> SHIFT, 0, 255) for a in acc], axis=-1).astype(np.uint8)  # (>> on int64: arithmetic)


def yuv_to_rgb_real(Y, U, V, yuv):
    """The real-valued formula the integers approximate, float64, clipped to [0, 255] and NOT rounded."""
    yoff, (cy, cvr, cug, cvg, cub) = YUV[yuv]
    Y, U, V = (np.asarray(a).astype(np.float64) for a in (Y, U, V))
    yy = np.maximum(Y - yoff, 0.0) * cy
    rgb = (yy + cvr * (V - 128), yy - cug * (U - 128) - cvg * (V - 128), yy + cub * (U - 128))
    return np.stack([np.clip(a, 0.0, 255.0) for a in rgb], axis=-1)


def demosaic(mosaic, pattern):
    """uint8 [h,w] mosaic, pattern 'rggb' | 'grbg' | 'gbrg' | 'bggr' -> uint8 [h,w,3]: bilinear on the 3x3 window of the
    mosaic extended by reflect-101."""
    h, w = mosaic.shape
    P = np.pad(mosaic.astype(np.int64), 1, mode="reflect")  # numpy's 'reflect' is reflect-101: -1 -> 1, n -> n - 2
    C = P[1:-1, 1:-1]
    N, S, Wn, E = P[:-2, 1:-1], P[2:, 1:-1], P[1:-1, :-2], P[1:-1, 2:]
    NW, NE, SW, SE = P[:-2, :-2], P[:-2, 2:], P[2:, :-2], P[2:, 2:]
    cross, diag = (N + S + Wn + E + 2) >> 2, (NW + NE + SW + SE + 2) >> 2
    hor, ver = (Wn + E + 1) >> 1, (N + S + 1) >> 1
    out = np.zeros((h, w, 3), np.int64)
    chan = dict(r=0, g=1, b=2)
    for py in range(2):
        for px in range(2):
            colour = pattern[2 * py + px]
            site = (slice(py, None, 2), slice(px, None, 2))
            if colour == "g":
                row_colour = pattern[2 * py + (px ^ 1)]  # its row neighbours
                col_colour = pattern[2 * (py ^ 1) + px]  # its column neighbours
                out[site + (1,)] = C[site]
                out[site + (chan[row_colour],)] = hor[site]
                out[site + (chan[col_colour],)] = ver[site]
            else:
                out[site + (chan[colour],)] = C[site]
                out[site + (1,)] = cross[site]
                out[site + (chan["b" if colour == "r" else "r"],)] = diag[site]
    return out.astype(np.uint8)


def decode(frame, fmt, h, w, yuv="bt601", pitch=None):
    """D_F: the frame's bytes (any shape, ``nbytes`` of ``layout``) -> uint8 [h,w,3] RGB."""
    rows, row_bytes, p, nbytes = layout(fmt, h, w, pitch)
    b = np.asarray(frame, np.uint8).reshape(-1)
    assert b.size == nbytes, (b.size, nbytes)
    b = b.reshape(rows, p)[:, :row_bytes]
    if fmt == "mono8":
        return np.repeat(b[:h, :, None], 3, axis=2)
    if fmt in ("yuyv", "uyvy"):
        q = b.reshape(h, w // 2, 4)
        yo = 0 if fmt == "yuyv" else 1
        Y = np.stack([q[..., yo], q[..., yo + 2]], axis=-1).reshape(h, w)
        U, V = np.repeat(q[..., 1 - yo], 2, axis=1), np.repeat(q[..., 3 - yo], 2, axis=1)
        return yuv_to_rgb(Y, U, V, yuv)
    if fmt == "nv12":
        Y, uv = b[:h], b[h:].reshape(h // 2, w // 2, 2)
        U, V = (np.repeat(np.repeat(uv[..., k], 2, axis=0), 2, axis=1) for k in (0, 1))
        return yuv_to_rgb(Y, U, V, yuv)
    assert fmt.startswith("bayer_"), fmt
    return demosaic(b, fmt[len("bayer_"):])


def mosaic_of(rgb, pattern):
    """The mosaic a sensor with this pattern records of an RGB image [h,w,3]."""
    h, w = rgb.shape[:2]
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ch = np.array([dict(r=0, g=1, b=2)[c] for c in pattern])[2 * (yy & 1) + (xx & 1)]
    return np.take_along_axis(rgb, ch[..., None], axis=2)[..., 0].astype(np.uint8)


def random_frame(rng, fmt, h, w):
    """A tight frame of random bytes, flat."""
    return rng.integers(0, 256, layout(fmt, h, w)[3], dtype=np.uint8)


def with_pitch(frame, fmt, h, w, pitch, fill):
    """The tight ``frame`` laid out with ``pitch`` bytes per row; the padding bytes are ``fill`` (a byte, or a callable
    returning an array of the padding's shape)."""
    rows, row_bytes, _, _ = layout(fmt, h, w)
    out = np.empty((rows, pitch), np.uint8)
    out[:, :row_bytes] = np.asarray(frame, np.uint8).reshape(rows, row_bytes)
    out[:, row_bytes:] = fill((rows, pitch - row_bytes)) if callable(fill) else fill
    return out.reshape(-1)
