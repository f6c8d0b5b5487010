"""fp64 numpy restatements of the two live-session kernels (include/codd_hip.h: codd_ingest_pair, codd_export_depth),
written from their stated contracts, not from the kernels."""
import numpy as np

MEAN = np.array([123.675, 116.28, 103.53], np.float32).astype(np.float64)  # RGB order; the fp32 values the kernel is given
STD = np.array([58.395, 57.12, 57.375], np.float32).astype(np.float64)


def remap(img, map_x, map_y):
    """Bilinear sample of ``img`` [h,w,3] at (map_x, map_y) [h,w]: fp64 [h,w,3] in raw uint8 units.  Taps outside the
    source contribute 0; a non-finite map entry gives 0; nothing is rounded back to uint8."""
    h, w = img.shape[:2]
    src = img.astype(np.float64)
    sx, sy = np.asarray(map_x, np.float64), np.asarray(map_y, np.float64)
    finite = np.isfinite(sx) & np.isfinite(sy)
    sx, sy = np.where(finite, sx, -10.0), np.where(finite, sy, -10.0)
    # (far outside is all zeros anyway: clip so that the integer conversion below is defined)
    sx, sy = np.clip(sx, -10.0, w + 10.0), np.clip(sy, -10.0, h + 10.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = (sx - x0)[..., None], (sy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(inside[..., None], v, 0.0)

    top = tap(y0, x0) * (1 - ax) + tap(y0, x0 + 1) * ax
    bot = tap(y0 + 1, x0) * (1 - ax) + tap(y0 + 1, x0 + 1) * ax
    return np.where(finite[..., None], top * (1 - ay) + bot * ay, 0.0)


def ingest(img, H, W, bgr, maps=None):
    """uint8 [h,w,3] -> fp64 [3,H,W]: (rectified,) reflect-padded (BORDER_REFLECT_101, bottom / right), RGB, normalised."""
    h, w = img.shape[:2]
    v = img.astype(np.float64) if maps is None else remap(img, *maps)
    v = np.pad(v, ((0, H - h), (0, W - w), (0, 0)), mode="reflect")
    if bgr:
        v = v[..., ::-1]
    return np.transpose((v - MEAN) / STD, (2, 0, 1))


def export(disp, h, w, mode, calib=1.0):
    """Padded disparity [H,W] fp32 -> the cropped result: 'disp' fp32, 'depth' fp64 calib / disp, 'disp_u16' uint16
    round-half-even(disp * 256) clamped to [0, 65535] with non-finite -> 0."""
    d = np.asarray(disp)[:h, :w]
    if mode == "disp":
        return d.copy()
    if mode == "depth":
        with np.errstate(divide="ignore"):
            return np.float64(np.float32(calib)) / d.astype(np.float64)
    assert mode == "disp_u16", mode
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.rint(d.astype(np.float64) * 256.0), 0.0, 65535.0)  # np.rint rounds half to even
    return np.where(np.isfinite(d), q, 0.0).astype(np.uint16)
