"""Restatement of codd_export_confidence (include/codd_hip.h) shared by the CPU and the GPU tests: the flags computed
with np.float32 operands row by row, the photometric residual in float64 with a per-element bound, the rule the MISMATCH
bit has to follow, and the cases.

Flags.  Every step the header fixes to an fp32 operation -- u = (float)x - d, f = floor(u), r = floor(u + 0.5f),
d + occ_px, the maximum over the offers -- is one numpy operation on np.float32 scalars, which round as the hardware
does, so bits 1 (OUT_OF_VIEW), 2 (OCCLUDED) and 128 (INVALID) are exact by construction and are compared bit for bit.
The z-buffer is a plain Python loop over the pixels of a row; it shares nothing with the kernel's passes.

Residual.  a = u - (float)f is exact in fp32 (f <= u < f + 1 are neighbours within a factor of two, or f = 0), so the
reference starts from the same fp32 u and a and evaluates

    residual = (1/3) sum_c stdv_c |L_c - (R0_c (1 - a) + R1_c a)|

in float64.  The fp32 expression of the header rounds, on the path of each input to the result:
    1 - a                      1 rounding   (R0 only)
    R0 (1 - a), R1 a           1            (R0, R1)
    their sum                  1            (R0, R1)
    L - Rv                     1            (all)
    |.| * stdv_c               1            (all)
    (e0 + e1) + e2             2 at most    (all)
    * (1/3)                    1, and the constant 1.f / 3.f is itself rounded: 1   (all)
which is 9 roundings for R0, 8 for R1 and 6 for L.  With unit roundoff eps = 2^-24 every term of the sum therefore
carries a factor (1 + delta)^k with k <= 9, |delta| <= eps, and |(1 + delta)^9 - 1| <= 9 eps / (1 - 9 eps) < 10 eps.
Taking absolute values term by term (|x| is 1-Lipschitz) gives

    |fp32 residual - exact residual| <= C * 2^-24 * M,   C = 10,
    M = (1/3) sum_c stdv_c (|L_c| + (1 - a) |R0_c| + a |R1_c|).

A fused multiply-add only removes roundings.  The float64 evaluation itself errs by about 10 * 2^-53 * M, nine orders
below the bound.  stdv enters both sides as the same fp32 numbers.

MISMATCH (bit 4) must equal ``ref_residual > tau`` wherever |ref_residual - tau| exceeds that pixel's bound; inside it
either answer is right.  The cases are built so that at most 1 % of a case's pixels are inside (tests/test_live_conf.py
asserts that on the reference alone).
"""
import numpy as np

OUT_OF_VIEW, OCCLUDED, MISMATCH, INVALID = 1, 2, 4, 128
C_BOUND = 10.0  # roundings on the longest path (9), rounded up for the second-order terms: see above
EPS = 2.0 ** -24
STD = (58.395, 57.12, 57.375)  # ops.IMAGENET_STD
MEAN = (123.675, 116.28, 103.53)
OCC_PX, TAU = 1.0, 24.0

# ((h, w), (H, W)): crop inside the padded planes
CASES = [((37, 61), (64, 64)),
         ((5, 3), (64, 64)),  # a row shorter than one 4-pixel store
         ((3, 1), (64, 64)),
         ((9, 517), (64, 576)),  # more than one pass of 256 lanes over 4-pixel units, and no multiple of 4
         ((64, 64), (64, 64))]  # no padding
AWKWARD = (0.0, -1.5, float("nan"), float("inf"), 1e-9)  # the last one leaves u == x


def awkward_positions(h, w):
    """Where case() puts AWKWARD[k % 5], k < 10 (every value twice): fixed positions folded into the crop."""
    return [((1 + 2 * k) % h, (2 + 3 * k) % w) for k in range(2 * len(AWKWARD))]


def _background(h, w, H, W):
    """(continuous, quarter-integer) slanted background disparity of the padded plane; base scales with narrow crops."""
    base = min(3.0, w / 8.0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cont = base + 0.02 * x + 0.03 * y
    return base, cont, (np.round(4.0 * cont) / 4.0).astype(np.float32)


def boxes(h, w):
    """The two fronto-parallel foreground boxes (y0, y1, x0, x1, d) of a crop; none in a crop narrower than 32."""
    if w < 32 or h < 8:
        return []
    return [(h // 4, h // 2, w // 3, w // 3 + max(w // 5, 4), 9.5),
            (h // 2 + 2, max(h - 3, h // 2 + 3), (2 * w) // 3, (2 * w) // 3 + max(w // 6, 4), 14.75)]


def _texture(c, y, x):
    """Grey level of the scene's surface at (possibly fractional) left-image position x of row y, channel c."""
    return (118.0 + 60.0 * np.sin(2 * np.pi * (x / 17.0 + y / 29.0 + c / 3.0))
            + 25.0 * np.sin(2 * np.pi * (x / 7.3 - y / 11.0 + c / 5.0)))


def case(shape, seed=0):
    """dict(disp fp32 [H,W], left / right fp32 [3,H,W] normalised, crop, padded, boxes).  The right image is the left one
    seen through the BACKGROUND disparity (so the boxes mismatch) plus +-2 grey levels of noise."""
    (h, w), (H, W) = shape
    rng = np.random.default_rng(1000 * h + w + seed)
    base, _, disp = _background(h, w, H, W)
    for y0, y1, x0, x1, d in boxes(h, w):
        disp[y0:y1, x0:x1] = d
    if w >= 2:
        disp[h - 1, 1] = 1.0  # u == 0 exactly: in view
    for (y, x), v in zip(awkward_positions(h, w), AWKWARD + AWKWARD):
        disp[y, x] = v
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    left = np.stack([_texture(c, yy, xx) for c in range(3)])
    # right column x' shows the background point whose left column x solves x - (base + 0.02 x + 0.03 y) = x'
    src = (xx + base + 0.03 * yy) / (1.0 - 0.02)
    right = np.stack([_texture(c, yy, src) for c in range(3)]) + rng.uniform(-2.0, 2.0, (3, H, W))
    norm = lambda g: ((np.clip(g, 0.0, 255.0).astype(np.float32) - np.array(MEAN, np.float32)[:, None, None])  # noqa: E731
                      / np.array(STD, np.float32)[:, None, None]).astype(np.float32)
    return dict(disp=disp, left=norm(left), right=norm(right), crop=(h, w), padded=(H, W), boxes=boxes(h, w))


def flags_reference(disp, crop, occ_px=OCC_PX):
    """Bits 1, 2, 128 of the crop, uint8 [h,w], and (u, f, r) as fp32 / int arrays (-1 where the pixel has none)."""
    h, w = crop
    flags = np.zeros((h, w), np.uint8)
    U = np.full((h, w), np.nan, np.float32)
    F = np.full((h, w), -1, np.int64)
    R = np.full((h, w), -1, np.int64)
    occ = np.float32(occ_px)
    for y in range(h):
        zbuf = [np.float32(0.0)] * w
        for x in range(w):
            d = np.float32(disp[y, x])
            if not (np.isfinite(d) and d > 0):
                flags[y, x] = INVALID
                continue
            u = np.float32(x) - d  # one fp32 subtraction
            if u < 0:
                flags[y, x] = OUT_OF_VIEW
                continue
            f = int(np.floor(u))
            U[y, x], F[y, x], R[y, x] = u, f, int(np.floor(u + np.float32(0.5)))
            for c in (f, f + 1):
                if c < w and d > zbuf[c]:
                    zbuf[c] = d
        for x in range(w):
            if R[y, x] >= 0:
                assert R[y, x] in (F[y, x], F[y, x] + 1) and R[y, x] < w
                d = np.float32(disp[y, x])
                if zbuf[R[y, x]] > d + occ:  # one fp32 add
                    flags[y, x] |= OCCLUDED
    return flags, U, F, R


def _taps(c, U, F):
    """L, R0, R1 [3,h,w] and a [h,w] (fp32 values) of the pixels that have a residual; ``ok`` marks them."""
    h, w = U.shape
    ok = F >= 0
    f = np.where(ok, F, 0)
    x1 = np.minimum(f + 1, w - 1)
    rows = np.arange(h)[:, None]
    L = c["left"][:, :h, :w]
    R0 = c["right"][:, rows, f]
    R1 = c["right"][:, rows, x1]
    a = (np.where(ok, U, 0).astype(np.float32) - f.astype(np.float32)).astype(np.float32)
    return ok, L, R0, R1, a


def residual_reference(c, U, F, std=STD):
    """(residual float64 [h,w], NaN where the pixel has none; bound float64 [h,w])."""
    ok, L, R0, R1, a = _taps(c, U, F)
    s = np.array(std, np.float32).astype(np.float64)[:, None, None]
    L, R0, R1, a = (t.astype(np.float64) for t in (L, R0, R1, a))
    res = (s * np.abs(L - (R0 * (1.0 - a) + R1 * a))).sum(0) / 3.0
    M = (s * (np.abs(L) + (1.0 - a) * np.abs(R0) + a * np.abs(R1))).sum(0) / 3.0
    return np.where(ok, res, np.nan), np.where(ok, C_BOUND * EPS * M, 0.0)


def residual_fp32(c, U, F, std=STD):
    """The header's expression evaluated operation by operation in np.float32 (what the kernel computes)."""
    ok, L, R0, R1, a = _taps(c, U, F)
    s = np.array(std, np.float32)
    b = np.float32(1.0) - a
    e = [np.abs(L[k] - (R0[k] * b + R1[k] * a)) * s[k] for k in range(3)]
    res = ((e[0] + e[1]) + e[2]) * (np.float32(1.0) / np.float32(3.0))
    assert res.dtype == np.float32
    return np.where(ok, res, np.float32(np.nan))


def reference(c, occ_px=OCC_PX, tau=TAU, images=True):
    """dict(flags124: bits 1 | 2 | 128, residual, bound, mismatch: the rule's answer, decided: where the rule binds)."""
    flags, U, F, R = flags_reference(c["disp"], c["crop"], occ_px)
    out = dict(flags124=flags, U=U, F=F)
    if images:
        res, bound = residual_reference(c, U, F)
        with np.errstate(invalid="ignore"):
            out.update(residual=res, bound=bound, mismatch=res > tau, decided=~(np.abs(res - tau) <= bound))
    return out


def check_outputs(flags, residual, ref, tau=TAU, name=""):
    """The GPU (or fp32) outputs against ``reference``: exact bits 1, 2, 128; residual within the bound and NaN exactly
    where the reference is; bit 4 by the rule.  Returns the largest error / bound ratio."""
    assert flags.dtype == np.uint8 and flags.shape == ref["flags124"].shape
    assert np.array_equal(flags & 0x83, ref["flags124"]), f"{name}: bits 1, 2, 128 differ at {np.argwhere((flags & 0x83) != ref['flags124'])[:8].tolist()}"
    assert not (flags & 0x78).any(), f"{name}: undefined bits set"
    got4 = (flags & MISMATCH) != 0
    if "residual" not in ref:
        assert not got4.any(), f"{name}: MISMATCH set without images"
        return 0.0
    nan = np.isnan(ref["residual"])
    assert np.array_equal(np.isnan(residual), nan), f"{name}: NaN pattern of the residual differs"
    err = np.abs(np.where(nan, 0.0, residual.astype(np.float64) - np.where(nan, 0.0, ref["residual"])))
    ratio = float((err[~nan] / ref["bound"][~nan]).max()) if (~nan).any() else 0.0
    print(f"{name}: residual error / bound max {ratio:.3f}, largest error {err.max():.3e}")
    assert (err <= ref["bound"]).all(), f"{name}: residual outside the bound, ratio {ratio}"
    d = ref["decided"]
    assert np.array_equal(got4[d], ref["mismatch"][d]), f"{name}: MISMATCH differs from the reference outside the bound"
    assert not got4[nan].any()
    return ratio
