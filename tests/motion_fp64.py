"""fp64 references, product-shaped inputs and bounds for the RAFT3D kernels around the update loop (correlation
pyramid, pyramid lookup, per-iteration geometry, induced flow, disparity -> depth, 2x2 pooling, instance norm, convex
up-sampling), for tests/test_motion_fp64_reference.py (CPU: the fp32 oracle against these references -- the measurement
that sets every constant below -- and the power of the bounds) and tests/test_gpu_motion_fp64.py (the HIP kernels).

Every reference returns its value AND the first-order magnitude ``M`` of the arithmetic that forms it; the bound of an
output element is  |got - ref64| <= c * 2^-24 * M  with one scalar ``c`` per kernel (C below).  ``c`` is 4 x the worst
|oracle32 - ref64| / (2^-24 M) that the project's fp32 CPU oracle reaches on these very inputs, rounded up to two
digits (MEASURED holds the measured values; test_fp32_oracle_within_a_quarter_of_every_bound re-measures them).  4 x:
a GPU evaluation differs from the CPU's fp32 by FMA contraction, the order of the 4- and 9-term sums and libm functions
that are allowed 1-2 ulp; none of that is worth more than a small factor over an independent fp32 evaluation.

Four magnitudes carry a term for a property of fp32 arithmetic that the plain sum of |terms| misses; each is explained
where it is formed: the lookup's fraction of a level coordinate inside (-1, 0) (lookup), a soft-max weight that
underflows (_cvx_mag), the coordinate at which the 1/d2 sample is taken (geometry) and the uncertainty of a mean summed
in fp32 (instnorm).  The first three were needed for the fp32 CPU oracle itself, the last one for the HIP kernel."""
import math

import torch
import torch.nn.functional as F

from oracle import motion as om
from oracle import se3

F64 = torch.float64
U = 2.0 ** -24
MIN_DEPTH = om.MIN_DEPTH
BF = om.BF_DEFAULT

# (B, h, w) at 1/8 resolution: the benchmarked 960x576; 640x512 at B = 2; 1280x384 (KITTI); odd sizes (h*w = 16*141 + 1,
# not a multiple of 4, a row or column dropped at every pooling, one partial 64-pixel up-sampling segment) at B = 2; a
# map whose level 3 is 2x2 and whose last lookup workgroup is mostly tail
CASES = [(1, 72, 120), (2, 64, 80), (1, 48, 160), (2, 37, 61), (1, 17, 23)]
FULLRES_CASES = [CASES[0], CASES[3]]  # (induced_flow, disp_to_depth, subsample run at 8x these)
INORM_CASES = [(B, C, h, w) for C in (64, 128) for (B, h, w) in CASES] + [(1, 64, 288, 480)]
case_id = lambda c: "B%d_" % c[0] + "x".join(str(v) for v in c[1:])

# worst |oracle32 - ref64| / (2^-24 M) of the fp32 CPU oracle over the cases above (CPU measurement) ...
MEASURED = {
    "pyramid_fp32": 11.3, "lookup": 3.85, "xyz_uv": 1.43, "xyz_z": 1.68, "minfo_flow": 0.786, "minfo_twist": 3.98,
    "minfo_dz": 1.9, "induced_flow": 2.02, "disp_to_depth": 1.59, "avgpool2": 2.22, "instnorm": 1.13, "cvx": 9.15,
    "cvx_se3_t": 4.14, "cvx_se3_q": 6.54, "se3_exp_t": 2.58,
}
# ... and c = 4 x that, rounded up to two digits
C = {
    "pyramid_fp32": 46.0, "lookup": 16.0, "xyz_uv": 5.8, "xyz_z": 6.8, "minfo_flow": 3.2, "minfo_twist": 16.0,
    "minfo_dz": 7.6, "induced_flow": 8.1, "disp_to_depth": 6.4, "avgpool2": 8.9, "instnorm": 4.6, "cvx": 37.0,
    "cvx_se3_t": 17.0, "cvx_se3_q": 27.0, "se3_exp_t": 11.0,
}
# the project's split-bf16 / split-fp16 GEMM bounds (test_split_bf16_conv_every_launch_configuration)
SPLIT_BOUND = {"split": (3.5 * 2.0 ** -18, 2e-7), "split16": (2.0 ** -20, 2e-7)}
# th^2 >= 1e-6 as the fp32 code sees it: th^2 is a 3-term fp32 sum, a few 2^-24 off the fp64 value
TH2_CLOSED_FORM = 1e-6 * (1 - 2.0 ** -20)


def intrinsics(h, w, scale=1.0):
    """(fx, fy, cx, cy) of an h x w map at 1/8 resolution (scale = 8: the full-resolution frame)."""
    return (131.25 * scale, 131.25 * scale, (w / 2.0 - 0.25) * scale, (h / 2.0 + 0.375) * scale)


def _gen(tag, *shape):
    return torch.Generator().manual_seed(7919 * tag + sum((i + 1) * 131 * int(s) for i, s in enumerate(shape)))


# ------------------------------------------------------------------------------------------------ inputs
REGIMES = ("identity", "1e-4", "1e-3..1e-2", "0.1", "1..3")


def se3_field(B, h, w, tmax, g):
    """fp32 SE3 field [B,h,w,7] + the rotation regime of every pixel [B,h,w] (index into REGIMES): exact identity;
    |phi| ~ 1e-4 (the series branch); |phi| log-uniform in [1e-3, 1e-2] (the cancellation range of left_jac_apply,
    every 7th planted at 1.0005e-3); ~0.1; a few at 1 .. 3 rad, half of them stored with q.w < 0.  |t| <= tmax."""
    N = B * h * w
    r = torch.rand(N, generator=g)
    regime = torch.full((N,), 3, dtype=torch.long)
    regime[r < 0.70] = 2
    regime[r < 0.35] = 1
    regime[r < 0.15] = 0
    big = torch.randperm(N, generator=g)[:max(6, N // 400)]
    regime[big] = 4
    dirn = torch.randn(N, 3, generator=g, dtype=F64)
    dirn = dirn / dirn.norm(dim=-1, keepdim=True)
    u = torch.rand(N, generator=g, dtype=F64)
    ang = torch.zeros(N, dtype=F64)
    ang = torch.where(regime == 1, 1e-4 * (0.5 + u), ang)
    mid = 10.0 ** (-3.0 + u)
    cut = torch.zeros(N, dtype=torch.bool)
    cut[torch.nonzero(regime == 2)[::7, 0]] = True
    ang = torch.where(regime == 2, torch.where(cut, torch.full_like(u, 1.0005e-3), mid), ang)
    ang = torch.where(regime == 3, 0.1 * (0.5 + u), ang)
    ang = torch.where(regime == 4, 1.0 + 2.0 * u, ang)
    tau = (torch.randn(N, 3, generator=g, dtype=F64) * tmax / 3).clamp(-tmax, tmax)
    T = se3.exp(torch.cat([tau, dirn * ang[:, None]], -1)).float()
    T[regime == 0] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    T[big[::2], 3:] *= -1.0  # the same rotations, q.w < 0
    return T.view(B, h, w, 7).contiguous(), regime.view(B, h, w)


def depth_map(B, h, w, g):
    """Depths log-uniform over 0.7 .. 60 (210 / disparity, disparities up to 320), smooth at the scale of a few pixels
    (three random sinusoids in log depth) with 1 % per-pixel noise, as a depth map of a scene is."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=F64) / max(h, 8), torch.arange(w, dtype=F64) / max(w, 8), indexing="ij")
    f = torch.zeros(B, h, w, dtype=F64)
    for _ in range(3):
        a, fy, fx, ph = [torch.rand(B, 1, 1, generator=g, dtype=F64) for _ in range(4)]
        f = f + (0.3 + a) * torch.sin(2 * math.pi * ((fy * 2 - 1) * 1.5 * yy + (fx * 2 - 1) * 1.5 * xx + ph))
    lo, hi = f.amin((1, 2), keepdim=True), f.amax((1, 2), keepdim=True)
    d = 0.7 * torch.exp((f - lo) / (hi - lo) * math.log(60.0 / 0.7))
    d = d * (1 + 0.01 * torch.randn(B, h, w, generator=g, dtype=F64))
    return d.clamp(0.7, 60.0).float()


def near_patch(h, w):
    return min(h // 3, h - 2), max(0, min(w // 4, w - 3))


def geometry_case(B, h, w, scale=1, tag=1):
    """Inputs of raft_geometry / induced_flow at (scale h) x (scale w): dict(T, regime, d1, d2, K).  T: se3_field with
    |t| <= 0.3; d1, d2: depth_map; d1 with a few planted 0 and 0.02 (< MIN_DEPTH, t.z = 0.01 there) and a 2 x 2 patch at depth 0.3 that
    its own motion (t.z = -0.8) puts behind the camera, as gn_fp64.make_case does."""
    H, W = h * scale, w * scale
    g = _gen(tag, B, H, W)
    T, regime = se3_field(B, H, W, 0.3, g)
    d1, d2 = depth_map(B, H, W, g), depth_map(B, H, W, g)
    n = max(1, (H * W) // 3000)
    for b in range(B):
        at = torch.randperm(H * W, generator=g)[:2 * n]
        d1[b].view(-1)[at[:n]] = 0.0
        d1[b].view(-1)[at[n:]] = 0.02
        T[b].view(-1, 7)[at, 2] = 0.01  # (so that these stay within MIN_DEPTH of the camera plane after the motion)
    py, px = near_patch(H, W)
    d1[:, py:py + 2, px:px + 2] = 0.3
    T[:, py:py + 2, px:px + 2, 2] = -0.8
    return dict(T=T, regime=regime, d1=d1, d2=d2, K=intrinsics(h, w, scale))


def lookup_coords(B, h, w, tag=2):
    """[B,h,w,2] fp32 (x, y) = pixel + N(0, 6) flow, with planted positions in the first row of every item: exact
    integers; exactly (w-1, h-1); inside (-4, -3) on both axes (only the last tap in range); just outside on every
    side; -50; 1e6; and an exact integer at the very last pixel (the tail of the last workgroup)."""
    g = _gen(tag, B, h, w)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    c = torch.stack([xx, yy], -1)[None] + 6.0 * torch.randn(B, h, w, 2, generator=g)
    plant = [(3.0, 2.0), (w - 1.0, h - 1.0), (-3.25, -3.5), (-4.25, 5.0), (w + 3.25, 5.0), (5.0, -4.25), (5.0, h + 3.25),
             (-50.0, 4.0), (7.5, 1e6), (1e6, -50.0), (0.0, 0.0), (w - 1.5, h - 1.0)]
    for i, p in enumerate(plant):
        c[:, 0, i] = torch.tensor(p)
    c[:, h - 1, w - 1] = torch.tensor((w - 2.0, h - 3.0))
    return c.contiguous()


def features(B, h, w, tag=3):
    """Two feature maps [B,128,h,w] like the encoder's output: N(0, 1) with a log-normal scale per channel."""
    g = _gen(tag, B, h, w)
    s = torch.exp(0.5 * torch.randn(2, 1, 128, 1, 1, generator=g))
    return (torch.randn(B, 128, h, w, generator=g) * s[0]).contiguous(), (torch.randn(B, 128, h, w, generator=g) * s[1]).contiguous()


ONE_HOT = 80.0


def upsample_case(B, h, w, tag=4):
    """dict(T, regime, mask, data6 / data3 / data2 [B,h,w,D], weight [B,3,h,w], hot = [(b, y, x, k)]): se3_field with
    |t| <= 1; a mask of N(0, 2) logits; at the pixels ``hot`` (corners and borders included) the 9 logits of all 64
    sub-pixels are one-hot, +80 at neighbour k and -80 elsewhere: the soft-max saturates."""
    g = _gen(tag, B, h, w)
    T, regime = se3_field(B, h, w, 1.0, g)
    mask = 2.0 * torch.randn(B, 576, h, w, generator=g)
    hot = [(0, 0, 0, 4), (0, 0, 0 + 1, 0), (B - 1, h - 1, w - 1, 8), (B - 1, h - 1, 0, 4), (0, h // 2, w - 1, 5),
           (0, h // 2, w // 2, 4), (B - 1, h // 3, w // 3, 1), (0, 0, w - 1, 2)]
    m = mask.view(B, 9, 64, h, w)
    for (b, y, x, k) in hot:
        m[b, :, :, y, x] = -ONE_HOT
        m[b, k, :, y, x] = ONE_HOT
    d = {D: torch.randn(B, h, w, D, generator=g) * (1.0 + torch.arange(D)) for D in (6, 3, 2)}
    wgt = torch.sigmoid(1.5 * torch.randn(B, 3, h, w, generator=g))
    return dict(T=T, regime=regime, mask=mask.contiguous(), data6=d[6], data3=d[3], data2=d[2], weight=wgt, hot=hot)


def instnorm_case(B, Cc, h, w, tag=5):
    """(x, res) [B,C,h,w]: planes N(1, 3^2); plane (b, 1) and (b, 9) with |mean| = 300 std; plane (b, 2) constant
    (variance 0); plane (b, 3) of 1e-3 scale around 0 (where eps = 1e-5 matters)."""
    g = _gen(tag, B, Cc, h, w)
    x = torch.randn(B, Cc, h, w, generator=g) * 3 + 1
    x[:, 1] = torch.randn(B, h, w, generator=g) * 0.5 + 150.0
    x[:, 9] = torch.randn(B, h, w, generator=g) * 2.0 - 600.0
    x[:, 2] = 1.7
    x[:, 3] = torch.randn(B, h, w, generator=g) * 1e-3
    return x.contiguous(), torch.randn(B, Cc, h, w, generator=g).contiguous()


def disparity_map(B, H, W, tag=6):
    """Disparities log-uniform 0.5 .. 320, with a few exact 0, small negative and -1e-5 (the pole of the formula)."""
    g = _gen(tag, B, H, W)
    d = 0.5 * torch.exp(torch.rand(B, 1, H, W, generator=g) * math.log(640.0))
    f = d.view(-1)
    at = torch.randperm(f.numel(), generator=g)[:30]
    f[at[:10]] = 0.0
    f[at[10:20]] = -0.75
    f[at[20:]] = -1e-5
    return d.contiguous()


# ------------------------------------------------------------------------------------------------ references
def pooled(f2, i, ceil=False):
    """avg_pool2d(2)^i of f2 in fp64 (floor sizes, as reference blocks/corr.py:28-45 pools the volume -- pooling the
    second feature map is the same linear map)."""
    x = f2.to(F64)
    for _ in range(i):
        x = F.avg_pool2d(x, 2, stride=2, ceil_mode=ceil)
    return x


def pyramid_blocks(f1, f2, lvl, rows=1080, variant=None):
    """Yields (b, r0, r1, ref, M) over row blocks of level ``lvl`` of the all-pairs pyramid, fp64:
    ref = (f1 / 16)^T . avgpool2^lvl(f2) [r1 - r0, h2 * w2], M the same product of the absolute values.  Restates
    oracle.motion.corr_pyramid (pooling moved from the volume to f2).  In blocks, so that at 72x120 no second
    8640 x 8640 fp64 array exists.  variant "ceil": pooled with ceil sizes, the flat volume read at floor sizes."""
    B, D, h, w = f1.shape
    N = h * w
    n2 = (h >> lvl) * (w >> lvl)
    P = pooled(f2, lvl, ceil=variant == "ceil").reshape(B, D, -1)
    Pa = pooled(f2.abs(), lvl, ceil=variant == "ceil").reshape(B, D, -1)
    A = f1.to(F64).reshape(B, D, N) / 16.0
    for b in range(B):
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            ref, M = A[b, :, r0:r1].t() @ P[b], A[b, :, r0:r1].t().abs() @ Pa[b]
            if ref.shape[1] != n2:  # (the ceil variant: a wider row pitch, cut to the floor-sized volume)
                ref, M = ref[:, :n2], M[:, :n2]
            yield b, r0, r1, ref, M


def lookup(vols, coords, h, w, variant=None):
    """The 7x7 pyramid lookup in fp64 at fp32 coordinates [B,h,w,2] from fp32 (or fp64) volumes [B, h*w, h2*w2]
    -> (out, M, G) [B,196,h,w]: M = the same lookup of |vol| (the four weights are non-negative: the sum of |terms|;
    plus half the sum of the four |taps| per axis whose level coordinate lies in (-1, 0), see below),
    G = the sum of the absolute adjacent-tap differences of each sample.  Restates oracle.motion.corr_lookup_level
    (the 8x8 tap window is gathered once; zero outside the volume; channel = i*7 + j, i = x offset, j = y offset).
    variants: "channel_order" (j*7 + i), "level_coord" ((x + 0.5) / 2^i - 0.5), "clamp_edge", "shift" (window moved
    by one tap)."""
    B = coords.shape[0]
    N = h * w
    outs, Ms, Gs = [], [], []
    for lvl, vol in enumerate(vols):
        h2, w2 = h >> lvl, w >> lvl
        xy = coords.to(F64)[..., :2]
        bad = torch.isnan(xy).any(-1)  # (a NaN coordinate: every tap out of range, the kernel's explicit branch)
        xy = torch.where(bad[..., None], torch.zeros_like(xy), xy)
        xy = (xy + 0.5) / 2 ** lvl - 0.5 if variant == "level_coord" else xy / 2 ** lvl
        x0, y0 = xy[..., 0], xy[..., 1]
        fx, fy = torch.floor(x0), torch.floor(y0)
        dx, dy = (x0 - fx)[..., None, None], (y0 - fy)[..., None, None]
        o = torch.arange(8) - (2 if variant == "shift" else 3)
        ix = fx.clamp(-16, w2 + 16).long()[..., None] + o  # [B,h,w,8]
        iy = fy.clamp(-16, h2 + 16).long()[..., None] + o
        ok = ((iy >= 0) & (iy < h2))[..., :, None] & ((ix >= 0) & (ix < w2))[..., None, :] & ~bad[..., None, None]
        idx = iy.clamp(0, h2 - 1)[..., :, None] * w2 + ix.clamp(0, w2 - 1)[..., None, :]  # [B,h,w,8(y),8(x)]
        t = torch.gather(vol.reshape(B, N, h2 * w2), 2, idx.reshape(B, N, 64)).to(F64).view(B, h, w, 8, 8)
        if variant != "clamp_edge":
            t = t * ok
        t00, t01, t10, t11 = t[..., :7, :7], t[..., :7, 1:], t[..., 1:, :7], t[..., 1:, 1:]  # t[y][x]: 01 = x + 1
        w00, w01, w10, w11 = (1 - dx) * (1 - dy), dx * (1 - dy), (1 - dx) * dy, dx * dy
        v = w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11
        M = w00 * t00.abs() + w01 * t01.abs() + w10 * t10.abs() + w11 * t11.abs()
        # a level coordinate inside (-1, 0): x - floor(x) = x + 1 is not exact in fp32 (x carries bits below 2^-24), the
        # fraction is off by up to 2^-25 and with it each weight, however small the weight itself is
        inexact = 0.5 * (((x0 > -1) & (x0 < 0)).to(F64) + ((y0 > -1) & (y0 < 0)).to(F64))[..., None, None]
        M = M + inexact * (t00.abs() + t01.abs() + t10.abs() + t11.abs())
        G = (t01 - t00).abs() + (t11 - t10).abs() + (t10 - t00).abs() + (t11 - t01).abs()
        chan = (lambda a: a) if variant == "channel_order" else (lambda a: a.transpose(-1, -2))  # [j][i] -> [i][j]
        outs.append(chan(v).reshape(B, h, w, 49))
        Ms.append(chan(M).reshape(B, h, w, 49))
        Gs.append(chan(G).reshape(B, h, w, 49) * torch.maximum(xy.abs().amax(-1), torch.ones(()))[..., None])
    fin = lambda a: torch.cat(a, -1).permute(0, 3, 1, 2).contiguous()
    return fin(outs), fin(Ms), fin(Gs)  # (G comes multiplied by max(|x|, |y|, 1) of the level coordinate)


def bilinear(img, x, y, nearest=False):
    """Bilinear sample of img [B,h,w] at (x, y) [B,...] in pixel units, zero outside, align_corners = True -> (value,
    sum_k w_k |tap_k|, Gx, Gy): Gx / Gy bound |d value / dx|, |d value / dy| (sums of absolute adjacent-tap
    differences).  Restates oracle.motion.sample_bilinear; an in-range tap enters as weight * tap even when the weight
    is 0 (0 * inf = NaN, as grid_sample and the kernel form it), a tap outside the image is 0; a NaN coordinate gives NaN."""
    B, h, w = img.shape
    bad = torch.isnan(x) | torch.isnan(y)
    xs, ys = torch.where(bad, torch.zeros_like(x), x), torch.where(bad, torch.zeros_like(y), y)
    if nearest:
        xs, ys = torch.round(xs), torch.round(ys)
    x0, y0 = torch.floor(xs), torch.floor(ys)
    ax, ay = xs - x0, ys - y0
    ix, iy = x0.clamp(-4, w + 4).long(), y0.clamp(-4, h + 4).long()
    flat = img.reshape(B, -1)

    def tap(jx, jy):
        ok = (jx >= 0) & (jx < w) & (jy >= 0) & (jy < h)
        v = torch.gather(flat, 1, (jy.clamp(0, h - 1) * w + jx.clamp(0, w - 1)).reshape(B, -1)).view_as(jx)
        return torch.where(ok, v, torch.zeros_like(v))

    t00, t01, t10, t11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
    ws = ((1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay)
    v = ws[0] * t00 + ws[1] * t01 + ws[2] * t10 + ws[3] * t11
    M = ws[0] * t00.abs() + ws[1] * t01.abs() + ws[2] * t10.abs() + ws[3] * t11.abs()
    nan = torch.full_like(v, float("nan"))
    Gx, Gy = (t01 - t00).abs() + (t11 - t10).abs(), (t10 - t00).abs() + (t11 - t01).abs()
    return torch.where(bad, nan, v), torch.where(bad, nan, M), Gx, Gy


def _project(X, K, peps=om.EPS):
    """oracle.motion.project restated with the epsilon as a parameter -> (uvz [..., 3], Z)."""
    fx, fy, cx, cy = K
    Z = X[..., 2] + peps
    return torch.stack([fx * (X[..., 0] / Z) + cx, fy * (X[..., 1] / Z) + cy, 1.0 / Z], -1), Z


def _project_mag(X, uvz, Z, S, K):
    """First-order magnitudes of a projection whose inputs carry the magnitude S = the 1-norm of what X was summed
    from: u: fx S / |Z| (1 + |X.x| / |Z|) + |u| + |cx| (the quotient's sensitivity to X.x and to Z, the product and
    the sum); v alike; 1 / Z: S / Z^2 + 1 / |Z|."""
    fx, fy, cx, cy = K
    aZ = Z.abs()
    return torch.stack([fx * S / aZ * (1 + X[..., 0].abs() / aZ) + uvz[..., 0].abs() + abs(cx),
                        fy * S / aZ * (1 + X[..., 1].abs() / aZ) + uvz[..., 1].abs() + abs(cy),
                        S / (aZ * aZ) + 1 / aZ], -1)


def geometry(T, d1, d2, K, variant=None):
    """raft_geometry in fp64 (reference raft3d.py:225-240) -> dict: xyz [B,h,w,3] and M_xyz; zinv (the bilinear 1/d2
    sample); raw / minfo [B,9,h,w] (before / after the +-50 clamp) and M_minfo; excluded [B,h,w] = |Z| < MIN_DEPTH (the
    one kind of pixel that is not compared).  Reuses oracle.motion.inv_project and oracle.se3.act / log fed fp64;
    project and the sampler are restated (_project, bilinear).
    M of the last channel: 10 x (sum_k w_k / d2_k + the magnitude of 1 / Z + Gx M_u + Gy M_v) -- the last two terms are
    the sample's first-order sensitivity to the coordinate it is taken at, times that coordinate's own error magnitude:
    the fp32 evaluation samples at ITS projected coordinate, not at the fp64 one.
    variants: "no_peps" (project without + 1e-5), "nearest" (1/d2 sampled nearest), "twist_scale" (twist not x 10)."""
    B, h, w = d1.shape
    T64, Kt = T.to(F64), torch.tensor([list(K)] * B, dtype=F64)
    X0 = om.inv_project(d1.to(F64), Kt)
    X1 = se3.act(T64, X0)
    xyz, Z = _project(X1, K, 0.0 if variant == "no_peps" else om.EPS)
    S = X0.abs().sum(-1) + T64[..., :3].abs().sum(-1)
    Mx = _project_mag(X1, xyz, Z, S, K)
    zinv, Mzs, Gx, Gy = bilinear(1.0 / d2.to(F64), xyz[..., 0], xyz[..., 1], nearest=variant == "nearest")
    yy, xx = torch.meshgrid(torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing="ij")
    tw = se3.log(T64)
    raw = torch.cat([xyz[..., :2] - torch.stack([xx, yy], -1), (1.0 if variant == "twist_scale" else 10.0) * tw,
                     10.0 * (zinv - xyz[..., 2])[..., None]], -1)
    Mtw = 10.0 * (tw[..., :3].abs().amax(-1) + tw[..., 3:].abs().amax(-1))
    Mdz = 10.0 * (Mzs + Mx[..., 2] + Gx * Mx[..., 0] + Gy * Mx[..., 1])
    Mm = torch.cat([Mx[..., :2], Mtw[..., None].expand(B, h, w, 6), Mdz[..., None]], -1)
    p = lambda a: a.permute(0, 3, 1, 2).contiguous()
    return dict(xyz=xyz, M_xyz=Mx, zinv=zinv, raw=p(raw), minfo=p(raw.clamp(-50.0, 50.0)), M_minfo=p(Mm),
                excluded=Z.abs() < MIN_DEPTH, Z=Z)


def induced_flow(T, depth, K):
    """project(T X0) - project(X0) in fp64 (reference projective_ops.py:55-68) -> (flow [B,H,W,3], M = the sum of the two
    projections' magnitudes, excluded = either |Z| < MIN_DEPTH).  Reuses oracle.motion.inv_project / oracle.se3.act."""
    B = depth.shape[0]
    T64, Kt = T.to(F64), torch.tensor([list(K)] * B, dtype=F64)
    X0 = om.inv_project(depth.to(F64), Kt)
    X1 = se3.act(T64, X0)
    a, Za = _project(X1, K)
    c, Zc = _project(X0, K)
    S0 = X0.abs().sum(-1)
    M = _project_mag(X1, a, Za, S0 + T64[..., :3].abs().sum(-1), K) + _project_mag(X0, c, Zc, S0, K)
    return a - c, M, (Za.abs() < MIN_DEPTH) | (Zc.abs() < MIN_DEPTH)


def disp_to_depth(disp, bf=BF, eps=1e-5):
    """clip(bf / (disp + 1e-5), 0, bf) in fp64 (reference motion.py:154-165; restates oracle.motion.disp_to_depth with
    bf = scale * fx folded) -> (depth, M = |bf / (disp + eps)| (|disp| + eps) / |disp + eps|: the quotient and the
    sum's cancellation at negative disparities).  The clip is 1-Lipschitz: the bound holds through it."""
    d = disp.to(F64)
    s = d + eps
    v = bf / s
    return v.clamp(0.0, bf), v.abs() * (d.abs() + eps) / s.abs()


def avgpool2(x):
    """F.avg_pool2d(x, 2) in fp64 -> (value, M = the same of |x|)."""
    return F.avg_pool2d(x.to(F64), 2, stride=2), F.avg_pool2d(x.to(F64).abs(), 2, stride=2)


def instnorm(x, res=None, relu=True, res_relu=None, unbiased=False, eps=1e-5):
    """InstanceNorm2d (affine = False, biased variance, eps 1e-5) in fp64 -> (value, M).  res_relu None: the plain
    form relu(norm(x) + res); else the record-writing form norm -> [relu] -> + res -> [res_relu].
    M = rstd (|x| + |mean| + std) + |y| + |res| with y the normalised value (without the |mean| term the bound fails on
    a constant plane and at |mean| = 300 std).  The std term: a mean formed from fp32 partial sums (the kernel's are
    sums of x - x[0], combined in fp64) is uncertain by a fraction of 2^-24 x the spread of what is summed, however
    small |mean| itself is; the normalised value inherits rstd x std <= 1 of it.  Without it the HIP kernel is at 13 x
    2^-24 M on the 1e-3-scale plane, at elements with |x| ~ |mean| ~ 0.01 std (measured on MI355X and reproduced
    by a CPU emulation of the kernel's summation order; the mean itself is within 0.25 x 2^-24 std)."""
    x64 = x.to(F64)
    mean = x64.mean((2, 3), keepdim=True)
    var = x64.var((2, 3), keepdim=True, unbiased=unbiased)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x64 - mean) * rstd
    r = torch.zeros_like(y) if res is None else res.to(F64)
    M = rstd * (x64.abs() + mean.abs() + torch.sqrt(var)) + y.abs() + r.abs()
    if res_relu is None:
        v = y + r
        return (F.relu(v) if relu else v), M
    v = F.relu(y) if relu else y
    if res is not None:
        v = v + r
        v = F.relu(v) if res_relu else v
    return v, M


def cvx(data, mask, variant=None):
    """Convex up-sampling in fp64: data [B,h,w,D], mask [B,576,h,w] -> [B,8h,8w,D].  Restates
    oracle.motion.cvx_upsample (soft-max over the 9 neighbours, zero border, neighbour k = ky*3 + kx).
    variants: "softmax64" (soft-max over the 64 sub-pixels), "order" (k = kx*3 + ky), "replicate" (border)."""
    B, h, w, D = data.shape
    m6 = mask.to(F64).view(B, 9, 8, 8, h, w)
    m = torch.softmax(m6.view(B, 9, 64, h, w), 2).view_as(m6) if variant == "softmax64" else torch.softmax(m6, 1)
    dp = F.pad(data.to(F64).permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate" if variant == "replicate" else "constant")
    out = torch.zeros(B, D, 8, 8, h, w, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            k = kx * 3 + ky if variant == "order" else ky * 3 + kx
            out = out + m[:, k][:, None] * dp[:, :, None, None, ky:ky + h, kx:kx + w]
    return out.permute(0, 4, 2, 5, 3, 1).reshape(B, 8 * h, 8 * w, D)


UNDERFLOW = 2.0 ** -102  # 2^-126 / 2^-24: a soft-max weight below the smallest normal fp32 number may be flushed to 0


def _cvx_mag(mag, mask, variant=None):
    """sum_k w_k mag_k + UNDERFLOW sum_k mag_k: the second term only matters where the soft-max is saturated (one-hot
    logits at +-80: exp(-160) is 0 in fp32 and 3e-70 in fp64)."""
    return cvx(mag, mask, variant) + UNDERFLOW * 9.0 * cvx(mag, torch.zeros_like(mask), variant)


def cvx_data(data, mask, variant=None):
    """(cvx, M = sum_k w_k |data_k| (+ the underflow term of _cvx_mag)) for modes 0 (data [B,h,w,D]) and, through
    permutes, 2."""
    return cvx(data, mask, variant), _cvx_mag(data.abs(), mask, variant)


def upsample_se3(T, mask, variant=None):
    """exp(cvx(log T)) in fp64 (reference se3_field.py:189-192; oracle.se3.log / exp fed fp64 around cvx) ->
    (T_up [B,8h,8w,7], M [B,8h,8w,7], th): quaternion M = 1; translation M = A (1 + [th^2 >= 1e-6] / th) with
    A = sum_k w_k (|tau_k|_inf + |t_k|_inf) over the 9 neighbours (the log side and the blend) and th the blended rotation
    angle (the exp side: (1 - cos th) / th^2 cancels in fp32, see test_se3_exp_table)."""
    T64 = T.to(F64)
    lg = se3.log(T64)
    tw = cvx(lg, mask, variant)
    out = se3.exp(tw)
    A = _cvx_mag((lg[..., :3].abs().amax(-1) + T64[..., :3].abs().amax(-1))[..., None], mask, variant)[..., 0]
    th = tw[..., 3:].norm(dim=-1)
    Mt = A * exp_factor(th)
    return out, torch.cat([Mt[..., None].expand(*Mt.shape, 3), torch.ones(*Mt.shape, 4, dtype=F64)], -1), th


def exp_factor(th):
    """1 + [th^2 >= 1e-6] / th: the growth of the fp32 error of V(phi) tau where c1 = (1 - cos th) / th^2 is formed in
    closed form (left_jac_apply: 1 - cos th is 5e-7 just above the threshold, the spacing of floats below 1 is 6e-8)."""
    return 1.0 + torch.where(th * th >= TH2_CLOSED_FORM, 1.0 / th.clamp(min=1e-30), torch.zeros_like(th))


# ------------------------------------------------------------------------------------------------ bounds
def ratio(got, ref, M, c, extra=None):
    """err / bound per element, bound = c 2^-24 M (+ extra); 0 where both are 0; inf where only the bound is."""
    err = (got.to(F64) - ref).abs()
    lim = c * U * M
    if extra is not None:
        lim = lim + extra
    r = torch.where(lim > 0, err / lim.clamp(min=1e-300), torch.full_like(err, float("inf")))
    return torch.where(err == 0, torch.zeros_like(err), r)


def worst(name, r, keep=None, regime=None, pix=None, quiet=False):
    """Worst err / bound over the elements ``keep`` with its location (and rotation regime, if a per-pixel ``regime``
    [B,h,w] is given: indexed by the leading dims of the location, or by ``pix(location)``); prints one line; NaN ratios
    count as failures (inf).  -> (worst ratio, the line)."""
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    if keep is not None:
        r = torch.where(keep.expand_as(r) if keep.dim() == r.dim() else keep, r, torch.zeros_like(r))
    v, at = r.reshape(-1).max(0)
    loc = tuple(int(i) for i in torch.unravel_index(at, r.shape))
    msg = f"{name}: worst err / bound {v.item():.3g} at {loc}"
    if regime is not None:
        msg += f" regime {REGIMES[int(regime[pix(loc) if pix else loc[:regime.dim()]])]}"
    if not quiet:
        print(msg)
    return v.item(), msg


# ------------------------------------------------------------------------------------------------ comparisons
# Each returns {key of C: worst err / (2^-24 M)} -- the figure that C is set from (CPU oracle) and checked against (GPU).
NCHW = lambda loc: (loc[0], loc[2], loc[3])


def within(res, frac=1.0, what=""):
    """Every measured figure of ``res`` is at most frac * C[key] (key = the part before any ':')."""
    bad = {k: (v, frac * C[k.split(":")[0]]) for k, v in res.items() if not v <= frac * C[k.split(":")[0]]}
    assert not bad, (what, bad)


def pyramid_ratios(f1, f2, levels, name, mode="fp32"):
    """levels: 4 tensors [B, N, h2*w2] -> {"pyramid_fp32:L<i>": worst err / (2^-24 M)} for the exact-fp32 path, or
    {"split:L<i>": worst err / (rel M + abs)} under SPLIT_BOUND[mode] (to be <= 1)."""
    res = {}
    for lvl, got in enumerate(levels):
        top, at = 0.0, None
        for b, r0, r1, ref, Mg in pyramid_blocks(f1, f2, lvl):
            g = got[b, r0:r1].to(F64)
            if mode == "fp32":
                r = ratio(g, ref, Mg, 1.0)
            else:
                r = ratio(g, ref, Mg, 0.0, extra=SPLIT_BOUND[mode][0] * Mg + SPLIT_BOUND[mode][1])
            r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
            v, i = r.reshape(-1).max(0)
            if v.item() >= top:
                top, at = v.item(), (b, r0 + int(i) // r.shape[1], int(i) % r.shape[1])
        print(f"{name} pyramid[{mode}] level {lvl}: worst err / bound {top:.3g} at (b, n1, n2) = {at}")
        res[("pyramid_fp32" if mode == "fp32" else mode) + f":L{lvl}"] = top
    return res


def lookup_ratios(ref, got, name, extra_c=0.0):
    """ref = lookup(...) -> {"lookup:L<i>"}; extra_c: the fused form's G term, bound = c 2^-24 M + extra_c 2^-24 G."""
    out, Mg, G = ref
    res = {}
    for lvl in range(4):
        s = slice(49 * lvl, 49 * lvl + 49)
        if extra_c:
            r = ratio(got[:, s], out[:, s], Mg[:, s], C["lookup"], extra=extra_c * U * G[:, s]) * C["lookup"]
        else:
            r = ratio(got[:, s], out[:, s], Mg[:, s], 1.0)
        res[f"lookup:L{lvl}"] = worst(f"{name} lookup level {lvl}", r)[0]
    return res


def geometry_ratios(ref, xyz, minfo, regime, name):
    keep = ~ref["excluded"]
    rx = ratio(xyz, ref["xyz"], ref["M_xyz"], 1.0)
    rm = ratio(minfo, ref["minfo"], ref["M_minfo"], 1.0)
    k3, k4 = keep[..., None], keep[:, None]
    return {"xyz_uv": worst(f"{name} xyz.uv", rx[..., :2], k3, regime)[0],
            "xyz_z": worst(f"{name} xyz.1/Z", rx[..., 2:], k3, regime)[0],
            "minfo_flow": worst(f"{name} minfo flow", rm[:, :2], k4, regime, NCHW)[0],
            "minfo_twist": worst(f"{name} minfo twist", rm[:, 2:8], k4, regime, NCHW)[0],
            "minfo_dz": worst(f"{name} minfo dz", rm[:, 8:], k4, regime, NCHW)[0]}


def se3_up_ratios(ref, got, regime8, name):
    out, Mg, th = ref
    r = ratio(got, out, Mg, 1.0)
    return {"cvx_se3_t": worst(f"{name} upsample_se3 t", r[..., :3], None, regime8)[0],
            "cvx_se3_q": worst(f"{name} upsample_se3 q", r[..., 3:], None, regime8)[0]}
