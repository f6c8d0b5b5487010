"""fp64 reference, inputs and bounds for the forward splat (codd_splat of codd_amd/csrc/motion.hip: splat_count,
splat_reserve, splat_fill, splat_gather; wrapped by ops.splat), for tests/test_splat_fp64_reference.py (CPU: the fp32
oracle against this reference -- the measurement that sets every constant of C -- the share of fragile pixels and the
power of the bounds) and tests/test_gpu_splat_fp64.py (the HIP kernels and their scratch).

The reference shares nothing with oracle.motion.splat or the kernel's window logic:
  projection   fp64 from the fp32 inputs: X1 = T * inv_project(depth), z = X1.z, (u, v) = (fx X / z + cx, fy Y / z + cy);
               a point is valid when z > 0, |u| < 1e7 and |v| < 1e7;
  coverage     brute force, every valid point against every pixel centre (px + 0.5, py + 0.5): d^2 < R^2 (no window);
  compositing  per pixel all candidates sorted by (z, id), the 8 nearest kept, alpha = 1 - d^2 / R^2,
               w_k = alpha_k prod_{m<k} (1 - alpha_m), out = sum_k w_k f_k; the flow channels' f_k is
               project(X1) - project(X0) (motion_fp64.induced_flow); zout the nearest z (0: no candidate), or
               bf / (z + 1e-5f) with > W -> 0.
R and the 1e-5f of the disparity are fp32 values the kernel holds: the reference takes them as such (R = the fp32
evaluation of radius * min(H, W) / (2 H), eps = float32(1e-5)) and works in fp64 from there.

Bound of an output element: |got - ref64| <= c 2^-24 M + CF 2^-24 Mb, first order:
  S        = |X0|_1 + |t|_1, the magnitude of the sums that form X1;
  M(u)     = fx S / z (1 + |X| / z) + |u| + |cx|  (motion_fp64._project_mag without the epsilon),  M(v) alike, M(z) = S;
  M(a_k)   = (2 |du| M(u) + 2 |dv| M(v)) / R^2 + 1;
  dw_k/da_k = prod_{j<k} (1 - a_j),   dw_k/da_m = -a_k prod_{j<k, j != m} (1 - a_j)  for m < k;
  M(out)   = sum_k |f_k| sum_{m<=k} |dw_k/da_m| M(a_m)  +  sum_k w_k (|f_k| + M(f_k)),  M(f_k) = 0 for a feature channel
             (an input) and motion_fp64.induced_flow's magnitude for a flow channel;
  M(z)     = S;  M(disparity) = bf / (z + eps) (1 + (S + eps) / (z + eps)).
c: one per output class (C below), 4 x what the fp32 CPU oracle reaches on the same inputs (MEASURED).

Decisions.  fp32 may decide a comparison differently than fp64 when its operands are within their own error of each
other; CF 2^-24 M(operand) is the zone in which the reference calls a decision open.  CF = 8: the projection that forms
(u, v, z) is the one motion_fp64 bounds with c = 5.8 (u, v) and 6.8 (1 / Z).  The open decisions and what they move:
  (a) a candidate with |d^2 - R^2| inside the zone of d^2 (2 |du| M(u) + 2 |dv| M(v) + d^2 + R^2) that is the nearest
      in z of its pixel: zout and "covered";  any such candidate: the candidate count;
  (b) the same candidate, among the nine nearest of a pixel with 8 or more other candidates: out (it may evict one);
  (c) two of the nine nearest whose z differ by less than their zones without being equal: out (their order);
  (d) a point with z, |u| or |v| inside the zone of 0 / 1e7: everything at the pixels it may cover (one with z <= 0
      inside the zone could be valid anywhere: the whole item, which the 1 % cap then refuses);
  (e) bf / (z + eps) inside its zone of W: zout;
  (f) a kept candidate that induced_flow excludes (|Z| < MIN_DEPTH before or after the motion): the flow channels.
A boundary candidate (a) on a pixel with fewer than 8 others is NOT open for out: its weight goes to 0 continuously.  It
is composited with max(alpha, 0) and its M(alpha) enters Mb instead of M, so that the bound pays for its presence or
absence with the zone's own constant CF whatever c is.

Planted cases are built from exactly representable numbers (fx = fy = 32, integer cx, cy, identity rotations, depths
and targets on binary grids) such that the fp32 projection is EXACT: (u, v, z) carry no error, M(u) = M(v) = M(z) = 0,
every zone is empty and no pixel is fragile.  test_splat_fp64_reference.py verifies the claim: the fp32 evaluation of
(u, v, z) equals the fp64 one bit for bit on those cases."""
import functools

import numpy as np
import torch

import motion_fp64 as M
from motion_fp64 import U, _gen, depth_map, se3_field
from oracle import se3

F64 = torch.float64
CF = 8.0
EPS32 = float(np.float32(1e-5))  # the kernel's 1e-5f
LIMIT = 1e7
KEEP = 8

# worst |oracle32 - ref64| / (2^-24 M) of the fp32 CPU oracle per output class over CASES (CPU measurement) ...
MEASURED = {"composite": 0.861, "flow": 0.533, "zdepth": 2.18, "zdisp": 1.6}
# ... and c = 4 x that, rounded up to two digits
C = {"composite": 3.5, "flow": 2.2, "zdepth": 8.8, "zdisp": 6.4}


# ------------------------------------------------------------------------------------------------ cases
# name: (B, HT, WT, ds, o, radius, CA, with_flow, CB, bf)
CASES = {
    "1_9x13": (1, 9, 13, 1, 0, 2.0, 6, False, 0, 0.0),
    "2_B2_37x61_flow": (2, 37, 61, 1, 0, 2.0, 3, True, 3, M.BF),
    "3_61x37_r2": (1, 61, 37, 1, 0, 2.0, 4, False, 0, 0.0),
    "3_61x37_r4_flow": (1, 61, 37, 1, 0, 4.0, 4, True, 0, M.BF),
    "4_B2_150x246_ds4": (2, 150, 246, 4, 1, 4.0, 32, False, 0, 0.0),
    "5_64x96_r5.2": (1, 64, 96, 1, 0, 5.2, 5, False, 0, 0.0),
    "6_9x13_CA0_flow": (1, 9, 13, 1, 0, 2.0, 0, True, 2, M.BF),
}
PLANTED = ("pileup", "circle_R1", "circle_R2", "threshold", "ninth")
TMAX = 0.05  # |t| of the random fields: up to ~10 px of motion at depth 0.7, fx = 131.25


def radius_px(radius, H, W):
    """splat_radius_px as the host evaluates it, in fp32."""
    return float(np.float32(radius) * np.float32(min(H, W)) / (np.float32(2.0) * np.float32(H)))


def out_size(HT, WT, ds):
    return HT // ds, WT // ds


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(T [B,HT,WT,7], depth [B,HT,WT], featA / featB [B,C,H,W] or None, with_flow, H, W, oy, ox, ds, K, radius,
    bf, exact).  Random cases: se3_field (|t| <= TMAX) and depth_map with geometry_case's plants -- depths 0 and 0.02
    (t.z = 0.01 there), a 2 x 2 patch at depth 0.3 moved behind the camera (t.z = -0.8) -- and two points per side driven
    0.8 px and 3 px out of the frame (identity rotation, depth 4); all plants at positions the splat samples."""
    if name in PLANTED:
        return _planted(name)
    B, HT, WT, ds, o, radius, CA, with_flow, CB, bf = CASES[name]
    H, W = out_size(HT, WT, ds)
    tag = 40 + list(CASES).index(name)
    g = _gen(tag, B, HT, WT)
    T, _ = se3_field(B, HT, WT, TMAX, g)
    depth = depth_map(B, HT, WT, g)
    Tv = T[:, o:o + ds * H:ds, o:o + ds * W:ds]  # (views of the sampled positions: the plants go where the splat reads)
    dv = depth[:, o:o + ds * H:ds, o:o + ds * W:ds]
    n = max(1, (H * W) // 1000)
    for b in range(B):
        at = torch.randperm(H * W, generator=g)[:2 * n]
        ay, ax = at // W, at % W
        dv[b, ay[:n], ax[:n]] = 0.0
        dv[b, ay[n:], ax[n:]] = 0.02
        Tv[b, ay, ax, 2] = 0.01
    py, px = M.near_patch(H, W)
    dv[:, py:py + 2, px:px + 2] = 0.3
    Tv[:, py:py + 2, px:px + 2, 2] = -0.8
    K = M.intrinsics(H, W)
    fx, fy, cx, cy = K
    # out of the frame on each side: output-grid pixels (y, x) -> target (u, v)
    outs = [((H // 2, 1), (-0.8, None)), ((H // 2, 2), (-3.0, None)), ((H // 2, W - 2), (W + 0.8, None)),
            ((H // 2, W - 3), (W + 3.0, None)), ((1, W // 2), (None, -0.8)), ((2, W // 2), (None, -3.0)),
            ((H - 2, W // 2), (None, H + 0.8)), ((H - 3, W // 2), (None, H + 3.0))]
    for (y, x), (tu, tv) in outs:
        sy, sx = o + ds * y, o + ds * x
        tu = float(x) if tu is None else tu
        tv = float(y) if tv is None else tv
        T[:, sy, sx] = torch.tensor([(tu - x) * 4.0 / fx, (tv - y) * 4.0 / fy, 0, 0, 0, 0, 1.0])
        depth[:, sy, sx] = 4.0
    C_all = CA + CB
    feat = torch.randn(B, max(C_all, 1), H, W, generator=g)
    featA = feat[:, :CA].contiguous() if CA else None
    featB = feat[:, CA:CA + CB].contiguous() if CB else None
    return dict(name=name, T=T.contiguous(), depth=depth.contiguous(), featA=featA, featB=featB, with_flow=with_flow, H=H,
                W=W, oy=o, ox=o, ds=ds, K=K, radius=radius, bf=bf, exact=False, B=B)


PH, PW, PK = 48, 64, (32.0, 32.0, 32.0, 24.0)


def _place(T, depth, n, tu, tv, tz):
    """Pure translations that put the points n (flat ids of the PH x PW grid, depths on a binary grid) at (tu, tv, tz):
    t = P - X0 with P = ((tu - cx) tz / fx, (tv - cy) tz / fy, tz), every operation exact in fp32 for the grids used
    (fx = fy = 32; tu, tv multiples of 1/64; tz multiples of 1/256 below 8; depths multiples of 1/64 below 16)."""
    fx, fy, cx, cy = PK
    y, x = (n // PW).float(), (n % PW).float()
    d = depth.view(-1)[n]
    X0 = torch.stack([d * ((x - cx) / fx), d * ((y - cy) / fy), d], -1)
    P = torch.stack([(tu - cx) * tz / fx, (tv - cy) * tz / fy, tz], -1)
    T.view(-1, 7)[n, :3] = P - X0


def _planted(name):
    """The planted cases, B = 1, 48 x 64, K = (32, 32, 32, 24), identity rotations.  Background: depth 4, no motion (a
    point lands on its own pixel's corner (x, y): d^2 = 0.5 to four centres, far from any circle).
    pileup     every point moved onto one of three pixels (two adjacent), offsets on a 1/64 grid within 0.4 px of the
               centre, z = 4 (every fourth point: exact ties) or 4 + (n mod 211) / 256;
    circle_R*  around four target pixels, points at z = 2 at distance exactly R from the centre along +-x, +-y (not
               covered) and, around four others, at the next fp32 coordinate inside (covered);
    threshold  two points at the principal row with identity pose and depths eps and eps - 2 ulp(eps), eps = 1e-5f:
               z + eps is exact, bf = W * 2 eps, so bf / (z + eps) is exactly W (kept) and the next fp32 above (zeroed);
    ninth      nine points on one pixel, z = 2 + k / 256; the first eight 0.75 px off the centre, the ninth on it."""
    g = torch.Generator().manual_seed(5)
    T = torch.zeros(1, PH, PW, 7)
    T[..., 6] = 1.0
    depth = torch.full((1, PH, PW), 4.0)
    radius, bf = 2.0, 0.0
    if name == "pileup":
        depth = (torch.randint(0, 640, (1, PH, PW), generator=g).float() / 64.0 + 3.0)
        n = torch.arange(PH * PW)
        tgt = torch.tensor([[20.5, 10.5], [21.5, 10.5], [40.5, 30.5]])[n % 3]
        tz = torch.where(n % 4 == 0, torch.full((PH * PW,), 4.0), 4.0 + (n % 211).float() / 256.0)
        tu = tgt[:, 0] + torch.round(0.4 * torch.sin(n.float() * 0.37) * 64.0) / 64.0
        tv = tgt[:, 1] + torch.round(0.4 * torch.cos(n.float() * 0.73) * 64.0) / 64.0
        _place(T, depth, n, tu, tv, tz)
    elif name.startswith("circle"):
        R = 1.0 if name == "circle_R1" else 2.0
        radius = 2.0 * R
        ids, tus, tvs = [], [], []
        for j, (ux, uy) in enumerate(((20.5, 10.5), (40.5, 10.5), (20.5, 30.5), (40.5, 30.5))):
            for inside, (cx_, cy_) in ((False, (ux, uy)), (True, (ux + 6.0, uy + 6.0))):
                dx, dy = ((R, 0.0), (-R, 0.0), (0.0, R), (0.0, -R))[j]
                pu, pv = np.float32(cx_ + dx), np.float32(cy_ + dy)
                if inside:
                    pu = np.nextafter(pu, np.float32(cx_)) if dx else pu
                    pv = np.nextafter(pv, np.float32(cy_)) if dy else pv
                ids.append(int(pv) * PW + int(pu))  # (the source pixel under the target, at depth 2: |t| stays below 1/8)
                tus.append(float(pu))
                tvs.append(float(pv))
        n = torch.tensor(ids)
        depth.view(-1)[n] = 2.0
        # (a coordinate next to a half-integer is no multiple of 1/64; with tz = 2, fx = 32 and the source next to the
        # target, (tu - cx) tz / fx, t = P - X0 and X0 + t are still exact)
        _place(T, depth, n, torch.tensor(tus), torch.tensor(tvs), torch.full((len(ids),), 2.0))
    elif name == "threshold":
        eps = np.float32(1e-5)
        ulp = np.float32(np.spacing(eps))
        depth[0, 24, 32] = float(eps)
        depth[0, 24, 48] = float(np.float32(eps - np.float32(2.0) * ulp))
        bf = float(np.float32(PW) * (eps + eps))
    elif name == "ninth":
        n = torch.arange(9) * 5 + 7 * PW + 2
        k = torch.arange(9).float()
        ang = [(0.75, 0.0), (-0.75, 0.0), (0.0, 0.75), (0.0, -0.75), (0.5, 0.5), (-0.5, 0.5), (0.5, -0.5), (-0.5, -0.5), (0.0, 0.0)]
        off = torch.tensor(ang)
        _place(T, depth, n, 30.5 + off[:, 0], 20.5 + off[:, 1], 2.0 + k / 256.0)
    feat = torch.randn(1, 5, PH, PW, generator=g)
    return dict(name=name, T=T, depth=depth, featA=feat, featB=None, with_flow=False, H=PH, W=PW, oy=0, ox=0, ds=1, K=PK,
                radius=radius, bf=bf, exact=True, B=1)


def sampled(c):
    """(T [B,H,W,7], depth [B,H,W]) at the sampled positions, fp32."""
    sl = (slice(None), slice(c["oy"], c["oy"] + c["ds"] * c["H"], c["ds"]), slice(c["ox"], c["ox"] + c["ds"] * c["W"], c["ds"]))
    return c["T"][sl].contiguous(), c["depth"][sl].contiguous()


# ------------------------------------------------------------------------------------------------ reference
def project_points(Ts, d, K, exact=False):
    """fp64 (or whatever dtype Ts has) projection of the H x W points of one item -> dict(u, v, z, valid, Mu, Mv, Mz),
    flat [H W].  Restates motion.py:82-130 / se3.h (inv_project, SE3 action, perspective divide without epsilon)."""
    H, W = d.shape
    fx, fy, cx, cy = K
    dt = Ts.dtype
    yy, xx = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    X0 = torch.stack([d * ((xx - cx) / fx), d * ((yy - cy) / fy), d], -1).reshape(-1, 3)
    Tf = Ts.reshape(-1, 7)
    X1 = se3.qrot(Tf[:, 3:], X0) + Tf[:, :3]
    z = X1[:, 2]
    pos = z > 0
    zs = torch.where(pos, z, torch.ones_like(z))
    u, v = fx * X1[:, 0] / zs + cx, fy * X1[:, 1] / zs + cy
    valid = pos & (u.abs() < LIMIT) & (v.abs() < LIMIT)
    S = X0.abs().sum(-1) + Tf[:, :3].abs().sum(-1)
    Mu = fx * S / zs * (1 + X1[:, 0].abs() / zs) + u.abs() + abs(cx)
    Mv = fy * S / zs * (1 + X1[:, 1].abs() / zs) + v.abs() + abs(cy)
    Mz = S
    if exact:
        Mu, Mv, Mz = torch.zeros_like(Mu), torch.zeros_like(Mv), torch.zeros_like(Mz)
    return dict(u=u, v=v, z=z, valid=valid, Mu=Mu, Mv=Mv, Mz=Mz)


def _candidates(p, H, W, R, variant, exact):
    """Brute force: every valid (or (d)-uncertain) point against every pixel centre -> flat arrays over the (pixel,
    point) pairs with d^2 < R^2 + zone: pix, pid, d2, du, dv, inside, boundary."""
    half = 0.0 if variant == "centre0" else 0.5
    yy, xx = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    cxp, cyp = (xx + half).reshape(-1), (yy + half).reshape(-1)
    R2 = R * R
    take = torch.nonzero(p["valid"] | p["unc"])[:, 0]
    res = [[] for _ in range(6)]
    for s in range(0, len(take), 512):
        ids = take[s:s + 512]
        du = p["u"][ids, None] - cxp[None]
        dv = p["v"][ids, None] - cyp[None]
        d2 = du * du + dv * dv
        zone = CF * U * (2 * du.abs() * p["Mu"][ids, None] + 2 * dv.abs() * p["Mv"][ids, None] + d2 + R2)
        if exact:
            zone = torch.zeros_like(zone)
        near = d2 <= R2 + zone
        i, j = torch.nonzero(near, as_tuple=True)
        for k, a in enumerate((j, ids[i], d2[i, j], du[i, j], dv[i, j], zone[i, j])):
            res[k].append(a)
    pix, pid, d2, du, dv, zone = [torch.cat(a) if a else torch.zeros(0, dtype=torch.long if k < 2 else F64) for k, a in enumerate(res)]
    inside = (d2 <= R2) if variant == "le_circle" else (d2 < R2)
    boundary = ((d2 - R2).abs() <= zone) & (zone > 0)
    if variant in ("span_short1", "span_short2"):  # the kernel's window with span one / two short
        span = int(np.float32(R) + np.float32(1.5)) - int(variant[-1])
        ox = (pix % W) - torch.floor(p["u"][pid] - 0.5).long()
        oy = (pix // W) - torch.floor(p["v"][pid] - 0.5).long()
        inside &= (ox >= -span + 1) & (ox <= span) & (oy >= -span + 1) & (oy <= span)
    sel = inside | boundary
    return pix[sel], pid[sel], d2[sel], du[sel], dv[sel], inside[sel], boundary[sel]


def reference(c, variant=None):
    """The splat of case ``c`` in fp64 -> dict:
      out [B,C,H,W], M, Mb (bound: c 2^-24 M + CF 2^-24 Mb), cls [C] (0: a feature channel, 1: a flow channel);
      zout [B,H,W], Mzout;  cnt [B,H,W] candidates per pixel;  covered [B,H,W] = cnt > 0;  zpos = zout > 0;
      frag_out, frag_flow, frag_z, frag_cnt [B,H,W]: the pixels with an open decision for the feature channels, the
      flow channels (includes frag_out), zout / covered, and the candidate count;
      pts: per item the projection dict (u, v, z, valid, ...).
    variants (wrong on purpose, for the power test): "alpha_linear" (1 - d / R), "trans_first" (transmittance updated
    before the weight is taken), "largest_alpha" (the 8 largest alphas kept), "tie_high" (ties to the higher id),
    "le_circle" (d^2 <= R^2), "centre0" (pixel centres at +0), "R_half" (R = radius / 2), "span_short1" / "span_short2" (the
    kernel's window, ox and oy in [-span + 1, span] around floor(u - 0.5), with span one / two short), "flow_z_sign"."""
    B, H, W, K, exact = c["B"], c["H"], c["W"], c["K"], c["exact"]
    R = c["radius"] / 2.0 if variant == "R_half" else radius_px(c["radius"], H, W)
    R2 = R * R
    Ts32, d32 = sampled(c)
    CA = 0 if c["featA"] is None else c["featA"].shape[1]
    CB = 0 if c["featB"] is None else c["featB"].shape[1]
    HW = H * W
    flow = Mflow = flow_ex = None
    if c["with_flow"]:
        flow, Mflow, flow_ex = M.induced_flow(Ts32, d32, K)
        if variant == "flow_z_sign":
            flow = flow * torch.tensor([1.0, 1.0, -1.0], dtype=F64)
    cls = torch.tensor([0] * CA + ([1] * 3 if c["with_flow"] else []) + [0] * CB)
    Cn = len(cls)
    keys = ("out", "M", "Mb", "zout", "Mzout", "cnt", "covered", "frag_out", "frag_flow", "frag_z", "frag_cnt")
    acc = {k: [] for k in keys}
    pts = []
    for b in range(B):
        p = project_points(Ts32[b].to(F64), d32[b].to(F64), K, exact)
        # (d) a point whose validity is open; one that may be valid with an unknown (u, v) opens the whole item
        zz = CF * U * p["Mz"]
        pos = p["z"] > 0
        unc = (p["z"].abs() <= zz) & (zz > 0) & torch.isfinite(zz)  # (NaN / inf: invalid or decided alike on both sides)
        unc |= pos & torch.isfinite(p["Mu"] + p["Mv"]) & (p["Mu"] > 0) & (
            ((p["u"].abs() - LIMIT).abs() <= CF * U * p["Mu"]) | ((p["v"].abs() - LIMIT).abs() <= CF * U * p["Mv"]))
        p["unc"] = unc & ~torch.isnan(p["u"]) & ~torch.isnan(p["v"])
        lost = bool((unc & ~pos).any())
        pts.append(p)
        pix, pid, d2, du, dv, inside, boundary = _candidates(p, H, W, R, variant, exact)
        z = p["z"][pid]
        uncp = p["unc"][pid]
        # ---- per-pixel decisions
        cnt = torch.bincount(pix[inside & p["valid"][pid]], minlength=HW)
        frag_all = torch.zeros(HW, dtype=torch.bool)
        frag_all[pix[uncp]] = True
        if lost:
            frag_all[:] = True
        frag_cnt = frag_all.clone()
        frag_cnt[pix[boundary]] = True
        # ---- sort by (pixel, z, id), rank inside the pixel
        alpha = 1.0 - (d2.sqrt() / R if variant == "alpha_linear" else d2 / R2)
        alpha = torch.where(inside, alpha, torch.zeros_like(alpha)).clamp(min=0.0)
        idk = -pid if variant == "tie_high" else pid
        if variant == "largest_alpha":
            order = np.lexsort((idk.numpy(), -alpha.numpy(), pix.numpy()))
        else:
            order = np.lexsort((idk.numpy(), z.numpy(), pix.numpy()))
        order = torch.from_numpy(order)
        pix, pid, d2, du, dv, inside, boundary, z, alpha = [a[order] for a in (pix, pid, d2, du, dv, inside, boundary, z, alpha)]
        ntot = torch.bincount(pix, minlength=HW)
        start = torch.cumsum(ntot, 0) - ntot
        rank = torch.arange(len(pix)) - start[pix]
        if variant == "largest_alpha":  # the kept eight, then front to back
            keep8 = rank < KEEP
            o2 = torch.from_numpy(np.lexsort((pid[keep8].numpy(), z[keep8].numpy(), pix[keep8].numpy())))
            pix, pid, d2, du, dv, inside, boundary, z, alpha = [a[keep8][o2] for a in (pix, pid, d2, du, dv, inside, boundary, z, alpha)]
            n8 = torch.bincount(pix, minlength=HW)
            rank = torch.arange(len(pix)) - (torch.cumsum(n8, 0) - n8)[pix]
        nine = rank <= KEEP
        # (a) nearest candidate on the circle; (b) a boundary candidate among nine or more; (c) near-ties in z
        frag_z = frag_all.clone()
        frag_z[pix[boundary & (rank == 0)]] = True
        frag_out = frag_all.clone()
        frag_out[pix[boundary & nine & (ntot[pix] > KEEP)]] = True
        if len(pix) > 1:
            adj = (pix[1:] == pix[:-1]) & nine[1:]
            dz = (z[1:] - z[:-1]).abs()
            zmag = p["Mz"][pid]
            tie = adj & (dz > 0) & (dz <= CF * U * (zmag[1:] + zmag[:-1]))
            frag_out[pix[1:][tie]] = True
        # ---- padded [HW, 8] lists
        k8 = rank < KEEP
        slot = pix[k8] * KEEP + rank[k8]

        def pad(vals, fill=0.0):
            a = torch.full((HW * KEEP,), fill, dtype=vals.dtype)
            a[slot] = vals[k8]
            return a.view(HW, KEEP)

        a8 = pad(alpha)
        used = pad(torch.ones_like(alpha)) > 0
        id8 = pad(pid, 0)
        Ma = (2 * du.abs() * p["Mu"][pid] + 2 * dv.abs() * p["Mv"][pid]) / R2 + 1.0
        Ma8, bd8 = pad(Ma), pad(boundary.to(F64)) > 0
        one_m = 1.0 - a8
        w8 = torch.zeros_like(a8)
        tr = torch.ones(HW, dtype=F64)
        for k in range(KEEP):
            if variant == "trans_first":
                tr = tr * one_m[:, k]
            w8[:, k] = tr * a8[:, k]
            if variant != "trans_first":
                tr = tr * one_m[:, k]
        sens, sens_b = torch.zeros_like(a8), torch.zeros_like(a8)
        for k in range(KEEP):
            for m in range(k + 1):
                prod = torch.ones(HW, dtype=F64)
                for j in range(k):
                    if j != m:
                        prod = prod * one_m[:, j]
                dwa = (prod if m == k else a8[:, k] * prod) * Ma8[:, m]
                sens[:, k] += torch.where(bd8[:, m], torch.zeros_like(dwa), dwa)
                sens_b[:, k] += torch.where(bd8[:, m], dwa, torch.zeros_like(dwa))
        feats, fmags = [], []
        for ch in range(Cn):
            if cls[ch] == 1:
                kf = ch - CA
                f, fm = flow[b, ..., kf].reshape(-1), Mflow[b, ..., kf].reshape(-1)
            else:
                src = c["featA"][b, ch] if ch < CA else c["featB"][b, ch - CA - (3 if c["with_flow"] else 0)]
                f = src.reshape(-1).to(F64)
                fm = torch.zeros_like(f)
            feats.append(f)
            fmags.append(fm)
        out = torch.zeros(Cn, HW, dtype=F64)
        Mo, Mb = torch.zeros(Cn, HW, dtype=F64), torch.zeros(Cn, HW, dtype=F64)
        zero = torch.zeros(HW, KEEP, dtype=F64)
        for ch in range(Cn):
            f8 = torch.where(used, feats[ch][id8], zero)
            fm8 = torch.where(used, fmags[ch][id8], zero)
            out[ch] = torch.where(used, w8 * f8, zero).sum(1)
            Mo[ch] = (sens * f8.abs() + w8 * (f8.abs() + fm8)).sum(1)
            Mb[ch] = (sens_b * f8.abs()).sum(1)
        frag_flow = frag_out.clone()
        if c["with_flow"]:
            exk = torch.where(used, flow_ex[b].reshape(-1)[id8], torch.zeros_like(used))
            frag_flow |= exk.any(1)
        # ---- zout: the nearest z of the candidates inside the circle
        vin = inside & p["valid"][pid]
        zmin = torch.full((HW,), float("inf"), dtype=F64).scatter_reduce(0, pix[vin], z[vin], "amin")
        zS = torch.zeros(HW, dtype=F64).scatter_reduce(0, pix[vin], torch.where(z[vin] == zmin[pix[vin]], p["Mz"][pid[vin]], torch.zeros_like(z[vin])), "amax")
        covered = cnt > 0
        zn = torch.where(covered, zmin, torch.zeros_like(zmin))
        if c["bf"] > 0:
            s = zn + EPS32
            dsp = torch.full_like(s, c["bf"]) / s  # (a tensor quotient: scalar / tensor is a product with the reciprocal)
            Md = dsp * (1 + (zS + EPS32) / s)
            if exact:  # (z + eps is exact by construction: the quotient's own rounding is all there is)
                Md = dsp.abs()
            else:
                frag_z |= (dsp - W).abs() <= CF * U * Md  # (e)
            zo, Mzo = torch.where(dsp > W, torch.zeros_like(dsp), dsp), Md
        else:
            zo, Mzo = zn, zS
        for k, a in zip(keys, (out.view(Cn, H, W), Mo.view(Cn, H, W), Mb.view(Cn, H, W), zo.view(H, W), Mzo.view(H, W),
                               cnt.view(H, W), covered.view(H, W), frag_out.view(H, W), frag_flow.view(H, W),
                               frag_z.view(H, W), frag_cnt.view(H, W))):
            acc[k].append(a)
    r = {k: torch.stack(v) for k, v in acc.items()}
    r["zpos"] = r["zout"] > 0
    r["cls"], r["pts"], r["R"] = cls, pts, R
    return r


# ------------------------------------------------------------------------------------------------ comparison
def compare(name, ref, out, zout, c, quiet=False):
    """{class: worst err / (2^-24 M)} of (out [B,C,H,W], zout [B,1,H,W]) against ``ref`` off the fragile pixels, with the
    Mb term at its own constant CF: err' = max(0, err - CF 2^-24 Mb).  NaN on both sides counts as equal, on one side
    as a failure (inf).  Classes: composite, flow (if any), zdepth or zdisp."""
    res = {}
    o64 = out.to(F64)
    both = torch.isnan(o64) & torch.isnan(ref["out"])
    err = ((o64 - ref["out"]).abs() - CF * U * ref["Mb"]).clamp(min=0.0)
    lim = U * ref["M"]
    r = torch.where(lim > 0, err / lim.clamp(min=1e-300), torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where(both, torch.zeros_like(r), r)
    for k, key, frag in ((0, "composite", ref["frag_out"]), (1, "flow", ref["frag_flow"])):
        ch = torch.nonzero(ref["cls"] == k)[:, 0]
        if len(ch):
            res[key] = M.worst(f"{name} {key}", r[:, ch], ~frag[:, None], quiet=quiet)[0]
    key = "zdisp" if c["bf"] > 0 else "zdepth"
    rz = M.ratio(zout[:, 0], ref["zout"], ref["Mzout"], 1.0)
    res[key] = M.worst(f"{name} {key}", rz, ~ref["frag_z"], quiet=quiet)[0]
    return res


def within(res, frac=1.0, what=""):
    bad = {k: (v, frac * C[k]) for k, v in res.items() if not v <= frac * C[k]}
    assert not bad, (what, bad)


def shares(ref):
    """The fragile share of the covered pixels, per mask, the worst item."""
    cov = ref["covered"].flatten(1).sum(1).clamp(min=1).to(F64)
    return {k: float((ref[k] & ref["covered"]).flatten(1).sum(1).to(F64).div(cov).max()) for k in ("frag_out", "frag_flow", "frag_z", "frag_cnt")}
