"""fp64 windowed reference of the dense SE3 Gauss-Newton step (codd_se3_gn_step; reference se3_field.py:150-170), for
tests/test_gauss_newton_fp64_reference.py (CPU: the reference itself and the power of the bounds) and
tests/test_gpu_gauss_newton.py (the HIP kernels against it).

Plain semantics, as oracle.motion.se3_build states them: a_ij = sigmoid(-|ae_i - ae_j|^2) from the difference itself,
H_i = sum_j a_ij J^T W_j J, b_i = sum_j a_ij J^T W_j r_ij with the closed-form Jacobian of oracle/motion.py, pairs with
X_j.z < MIN_DEPTH or Y.z < MIN_DEPTH skipped, no skip of small affinities.  The (2r+1)^2 window is walked one row of
offsets at a time, vectorised over the pixels and the offsets of the row: no dense [N, N] pair matrix."""
import math

import torch
import torch.nn.functional as F

from oracle import motion as om
from oracle import se3

# The GPU bound, per pixel, in the twist domain:  |log(T_gpu o T_ref^-1)|_inf <= TOL_REL * |dx_ref|_inf + TOL_ABS.
# TOL_ABS: fp32 storage of T and the fp32 exp / compose of the retraction, a few ulps of max(1, |t|) (|t| < 1 here).
TOL_ABS = 1e-6
# TOL_REL: 4x the worst max(err - TOL_ABS, 0) / |dx_ref|_inf measured on MI355X over every case x builder {3, 5} x
# q4 {16, 192, 4096} of tests/test_gpu_gauss_newton.py: 4.19e-3 at (1, 48, 160, 32), q4 = 16 (2.85e-3 at q4 = 4096,
# 1.48e-3 at q4 = 192); at the benchmarked (1, 72, 120, 32): 1.1e-3 / 3.04e-4 / 4.96e-4 at q4 = 16 / 192 / 4096.
TOL_REL = 1.7e-2
# TOL_REL_HEADS: codd_se3_gn_step_heads (split / split16) against fp64 heads + the fp64 step, 4x the worst measured on
# MI355X: 3.10e-4 at (1, 72, 120, 32), split16 (3.03e-4 split; 1.56e-5 at (2, 37, 61, 32)).
TOL_REL_HEADS = 1.3e-3

F64 = torch.float64


def se3_inv(T):
    """[..., 7] -> T^-1 = (-R(q*) t, q*)."""
    qi = torch.cat([-T[..., 3:6], T[..., 6:]], -1)
    return torch.cat([-se3.qrot(qi, T[..., :3]), qi], -1)


def twist_error(T_got, T_ref):
    """|log(T_got o T_ref^-1)|_inf per pixel, fp64."""
    return se3.log(se3.compose(T_got.to(F64), se3_inv(T_ref.to(F64)))).abs().amax(-1)


def _rot(q):
    """unit quaternion [..., 4] (xyzw) -> R as nested lists of [...] tensors."""
    x, y, z, w = q.unbind(-1)
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _pair_terms(Ti, ai, Xj, tgj, wtj, aj, okj, K):
    """Per-pair Jacobian J [..., 3, 6], residual r [..., 3] and weights a_ij * w_j [..., 3] (0 for a skipped pair).
    i-quantities broadcast against j-quantities: Ti [..., 7], ai [C, ...]; Xj / tgj / wtj [3, ...], aj [C, ...],
    okj [...] (j inside the image)."""
    fx, fy, cx, cy = K
    R = _rot(Ti[..., 3:])
    Y = [R[k][0] * Xj[0] + R[k][1] * Xj[1] + R[k][2] * Xj[2] + Ti[..., k] for k in range(3)]
    ok = okj & (Xj[2] >= om.MIN_DEPTH) & (Y[2] >= om.MIN_DEPTH)
    d2 = ((ai - aj) ** 2).sum(0)
    a = torch.sigmoid(-d2) * ok
    Yx, Yy = Y[0], Y[1]
    Yz = torch.where(ok, Y[2], torch.ones_like(Y[2]))
    d = 1.0 / Yz
    o, z = torch.ones_like(d), torch.zeros_like(d)
    Jx = fx * torch.stack([d, z, -Yx * d * d, -Yx * Yy * d * d, o + Yx * Yx * d * d, -Yy * d], -1)
    Jy = fy * torch.stack([z, d, -Yy * d * d, -(o + Yy * Yy * d * d), Yx * Yy * d * d, Yx * d], -1)
    Jz = torch.stack([z, z, -d * d, -Yy * d * d, Yx * d * d, z], -1)
    J = torch.stack([Jx, Jy, Jz], -2)
    r = torch.stack([tgj[0] - (fx * Yx * d + cx), tgj[1] - (fy * Yy * d + cy), tgj[2] - d], -1)
    wk = a[..., None] * torch.stack([wtj[0], wtj[1], wtj[2]], -1)
    return J, r, wk


def _points(depth1, K):
    B = depth1.shape[0]
    return om.inv_project(depth1.to(F64), torch.tensor([list(K)] * B, dtype=F64)).permute(0, 3, 1, 2)  # [B,3,h,w]


def pair_term(T, ae8, target, weight, depth1, K8, b, yi, xi, yj, xj):
    """One pair's (H_ij [6, 6], b_ij [6]) in fp64: what pixel (yi, xi) of batch item b gets from neighbour (yj, xj)."""
    K = [float(v) for v in K8]
    X = _points(depth1, K)[b]
    J, r, wk = _pair_terms(T[b, yi, xi].to(F64), ae8[b, :, yi, xi].to(F64), X[:, yj, xj], target[b, :, yj, xj].to(F64),
                           weight[b, :, yj, xj].to(F64), ae8[b, :, yj, xj].to(F64), torch.tensor(True), K)
    Jw = J * wk[..., None]
    return Jw.transpose(-1, -2) @ J, (Jw * r[..., None]).sum(-2)


def normal_equations(T, ae8, target, weight, depth1, K8, radius, rows=None):
    """fp64 (H [B,n,w,6,6], b [B,n,w,6], Habs, babs) -- Habs / babs: the sums of the absolute values of the terms.
    T [B,h,w,7], ae8 [B,C,h,w] (= ae / 8), target = xyz + delta [B,3,h,w], weight [B,3,h,w], depth1 [B,h,w],
    K8 = (fx, fy, cx, cy).  ``rows`` = (y0, y1): only the pixels i of those rows (n = y1 - y0; default all)."""
    B, h, w = depth1.shape
    r = int(radius)
    y0, y1 = rows if rows is not None else (0, h)
    K = [float(v) for v in K8]
    C = ae8.shape[1]
    jq = torch.cat([_points(depth1, K), target.to(F64), weight.to(F64), ae8.to(F64), torch.ones(B, 1, h, w, dtype=F64)], 1)
    jq = F.pad(jq, (r, r, r, r))  # (the last channel, 0 in the padding, marks j inside the image)
    Ti = T[:, y0:y1].to(F64)[:, :, :, None]  # [B, n, w, 1, 7]: i broadcast over a row of offsets
    ai = ae8[:, :, y0:y1].to(F64).permute(1, 0, 2, 3)[..., None]  # [C, B, n, w, 1]
    n = y1 - y0
    H = torch.zeros(B, n, w, 6, 6, dtype=F64)
    bv = torch.zeros(B, n, w, 6, dtype=F64)
    Ha, ba = torch.zeros_like(H), torch.zeros_like(bv)
    for dy in range(-r, r + 1):
        # j rows y0 + dy .. y1 - 1 + dy of the padded image at every column offset dx = -r .. r: [ch, B, n, w, 2r+1]
        sl = jq[:, :, r + y0 + dy:r + y1 + dy].unfold(-1, w, 1).permute(1, 0, 2, 4, 3)
        J, res, wk = _pair_terms(Ti, ai, sl[0:3], sl[3:6], sl[6:9], sl[9:9 + C], sl[9 + C] > 0.5, K)
        Jw = J * wk[..., None]  # [B, n, w, 2r+1, 3, 6]: one batched [6, 3(2r+1)] x [3(2r+1), 6] product per pixel
        H += torch.einsum("byxdkp,byxdkq->byxpq", Jw, J)
        bv += torch.einsum("byxdkp,byxdk->byxp", Jw, res)
        Jwa = Jw.abs()
        Ha += torch.einsum("byxdkp,byxdkq->byxpq", Jwa, J.abs())
        ba += torch.einsum("byxdkp,byxdk->byxp", Jwa, res.abs())
    return H, bv, Ha, ba


def solve(H, b, lm=1e-4, ep=10.0):
    """dx of (H + (lm H_pp + ep) I) dx = b in fp64: H [..., 6, 6], b [..., 6] -> [..., 6]."""
    dg = torch.diagonal(H, dim1=-2, dim2=-1)
    return torch.linalg.solve(H + torch.diag_embed(lm * dg + ep), b[..., None])[..., 0]


def retract(dx, T):
    """exp(dx) o T in fp64."""
    return se3.compose(se3.exp(dx.to(F64)), T.to(F64))


def gn_step(T, ae8, target, weight, depth1, K8, radius, lm=1e-4, ep=10.0):
    """The step: dict(H, b, Habs, babs, dx, T_new), all fp64."""
    H, b, Ha, ba = normal_equations(T, ae8, target, weight, depth1, K8, radius)
    dx = solve(H, b, lm, ep)
    return dict(H=H, b=b, Habs=Ha, babs=ba, dx=dx, T_new=retract(dx, T))


def heads(hidden, Wm, bm):
    """The three 1x1 heads in fp64 from fp32 hidden channels [B,768,h,w], weights [38,256] and biases [38] (ae rows
    0..31 read channels 0..255, delta 32..34 read 256..511, weight 35..37 read 512..767; motion.pack_head_matrix)
    -> (ae, delta, weight, the weight logits, sum |w||x| per weight row)."""
    x, W, bb = hidden.to(F64), Wm.to(F64), bm.to(F64)
    grp = lambda i: x[:, 256 * i:256 * (i + 1)]
    lin = lambda i, lo, hi: torch.einsum("oc,bchw->bohw", W[lo:hi], grp(i)) + bb[lo:hi, None, None]
    pre = lin(2, 35, 38)
    mag = torch.einsum("oc,bchw->bohw", W[35:38].abs(), grp(2).abs())
    return lin(0, 0, 32), lin(1, 32, 35), torch.sigmoid(pre), pre, mag


# ------------------------------------------------------------------------------ inputs shaped like the update loop's
# (B, h, w, radius): the benchmarked 960x576 / 8; 640x512 / 8 at B = 2; 1280x384 / 8; odd width, partial tiles and
# B = 2; odd width at a small radius; a map smaller than one tile; self-pairs only
CASES = [(1, 72, 120, 32), (2, 64, 80, 32), (1, 48, 160, 32), (2, 37, 61, 32), (1, 21, 45, 6), (1, 5, 3, 32),
         (1, 16, 24, 0)]
# |a|^2 = |ae / 8|^2 of the update loop: a 640x512 frame of the conditioned weight set (codd_amd.synth) through the CPU
# oracle, all 16 iterations: max |ae / 8| 0.66 .. 0.75, median |a|^2 0.86 .. 0.90, max |a|^2 1.72 .. 1.91 (the random
# set at gain 1.4: 0.65 .. 0.74, 0.88 .. 0.91, 1.77 .. 1.91)
A2_MEDIAN, A2_MAX = 0.9, 1.9
NEAR = 0.3  # depth of the near patch that some pixels' motion puts behind MIN_DEPTH


def make_case(B, h, w, radius, seed=0, common=False):
    """fp32 inputs of codd_se3_gn_step: dict(T, ae, xyz, delta, weight, d1, K8, radius, target, segment).  Five segments
    per item (Voronoi cells): piecewise-constant embeddings with noise (intra-segment affinities ~0.3-0.45, between
    segments ~0.15), a depth plane each (2..60), a small motion each; delta and weight in the ranges of the heads; a few
    depths below MIN_DEPTH; a near patch (depth NEAR) that three pixels' motion moves behind Y.z = MIN_DEPTH.
    ``common``: every embedding carries one large common component, |a|^2 ~ A2_MAX (the top of the measured range),
    with the same differences."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * h + 13 * w + B)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    K8 = (131.25, 131.25, w / 2.0 - 0.25, h / 2.0 + 0.375)
    ns = 5
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    sy, sx = ru(B, ns, 1, 1) * h, ru(B, ns, 1, 1) * w
    lab = ((yy - sy) ** 2 + (xx - sx) ** 2).argmin(1)  # [B,h,w]
    pick = lambda v: v[torch.arange(B)[:, None, None], lab]  # per-segment values [B, ns, ...] -> [B, h, w, ...]
    # embeddings (ae = 8 a): centres of |a|^2 ~ A2_MEDIAN, per-segment noise of 0.05 .. 0.12 per channel
    cen = rn(B, ns, 32) * math.sqrt(A2_MEDIAN / 32)
    sig = 0.05 + 0.07 * ru(B, ns, 1)
    a8 = pick(cen) + pick(sig) * rn(B, h, w, 32)
    if common:
        c = rn(32)
        a8 = a8 * 0.35 + c * math.sqrt(A2_MAX / float((c * c).sum()))
    ae = (8.0 * a8).permute(0, 3, 1, 2).contiguous()
    # depth: a plane per segment, 2 .. 60
    base = torch.exp(math.log(2.5) + ru(B, ns) * math.log(20.0))
    gy, gx = (ru(B, ns) - 0.5) * 0.4, (ru(B, ns) - 0.5) * 0.4
    d1 = pick(base[..., None]).squeeze(-1) * (1 + pick(gy[..., None]).squeeze(-1) * (yy / h - 0.5)
                                               + pick(gx[..., None]).squeeze(-1) * (xx / w - 0.5))
    d1 = (d1 * (1 + 0.01 * rn(B, h, w))).clamp(2.0, 60.0)
    # motion: a twist per segment + small per-pixel noise
    tw = pick(rn(B, ns, 6) * torch.tensor([0.05, 0.05, 0.05, 0.01, 0.01, 0.01])) + \
        rn(B, h, w, 6) * torch.tensor([0.003, 0.003, 0.003, 0.0005, 0.0005, 0.0005])
    T = se3.exp(tw)
    # a few depths below MIN_DEPTH (masked as neighbours)
    for b in range(B):
        for k in range(4):
            d1[b, int(ru(1) * h), int(ru(1) * w)] = 0.02 if k % 2 else 0.0
    # the near patch and the three pixels whose motion puts it behind MIN_DEPTH
    py, px = min(h // 3, h - 2), max(0, min(w // 4, w - 3))
    d1[:, py:py + 2, px:px + 2] = NEAR
    Kt = torch.tensor([list(K8)] * B)
    xyz = om.project(se3.act(T, om.inv_project(d1, Kt)), Kt)  # (raft_geometry's xyz, before the push below)
    for (y, x) in ((py, px + 2), (py + 1, px + 2), (py, px)):
        T[:, y, x, 2] = -(NEAR + 0.05)
    # heads-like delta (|delta| <= 0.1) and weight (0.1 .. 0.95)
    delta = (pick(rn(B, ns, 3) * 0.02) + rn(B, h, w, 3) * 0.03).clamp(-0.1, 0.1).permute(0, 3, 1, 2).contiguous()
    weight = torch.sigmoid(0.5 + 1.2 * rn(B, 3, h, w))
    target = (xyz.permute(0, 3, 1, 2) + delta).contiguous()  # (fp32, as the prep kernel forms it)
    return dict(T=T.contiguous(), ae=ae, xyz=xyz.contiguous(), delta=delta, weight=weight, d1=d1.contiguous(), K8=K8,
                radius=radius, target=target, segment=lab)


def reference(c):
    """gn_step of a make_case dict."""
    return gn_step(c["T"], c["ae"] / 8.0, c["target"], c["weight"], c["d1"], c["K8"], c["radius"])


def bound(dx):
    """The per-pixel GPU bound for reference steps dx [..., 6]."""
    return TOL_REL * dx.abs().amax(-1) + TOL_ABS


# ------------------------------------------------------------------------------ the builders' work split, restated
def gn_groups(nj, q4, gmax):
    """codd_amd/csrc/motion.hip gn_groups."""
    return max(1, min((nj + q4 // 2) // q4, gmax))


def slot_starts(h, w, radius, q4, tile_y, tile_x):
    """The first neighbour (y, x) of every wave slot of tile (tile_y, tile_x), as se3_gn_build_kernel<false|true> cut the
    tile's clipped window: G = gn_groups(nj, q4, gmax) workgroups x 4 waves, slot s starts at nj * s // (4 G)."""
    q4 = max(q4, 16)
    gmax = gn_groups((8 + 2 * radius) ** 2, q4, 1 << 20)
    ty0, tx0 = 8 * tile_y, 8 * tile_x
    ylo, yhi = max(ty0 - radius, 0), min(ty0 + 7 + radius, h - 1)
    xlo, xhi = max(tx0 - radius, 0), min(tx0 + 7 + radius, w - 1)
    ncols = xhi - xlo + 1
    nj = (yhi - ylo + 1) * ncols
    nslots = 4 * gn_groups(nj, q4, gmax)
    return [(ylo + s0 // ncols, xlo + s0 % ncols) for s0 in (nj * s // nslots for s in range(nslots))]
