"""fp64 references, product-shaped inputs and bounds for HITNet's non-convolution kernels (tile cost volume + arg-min,
slanted-plane warp costs, plane up-sampling, hypothesis selection: csrc/stereo.hip) and Fusion's kernels (quarter- and
full-resolution cues, the fused forget branch, the blend: csrc/fusion.hip), for
tests/test_stereo_fusion_fp64_reference.py (CPU: the references pinned to the oracle and the golden arrays, the fp32
oracle measured against them -- the measurement that sets every constant below -- and the power of the bounds) and
tests/test_gpu_stereo_fusion_fp64.py (the HIP kernels).  Shaped like tests/motion_fp64.py, whose ``U``, ``ratio`` and
``worst`` are reused.

Every reference returns its value AND the first-order magnitude ``M`` of the arithmetic that forms it; the bound of an
output element is  |got - ref64| <= c * 2^-24 * M  with one scalar ``c`` per kernel figure (C below).  ``c`` is 4 x the
worst |oracle32 - ref64| / (2^-24 M) that the project's fp32 CPU oracle (oracle/stereo.py, oracle/fusion.py) reaches on
these very inputs, rounded up to two digits (MEASURED; test_fp32_oracle_within_a_quarter_of_every_bound re-measures
it).  4 x: the convention of motion_fp64 (FMA contraction, summation order, 1-2 ulp libm).  M = 0 means: exact.

Two magnitudes carry a term beyond the plain sum of |terms|, each explained where it is formed: a warp cost (warp_rows)
samples the right feature row at a coordinate ``xs`` that is itself an fp32 result, so the sample inherits the
coordinate's rounding (2^-24 x the magnitudes xs is formed from) times the row's local gradient (the largest adjacent
tap difference per channel) -- the same term serves Fusion's stereo costs (xs = x - pred / ds); and a sigmoid that
underflows in fp32 (forget).  Both were needed for the fp32 CPU oracle itself."""
import math

import torch
import torch.nn.functional as F

from motion_fp64 import U, ratio, worst, _gen  # noqa: F401  (re-exported for the two test modules)

F64 = torch.float64

# ------------------------------------------------------------------------------------------------ cases
# tile_warp_cost (B, C, Ht, Wt, fr shifted by 4 bytes): 960x576 at its three finest levels (61 440 B staged and 256-thread
# groups; 128-thread; 64-thread), 640x512 at B = 2, KITTI 1280x384 finest (81 920 B: the opt-in path), odd sizes at B = 2,
# a row too large to stage (102 400 B), and a staged-size case whose fr is not 16-byte aligned (unstaged by alignment)
WARP_CASES = [(1, 16, 144, 240, 0), (1, 16, 72, 120, 0), (1, 24, 36, 60, 0), (2, 16, 128, 160, 0), (1, 16, 96, 320, 0),
              (2, 32, 37, 61, 0), (1, 32, 5, 200, 0), (1, 24, 36, 60, 1)]
# tile_costvol_argmin (B, Ht, Wt, D) at 16 channels: the five levels of 960x576 at max_disp 320; B = 2; D % 4 != 0 (the
# scalar kernel); D > 4 Wt (every tile has zero-padded candidates)
COSTVOL_CASES = [(1, 9, 15, 20), (1, 18, 30, 40), (1, 36, 60, 80), (1, 72, 120, 160), (1, 144, 240, 320),
                 (2, 128, 160, 320), (2, 37, 61, 25), (1, 18, 30, 50), (1, 5, 7, 1), (1, 4, 3, 20)]
HYP_CASES = [(1, 72, 120), (2, 37, 61), (1, 1, 1)]
# Fusion (B, H, W, P, ds, CF, CS); the last one: channel counts that the 8 / 4 channel slices do not divide (cues_lr only)
FUSION_CASES = [(1, 576, 960, 3, 4, 32, 24), (2, 512, 640, 3, 4, 32, 24), (1, 384, 1280, 3, 4, 32, 24),
                (2, 148, 268, 3, 4, 32, 24), (2, 148, 268, 5, 4, 32, 24), (1, 288, 480, 5, 4, 32, 24),
                (1, 74, 134, 3, 2, 32, 24), (1, 8, 12, 3, 4, 32, 24)]
CUES_LR_CASES = FUSION_CASES + [(2, 148, 268, 3, 4, 36, 20)]
case_id = lambda c: "B%d_" % c[0] + "x".join(str(v) for v in c[1:])

NEAR_TIE_CAP = 1e-3  # at most this share of a case's tiles may differ from the reference's arg-min (near ties only)

# worst |oracle32 - ref64| / (2^-24 M) of the fp32 CPU oracle over the cases above (CPU measurement) ...
MEASURED = {
    "costvol": 4.38, "warp_fea": 5.73, "warp_cost": 5.29, "hyp_upsample": 1.91, "hyp_select": 1.0, "cues_corr": 5.98,
    "cues_cost": 3.94, "cues_fr": 0.999, "forget": 1.77, "blend": 2.34,
}
# ... and c = 4 x that, rounded up to two digits
C = {
    "costvol": 18.0, "warp_fea": 23.0, "warp_cost": 22.0, "hyp_upsample": 7.7, "hyp_select": 4.0, "cues_corr": 24.0,
    "cues_cost": 16.0, "cues_fr": 4.0, "forget": 7.1, "blend": 9.4,
}


def within(res, frac=1.0, what=""):
    """Every measured figure of ``res`` is at most frac * C[key] (key = the part before any ':')."""
    bad = {k: (v, frac * C[k.split(":")[0]]) for k, v in res.items() if not v <= frac * C[k.split(":")[0]]}
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------ inputs
def lrelu_features(g, *shape, slope=0.2):
    """Feature maps as a (leaky-)ReLU leaves them: N(0, 1) with a log-normal scale per channel, then the activation."""
    s = torch.exp(0.4 * torch.randn(1, shape[1], 1, 1, generator=g))
    return F.leaky_relu(torch.randn(*shape, generator=g) * s, slope).contiguous()


def smooth_disparity(B, H, W, g, dmax, noise=0.25):
    """[B,1,H,W] fp32 >= 0: three random sinusoids spread over 0 .. dmax plus N(0, noise) per pixel (the depth_map idea
    of motion_fp64: a disparity map of a scene is smooth at the scale of a few pixels)."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=F64) / max(H, 8), torch.arange(W, dtype=F64) / max(W, 8), indexing="ij")
    f = torch.zeros(B, H, W, dtype=F64)
    for _ in range(3):
        a, fy, fx, ph = [torch.rand(B, 1, 1, generator=g, dtype=F64) for _ in range(4)]
        f = f + (0.3 + a) * torch.sin(2 * math.pi * ((fy * 2 - 1) * 1.5 * yy + (fx * 2 - 1) * 1.5 * xx + ph))
    lo, hi = f.amin((1, 2), keepdim=True), f.amax((1, 2), keepdim=True)
    d = (f - lo) / (hi - lo).clamp(min=1e-9) * dmax + noise * torch.randn(B, H, W, generator=g, dtype=F64)
    return d.clamp(min=0.0).float()[:, None].contiguous()


def warp_plants(Ht, Wt):
    """name -> (ty, tx, (d, dx, dy)) of the planted hypotheses of warp_case (W = 4 Wt): see warp_case."""
    W = 4 * Wt
    return {"integer_and_zero": (0, 0, (0.0, 0.0, 0.0)), "w_minus_1": (0, Wt - 1, (0.0, 0.0, 0.0)),
            "inside_-1_0": (0, 1, (4.5, 0.0, 0.0)), "beyond_-4": (Ht - 1, 0, (10.0, 0.0, 0.0)),
            "beyond_w+4": (Ht - 1, Wt - 1, (-12.0, 0.0, 0.0)), "1e6": (Ht // 2, Wt // 2, (1e6, 0.0, 0.0)),
            "slanted": (Ht // 2, 0, (2.5, 0.5, -0.5)), "w_minus_1_last_row": (Ht - 1, Wt - 2, (-4.0, 0.0, 0.0)),
            "_W": W}


def warp_case(case):
    """Inputs of tile_warp_cost: dict(fl, fr [B,C,4Ht,4Wt] leaky-ReLU features, h0, h1 [B,16,Ht,Wt] hypotheses (d smooth
    over 0 .. 0.6 W with noise, |dx|, |dy| <= 0.5, 13 descriptor channels)).  Planted in every item and both sets
    (warp_plants): d = 0 with a flat plane in the first tile (samples at exact integers, disparity 0) and in the last tile
    of the first row (its last sample is exactly W - 1); a sample inside (-1, 0); all four taps out of range beyond -4
    (first tile of the last row) and beyond W + 4 (the very last tile: the last lane of the last workgroup); 1e6; a
    slanted plane in the first column; a sample at exactly W - 1 in the last row."""
    B, Cc, Ht, Wt = case[:4]
    g = _gen(11, B, Cc, Ht, Wt)
    fl, fr = lrelu_features(g, B, Cc, 4 * Ht, 4 * Wt), lrelu_features(g, B, Cc, 4 * Ht, 4 * Wt)
    hyps = []
    for _ in range(2):
        h = torch.randn(B, 16, Ht, Wt, generator=g)
        h[:, 0:1] = smooth_disparity(B, Ht, Wt, g, 0.6 * 4 * Wt)
        h[:, 1:3] = (0.2 * h[:, 1:3]).clamp(-0.5, 0.5)
        for name, v in warp_plants(Ht, Wt).items():
            if name[0] != "_":
                h[:, 0:3, v[0], v[1]] = torch.tensor(v[2])
        hyps.append(h.contiguous())
    return dict(fl=fl, fr=fr, h0=hyps[0], h1=hyps[1])


def costvol_case(case):
    """(tl [B,16,Ht,Wt], tr [B,16,Ht,4Wt]): tr leaky-ReLU features; tl = tr at a smooth true disparity (where that lies
    inside the row and below D) + 30 % noise, independent features elsewhere -- so the arg-min is a decided match on most
    tiles, a contest of unrelated candidates on the rest.  Planted: all-zero left features (cost 0 at every zero-padded
    candidate: exact ties that ARE the minimum) in the first three tiles of the first row and in tile 1 of the last row;
    the last tile of the last row keeps a true match at disparity 0."""
    B, Ht, Wt, D = case
    g = _gen(12, B, Ht, Wt, D)
    tr = lrelu_features(g, B, 16, Ht, 4 * Wt)
    tl = lrelu_features(g, B, 16, Ht, Wt)
    dt = torch.round(smooth_disparity(B, Ht, Wt, g, 0.8 * D)[:, 0]).long()  # [B,Ht,Wt]
    dt[:, Ht - 1, Wt - 1] = 0
    src = 4 * torch.arange(Wt)[None, None, :] - dt
    ok = (src >= 0) & (dt < D)
    match = torch.gather(tr, 3, src.clamp(0, 4 * Wt - 1)[:, None].expand(B, 16, Ht, Wt))
    match = match + 0.3 * torch.randn(B, 16, Ht, Wt, generator=g) * match.abs().mean()
    tl = torch.where(ok[:, None], match, tl)
    tl[:, :, 0, :3] = 0.0
    tl[:, :, Ht - 1, min(1, Wt - 1)] = 0.0
    tl[:, :, Ht - 1, Wt - 1] = tr[:, :, Ht - 1, 4 * (Wt - 1)]
    return tl.contiguous(), tr.contiguous()


def hyp_case(case):
    """dict(prev [B,16,h,w] (hyp_upsample's input), cur, prv [B,16,h,w], upd [B,34,h,w] (hyp_select's operands)):
    d >= 0 smooth, slopes <= 0.5; updates N(0, 0.5) so that ReLU(d + update) clips some; confidences N(0, 1) with exact
    ties (must pick "previous") along the first row, at the last pixel and on every 7th pixel."""
    B, h, w = case
    g = _gen(13, B, h, w)
    out = {}
    for k in ("prev", "cur", "prv"):
        t = torch.randn(B, 16, h, w, generator=g)
        t[:, 0:1] = smooth_disparity(B, h, w, g, 2.0)
        t[:, 1:3] = (0.2 * t[:, 1:3]).clamp(-0.5, 0.5)
        out[k] = t.contiguous()
    out["prev"][:, 0:1] = smooth_disparity(B, h, w, g, 160.0)
    upd = torch.randn(B, 34, h, w, generator=g)
    upd[:, 2:] *= 0.5
    flat = upd.view(B, 34, -1)
    flat[:, 1, ::7] = flat[:, 0, ::7]
    upd[:, 1, 0, :] = upd[:, 0, 0, :]
    upd[:, 1, h - 1, w - 1] = upd[:, 0, h - 1, w - 1]
    out["upd"] = upd.contiguous()
    return out


def fusion_plants(H, W, ds):
    """name -> (low-res y, x, pred_curr value or None, pred_warp value or None) at the full-resolution pixel
    (ds y + ds/2 - 1, ds x + ds/2 - 1) that fusion_cues_lr reads; w = W / ds.  The sample position is x - pred / ds."""
    h, w = H // ds, W // ds
    return {"corner": (0, 0, 0.0, -ds * (w + 6.0)),          # pc: xs = 0 (integer, disparity 0); pw: xs = w + 6 (all taps out)
            "w_minus_1": (0, w - 1, 0.0, ds * 2.0),          # pc: xs = w - 1 exactly; pw: xs = w - 3
            "last_row": (h - 1, 0, ds * 0.5, ds * 6.0),      # pc: xs = -0.5 inside (-1, 0); pw: xs = -6 (beyond -4)
            "last_pixel": (h - 1, w - 1, ds * 1e6, ds * 1.25),  # pc: xs ~ -1e6; pw: a general position
            "interior": (h // 2, w // 2, ds * 1.0, None)}     # pc: an exact integer inside the row


def fusion_case(case):
    """Inputs of Fusion's kernels: dict(pc, pw [B,1,H,W], flow, conf [B,3,H,W], fc, fw [B,CF,h,w], fl, fr [B,CS,h,w]).
    pc: smooth_disparity over 0 .. min(320, 0.6 W); pw = pc + N(0, 0.3) on most pixels, pc + U(-250, 250) (kept > 0) on
    3 %; holes pw == 0 in a rectangle and at 20 isolated pixels (the first and the last pixel of the frame among them);
    8 negative pw values (the > 0 mask); the sample-position plants of fusion_plants.  fc: N(0, 1) with a per-channel
    scale (key_layer ends in a convolution), fw = 0.8 fc + 0.6 noise with a zero rectangle (warped from outside the
    view); fl, fr: leaky-ReLU features."""
    B, H, W, P, ds, CF, CS = case
    h, w = H // ds, W // ds
    g = _gen(14, B, H, W, P, ds, CF, CS)
    pc = smooth_disparity(B, H, W, g, min(320.0, 0.6 * W))
    pw = pc + 0.3 * torch.randn(B, 1, H, W, generator=g)
    far = torch.rand(B, 1, H, W, generator=g) < 0.03
    pw = torch.where(far, pc + (torch.rand(B, 1, H, W, generator=g) * 500 - 250), pw).clamp(min=0.01)
    pw[:, :, H // 4:H // 4 + H // 8 + 1, W // 3:W // 3 + W // 6 + 1] = 0.0
    for b in range(B):
        at = torch.randperm(H * W, generator=g)[:28]
        pw[b].view(-1)[at[:20]] = 0.0
        pw[b].view(-1)[at[20:]] = -3.0
    pw[:, :, 0, 0] = 0.0
    pw[:, :, H - 1, W - 1] = 0.0
    so = ds // 2 - 1
    for name, (y, x, vc, vw) in fusion_plants(H, W, ds).items():
        if vc is not None:
            pc[:, 0, ds * y + so, ds * x + so] = vc
        if vw is not None:
            pw[:, 0, ds * y + so, ds * x + so] = vw
    s = torch.exp(0.4 * torch.randn(1, CF, 1, 1, generator=g))
    fc = torch.randn(B, CF, h, w, generator=g) * s
    fw = 0.8 * fc + 0.6 * torch.randn(B, CF, h, w, generator=g) * s
    fw[:, :, h // 2:h // 2 + h // 5 + 1, :w // 6 + 1] = 0.0
    return dict(pc=pc.contiguous(), pw=pw.contiguous(), flow=(5.0 * torch.randn(B, 3, H, W, generator=g)).contiguous(),
                conf=torch.sigmoid(torch.randn(B, 3, H, W, generator=g)).contiguous(), fc=fc.contiguous(),
                fw=fw.contiguous(), fl=lrelu_features(g, B, CS, h, w), fr=lrelu_features(g, B, CS, h, w))


def forget_weights(case, cues):
    """The three forget_head layers as a state dict (oracle key names, fp32): N(0, 1 / fan_in) weights, N(0, 0.1)
    biases; then the last layer is scaled by a power of two (exact in every arithmetic) so that the 40th percentile of
    the reference logits |v| on ``cues`` (the fp64 cue tensor of this case) is about 1: logits in the middle of the
    sigmoid on a good share of the pixels, saturated ones at the holes and the far pixels (cues of up to 320)."""
    NC = cues.shape[1]
    g = _gen(15, *case)
    sd = {"fusion.forget_head.0.weight": torch.randn(16, NC, 1, 1, generator=g) / NC ** 0.5,
          "fusion.forget_head.0.bias": 0.1 * torch.randn(16, generator=g),
          "fusion.forget_head.1.weight": torch.randn(8, 16, 3, 3, generator=g) / 12.0,
          "fusion.forget_head.1.bias": 0.1 * torch.randn(8, generator=g),
          "fusion.forget_head.2.weight": torch.randn(1, 8, 1, 1, generator=g) / 8 ** 0.5,
          "fusion.forget_head.2.bias": 0.1 * torch.randn(1, generator=g)}
    v = forget(cues, sd)["v"]
    q = torch.quantile(v.abs().reshape(-1)[::7], 0.4).item()
    s = 2.0 ** round(math.log2(1.0 / max(q, 1e-30)))
    sd["fusion.forget_head.2.weight"] = sd["fusion.forget_head.2.weight"] * s
    sd["fusion.forget_head.2.bias"] = sd["fusion.forget_head.2.bias"] * s
    return sd


def blend_case(case):
    """(wf_lr [B,1,H/ds,W/ds], wr [B,1,H,W]): sigmoid outputs, N(0, 2) logits (some near 0 and 1)."""
    B, H, W, P, ds = case[:5]
    g = _gen(16, B, H, W, ds)
    return (torch.sigmoid(2 * torch.randn(B, 1, H // ds, W // ds, generator=g)).contiguous(),
            torch.sigmoid(2 * torch.randn(B, 1, H, W, generator=g)).contiguous())


# ------------------------------------------------------------------------------------------------ references: stereo
def costvol(tl, tr, D, variant=None):
    """The tile cost volume in fp64: cv[b,d,y,x] = sum_c |L[c,y,x] - R~[c,y,4x-d]|, R~ = 0 outside the row (reference
    initialization.py:18-45; restates oracle.stereo.tile_cost_volume) and Mv = sum_c (|L| + |R~|) -> dict(cv, Mv
    [B,D,Ht,Wt], cost = the minimum, arg = its FIRST index, gap = the distance to the best cost at any disparity that does
    not tie exactly (inf if none), tied = more than one disparity attains the minimum exactly).  Sums run in channel
    order, so mathematically equal costs (the zero-padded candidates d > 4x all cost sum |L|) are equal bit for bit.
    variants: "clamp" (the row's border value instead of zero), "last" (last arg-min among exact ties)."""
    B, Cc, Ht, Wt = tl.shape
    Wr = tr.shape[3]
    L, R = tl.to(F64), tr.to(F64)
    cv, Mv = torch.empty(B, D, Ht, Wt, dtype=F64), torch.empty(B, D, Ht, Wt, dtype=F64)
    x4 = 4 * torch.arange(Wt)
    for d0 in range(0, D, 16):
        d = torch.arange(d0, min(D, d0 + 16))
        idx = x4[None, :] - d[:, None]  # [dc, Wt]
        ok = ((idx >= 0) & (idx < Wr)).to(F64)
        if variant == "clamp":
            ok = torch.ones_like(ok)
        acc, mag = torch.zeros(B, Ht, len(d), Wt, dtype=F64), torch.zeros(B, Ht, len(d), Wt, dtype=F64)
        for c in range(Cc):
            g = R[:, c][:, :, idx.clamp(0, Wr - 1)] * ok  # [B,Ht,dc,Wt]
            acc = acc + (L[:, c][:, :, None, :] - g).abs()
            mag = mag + L[:, c][:, :, None, :].abs() + g.abs()
        cv[:, d0:d0 + len(d)] = acc.permute(0, 2, 1, 3)
        Mv[:, d0:d0 + len(d)] = mag.permute(0, 2, 1, 3)
    cost, arg = cv.min(1)
    tie = cv == cost[:, None]
    arg = tie.to(torch.uint8).argmax(1)  # the first index of the minimum
    if variant == "last":
        arg = D - 1 - tie.flip(1).to(torch.uint8).argmax(1)
    gap = torch.where(tie, torch.full_like(cv, float("inf")), cv - cost[:, None]).amin(1)
    return dict(cv=cv, Mv=Mv, cost=cost, arg=arg, gap=gap, tied=tie.sum(1) > 1)


def argmin_check(ref, got_cost, got_d, c):
    """The arg-min rule: ``got_d`` [B,Ht,Wt] must be the reference's first arg-min, except where the reference's gap to
    the pick is within the cost bound 2 c 2^-24 M (a near tie; never a LATER member of an exact tie: the first index is
    required there) -> dict(cost = worst err / (2^-24 M) of got_cost against the reference cost AT THE PICK, near = share
    of tiles that used the near-tie excuse, wrong = number of tiles that differ without excuse, where = the first such)."""
    cv, Mv = ref["cv"], ref["Mv"]
    D = cv.shape[1]
    gd = got_d.long()
    assert ((got_d == gd) & (gd >= 0) & (gd < D)).all(), "arg-min outside [0, D) or not an integer"
    c_at, M_at = cv.gather(1, gd[:, None])[:, 0], Mv.gather(1, gd[:, None])[:, 0]
    M_min = Mv.gather(1, ref["arg"][:, None])[:, 0]
    diff = gd != ref["arg"]
    in_tie = c_at == ref["cost"]
    near = diff & ~in_tie & ((c_at - ref["cost"]) <= 2 * c * U * torch.maximum(M_at, M_min))
    wrong = diff & ~near
    where = tuple(int(i) for i in torch.nonzero(wrong)[0]) if wrong.any() else None
    r = ratio(got_cost, c_at, M_at, 1.0)
    return dict(cost=worst("cost at the pick", r, quiet=True)[0], near=near.double().mean().item(), wrong=int(wrong.sum()),
                where=where)


def near_tie_share(ref, c):
    """The share of tiles whose best non-tying other disparity lies within 2 c 2^-24 M of the minimum (reference alone)."""
    M_min = ref["Mv"].gather(1, ref["arg"][:, None])[:, 0]
    return (ref["gap"] <= 2 * c * U * M_min).double().mean().item()


def warp_rows(fl, fr, xs, X, variant=None):
    """sum_c |fl - lerp(fr row, xs - k)| for k = -1, 0, 1 in fp64 -> (cost [B,3,H,W], M [B,3,H,W]).  fl, fr [B,C,H,W];
    xs [B,H,W] the k = 0 sample position, X [B,H,W] the sum of the magnitudes it is formed from.  Bilinear in x, zero
    outside the row (restates oracle.stereo.warp_x); a non-finite position gives NaN.
    M = sum_c (|l| + (1 - a)|t0| + a|t1|) + X sum_c max |adjacent tap difference| (over the sampled interval and its two
    neighbours): the second term is the sample's first-order sensitivity to the position it is taken at, times that
    position's own rounding -- the fp32 evaluation samples at ITS xs, not at the fp64 one.
    variant "clamp": the border value instead of zero outside the row."""
    B, Cc, H, W = fl.shape
    bad = ~torch.isfinite(xs)
    xz = torch.where(bad, torch.zeros_like(xs), xs)
    f0 = torch.floor(xz)
    a = xz - f0
    i0 = f0.clamp(-8, W + 8).long()
    idx = [i0 + j for j in range(-2, 4)]
    ok = [torch.ones_like(i, dtype=torch.bool) if variant == "clamp" else (i >= 0) & (i < W) for i in idx]
    idx = [i.clamp(0, W - 1) for i in idx]
    cost, M0, G = [torch.zeros(B, 3, H, W, dtype=F64) for _ in range(3)]
    for c in range(Cc):
        row, l = fr[:, c].to(F64), fl[:, c].to(F64)
        t = [torch.where(o, torch.gather(row, 2, i), torch.zeros_like(l)) for i, o in zip(idx, ok)]  # offsets -2 .. 3
        dif = [(t[j + 1] - t[j]).abs() for j in range(5)]
        for kk in range(3):  # k = kk - 1 samples at xs - k: taps at offsets (-k, -k + 1) -> t[2 - k], t[3 - k]
            lo = 3 - kk
            cost[:, kk] += (l - ((1 - a) * t[lo] + a * t[lo + 1])).abs()
            M0[:, kk] += l.abs() + (1 - a) * t[lo].abs() + a * t[lo + 1].abs()
            G[:, kk] += torch.maximum(torch.maximum(dif[lo - 1], dif[lo]), dif[lo + 1])
    nan = torch.full_like(cost, float("nan"))
    bad = bad[:, None].expand_as(cost)
    return torch.where(bad, nan, cost), torch.where(bad, nan, M0 + X[:, None] * G)


def plane_positions(hyp, variant=None):
    """The sample positions of a slanted tile hypothesis hyp [B,>=3,Ht,Wt] (d, dx, dy) at full resolution, fp64 ->
    (xs [B,4Ht,4Wt] = 4 tx + ix - (d + (ix - 1.5) dx + (iy - 1.5) dy), X = |x| + |d| + 1 + 2 (1.5 |dx| + 1.5 |dy|): the
    magnitudes xs is summed from -- the pixel, the disparity, the k = +-1 offset, and each slope term twice (its product
    and its sum are both rounded).  Restates oracle.stereo.to_plane (reference propagation.py:10-23).
    variant "offset": the plane centred at (ix - 2), (iy - 2)."""
    B, _, Ht, Wt = hyp.shape
    up = lambda t: t.to(F64).repeat_interleave(4, 1).repeat_interleave(4, 2)
    d, dx, dy = up(hyp[:, 0]), up(hyp[:, 1]), up(hyp[:, 2])
    o = (torch.arange(4, dtype=F64) - (2.0 if variant == "offset" else 1.5))
    ox, oy = o.repeat(Wt)[None, None, :], o.repeat(Ht)[None, :, None]
    x = torch.arange(4 * Wt, dtype=F64)[None, None, :]
    xs = x - (d + ox * dx + oy * dy)
    return xs, x + d.abs() + 1.0 + 3.0 * (dx.abs() + dy.abs())


def tile_warp(fl, fr, hyp, variant=None):
    """tile_warp_cost in fp64 -> (out [B,64,Ht,Wt] = [16 channels sum_c |fl| | 48 warp costs, channel
    16 + (k + 1) 16 + iy 4 + ix], M, xs): reference propagation.py:61-86, :157 as oracle.stereo.tile_warping /
    tile_update state it; restated through plane_positions and warp_rows.  M of the first 16 channels: the value itself.
    variants: "swap_k" (k = -1 and k = +1 exchanged), "offset", "clamp"."""
    xs, X = plane_positions(hyp, "offset" if variant == "offset" else None)
    cost, Mc = warp_rows(fl, fr, xs, X, "clamp" if variant == "clamp" else None)
    if variant == "swap_k":
        cost, Mc = cost.flip(1), Mc.flip(1)
    fea = fl.to(F64).abs().sum(1, keepdim=True)
    un = lambda t: F.pixel_unshuffle(t, 4)
    return torch.cat([un(fea), un(cost)], 1), torch.cat([un(fea), un(Mc)], 1), xs


def hyp_upsample(h, scale):
    """Plane up-sampling x2 in fp64 (reference propagation.py:26-32; restates oracle.stereo.upsample_hyp): channel 0 =
    (d -+ 0.5 dx -+ 0.5 dy) scale, M = (|d| + 0.5 |dx| + 0.5 |dy|) scale; channels 1 .. 15 are copies: M = 0 (exact)."""
    h64 = h.to(F64)
    up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    B, _, hh, ww = h.shape
    cx = torch.tensor([-0.5, 0.5], dtype=F64).repeat(ww)[None, None, None, :]
    cy = torch.tensor([-0.5, 0.5], dtype=F64).repeat(hh)[None, None, :, None]
    d, dx, dy = up(h64[:, 0:1]), up(h64[:, 1:2]), up(h64[:, 2:3])
    v = torch.cat([(d + cx * dx + cy * dy) * scale, up(h64[:, 1:])], 1)
    M = torch.cat([(d.abs() + 0.5 * dx.abs() + 0.5 * dy.abs()) * scale, torch.zeros_like(up(h64[:, 1:]))], 1)
    return v, M


def hyp_select(upd, cur, prv, variant=None):
    """Hypothesis selection in fp64 (reference propagation.py:225-240; restates the tail of oracle.stereo.tile_update):
    confidence upd[:, 1] > upd[:, 0] picks cur + upd[:, 18:34], else (ties included) prv + upd[:, 2:18]; ReLU on channel
    0 -> (value, M = |a| + |b|, sel).  The selection compares inputs: exact.  variant "ties_current": >= for >."""
    u = upd.to(F64)
    sel = (u[:, 1:2] >= u[:, 0:1]) if variant == "ties_current" else (u[:, 1:2] > u[:, 0:1])
    a = torch.where(sel, cur.to(F64), prv.to(F64))
    b = torch.where(sel, u[:, 18:34], u[:, 2:18])
    v = a + b
    v = torch.cat([F.relu(v[:, :1]), v[:, 1:]], 1)
    return v, a.abs() + b.abs(), sel


# ------------------------------------------------------------------------------------------------ references: fusion
def _patch(k, m, P, dil=2, pad_mode="constant"):
    """Yields (tap index, m shifted to tap (ky, kx) = m~[y + dil ky - pad, x + dil kx - pad]) of nn.Unfold(kernel P,
    padding dil (P - 1) / 2, dilation dil): reference fusion.py:66-70, 412-425."""
    H, W = k.shape[2:]
    pad = dil * (P - 1) // 2
    mp = F.pad(m, (pad, pad, pad, pad), mode=pad_mode)
    for ky in range(P):
        for kx in range(P):
            yield ky * P + kx, mp[:, :, dil * ky:dil * ky + H, dil * kx:dil * kx + W]


def patch_corr(k, m, P, drop=None, dil=2, norm=True):
    """Pixel-to-patch correlation in fp64 (reference fusion.py:168-198; restates oracle.fusion.px2patch for C > 1):
    out[:, tap] = <k, m~(tap)> / sqrt(C), M = sum_c |k| |m~| / sqrt(C); tap ``drop`` left out."""
    k64, m64 = k.to(F64), m.to(F64)
    s = 1.0 / math.sqrt(k.shape[1]) if norm else 1.0
    v, M = [], []
    for t, sh in _patch(k64, m64, P, dil):
        if t != drop:
            v.append((k64 * sh).sum(1, keepdim=True) * s)
            M.append((k64.abs() * sh.abs()).sum(1, keepdim=True) * s)
    return torch.cat(v, 1), torch.cat(M, 1)


def cues_lr(c, P, ds, variant=None):
    """fusion_cues_lr in fp64 on a fusion_case dict -> (corr_feat [B,3P^2+4,h,w], M, dsub [B,2,h,w] = the sub-sampled
    (pc, pw), xs [B,2,h,w] = the two sample positions).  Channels: P^2 cross correlations <fc, fw~>, P^2-1 self
    correlations of fc and of fw (tap P^2 // 2 dropped), 3 costs sum_c |fl - warp(fr, pc / ds + k)| / (CS / 24), 3 for
    pw (reference fusion.py:200-318; restates oracle.fusion.input_cues()[0], disparity_confidence).  Cost positions:
    xs = x - p / ds, X = |x| + 2 |p| / ds + 1 (the quotient and the difference are both rounded; the k offset).
    variants: "offset" (sub-sampled at ds / 2), "dilation" (1 for 2), "drop" (tap P^2 // 2 + 1 dropped), "norm"
    (1 / sqrt(CF) omitted)."""
    so = ds // 2 - (0 if variant == "offset" else 1)
    P2 = P * P
    dsub = torch.cat([c["pc"][..., so::ds, so::ds], c["pw"][..., so::ds, so::ds]], 1).to(F64)
    dil, drop, norm = (1 if variant == "dilation" else 2), P2 // 2 + (1 if variant == "drop" else 0), variant != "norm"
    parts = [patch_corr(c["fc"], c["fw"], P, None, dil, norm), patch_corr(c["fc"], c["fc"], P, drop, dil, norm),
             patch_corr(c["fw"], c["fw"], P, drop, dil, norm)]
    B, CS, h, w = c["fl"].shape
    x = torch.arange(w, dtype=F64)[None, None, :].expand(B, h, w)
    xs = []
    for s in range(2):
        p = dsub[:, s] / ds
        xs.append(x - p)
        cost, Mc = warp_rows(c["fl"], c["fr"], xs[-1], x + 2 * p.abs() + 1.0)
        parts.append((cost / (CS / 24.0), Mc / (CS / 24.0)))
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), dsub, torch.stack(xs, 1)


def cues_fr(c, P, variant=None):
    """fusion_cues_fr in fp64 -> (corr_feat_fr [B,3P^2+5,H,W], M): P^2 |pc - pw~(tap)|, P^2-1 |pc - pc~|, P^2-1
    |pw - pw~| (taps of dilation 2, zero padding, tap P^2 // 2 dropped), flow_warp, (pw > 0), conf_warp (reference
    fusion.py:243-318; restates oracle.fusion.input_cues()[1]).  M = |a| + |b| of each difference, 0 (exact) for the
    copied channels and the mask.  variant "replicate": replicate padding."""
    pc, pw = c["pc"].to(F64), c["pw"].to(F64)
    P2 = P * P
    mode = "replicate" if variant == "replicate" else "constant"
    v, M = [], []
    for k, m, drop in ((pc, pw, None), (pc, pc, P2 // 2), (pw, pw, P2 // 2)):
        for t, sh in _patch(k, m, P, 2, mode):
            if t != drop:
                v.append((k - sh).abs())
                M.append(k.abs() + sh.abs())
    tail = torch.cat([c["flow"].to(F64), (c["pw"] > 0).to(F64), c["conf"].to(F64)], 1)
    return torch.cat(v + [tail], 1), torch.cat(M + [torch.zeros_like(tail)], 1)


UNDERFLOW = 2.0 ** -102  # 2^-126 / 2^-24 (as motion_fp64.UNDERFLOW)


def _head(sd, p="fusion.forget_head"):
    g = lambda k: sd[f"{p}.{k}"].to(F64)
    return g("0.weight"), g("0.bias"), g("1.weight"), g("1.bias"), g("2.weight"), g("2.bias")


def forget(cues, sd):
    """The forget head on the fp64 cue tensor, LAYER BY LAYER in fp64 with the fp32 weights of ``sd`` (Conv1x1 nc -> 16,
    Conv3x3 16 -> 8 with zero padding, Conv1x1 8 -> 1; reference fusion.py:123-132; restates oracle.fusion.forget_head)
    -> dict(v = the logit, Mv = sum |w2| |W1| |W0| |cue| + the bias terms (the same three layers with absolute weights,
    biases and inputs), wr = sigmoid(v), M = sigma'(v) Mv + sigma(v) + UNDERFLOW: the logit's bound carried through the
    sigmoid, the sigmoid's own rounding, and -- the one term beyond first order -- the smallest normal fp32 number / 2^-24:
    below v = -87.3 the fp32 sigmoid is subnormal and below -88.7 exp(-v) overflows and the quotient is 0, where fp64
    still holds 1e-39; the fp32 CPU oracle needs the term (2e4 x the bound without it, at the 1e6 plants))."""
    W0, b0, W1, b1, w2, b2 = _head(sd)
    v = F.conv2d(F.conv2d(F.conv2d(cues, W0, b0), W1, b1, padding=1), w2, b2)
    Mv = F.conv2d(F.conv2d(F.conv2d(cues.abs(), W0.abs(), b0.abs()), W1.abs(), b1.abs(), padding=1), w2.abs(), b2.abs())
    s = torch.sigmoid(v)
    return dict(v=v, Mv=Mv, wr=s, M=s * (1 - s) * Mv + s + UNDERFLOW)


def merge_forget(sd, dtype=F64):
    """The head merged into one 3x3 convolution of the cue map, products formed in ``dtype``: -> [W_eff 9 x nc | beta 9 |
    c0] (W_eff[k] = w2 . W1[:, :, k] . W0, beta_k = w2 . W1[:, :, k] . b0, c0 = w2 . b1 + b2), the layout
    codd_fusion_forget takes."""
    W0, b0, W1, b1, w2, b2 = [t.to(dtype) for t in _head(sd)]
    A = torch.einsum("o,oikl->kli", w2[0, :, 0, 0], W1).reshape(9, -1)
    return torch.cat([(A @ W0[:, :, 0, 0]).reshape(-1), A @ b0, (w2[0, :, 0, 0] @ b1 + b2[0]).reshape(1)])


def forget_merged(cues, weff, beta_outside=False):
    """The merged form in fp64: v(p) = c0 + sum over the 3x3 taps k with p + k INSIDE the image of
    (W_eff[k] . cues(p + k) + beta_k) -> the logit.  beta_outside: beta_k added for taps outside the image too (wrong: the
    zero padding of the 3x3 layer acts on the 16-channel map, bias included)."""
    B, NC, H, W = cues.shape
    weff = weff.to(F64)
    We, beta, c0 = weff[:9 * NC].view(9, NC, 1, 1), weff[9 * NC:9 * NC + 9], weff[9 * NC + 9]
    d = F.conv2d(cues, We, beta)  # [B,9,H,W]: tap k's contribution when read AT p + k
    v = torch.full((B, 1, H, W), float(c0), dtype=F64)
    for k in range(9):
        dk = F.pad(d[:, k:k + 1], (1, 1, 1, 1))
        if beta_outside:
            dk = dk + beta[k] * (1 - F.pad(torch.ones(1, 1, H, W, dtype=F64), (1, 1, 1, 1)))
        v = v + dk[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W]
    return v


def blend(pc, pw, wf_lr, wr, ds, variant=None):
    """fusion_blend in fp64 (reference fusion.py:344-355, 383-394; restates the tail of oracle.fusion.memory_query):
    wf = nearest ds-fold up-sampling of wf_lr, both weights masked by pw > 0, fused = pc (1 - wf wr) + pw wf wr ->
    dict(fused, M = |pc| (1 + wf wr) + |pw| wf wr, wf, wr (a product with 0 or 1: exact), valid).
    variants: "no_mask", "wf_offset" (wf_lr read at (y + ds/2 - 1) / ds, (x + ds/2 - 1) / ds)."""
    B, _, H, W = pc.shape
    p, q = pc.to(F64), pw.to(F64)
    valid = (pw > 0).to(F64)
    if variant == "no_mask":
        valid = torch.ones_like(valid)
    o = ds // 2 - 1 if variant == "wf_offset" else 0
    iy = ((torch.arange(H) + o) // ds).clamp(max=H // ds - 1)
    ix = ((torch.arange(W) + o) // ds).clamp(max=W // ds - 1)
    wf = wf_lr.to(F64)[:, :, iy][:, :, :, ix] * valid
    w = wr.to(F64) * valid
    return dict(fused=p * (1 - wf * w) + q * wf * w, M=p.abs() * (1 + wf * w) + q.abs() * wf * w, wf=wf, wr=w, valid=valid)


# ------------------------------------------------------------------------------------------------ comparisons
# Each returns {key of C: worst err / (2^-24 M)} -- the figure that C is set from (CPU oracle) and checked against (GPU).
def warp_ratios(ref, got, name, keep=None):
    r = ratio(got, ref[0], ref[1], 1.0)
    k = (lambda sl: None) if keep is None else (lambda sl: keep[:, sl])  # keep: per element, [B,64,Ht,Wt]
    return {"warp_fea": worst(f"{name} tile_warp sum|fl|", r[:, :16], k(slice(0, 16)))[0],
            "warp_cost": worst(f"{name} tile_warp costs", r[:, 16:], k(slice(16, None)))[0]}


def cues_lr_ratios(ref, got, P, name, keep=None):
    r = ratio(got, ref[0], ref[1], 1.0)
    n = 3 * P * P - 2
    k = (lambda sl: None) if keep is None else (lambda sl: keep[:, sl])  # keep: per element, [B,3P^2+4,h,w]
    return {"cues_corr": worst(f"{name} cues_lr correlations", r[:, :n], k(slice(0, n)))[0],
            "cues_cost": worst(f"{name} cues_lr stereo costs", r[:, n:], k(slice(n, None)))[0]}


def forget_ratio(ref, got, name, keep=None):
    return {"forget": worst(f"{name} forget", ratio(got, ref["wr"], ref["M"], 1.0), keep)[0]}
