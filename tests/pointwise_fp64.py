"""fp64 references, cases and bounds for the pointwise kernels that the other fp64 modules leave out: the stand-alone GRU
gates (csrc/motion.hip), the context-network helpers and the state copy (csrc/context.hip, codd_context_split,
ops.batch_pair), the three metric kernels and the two ablation kernels (csrc/fusion.hip); for
tests/test_pointwise_fp64_reference.py (CPU: the fp32 oracle / restatement of each operation against these references --
the measurement that sets every constant below -- the power of the bounds, the threshold clearance of the metric inputs
and the tie measurement of the nearest warp) and tests/test_gpu_pointwise_fp64.py (the HIP kernels).

Every reference returns its value AND the first-order magnitude ``M`` of the arithmetic that forms it; the bound of an
output element is |got - ref64| <= c * 2^-24 * M with one ``c`` per figure (C below) = 4 x the worst
|oracle32 - ref64| / (2^-24 M) of the project's fp32 CPU oracle or restatement on this module's own cases, rounded up to
two digits (MEASURED; re-measured by test_fp32_oracle_within_a_quarter_of_every_bound).  Copies, selections, masks and
counts have M = 0: they are exact.

Two rules are the kernels' documented ones (include/codd_hip.h) and are restated here rather than taken from a torch
function: a batch of B is B frames added in index order (one mean per item, an empty item adds nothing), and the nearest
warp samples at rint(float32(x) + fx), half to even on the fp32 sum, inside when the ROUNDED value lies in the map."""
import math

import torch
import torch.nn.functional as F

from conv_fp64 import PLANTED, UNDERFLOW, decode, records  # noqa: F401  (re-exported for the two test modules)
from motion_fp64 import U, _gen, induced_flow, ratio, se3_field, worst  # noqa: F401

F64 = torch.float64
LO, HI, THR, BF = 1.0, 210.0, 3.0, 210.0
REL_EPS = float(torch.tensor(1e-3, dtype=torch.float32))  # the kernel's (and torch's fp32) 1e-3f, not the double 1e-3
case_id = lambda c: "x".join(str(v) for v in c)

# (B, H, W, h, w): today's case; a second trip of the 128 x 256 stride loop with a ragged tail at B = 2; 127 idle blocks;
# crop = map; KITTI
METRIC_CASES = [(1, 64, 96, 60, 90), (2, 192, 256, 150, 230), (1, 8, 8, 1, 1), (2, 40, 56, 40, 56), (1, 384, 1280, 375, 1242)]
TEPE_VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (gt_mask = the KITTI dummy, gt2_prev given)
FLOW_KINDS = ("float", "q64", "half")
# (B, C, Hi, Wi, Ho, Wo, align_corners): HRModule up paths x2 / x4 / x8; ResizeConcatConv; non-integer ratios in both
# modes; down-scaling; Ho == 1, Wo == 1, Hi == 1 (the ``Ho > 1 ?`` branch); B = 2 with C = 3; 1/32 -> 1/4 of a 576 x 960
# frame at the 18 channels of the fuse layer and at the 144 of ResizeConcatConv
RESIZE_CASES = [(1, 2, 5, 7, 10, 14, 0), (1, 2, 3, 5, 12, 20, 0), (1, 2, 3, 5, 24, 40, 0), (1, 2, 9, 15, 18, 30, 1),
                (1, 2, 9, 15, 36, 60, 1), (1, 2, 5, 7, 13, 17, 0), (1, 2, 5, 7, 13, 17, 1), (1, 2, 13, 17, 5, 7, 0),
                (1, 2, 13, 17, 5, 7, 1), (1, 2, 5, 7, 1, 9, 1), (1, 2, 5, 7, 9, 1, 1), (1, 2, 1, 7, 4, 9, 1),
                (2, 3, 5, 7, 10, 14, 0), (2, 3, 9, 15, 18, 30, 1), (1, 18, 18, 30, 144, 240, 0), (1, 144, 18, 30, 144, 240, 1)]
RESIZE_FORMS = ("overwrite", "accumulate", "relu", "extra", "extra_accumulate")
ADD_RELU_N = [1, 255, 257, 1 * 18 * 144 * 240]
SPLIT_CASES = [(1, 1, 1), (2, 5, 7), (1, 72, 120)]  # context_split (B, h, w)
GATE_CASES = [(1, 1, 1), (2, 5, 7), (2, 37, 61), (1, 72, 120)]
SELECT_CASES = [(1, 3, 300, 3, 300), (2, 8, 12, 6, 9)]  # (B, H, W, hg, wg)
GT_MOTION_CASES = [(1, 4, 8, 260, 8, 260), (2, 24, 16, 24, 13, 22)]  # (B, C, H, W, hg, wg)

# worst |oracle32 - ref64| / (2^-24 M) over the cases above (CPU measurement; which oracle: DESIGN.md) ...
MEASURED = {
    "gate_z": 1.93, "gate_rh": 1.28, "gate_q": 1.03, "resize": 1.17, "add_relu": 1.0, "ctx_tanh": 1.07, "kalman": 0.398,
    "gt_avg": 0.5, "disp_epe": 0.295, "tepe": 1.0, "tepe_rel": 0.995, "flow_mag": 1.83, "sf_epe3": 0.319, "sf_epe2": 0.539,
}
# ... and c = 4 x that, rounded up to two digits
C = {
    "gate_z": 7.8, "gate_rh": 5.2, "gate_q": 4.2, "resize": 4.7, "add_relu": 4.0, "ctx_tanh": 4.3, "kalman": 1.6,
    "gt_avg": 2.0, "disp_epe": 1.2, "tepe": 4.0, "tepe_rel": 4.0, "flow_mag": 7.4, "sf_epe3": 1.3, "sf_epe2": 2.2,
}
EXACT = ("count", "select", "copy")  # figures with M = 0


def within(res, frac=1.0, what=""):
    """Every measured figure of ``res`` is at most frac * C[key] (key = the part before any ':')."""
    bad = {k: (v, frac * C[k.split(":")[0]]) for k, v in res.items() if not v <= frac * C[k.split(":")[0]]}
    assert not bad, (what, bad)


def fig(name, got, ref, M, keep=None):
    """worst |got - ref| / (2^-24 M) of one figure (0 where both agree exactly, inf where M = 0 and they do not)."""
    return worst(name, ratio(got, ref, M, 1.0), keep, quiet=True)[0]


# ------------------------------------------------------------------------------------------------ GRU gates
def gate_inputs(B, h, w, tag=21):
    """t1, t2 [B,256,h,w] and q1, q2 [B,128,h,w] (the gate convolutions' outputs), inp / cor / mot [B,384,h,w], hidden
    state [B,128,h,w] = tanh features; channels 1 .. 4 of the z, r and q blocks carry pre-activations planted beyond +-20
    and +-90 (saturation; expf overflows to inf), as conv_fp64.gate_inputs does."""
    g = _gen(tag, B, h, w)
    r = lambda c: torch.randn(B, c, h, w, generator=g)
    d = dict(t1=r(256), t2=r(256), q1=r(128), q2=r(128), inp=torch.relu(r(384)) * 1.5, cor=r(384) * 0.5, mot=r(384) * 0.5,
             h=torch.tanh(r(128) * 1.5))
    plant = torch.tensor(PLANTED).view(1, 4, 1, 1)
    for blk in (0, 128):
        d["t1"][:, blk + 1:blk + 5] += plant
    d["q1"][:, 1:5] += plant
    return {k: v.contiguous() for k, v in d.items()}


def _isum(d, lo, hi, summed):
    """(inp + cor) + mot over channels [lo, hi) in fp64 and the sum of |terms|; ``summed``: cor = mot = None (inp holds
    the sum already)."""
    if summed:
        return d["inp"][:, lo:hi].to(F64), d["inp"][:, lo:hi].to(F64).abs()
    t = [d[k][:, lo:hi].to(F64) for k in ("inp", "cor", "mot")]
    return t[0] + t[1] + t[2], t[0].abs() + t[1].abs() + t[2].abs()


def gate_zr(d, summed=False, variant=None):
    """codd_gru_gate_zr in fp64 -> {"gate_z": (zr [B,256,h,w], M), "gate_rh": (r * h, M)}: zr = sigmoid((t1 + t2) +
    isum), magnitudes as conv_fp64.gate2_ref (0.25 = the sigmoid's slope, + the value, + UNDERFLOW).
    variant "swap_zr": the z and r halves exchanged."""
    s, Ms = _isum(d, 0, 256, summed)
    t1, t2 = d["t1"].to(F64), d["t2"].to(F64)
    pre, Mp = (t1 + t2) + s, t1.abs() + t2.abs() + Ms
    zr = torch.sigmoid(pre)
    if variant == "swap_zr":
        zr, Mp = torch.cat([zr[:, 128:], zr[:, :128]], 1), torch.cat([Mp[:, 128:], Mp[:, :128]], 1)
    Mzr = 0.25 * Mp + zr + UNDERFLOW
    hh = d["h"].to(F64)
    rh = zr[:, 128:] * hh
    return {"gate_z": (zr, Mzr), "gate_rh": (rh, Mzr[:, 128:] * hh.abs() + rh.abs())}


def gate_q(d, zr, summed=False, variant=None):
    """codd_gru_gate_q in fp64 with z = zr[:, :128] as the device holds it -> (h' = (1 - z) h + z tanh((q1 + q2) +
    isum[256:384]), M as conv_fp64.gate3_ref).  variants: "q_block" (inp read at channel block 128), "blend_swap"
    (z h + (1 - z) q)."""
    o = 128 if variant == "q_block" else 256
    s, Ms = _isum(d, o, o + 128, summed)
    q1, q2, hh, z = d["q1"].to(F64), d["q2"].to(F64), d["h"].to(F64), zr[:, :128].to(F64)
    q = torch.tanh((q1 + q2) + s)
    Mq = q1.abs() + q2.abs() + Ms + q.abs()
    val = z * hh + (1 - z) * q if variant == "blend_swap" else (1 - z) * hh + z * q
    return val, z.abs() * Mq + hh.abs() + (z * hh).abs() + (z * q).abs() + val.abs()


def gate_oracle32(d, summed=False):
    """The arithmetic of oracle.motion.conv_gru in fp32 torch, the six convolution results given: -> (zr, rh, h')."""
    tot = d["inp"] if summed else sum(d[k] for k in ("inp", "cor", "mot"))
    z = torch.sigmoid(d["t1"][:, :128] + d["t2"][:, :128] + tot[:, :128])
    r = torch.sigmoid(d["t1"][:, 128:] + d["t2"][:, 128:] + tot[:, 128:256])
    rh = r * d["h"]
    q = torch.tanh(d["q1"] + d["q2"] + tot[:, 256:])
    return torch.cat([z, r], 1), rh, (1 - z) * d["h"] + z * q


# ------------------------------------------------------------------------------------------------ context helpers
def resize_inputs(case, tag=31):
    """x [B,C,Hi,Wi] ~ N(0, 1) with a scale per channel, out0 (the pre-filled output of the accumulate forms) and extra
    [B,C,Ho,Wo]."""
    B, Cc, Hi, Wi, Ho, Wo, ac = case
    g = _gen(tag, *case)
    x = torch.randn(B, Cc, Hi, Wi, generator=g) * torch.exp(torch.randn(1, Cc, 1, 1, generator=g))
    return x.contiguous(), torch.randn(B, Cc, Ho, Wo, generator=g), torch.randn(B, Cc, Ho, Wo, generator=g)


def _src_coord(n_in, n_out, ac, variant):
    o = torch.arange(n_out, dtype=F64)
    if variant == "ac_swap":
        ac = not ac
    if ac:
        return (n_in - 1) / (n_out - 1) * o if n_out > 1 else torch.zeros(n_out, dtype=F64)
    if variant == "no_half":
        return (n_in / n_out) * o
    return ((n_in / n_out) * (o + 0.5) - 0.5).clamp(min=0.0)


def resize(x, size, ac, form="overwrite", out0=None, extra=None, variant=None):
    """codd_resize_bilinear(_add) in fp64 (F.interpolate(mode="bilinear") semantics) -> (value, M).  The blend is taken
    at the EXACT source coordinate; the kernel (and torch) form the coordinate in fp32, so M carries, next to the sum of
    the |weighted taps|, the coordinate's magnitude (|s| + 1: its rounding is 2^-24 of that) times the largest adjacent
    tap difference within one cell of the sampled one, per axis -- the term stereo_fusion_fp64.warp_rows uses for a
    sampled coordinate.  Bilinear interpolation is continuous across a cell boundary, so a y0 that differs by one from
    the exact one is covered by that term.  forms: RESIZE_FORMS; the sums are ((out0 + extra) + blend) as the kernel adds.
    variants: "ac_swap" (align_corners modes exchanged), "no_half" (the half-pixel offset dropped)."""
    B, Cc, Hi, Wi = x.shape
    Ho, Wo = size
    x64 = x.to(F64)
    sy, sx = _src_coord(Hi, Ho, ac, variant), _src_coord(Wi, Wo, ac, variant)
    y0, x0 = sy.floor().clamp(max=Hi - 1).long(), sx.floor().clamp(max=Wi - 1).long()
    y1, x1 = (y0 + 1).clamp(max=Hi - 1), (x0 + 1).clamp(max=Wi - 1)
    ly, lx = (sy - y0).view(-1, 1), (sx - x0).view(1, -1)
    tap = lambda a, yy, xx: a[:, :, yy][:, :, :, xx]
    blend = lambda a: (1 - ly) * ((1 - lx) * tap(a, y0, x0) + lx * tap(a, y0, x1)) + \
        ly * ((1 - lx) * tap(a, y1, x0) + lx * tap(a, y1, x1))
    v, Mv = blend(x64), blend(x64.abs())
    gy = F.pad((x64[:, :, 1:] - x64[:, :, :-1]).abs(), (0, 0, 0, 1))
    gx = F.pad((x64[:, :, :, 1:] - x64[:, :, :, :-1]).abs(), (0, 1, 0, 0))
    gy, gx = F.max_pool2d(gy, 3, 1, 1), F.max_pool2d(gx, 3, 1, 1)
    near = lambda a: torch.maximum(torch.maximum(tap(a, y0, x0), tap(a, y0, x1)), torch.maximum(tap(a, y1, x0), tap(a, y1, x1)))
    Mv = Mv + (sy.view(-1, 1) + 1) * near(gy) + (sx.view(1, -1) + 1) * near(gx)
    base, Mb = torch.zeros_like(v), torch.zeros_like(v)
    if form in ("accumulate", "extra_accumulate"):
        base, Mb = base + out0.to(F64), Mb + out0.to(F64).abs()
    if form in ("extra", "extra_accumulate"):
        base, Mb = base + extra.to(F64), Mb + extra.to(F64).abs() + base.abs()
    val = v + base
    M = Mv + Mb + (val.abs() if form != "overwrite" else 0.0)
    return (F.relu(val) if form == "relu" else val), M


def resize_oracle32(x, size, ac, form, out0, extra):
    """F.interpolate as oracle/hrnet.py calls it, and the kernel's order of the two fp32 additions."""
    v = F.interpolate(x, size=size, mode="bilinear", align_corners=bool(ac))
    if form == "accumulate":
        v = v + out0
    elif form == "extra":
        v = v + extra
    elif form == "extra_accumulate":
        v = v + (out0 + extra)
    return F.relu(v) if form == "relu" else v


def add_relu(a, b=None, relu=True):
    """relu?(a + b) in fp64 -> (value, M = |a| + |b|; 0 without b: a copy through the ReLU is exact)."""
    a64 = a.to(F64)
    if b is None:
        return (F.relu(a64) if relu else a64), torch.zeros_like(a64)
    v = a64 + b.to(F64)
    return (F.relu(v) if relu else v), a64.abs() + b.to(F64).abs()


def split_input(B, h, w, tag=41):
    """The context network's output [B,512,h,w]: N(0, 2) with +-100 planted in the first pixels of the tanh half."""
    x = torch.randn(B, 512, h, w, generator=_gen(tag, B, h, w)) * 2.0
    x[:, 1:128:16, 0, 0] = 100.0
    x[:, 2:128:16, h - 1, w - 1] = -100.0
    return x.contiguous()


def context_split(x):
    """net = tanh(x[:, :128]) (M = |net|: the argument is exact, the error is tanhf's own), inp = relu(x[:, 128:]) (M = 0)
    -> ((net, M), (inp, M))."""
    x64 = x.to(F64)
    net, inp = torch.tanh(x64[:, :128]), F.relu(x64[:, 128:])
    return (net, net.abs()), (inp, torch.zeros_like(inp))


def special_words(n, tag=51):
    """n fp32 words that an arithmetic "copy" would change: -0.0, NaNs with payloads, +-inf, denormals, among N(0, 1)."""
    v = torch.randn(n, generator=_gen(tag, n))
    bits = torch.tensor([-2 ** 31, 0x7FC00001, 0x7F800123, -0x3FFFFF, 0x7F800000, -0x800000, 1, 0x7FFFFF, -2 ** 31 + 5],
                        dtype=torch.int32)
    k = min(n, bits.numel())
    v.view(torch.int32)[torch.arange(k) * max(1, n // k)] = bits[:k]
    return v


# ------------------------------------------------------------------------------------------------ nearest warp
def flows(kind, B, H, W, h, w, g, std=2.5):
    """[B,2,H,W] flows of one of FLOW_KINDS: "float" -- N(0, std) nudged so that every fp32 sample coordinate x + fx of
    the crop stays at least 2^-10 away from a half-integer; "q64" -- quantised to 1/64 px (KITTI's format); "half" --
    every coordinate an exact half-integer."""
    f = torch.randn(B, 2, H, W, generator=g) * std
    if kind == "q64":
        return (f * 64).round() / 64
    if kind == "half":
        return f.round() + 0.5
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([xx, yy])[None]
    for _ in range(8):
        c = base + f
        near = ((c - c.floor()) - 0.5).abs() < 2.0 ** -10 * 1.5
        if not near.any():
            break
        f = torch.where(near, f + 2.0 ** -6, f)
    return f.contiguous()


def warp_source(flow, h, w, scale_variant=False):
    """The kernels' rule: flow [B,2,h,w] (the crop) -> (sy, sx long [B,h,w], clamped into the map; inside [B,h,w] bool):
    rint(float32(x) + fx), half to even on the fp32 sum, inside decided on the rounded value."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    f = flow.float() * (0.25 if scale_variant else 1.0)
    sx, sy = torch.round(xx[None] + f[:, 0]), torch.round(yy[None] + f[:, 1])
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    return sy.clamp(0, h - 1).long(), sx.clamp(0, w - 1).long(), inside


def gather_hw(img, sy, sx):
    """img [B,C,h,w] at (sy, sx) [B,h,w] -> [B,C,h,w]."""
    B, Cc, h, w = img.shape
    idx = (sy * w + sx).view(B, 1, -1).expand(B, Cc, -1)
    return torch.gather(img.reshape(B, Cc, -1), 2, idx).view(B, Cc, h, w)


def grid_sample_source(flow):
    """Where metrics.flow_warp_nearest (grid_sample's normalise / un-normalise arithmetic) samples: (index map [B,h,w]
    of the source pixel, inside [B,h,w]) -- read off a warped index image."""
    from codd_amd import metrics
    B, _, h, w = flow.shape
    ids = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w).expand(B, 1, h, w)
    out, valid = metrics.flow_warp_nearest(ids, flow)
    return out[:, 0].long(), valid[:, 0]


# ------------------------------------------------------------------------------------------------ metrics
def _spots(h, w, k):
    """k distinct crop pixels (y, x) spread over the crop (wrapping when the crop has fewer than k pixels)."""
    n = h * w
    step = max(1, n // (k + 1))
    return [divmod(((i + 1) * step + (i if n > 2 * k else 0)) % n, w) for i in range(k)]


def metrics_case(case, kind="float", empty_item=None, tag=61):
    """Inputs of the three metric kernels on padded [B,*,H,W] maps with the crop (h, w): dict(pred0, gt0, pred1, gt1 (the
    previous and the current frame), flow, gt2, dchange, occ, Ts, K, plant [B,1,H,W] bool).  Planted in item 0 at exactly
    representable values (flow 0 there unless said): gt == lo, gt == hi, pred - gt == +-thr, flow (126, 168) (|flow| ==
    bf exactly), dchange == -bf, tepe == 3, rel == 1 (pred0 = 0: depth clamps to bf), pred0 < 0 (depth clamps to 0; T =
    identity there, so that the pixel's error stays |dchange| = 1 exactly), a pixel whose 2-D and 3-D scene-flow errors are
    exactly 1, an invalid block.  ``empty_item``: that item's ground
    truth is all invalid.  Away from the plants ``clear_thresholds`` has moved every thresholded quantity off its
    threshold by more than its bound (by invalidating gt0 / gt1 there)."""
    B, H, W, h, w = case
    g = _gen(tag + FLOW_KINDS.index(kind), *case)
    r = lambda c: torch.randn(B, c, H, W, generator=g)
    gt0, gt1 = (r(1) * 40 + 60).clamp(0, 250), (r(1) * 40 + 60).clamp(0, 250)
    pred0, pred1 = gt0 + r(1) * 3, gt1 + r(1) * 3
    gt2 = (gt0 + r(1) * 2).clamp(min=0.0)
    gt2[torch.rand(B, 1, H, W, generator=g) < 0.1] = 0.0
    fl = flows(kind, B, H, W, h, w, g)
    dch = r(1) * 2
    occ = (torch.rand(B, 1, H, W, generator=g) < 0.1).to(torch.uint8) * torch.randint(1, 256, (B, 1, H, W), generator=g).to(torch.uint8)
    Ts = se3_field(B, H, W, 0.3, g)[0]
    K = (0.9 * w, 0.9 * w, w / 2.0 - 0.25, h / 2.0 + 0.375)
    plant = torch.zeros(B, 1, H, W, dtype=torch.bool)
    if H > 12 and W > 32:
        gt0[0, 0, 5:9, 7:30] = 0.0
        gt1[0, 0, 5:9, 7:30] = 0.0
    P = dict(zip(("lo", "hi", "thr+", "thr-", "bf", "dc", "te3", "rel1", "neg", "sf1"), _spots(h, w, 10)))
    for y, x in P.values():
        fl[0, :, y, x] = 0.0
        plant[0, 0, y, x] = True
        occ[0, 0, y, x] = 0
        gt2[0, 0, y, x] = gt0[0, 0, y, x].round() + 1.0

    def put(name, **kv):
        y, x = P[name]
        for k, v in kv.items():
            dict(gt0=gt0, gt1=gt1, pred0=pred0, pred1=pred1, dch=dch, gt2=gt2)[k][0, 0, y, x] = v

    put("lo", gt0=LO, gt1=LO)
    put("hi", gt0=HI, gt1=HI)
    put("thr+", gt0=64.0, gt1=64.0, pred0=67.0, pred1=67.0)
    put("thr-", gt0=64.0, gt1=64.0, pred0=61.0, pred1=61.0)
    put("bf", gt0=64.0, gt1=64.0)
    fl[0, :, P["bf"][0], P["bf"][1]] = torch.tensor([126.0, 168.0])
    put("dc", gt0=64.0, gt1=64.0, dch=-BF)
    put("te3", gt0=60.0, gt1=62.0, pred0=65.0, pred1=70.0, gt2=62.0)
    put("rel1", gt0=50.0, gt1=50.0, pred0=0.0, pred1=REL_EPS, gt2=50.0)
    put("neg", gt0=64.0, gt1=66.0, pred0=-2.0, dch=1.0)  # est = 0 exactly: the 3-D error is |dchange| = 1, not < 1
    put("sf1", gt0=64.0, dch=0.0)  # est = 0 and flow (1, 0): both errors are exactly 1; an ordinary pixel for tepe
    fl[0, :, P["sf1"][0], P["sf1"][1]] = torch.tensor([1.0, 0.0])
    for k in ("neg", "sf1"):
        Ts[0, P[k][0], P[k][1]] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    if h * w > 10:
        plant[0, 0, P["sf1"][0], P["sf1"][1]] = False
    if empty_item is not None:
        gt0[empty_item], gt1[empty_item], plant[empty_item] = 0.0, 0.0, False
    d = dict(pred0=pred0, gt0=gt0, pred1=pred1, gt1=gt1, flow=fl.contiguous(), gt2=gt2, dchange=dch, occ=occ, Ts=Ts, K=K,
             plant=plant, case=case, kind=kind)
    clear_thresholds(d)
    return d


def dummy_mask(d):
    from codd_amd import metrics
    return metrics.temporal_mask_source(torch.zeros_like(d["gt1"]))


def _crop(t, h, w):
    return t[..., :h, :w]


def disp_elems(d, frame=1, dt=F64):
    """Per-pixel quantities of codd_disp_metrics on the crop: (mask, err, M_err = |err|: one fp32 subtraction).  dt =
    torch.float32: the same arithmetic in fp32 (what SequenceMetrics.update forms per pixel)."""
    B, H, W, h, w = d["case"]
    p, g = _crop(d["pred%d" % frame], h, w).to(dt), _crop(d["gt%d" % frame], h, w).to(dt)
    err = (p - g).abs()
    return (g > LO) & (g < HI), err, err


def tepe_elems(d, use_mask=False, use_gt2=False, variant=None, dt=F64):
    """Per-pixel quantities of codd_tepe_metrics on the crop -> dict(mask, te, Mte, rel, Mrel, mag).  use_mask: the
    current frame's validity comes from the KITTI dummy (and its ground truth is all zero); use_gt2: gt2 replaces the
    warped ground truth and must be > 0.  M: te = |(pw - pp) - (gw - gp)| -> |pw - pp| + |gw - gp| + te; rel = te / (|dgt|
    + 1e-3f) -> M_te / den + 3 rel (the difference, the sum and the quotient).  variant "mask_unwarped": the warped mask
    taken at the un-warped position.  dt = torch.float32: the same arithmetic in fp32 (SequenceMetrics.update's, per
    pixel, under the exact warp rule)."""
    B, H, W, h, w = d["case"]
    c = lambda k: _crop(d[k], h, w)
    gt1 = torch.zeros_like(c("gt1")) if use_mask else c("gt1")
    gm = _crop(dummy_mask(d), h, w) if use_mask else gt1
    fl = c("flow")
    mag = fl.to(dt).pow(2).sum(1, keepdim=True).sqrt()
    sy, sx, inside = warp_source(fl, h, w)
    valid1 = (gm > LO) & (gm < HI) & (mag < BF)
    mw = valid1 if variant == "mask_unwarped" else gather_hw(valid1.to(torch.uint8), sy, sx).bool()
    gw, pw = gather_hw(gt1, sy, sx).to(dt), gather_hw(c("pred1"), sy, sx).to(dt)
    mc = valid1
    if use_gt2:
        gw = c("gt2").to(dt)
        mc = mc & (gw > 0)
    gp, pp = c("gt0").to(dt), c("pred0").to(dt)
    mask = (gp > LO) & (gp < HI) & mw & mc & inside[:, None]
    dgt = gw - gp
    te = ((pw - pp) - dgt).abs()
    Mte = (pw - pp).abs() + dgt.abs() + te
    den = dgt.abs() + REL_EPS
    rel = te / den
    return dict(mask=mask, te=te, Mte=Mte, rel=rel, Mrel=Mte / den + 3 * rel, mag=mag)


def sceneflow_elems(d, use_occ=True):
    """Per-pixel quantities of codd_sceneflow_metrics on the crop -> dict(mask, e3, M3, e2, M2): est = induced_flow(Ts,
    clip(bf / pred0, 0, bf)) (motion_fp64.induced_flow and its magnitudes), est.z * bf; e = |est - gt|_2 with M = sum_k
    |e_k| M_k / e + e (the root's first-order sensitivity)."""
    B, H, W, h, w = d["case"]
    c = lambda k: _crop(d[k], h, w)
    gp, fl, dc = c("gt0").to(F64), c("flow").to(F64), c("dchange").to(F64)
    mask = (gp > LO) & (gp < HI) & (fl.pow(2).sum(1, keepdim=True).sqrt() < BF) & (dc.abs() < BF)
    if use_occ:
        mask = mask & (c("occ") == 0)
    depth = torch.clip(BF / c("pred0").to(F64)[:, 0], min=0.0, max=BF)
    flow3, Mf, _ = induced_flow(d["Ts"][:, :h, :w], depth, d["K"])
    gt3 = torch.cat([fl, dc], 1).permute(0, 2, 3, 1)
    sc = torch.tensor([1.0, 1.0, BF], dtype=F64)
    e = flow3 * sc - gt3
    Me = Mf * sc + gt3.abs() + e.abs()
    out = dict(mask=mask[:, 0])
    for name, k in (("3", 3), ("2", 2)):
        n = e[..., :k].pow(2).sum(-1).sqrt()
        out["e" + name] = n
        out["M" + name] = (e[..., :k].abs() * Me[..., :k]).sum(-1) / n.clamp(min=1e-300) + n
    return out


def _near(q, thr, M, c):
    """0 < |q - thr| <= 2 c 2^-24 M: the fp32 evaluation may land on the other side (twice the bound, for margin)."""
    gap = (q - thr).abs()
    return (gap > 0) & (gap <= 2 * c * U * M)


CLEAR_C = 64.0  # the clearance is asserted for any c up to this (every C of the metric figures is far below)


def threshold_violations(d):
    """[B,1,h,w] bool per kernel: non-planted crop pixels whose thresholded quantity is within its own bound of the
    threshold -> (disp, prev): ``disp`` concerns gt1 (codd_disp_metrics on the current frame), ``prev`` gt0 (tepe in all
    four variants and scene flow, whose masks both require gt0 valid)."""
    B, H, W, h, w = d["case"]
    free = ~_crop(d["plant"], h, w)
    m, err, Merr = disp_elems(d)
    bad1 = m & _near(err, THR, Merr, CLEAR_C) & free
    m0, err0, Merr0 = disp_elems(d, 0)
    bad0 = m0 & _near(err0, THR, Merr0, CLEAR_C) & free
    for um, ug in TEPE_VARIANTS:
        t = tepe_elems(d, um, ug)
        bad0 = bad0 | (t["mask"] & (_near(t["te"], 3.0, t["Mte"], CLEAR_C) | _near(t["rel"], 1.0, t["Mrel"], CLEAR_C)) & free)
    for uo in (False, True):
        s = sceneflow_elems(d, uo)
        bad0 = bad0 | ((s["mask"] & (_near(s["e3"], 1.0, s["M3"], CLEAR_C) | _near(s["e2"], 1.0, s["M2"], CLEAR_C)))[:, None] & free)
    return bad1, bad0


def clear_thresholds(d):
    """Invalidate the ground truth (gt := 0) at the violating pixels.  Removing a pixel from a mask adds none to any
    mask, so one pass suffices; test_metric_inputs_clear_every_threshold asserts the result."""
    B, H, W, h, w = d["case"]
    bad1, bad0 = threshold_violations(d)
    _crop(d["gt1"], h, w)[bad1] = 0.0
    _crop(d["gt0"], h, w)[bad0] = 0.0
    d["cleared"] = int(bad1.sum()) + int(bad0.sum())


def _means(mask, cols, variant=None):
    """Per item: the mean of each (value, M) column over the mask -> (rows [B,k], Ms [B,k], count [B]); an empty item
    gives zeros.  variant "crop_mean": divided by the crop's pixel count instead of the mask's."""
    B = mask.shape[0]
    m = mask.reshape(B, -1).to(F64)
    cnt = m.sum(1)
    den = torch.full_like(cnt, m.shape[1]) if variant == "crop_mean" else cnt.clamp(min=1)
    rows = [torch.where(mask.reshape(B, -1), v.reshape(B, -1), torch.zeros((), dtype=F64)).sum(1) / den for v, _ in cols]
    Ms = [torch.where(mask.reshape(B, -1), M.reshape(B, -1), torch.zeros((), dtype=F64)).sum(1) / den for _, M in cols]
    return torch.stack(rows, 1), torch.stack(Ms, 1), cnt


def _gt(q, thr, variant):
    return ((q >= thr) if variant == "ge" else (q > thr)).to(F64)


def disp_metrics(d, variant=None):
    """codd_disp_metrics of the current frame -> (rows [B,3] = what each item adds to meters (epe, rate, 1), M [B,3])."""
    mask, err, Merr = disp_elems(d)
    z = torch.zeros_like(err)
    rows, Ms, cnt = _means(mask, [(err, Merr), (_gt(err, THR, variant), z)], variant)
    ok = (cnt > 0).to(F64)[:, None]
    return torch.cat([rows, torch.ones_like(ok)], 1) * ok, torch.cat([Ms, torch.zeros_like(ok)], 1) * ok


def tepe_metrics(d, use_mask=False, use_gt2=False, variant=None):
    """codd_tepe_metrics -> (rows [B,7], M [B,7]): mean tepe, (tepe > 3) rate, mean rel, (rel > 1) rate, 1 (non-empty
    items only), mean |flow| over the crop, 1."""
    t = tepe_elems(d, use_mask, use_gt2, variant)
    z = torch.zeros_like(t["te"])
    rows, Ms, cnt = _means(t["mask"], [(t["te"], t["Mte"]), (_gt(t["te"], 3.0, variant), z), (t["rel"], t["Mrel"]),
                                       (_gt(t["rel"], 1.0, variant), z)], variant)
    ok = (cnt > 0).to(F64)[:, None]
    B = cnt.shape[0]
    mag = t["mag"].reshape(B, -1).mean(1, keepdim=True)
    one = torch.ones(B, 1, dtype=F64)
    return torch.cat([rows * ok, ok, mag, one], 1), torch.cat([Ms * ok, 0 * ok, mag, 0 * one], 1)


def sceneflow_metrics(d, use_occ=True, variant=None):
    """codd_sceneflow_metrics -> (rows [B,5] = count, sum e3, sum e2, #(e3 < 1), #(e2 < 1), M [B,5]).  variant "ge":
    <= in place of <."""
    s = sceneflow_elems(d, use_occ)
    B = s["mask"].shape[0]
    m = s["mask"].reshape(B, -1)
    su = lambda v: torch.where(m, v.reshape(B, -1), torch.zeros((), dtype=F64)).sum(1)
    lt = (lambda q: (q <= 1.0).to(F64)) if variant == "ge" else (lambda q: (q < 1.0).to(F64))
    rows = torch.stack([m.to(F64).sum(1), su(s["e3"]), su(s["e2"]), su(lt(s["e3"])), su(lt(s["e2"]))], 1)
    z = torch.zeros(B, dtype=F64)
    return rows, torch.stack([z, su(s["M3"]), su(s["M2"]), z, z], 1)


def element_figures(d, n_sf=48):
    """The per-pixel figures behind the meters: worst |fp32 - ref64| / (2^-24 M) of the restatement's arithmetic per
    masked pixel -> {"disp_epe", "tepe", "tepe_rel", "flow_mag", "sf_epe3", "sf_epe2"}.  A mean over N pixels averages
    the roundings out (its own figure is ~1 / sqrt(N) of these), but its bound has to hold for any N -- a 1 x 1 crop
    included -- so each c of a mean is set from its elements: |mean error| <= mean(c 2^-24 M_i).  Scene flow: n_sf
    single-pixel masks through metrics.scene_flow_sums (every other ground-truth pixel invalidated)."""
    from codd_amd import metrics
    B, H, W, h, w = d["case"]
    res = {}
    m, e64, M = disp_elems(d)
    res["disp_epe"] = fig("err", disp_elems(d, dt=torch.float32)[1], e64, M, m)
    for um, ug in TEPE_VARIANTS:
        t, t32 = tepe_elems(d, um, ug), tepe_elems(d, um, ug, dt=torch.float32)
        assert torch.equal(t["mask"], t32["mask"])
        for key, v, Mk, keep in (("tepe", "te", "Mte", t["mask"]), ("tepe_rel", "rel", "Mrel", t["mask"]), ("flow_mag", "mag", "mag", None)):
            res[key] = max(res.get(key, 0.0), fig(key, t32[v], t[v], t[Mk], keep))
    s = sceneflow_elems(d, False)
    at = torch.nonzero(s["mask"][0].reshape(-1))[:, 0]
    at = at[torch.randperm(at.numel(), generator=_gen(63, *d["case"]))[:n_sf]]
    meta = dict(disp_range=(LO, HI), intrinsics=d["K"])
    c = lambda k: _crop(d[k][:1], h, w).contiguous()
    for i in at.tolist():
        g0 = torch.zeros_like(c("gt0"))
        g0.view(-1)[i] = c("gt0").view(-1)[i]
        got = metrics.scene_flow_sums(d["Ts"][:1, :h, :w], c("pred0"), g0, c("flow"), c("dchange"), None, meta, d["K"])
        assert got[0] == 1
        for key, col, e, Mk in (("sf_epe3", 1, "e3", "M3"), ("sf_epe2", 2, "e2", "M2")):
            res[key] = max(res.get(key, 0.0), fig(key, got[col], s[e][0].reshape(-1)[i], s[Mk][0].reshape(-1)[i]))
    return res


METRIC_KEYS = {"disp": ("disp_epe", "count", "count"),
               "tepe": ("tepe", "count", "tepe_rel", "count", "count", "flow_mag", "count"),
               "sceneflow": ("count", "sf_epe3", "sf_epe2", "count", "count")}


def meter_figures(kind, got, ref, M, name=""):
    """got / ref / M [..., k] meters of one metric kernel -> {key of C: worst err / (2^-24 M)} and, under "count", 0 or
    inf for the exact columns."""
    res = {}
    for i, key in enumerate(METRIC_KEYS[kind]):
        v = fig(f"{name} {kind}[{i}]", got[..., i], ref[..., i], M[..., i] if key != "count" else 0 * M[..., i])
        res[key] = max(res.get(key, 0.0), v)
    return res


def metrics_oracle32(d, use_mask=False, use_gt2=False, use_occ=True):
    """codd_amd.metrics.SequenceMetrics.update / scene_flow_sums, one item at a time (a batch is B frames) on the cropped
    maps -> (disp [B,3], tepe [B,7], sceneflow [B,5]) in the kernels' meter layout."""
    from codd_amd import metrics
    B, H, W, h, w = d["case"]
    meta = dict(disp_range=(LO, HI), intrinsics=d["K"])
    rd, rt, rs = [], [], []
    for b in range(B):
        c = lambda k: _crop(d[k][b:b + 1], h, w).contiguous()
        gt1 = torch.zeros_like(c("gt1")) if use_mask else c("gt1")
        sm = metrics.SequenceMetrics(meta, torch.device("cpu"))
        sm.update(c("pred0"), c("gt0"), c("flow"), gt_disp2=c("gt2") if use_gt2 else None)
        sm.update(c("pred1"), gt1)
        m = sm.m
        rt.append(torch.stack([m["tepe"].s, m["th3_tepe"].s, m["tepe_rel"].s, m["th1_tepe_rel"].s, m["tepe"].n,
                               m["flow_mag"].s, m["flow_mag"].n]))
        s1 = metrics.SequenceMetrics(meta, torch.device("cpu"))
        s1.update(c("pred1"), c("gt1"))
        rd.append(torch.stack([s1.m["epe"].s, s1.m["th3"].s, s1.m["epe"].n]))
        rs.append(metrics.scene_flow_sums(d["Ts"][b:b + 1, :h, :w], c("pred0"), c("gt0"), c("flow"), c("dchange"),
                                          c("occ") if use_occ else None, meta, d["K"]))
    return torch.stack(rd), torch.stack(rt), torch.stack(rs)


# ------------------------------------------------------------------------------------------------ ablation kernels
def select_inputs(case, K, tag=71):
    """cur, warp [B,1,H,W], gt [B,1,hg,wg] with the planted pixels of item 0's first row: warp == 0, warp == -0.0, warp <
    0, |warp - cur| == 1 exactly (both signs), d == +-1 exactly, gt == 0, a NaN gt.  Away from them every threshold (|w
    - c| vs 1 with the gain K's blend, d vs +-1) is cleared by setting cur = warp where it is not."""
    B, H, W, hg, wg = case
    g = _gen(tag, *case)
    cur = torch.rand(B, 1, H, W, generator=g) * 100 + 1
    warp = cur + torch.randn(B, 1, H, W, generator=g) * 0.8
    warp[torch.rand(B, 1, H, W, generator=g) < 0.1] = 0.0
    gt = cur[:, :, :hg, :wg] + torch.randn(B, 1, hg, wg, generator=g) * 1.5
    gt[torch.rand(B, 1, hg, wg, generator=g) < 0.1] = 0.0
    c64, w64 = cur.to(F64), warp.to(F64)
    gp = F.pad(gt, (0, W - wg, 0, H - hg)).to(F64)
    dd = (c64 - gp).abs() - (w64 - gp).abs()
    Md = 2 * ((c64 - gp).abs() + (w64 - gp).abs())
    near = _near((w64 - c64).abs(), 1.0, (w64 - c64).abs(), CLEAR_C) | _near(dd, 1.0, Md, CLEAR_C) | _near(dd, -1.0, Md, CLEAR_C)
    warp = torch.where(near, cur, warp)
    row = [(8.0, 0.0, 8.0), (8.0, -0.0, 8.0), (8.0, -3.0, 8.0), (8.0, 9.0, 8.5), (9.0, 8.0, 8.5), (10.0, 9.0, 9.0),
           (9.0, 10.0, 9.0), (8.0, 8.5, 0.0), (8.0, 8.5, float("nan"))]  # (cur, warp, gt)
    for i, (c, w_, g_) in enumerate(row):
        cur[0, 0, 0, i], warp[0, 0, 0, i], gt[0, 0, 0, i] = c, w_, g_
    return cur.contiguous(), warp.contiguous(), gt.contiguous()


def fusion_select(mode, cur, warp, gt=None, K=0.5, variant=None):
    """codd_fusion_select in fp64 -> (value, M, blended): the selections are exact (M = 0 where ``cur`` or ``warp`` is
    passed through); the Kalman blend w + K (c - w) has M = |w| + K (|c| + |w|) + |v|, the GT average (c + w) / 2 has
    |c| + |w|.  variant "ge": >= / <= at the thresholds."""
    c, w = cur.to(F64), warp.to(F64)
    gt_ = (lambda a, b: a >= b) if variant == "ge" else (lambda a, b: a > b)
    if mode == "kalman":
        v = w + K * (c - w)
        keep = (w <= 0) | gt_((w - c).abs(), 1.0)
        return torch.where(keep, c, v), torch.where(keep, 0 * v, w.abs() + K * (c.abs() + w.abs()) + v.abs()), ~keep
    H, W = cur.shape[-2:]
    g = F.pad(gt.to(F64), (0, W - gt.shape[-1], 0, H - gt.shape[-2]))
    d = (c - g).abs() - (w - g).abs()
    avg = ~gt_(-d, 1.0) & ~gt_(d, 1.0)
    v = torch.where(gt_(-d, 1.0), c, torch.where(gt_(d, 1.0), w, (c + w) / 2))
    keep = (w <= 0) | ~(g > 0)
    return torch.where(keep, c, v), torch.where(keep | ~avg, 0 * v, c.abs() + w.abs()), avg & ~keep


def gt_motion_inputs(case, kind, tag=81):
    """img [B,3,H,W], feat [B,C,H/4,W/4], disp [B,H,W], flow [B,2,hg,wg] of ``kind``, dchange [B,1,hg,wg], occ bytes
    (0, 1 and 255)."""
    B, Cc, H, W, hg, wg = case
    g = _gen(tag + FLOW_KINDS.index(kind), *case)
    img, feat = torch.randn(B, 3, H, W, generator=g), torch.randn(B, Cc, H // 4, W // 4, generator=g)
    disp = torch.rand(B, H, W, generator=g) * 100 + 1
    fl = flows(kind, B, hg, wg, hg, wg, g, std=1.5)
    dch = torch.randn(B, 1, hg, wg, generator=g) * 2
    u = torch.rand(B, 1, hg, wg, generator=g)
    occ = torch.where(u < 0.1, 1, torch.where(u < 0.2, 255, 0)).to(torch.uint8)
    return img, feat, disp, fl, dch, occ


def gt_motion(img, feat, disp, flow, dch, occ, variant=None):
    """codd_gt_motion under the warp rule above -> [img_warp, feat_warp, conf, disp_warp [B,1,H,W], flow3], all exact
    (disp - dchange is one fp32 operation = the fp64 difference rounded to fp32).  Quarter-resolution features move by
    the FULL-resolution flow at [2::4, 2::4], unscaled (variant "quarter_scale": x 1/4)."""
    B, _, H, W = img.shape
    pad = (0, W - flow.shape[-1], 0, H - flow.shape[-2])
    fl, dc, oc = F.pad(flow, pad), F.pad(dch, pad), F.pad(occ, pad) != 0
    sy, sx, inside = warp_source(fl, H, W)
    ok = (inside & ~oc[:, 0])[:, None]
    both = gather_hw(torch.cat([img, disp[:, None]], 1), sy, sx)
    img_w = torch.where(ok, both[:, :3], torch.zeros(()))
    disp_w = torch.where(ok, (both[:, 3:].to(F64) - dc.to(F64)).float(), torch.zeros(()))
    fq = fl[:, :, 2::4, 2::4]
    qy, qx, qin = warp_source(fq, H // 4, W // 4, scale_variant=variant == "quarter_scale")
    feat_w = torch.where(qin[:, None], gather_hw(feat, qy, qx), torch.zeros(()))
    return [img_w, feat_w, torch.ones_like(img), disp_w, torch.cat([fl, dc], 1)]


def metrics_item(d, b):
    """Item ``b`` of a metrics case as a case of its own at B = 1 (fresh, contiguous tensors)."""
    B, H, W, h, w = d["case"]
    out = {k: (v[b:b + 1].clone() if torch.is_tensor(v) else v) for k, v in d.items()}
    out["case"] = (1, H, W, h, w)
    return out
