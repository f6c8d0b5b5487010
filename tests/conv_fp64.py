"""fp64 reference, record codec, inputs, bounds and the shipped-tune-db case list for the convolution family (conv.hip,
conv_kernel.h, conv_quad_kernel.h, conv_bf16*.h/.hip and the record converter codd_split_bf16), for
tests/test_conv_fp64_reference.py (CPU: the reference pinned against torch's own fp64 convolutions, the codec pinned by
bit patterns, the measurement of ``c``, the operand bounds by emulation, the power of the bounds) and
tests/test_gpu_conv_fp64.py (the HIP kernels on every entry of codd_amd/tuned/mi355x.json).

``conv_ref`` returns the value AND the first-order magnitude ``M`` of the arithmetic that forms it, evaluated by the same
tap loop on |w|, |x|:  M_pre = sum |w||x| + |bias| + |res1| + |res2|;  M = L * M_pre + |act(v)| + |post| with ``L`` the
activation's Lipschitz constant (LIPSCHITZ), + UNDERFLOW where fp32 expf underflows (sigmoid, mish).  The bound of an
output element is

    |got - ref64| <= (e_mode + c * 2^-24) * M

``c`` (C) is the accumulation constant, the family's one measured number: 4 x the worst |fp32 - ref64| / (2^-24 M) of two
plain fp32 CPU evaluations (torch's fp32 convolution; one product at a time, separate multiply and add, in the k order
conv.hip documents: chunk, tap, channel) over the case inputs, rounded up to two digits.  4 x for the reason
motion_fp64 gives: a GPU evaluation differs from an independent fp32 one by FMA contraction, the order of the partial
sums (MFMA k-blocks, k-split pairs) and 1-2 ulp libm functions, none worth more than a small factor.  ``e_mode`` (E_MODE)
is the operand term, derived from the record format: with u the relative residual of one operand's record a product is
off by 2u + u^2: bf16 (u = 2^-9) 2^-8 (1 + 2^-10); fp16 (u = 2^-11) 2^-10 (1 + 2^-12); the split formats keep the
project's own 3.5 * 2^-18 / 2^-20 (motion_fp64.SPLIT_BOUND).  These are the formats' TYPICAL residuals, not their worst
cases (bf16 rounds to 8 significant bits: up to 2^-8 |x| at the bottom of a binade, 2^-9 |x| at its top; hi + lo up to
2^-17 |x|): what makes them bounds of a SUM is asserted, not assumed -- test_emulated_record_formats_stay_inside_e_mode
holds an emulation of every format to e_mode * sum |w||x| on every element of every layer of the sweep.  The fp16 formats
add an absolute floor (f16_floor).

Scope of this module: what ``ops.conv2d`` can express -- one or two concatenated inputs, stride,
asymmetric padding, dilation, out_hw, bias, act(conv + bias + res1 + res2) + post, the seven CODD_ACT_*, the k2 s2
transposed convolution, the same with record tensors as input (xs) or output (xs_out), the dil2 dual tap sets and the
three gate epilogues, and the two-stage rolling launches (modes 0 / 1 / 2 of ops.PackedRoll).  The GPU module runs the whole
db and the rolling launches (DESIGN.md finding 69)."""
import collections
import json
import math
import os

import torch
import torch.nn.functional as F

from motion_fp64 import SPLIT_BOUND

F64 = torch.float64
U = 2.0 ** -24
UNDERFLOW = 2.0 ** -102  # 2^-126 / 2^-24 (as motion_fp64.UNDERFLOW): an fp32 expf that underflows to 0 / a subnormal
DB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "codd_amd", "tuned", "mi355x.json")
ACTS = ("none", "lrelu", "relu", "sigmoid", "tanh", "mish", "relu_ch0")
B = 2

# sup |mish'(v)|: mish'(v) = tanh(sp) + v sigmoid(v) (1 - tanh(sp)^2), sp = log(1 + e^v); its maximum 1.0884 is at
# v = 1.4904 (test_mish_lipschitz_constant re-derives it on a grid in fp64)
MISH_LIPSCHITZ = 1.0885
LIPSCHITZ = dict(none=1.0, lrelu=1.0, relu=1.0, tanh=1.0, relu_ch0=1.0, sigmoid=0.25, mish=MISH_LIPSCHITZ)

# worst |fp32 - ref64| / (2^-24 M) over the inputs of C_CASES (CPU measurement, test_measured_c): (a) torch's fp32
# convolution, (b) one product at a time in the order chunk, tap, channel ...
MEASURED = {"torch_fp32": 9.89, "sequential_fp32": 12.1}
# ... and c = 4 x the worst of the two, rounded up to two digits
C = 49.0
E_MODE = {"fp32": 0.0, "bf16": 2.0 ** -8 * (1 + 2.0 ** -10), "fp16": 2.0 ** -10 * (1 + 2.0 ** -12),
          "split": SPLIT_BOUND["split"][0], "split16": SPLIT_BOUND["split16"][0]}
MODE_OF_TERMS = {0: "fp32", 1: "bf16", 3: "split", 16: "fp16", 48: "split16"}
WIDE_MODES = ("fp32", "split", "bf16")  # channel scales over 1e-3 .. 1e3; the fp16 formats get 0.25 .. 4 (range caveat)


# ------------------------------------------------------------------------------------------------ tune db
Entry = collections.namedtuple(
    "Entry", "sig terms gate cout_eff cin kh kw mb deconv H W B sy sx dy dx pl two split co dil2 cfg")
Layer = collections.namedtuple("Layer", "cout_eff cin kh kw deconv sy sx dy dx pl two")


def parse_sig(sig, cfg=()):
    """One of the three signature forms of the tune db (built by ops._plain_sig / ops._gate_sig; the comment above
    ops._plain_key states them) -> Entry:
        cout_eff,cin,kh,kw,mb,deconv|Hout,Wout,B,sy,sx,dy,dx,pl,two                      (precision fp32)
        b<terms>|cout_eff,cin,kh,kw,mb,deconv|Hout,Wout,B,sy,sx,dy,dx,pl,two[|split][|co]
        g<gate>,b<terms>|cout,cin,kh,kw|H,W,B,pad,dil,dil2"""
    parts = sig.split("|")
    ints = lambda s: [int(v) for v in s.split(",")]
    if parts[0][:1] == "g":
        gate, terms = (int(v[1:]) for v in parts[0].split(","))
        cout, cin, kh, kw = ints(parts[1])
        H, W, Bn, pad, dil, dil2 = ints(parts[2])
        assert len(parts) == 3, sig
        return Entry(sig, terms, gate, cout, cin, kh, kw, None, 0, H, W, Bn, 1, 1, dil, dil, pad, 0, False, False, dil2,
                     tuple(cfg))
    terms = 0
    if parts[0][:1] == "b":
        terms = int(parts[0][1:])
        parts = parts[1:]
    cout_eff, cin, kh, kw, mb, deconv = ints(parts[0])
    H, W, Bn, sy, sx, dy, dx, pl, two = ints(parts[1])
    flags = parts[2:]
    assert set(flags) <= {"split", "co"} and (terms or not flags), sig
    return Entry(sig, terms, 0, cout_eff, cin, kh, kw, mb, deconv, H, W, Bn, sy, sx, dy, dx, pl, two, "split" in flags,
                 "co" in flags, 0, tuple(cfg))


def layer_of(e):
    return Layer(e.cout_eff, e.cin, e.kh, e.kw, e.deconv, e.sy, e.sx, e.dy, e.dx, e.pl, e.two)


def load_db():
    return [parse_sig(k, v) for k, v in json.load(open(DB)).items()]


def triples(entries=None):
    """The db without H, W, B: distinct (terms, gate, layer, dil2, split, co, configuration), in db order -> one
    representative Entry each."""
    seen = {}
    for e in load_db() if entries is None else entries:
        seen.setdefault((e.terms, e.gate, layer_of(e), e.mb, e.dil2, e.split, e.co, e.cfg), e)
    return list(seen.values())


def plain_triples():
    """The triples ops.conv2d launches without record tensors: no gate, no |split."""
    return [e for e in triples() if not e.gate and not e.split]


def tile_of(cfg):
    """(rows, columns) of a workgroup's output tile."""
    if len(cfg) > 4 and cfg[4] == 2:
        return cfg[1], 16 * cfg[0]
    npb, nw = cfg[0], cfg[1]
    xb = 2 if npb >= 2 else 1
    return nw * (npb // xb), 16 * xb


def pad_of(e):
    """(top, left, bottom, right) of the call site: symmetric, except HITNet's 4 x 1-stride tile layer (right pad 3)."""
    if e.kh == 4 and (e.sy, e.sx) == (4, 1):
        return (0, 0, 0, 3)
    return (e.pl, e.pl, e.pl, e.pl)


Geom = collections.namedtuple("Geom", "layer Hin Win Hout Wout pad")


def geometry(e):
    """The smallest map at which this entry's kernel can still go wrong: two tiles in each direction with a ragged
    second one, Hout = th + 3, Wout = tw + 5 (the quad layout needs input rows of a multiple of 4 floats: the nearest
    Wout to tw + 5 that has such an input).  The layer keeps its channels, kernel, stride, dilation and padding."""
    th, tw = tile_of(e.cfg)
    quad = len(e.cfg) > 4 and e.cfg[4] == 1
    pt, pl, pb, pr = pad_of(e)
    Hout = th + 3
    Hin = (Hout - 1) * e.sy + e.dy * (e.kh - 1) + 1 - pt - pb + (e.sy - 1)
    for Wout in (tw + 5, tw + 4, tw + 6, tw + 3, tw + 7, tw + 8, tw + 2, tw + 9):
        lo = (Wout - 1) * e.sx + e.dx * (e.kw - 1) + 1 - pl - pr
        wins = [w for w in range(lo + e.sx - 1, lo - 1, -1) if w > 0 and (not quad or w % 4 == 0)]
        if wins:
            return Geom(layer_of(e), Hin, wins[0], Hout, Wout, (pt, pl, pb, pr))
    raise AssertionError(e.sig)


# ------------------------------------------------------------------------------------------------ reference
def _taps(x, w, stride, pad, dil, out_hw):
    """sum over taps and channels of w * x (fp64), as an explicit loop over taps: a shifted, strided slice of the
    zero-padded input and an einsum over channels per tap.  x [B,C,H,W], w [O,C,kh,kw], pad (t, l, b, r)."""
    Bn, Cn, H, W = x.shape
    O, _, kh, kw = w.shape
    (sy, sx), (dy, dx), (pt, pl, pb, pr) = stride, dil, pad
    Ho, Wo = out_hw
    need_h, need_w = (Ho - 1) * sy + dy * (kh - 1) + 1, (Wo - 1) * sx + dx * (kw - 1) + 1
    xp = torch.zeros(Bn, Cn, max(need_h, pt + H), max(need_w, pl + W), dtype=F64)
    xp[:, :, pt:pt + H, pl:pl + W] = x
    out = torch.zeros(Bn, O, Ho, Wo, dtype=F64)
    for ky in range(kh):
        for kx in range(kw):
            sl = xp[:, :, ky * dy:ky * dy + (Ho - 1) * sy + 1:sy, kx * dx:kx * dx + (Wo - 1) * sx + 1:sx]
            out += torch.einsum("oc,bchw->bohw", w[:, :, ky, kx], sl)
    return out


def _deconv_taps(x, w):
    """k2 s2 transposed convolution (store_mode 1): out[b, co, 2y + a, 2x + b'] = sum_ci x[b, ci, y, x] w[ci, co, a, b']
    -- quadrant (a, b') is channel block (a*2 + b') of the 1x1 convolution the kernel runs."""
    Bn, _, H, W = x.shape
    out = torch.zeros(Bn, w.shape[1], 2 * H, 2 * W, dtype=F64)
    for a in range(2):
        for b in range(2):
            out[:, :, a::2, b::2] = torch.einsum("co,bchw->bohw", w[:, :, a, b], x)
    return out


def mish64(v):
    return v * torch.tanh(F.softplus(v, threshold=700.0))


def act_ref(v, act):
    """(act(v), Lipschitz constant, underflow floor) in fp64; relu_ch0: ReLU on output channel 0 only."""
    if act == "none":
        a = v
    elif act == "lrelu":
        a = torch.where(v > 0, v, 0.2 * v)
    elif act == "relu":
        a = torch.relu(v)
    elif act == "sigmoid":
        a = torch.sigmoid(v)
    elif act == "tanh":
        a = torch.tanh(v)
    elif act == "mish":
        a = mish64(v)
    elif act == "relu_ch0":
        a = v.clone()
        a[:, :1] = torch.relu(v[:, :1])
    else:
        raise ValueError(act)
    return a, LIPSCHITZ[act], (UNDERFLOW if act in ("sigmoid", "mish") else 0.0)


def conv_lin(x, w, stride=(1, 1), pad=(0, 0, 0, 0), dil=(1, 1), out_hw=None, deconv=False):
    """(sum w x, sum |w||x|) in fp64 of the concatenated input x."""
    x, w = x.to(F64), w.to(F64)
    if deconv:
        return _deconv_taps(x, w), _deconv_taps(x.abs(), w.abs())
    if out_hw is None:
        kh, kw = w.shape[2:]
        out_hw = ((x.shape[2] + pad[0] + pad[2] - dil[0] * (kh - 1) - 1) // stride[0] + 1,
                  (x.shape[3] + pad[1] + pad[3] - dil[1] * (kw - 1) - 1) // stride[1] + 1)
    return _taps(x, w, stride, pad, dil, out_hw), _taps(x.abs(), w.abs(), stride, pad, dil, out_hw)


def epilogue(lin, Mlin, bias=None, act="none", res1=None, res2=None, post=None):
    """act(lin + bias + res1 + res2) + post and its magnitude (module docstring) -> (value, M, pre-activation)."""
    v, M = lin.clone(), Mlin.clone()
    if bias is not None:
        v += bias.to(F64).view(1, -1, 1, 1)
        M += bias.to(F64).abs().view(1, -1, 1, 1)
    for r in (res1, res2):
        if r is not None:
            v += r.to(F64)
            M += r.to(F64).abs()
    a, L, floor = act_ref(v, act)
    M = L * M + a.abs() + floor
    if post is not None:
        a = a + post.to(F64)
        M = M + post.to(F64).abs()
    return a, M, v


def conv_ref(x, w, bias=None, x2=None, stride=(1, 1), pad=(0, 0, 0, 0), dil=(1, 1), out_hw=None, act="none", res1=None,
             res2=None, post=None, deconv=False):
    """act(conv(cat[x, x2]) + bias + res1 + res2) + post in fp64 -> (value, M)."""
    xin = x if x2 is None else torch.cat([x, x2], 1)
    lin, Mlin = conv_lin(xin, w, stride, pad, dil, out_hw, deconv)
    return epilogue(lin, Mlin, bias, act, res1, res2, post)[:2]


F16_QUANTUM = 2.0 ** -25  # half the spacing of the fp16 subnormals (2^-24)


def f16_floor(x, w, stride=(1, 1), pad=(0, 0, 0, 0), dil=(1, 1), out_hw=None, deconv=False):
    """The term the fp16 record formats add to a bound, a property of the format that e_mode * M misses: a record
    element below 2^-14 in magnitude -- above all the lo part of ANY operand smaller than 2^-3, weights of a K = 1152
    layer included -- is an fp16 subnormal, rounded to a multiple of 2^-24 whatever its size, so every operand carries
    an ABSOLUTE residual of up to 2^-25 beside the relative one: a product w x is off by up to 2^-25 (|w| + |x|), the
    sum by  2^-25 * sum over the in-bounds taps of (|w| + |x|).  (This is the range caveat of
    ops.set_conv_precision; without it the emulation of split16 exceeds 2^-20 M by 1.46 x on the 256 x 128 x 3 x 3
    layer at O(1) inputs.)  -> that sum, to be passed to ``bound`` / ``ratio`` as ``floor``."""
    kw = dict(stride=stride, pad=pad, dil=dil, out_hw=out_hw, deconv=deconv)
    x, w = x.to(F64).abs(), w.to(F64).abs()
    return F16_QUANTUM * (conv_lin(x, torch.ones_like(w), **kw)[0] + conv_lin(torch.ones_like(x), w, **kw)[0])


def bound(M, mode, floor=None):
    """(e_mode + c 2^-24) M; + ``floor`` (f16_floor) for the fp16 record formats."""
    lim = (E_MODE[mode] + C * U) * M
    assert floor is not None or mode not in ("fp16", "split16")  # (a bound of these formats without it is not one)
    return lim if floor is None else lim + floor


def ratio(got, ref, M, mode, floor=None):
    """err / bound per element; 0 where the error is 0; NaN (a non-finite ``got``) counts as inf."""
    err = (got.to(F64) - ref).abs()
    lim = bound(M, mode, floor)
    r = torch.where(lim > 0, err / lim.clamp(min=1e-300), torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), r)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)


# ------------------------------------------------------------------------------------------------ record codec
def rec_dtype(terms):
    return torch.float16 if terms in (16, 48) else torch.bfloat16


def encode(x, terms):
    """fp32 -> (hi, lo) in the record's 16-bit format: hi = RNE(x), lo = RNE(x - hi) (fp32 subtraction, as the
    kernels); lo is None for the one-plane formats (terms 1 | 16)."""
    dt = rec_dtype(terms)
    x = x.float()
    hi = x.to(dt)
    lo = (x - hi.float()).to(dt) if terms in (3, 48) else None
    return hi, lo


def decode(hi, lo=None):
    return hi.to(F64) if lo is None else hi.to(F64) + lo.to(F64)


def records(x, x2, bt, bl, c8, hp, wp, terms):
    """The whole codd_split_bf16 buffer of cat[x, x2] as int16 [B][plane][octet][hp][wp][8]: image pixel (y, x) at
    (y + bt, x + bl), zero borders, zero channel padding."""
    xin = x if x2 is None else torch.cat([x, x2], 1)
    Bn, Cn, H, W = xin.shape
    planes = 2 if terms in (3, 48) else 1
    full = torch.zeros(Bn, 8 * c8, hp, wp)
    full[:, :Cn, bt:bt + H, bl:bl + W] = xin
    out = torch.zeros(Bn, planes, c8, hp, wp, 8, dtype=torch.int16)
    for p, plane in enumerate(encode(full, terms)[:planes]):
        out[:, p] = plane.view(torch.int16).view(Bn, c8, 8, hp, wp).permute(0, 1, 3, 4, 2)
    return out


def conv_lin_emulated(x, w, terms, stride=(1, 1), pad=(0, 0, 0, 0), dil=(1, 1), out_hw=None, deconv=False,
                      drop=()):
    """The products an MFMA kernel of this operand format forms, summed in fp64: both operands through ``encode``;
    hi*hi for the one-plane formats, hi*hi + hi*lo + lo*hi (w * x order) for the split ones.  ``drop``: product terms
    left out ("hilo" = w.hi * x.lo, "lohi" = w.lo * x.hi) -- the wrong variants of the power tests."""
    (xh, xl), (wh, wl) = encode(x, terms), encode(w, terms)
    kw = dict(stride=stride, pad=pad, dil=dil, out_hw=out_hw, deconv=deconv)
    s = conv_lin(xh, wh, **kw)[0]
    if xl is not None:
        if "hilo" not in drop:
            s = s + conv_lin(xl, wh, **kw)[0]
        if "lohi" not in drop:
            s = s + conv_lin(xh, wl, **kw)[0]
    return s


# ------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    return torch.Generator().manual_seed(104729 + sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _log_uniform(g, n, lo, hi):
    return torch.exp(torch.rand(n, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))


PLANTED = (25.0, -25.0, 95.0, -95.0)  # pre-activations beyond +-20 and +-90 (output channels 1 .. 4 where they exist)


def features(g, Bn, Cn, H, W, lo, hi, disparities):
    """[Bn,Cn,H,W] fp32 as the layers see them: N(0, 1) through a leaky ReLU / ReLU / tanh (by channel), a scale per
    channel log-uniform over lo .. hi; with ``disparities`` the first one or two channels are raw disparities 0 .. 320
    (smooth ramp + noise).  The batch items differ."""
    x = torch.randn(Bn, Cn, H, W, generator=g)
    kind = torch.arange(Cn) % 3
    x = torch.where((kind == 0).view(1, -1, 1, 1), F.leaky_relu(x, 0.2),
                    torch.where((kind == 1).view(1, -1, 1, 1), torch.relu(x), torch.tanh(x)))
    x = x * _log_uniform(g, Cn, lo, hi).view(1, -1, 1, 1)
    if disparities:
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        for c in range(min(2, Cn - 1) or 1):
            ramp = 320.0 * (0.15 + 0.7 * (0.6 * xx + 0.4 * yy if c == 0 else 1 - xx))
            x[:, c] = (ramp[None] * (1.0 - 0.3 * torch.arange(Bn).view(-1, 1, 1)) + torch.randn(Bn, H, W, generator=g)).clamp(0, 320)
    return x.contiguous()


Case = collections.namedtuple("Case", "geom wide act x x2 coff w bias res1 res2 post C0 C1")


def make_case(geom, wide, act="none", operands=()):
    """Seeded inputs of one (layer, map): B = 2, the input with per-channel scales over 1e-3 .. 1e3 (``wide``) or
    0.25 .. 4, weights N(0, 1) / sqrt(K) with a scale per output channel over the same range and 1 / sqrt of the input
    channel's scale per input channel (so that quiet channels still carry a visible share of every sum), biases at the
    output's scale -- planted at PLANTED / (typical |conv|) for the saturating activations --, res1 / res2 / post
    (``operands``) at the output's scale.  Two-input layers split cin as a call site does: x is a Slice at channel
    offset ``coff`` of a wider buffer (built by the GPU test), x2 a second tensor."""
    L = geom.layer
    lo, hi = (1e-3, 1e3) if wide else (0.25, 4.0)
    g = _gen(*L, geom.Hin, geom.Win, geom.Hout, geom.Wout, int(wide))
    disp = wide and (L.cin % 8 != 0 or L.cin <= 32)  # (raw disparities: not the fp16 formats' supported use)
    x = features(g, B, L.cin, geom.Hin, geom.Win, lo, hi, disp)
    si = x.abs().amax((0, 2, 3)).clamp(min=1e-6)
    if L.deconv:
        cout = L.cout_eff // 4
        K = L.cin
        w = torch.randn(L.cin, cout, 2, 2, generator=g)
        so = _log_uniform(g, cout, lo, hi)
        w = w * so.view(1, -1, 1, 1) / (si.sqrt().view(-1, 1, 1, 1) * math.sqrt(K))
    else:
        cout = L.cout_eff
        K = L.cin * L.kh * L.kw
        w = torch.randn(cout, L.cin, L.kh, L.kw, generator=g)
        so = _log_uniform(g, cout, lo, hi)
        if act in ("sigmoid", "tanh", "mish"):
            so[1:1 + len(PLANTED)] = 0.05  # planted channels: the bias sets the pre-activation
        w = w * so.view(-1, 1, 1, 1) / (si.sqrt().view(1, -1, 1, 1) * math.sqrt(K))
    bias = torch.randn(cout, generator=g) * so
    if act in ("sigmoid", "tanh", "mish"):
        n = min(len(PLANTED), cout - 1)
        bias[1:1 + n] = torch.tensor(PLANTED[:n])
    up = 2 if L.deconv else 1
    oshape = (B, cout, geom.Hout * up, geom.Wout * up)
    ops_ = {k: (torch.randn(*oshape, generator=g) * so.view(1, -1, 1, 1)).contiguous() if k in operands else None
            for k in ("res1", "res2", "post")}
    C1 = 0
    if L.two:  # the second tensor: one channel (a disparity / cost map) of an odd cin, else about a third
        C1 = 1 if L.cin % 2 else max(1, L.cin // 3)
    C0 = L.cin - C1
    return Case(geom, wide, act, x[:, :C0].contiguous(), x[:, C0:].contiguous() if C1 else None, 6 if L.two else 0,
                w.contiguous(), bias.contiguous(), ops_["res1"], ops_["res2"], ops_["post"], C0, C1)


def case_f16_floor(case):
    L, gm = case.geom.layer, case.geom
    x = case.x if case.x2 is None else torch.cat([case.x, case.x2], 1)
    floor = f16_floor(x, case.w, (L.sy, L.sx), gm.pad, (L.dy, L.dx), (gm.Hout, gm.Wout), bool(L.deconv))
    return LIPSCHITZ[case.act] * floor


def case_ref(case):
    L, gm = case.geom.layer, case.geom
    return conv_ref(case.x, case.w, case.bias, case.x2, (L.sy, L.sx), gm.pad, (L.dy, L.dx), (gm.Hout, gm.Wout), case.act,
                    case.res1, case.res2, case.post, bool(L.deconv))


def case_plan(e, index):
    """(activation, operands) a db triple runs with: the seven activations and the res1 / res2 / post combinations
    cycle over the layers in db order (the signature does not store them); the transposed convolution takes none."""
    act = ACTS[index % len(ACTS)]
    if e.deconv:
        return act if act != "relu_ch0" else "relu", ()
    return act, (("res1",), ("res1", "res2", "post"), (), ("post",), ("res1", "res2"))[index % 5]


# relative residual of a whole record (both planes where there are two): the worst case of the format (p = 8 / 11
# significant bits per plane), for outputs written as records (xs_out); the fp16 formats add F16_QUANTUM
REC_U = {1: 2.0 ** -8, 3: 2.0 ** -17, 16: 2.0 ** -11, 48: 2.0 ** -22}


def record_floor(ref, terms):
    """What storing ``ref`` as a record of this format may add to the error of an output element."""
    return REC_U[terms] * ref.abs() + (F16_QUANTUM if terms in (16, 48) else 0.0)


def split_triples():
    """The |split triples: convolutions pinned to the layout-2 kernel because their input only exists as records
    (xs) or their output is written as records (xs_out)."""
    return [e for e in triples() if not e.gate and e.split]


def sweep(entries=None):
    """The db sweep: {Layer: [(Entry, Geom, activation, operands)]} of every plain triple (plain_triples; or of
    ``entries``), grouped by layer so that one test runs at most about twenty launches and the references are shared."""
    order, out = {}, collections.OrderedDict()
    for e in plain_triples() if entries is None else entries:
        L = layer_of(e)
        i = order.setdefault(L, len(order))
        out.setdefault(L, []).append((e, geometry(e)) + case_plan(e, i))
    return out


def layer_id(L):
    return "%dx%dx%dx%d%s_s%d%d_d%d%d_p%d%s" % (L.cout_eff, L.cin, L.kh, L.kw, "T" if L.deconv else "", L.sy, L.sx, L.dy,
                                                 L.dx, L.pl, "_two" if L.two else "")


# the layers on which ``c`` is measured: the shipped layers of the largest K per kernel size, a 128 -> 128 3x3 layer, a dilated, a strided, a 7x7, a two-input 1x1 and the transposed convolution
def c_cases():
    by_layer = sweep()
    pick = []
    for want in [lambda L: (L.cin, L.kh, L.dy) == (128, 3, 1) and L.cout_eff == 128, lambda L: L.kh == 7 and L.cin >= 30,
                 lambda L: L.dy == 4, lambda L: L.sy == 2 and L.kh == 3 and L.cin >= 64, lambda L: L.kh == 1 and L.two,
                 lambda L: L.deconv, lambda L: L.kh == 4 and L.sy == 4 and L.sx == 1]:
        pick.append(next(L for L in by_layer if want(L)))
    pick.append(max((L for L in by_layer if L.kh == 3), key=lambda L: (L.cin * 9, -L.cout_eff)))
    pick.append(max((L for L in by_layer if L.kh == 1), key=lambda L: (L.cin, -L.cout_eff)))
    return [by_layer[L][0] for L in dict.fromkeys(pick)]


# ------------------------------------------------------------------------------------------------ gate epilogues
# The three ConvGRU gate epilogues of include/codd_hip.h (codd_conv_params.gate), as BasicUpdateBlock chains them on one
# hidden state h (G = 128 channels):
#   gate 1   t12 = dual(h; Wzr) + b                          [2G]   dual: 3x3 tap sets at dilation dil2 = 1 and dil = 4
#   gate 2   s = conv1x1(enc; Wm) + bm + ctx                 [3G]
#            z = sigmoid(s[:G] + t12[:G]);  r h = sigmoid(s[G:2G] + t12[G:]) * h  (records);  q-input = s[2G:]
#   gate 3   q = tanh(dual(r h; Wq) + bq + q-input);  h' = (1 - z) h + z q      (fp32 in place of h, and records)
# Every stage is referenced from the operands THE DEVICE HOLDS (the t12 / z / q-input / r h a previous launch wrote, read
# back exactly), so no stage's bound has to carry an earlier stage's error: the chain is the product's, the references
# are per launch.
GATE_G = 128


def dual_lin(x, w, dil, dil2):
    """(sum, sum of |terms|) of the dual tap sets: w [cout, cin, 2k, k], rows [0, k) at dilation dil2, rows [k, 2k)
    at dilation dil, both 'same' and centred on one pixel."""
    k = w.shape[3]
    a, Ma = conv_lin(x, w[:, :, :k], pad=(dil2 * (k // 2),) * 4, dil=(dil2, dil2))
    b, Mb = conv_lin(x, w[:, :, k:], pad=(dil * (k // 2),) * 4, dil=(dil, dil))
    return a + b, Ma + Mb


def gate_inputs(H, W):
    """Seeded inputs of the chain at an H x W map, B = 2: h = tanh features, ctx / enc = ReLU features (O(1) scales
    0.25 .. 4 per channel: a GRU's state is O(1) by construction), weights N(0, 1) / sqrt(K) with a scale per output
    channel, biases with pre-activations planted beyond +-20 and +-90 in the first channels of z, r and q."""
    g = _gen(H, W, 4242)
    f = lambda C, fn: (fn(torch.randn(B, C, H, W, generator=g)) * _log_uniform(g, C, 0.25, 4.0).view(1, -1, 1, 1)).contiguous()
    h = torch.tanh(torch.randn(B, GATE_G, H, W, generator=g) * 1.5).contiguous()
    ctx, enc = f(3 * GATE_G, torch.relu), f(3 * GATE_G, torch.relu)

    def wb(cout, cin, kh, kw):
        so = _log_uniform(g, cout, 0.25, 4.0)
        so[1:5] = 0.05
        w = torch.randn(cout, cin, kh, kw, generator=g) * so.view(-1, 1, 1, 1) / math.sqrt(cin * kh * kw)
        return w.contiguous(), (torch.randn(cout, generator=g) * so).contiguous()

    wzr, bzr = wb(2 * GATE_G, GATE_G, 6, 3)
    wm, bm = wb(3 * GATE_G, 3 * GATE_G, 1, 1)
    wq, bq = wb(GATE_G, GATE_G, 6, 3)
    bq[1:5] = torch.tensor(PLANTED)
    for blk in (0, GATE_G, 2 * GATE_G):  # z, r and the q-input stream
        bm[blk + 1:blk + 5] = torch.tensor(PLANTED)
        wm[blk + 1:blk + 5] = torch.randn(4, 3 * GATE_G, 1, 1, generator=g) * 0.05 / math.sqrt(3 * GATE_G)
    return dict(h=h, ctx=ctx, enc=enc, wzr=wzr, bzr=bzr, wm=wm, bm=bm, wq=wq, bq=bq)


def gate1_ref(h, wzr, bzr, dil=4, dil2=1):
    lin, M = dual_lin(h, wzr, dil, dil2)
    v, M, _ = epilogue(lin, M, bzr)
    return v, M


def gate2_ref(enc, wm, bm, ctx, t12, h):
    """-> {"z": (value, M), "rh": (value, M), "qin": (value, M)}; t12 [B,2G], h [B,G] as the device holds them."""
    G = GATE_G
    lin, Ml = conv_lin(enc, wm)
    s = lin + bm.to(F64).view(1, -1, 1, 1) + ctx.to(F64)
    Ms = Ml + bm.to(F64).abs().view(1, -1, 1, 1) + ctx.to(F64).abs()
    t12, h = t12.to(F64), h.to(F64)
    out = {}
    for name, blk in (("z", 0), ("rh", 1)):
        sg = torch.sigmoid(s[:, blk * G:(blk + 1) * G] + t12[:, blk * G:(blk + 1) * G])
        Msg = 0.25 * (Ms[:, blk * G:(blk + 1) * G] + t12[:, blk * G:(blk + 1) * G].abs()) + sg + UNDERFLOW
        out[name] = (sg, Msg) if name == "z" else (sg * h, Msg * h.abs() + (sg * h).abs())
    out["qin"] = (s[:, 2 * G:], Ms[:, 2 * G:] + s[:, 2 * G:].abs())
    return out


def gate3_ref(rh, wq, bq, z, qin, h, dil=4, dil2=1):
    """h' = (1 - z) h + z tanh(dual(rh) + bq + qin) -> (value, M); rh (the decoded records), z, qin, h as the device
    holds them.  M: the tanh's magnitude through z, + the terms of the blend (1 - z, its product with h, z q, the sum)."""
    lin, Ml = dual_lin(rh, wq, dil, dil2)
    z, qin, h = z.to(F64), qin.to(F64), h.to(F64)
    pre = lin + bq.to(F64).view(1, -1, 1, 1) + qin
    q = torch.tanh(pre)
    Mq = Ml + bq.to(F64).abs().view(1, -1, 1, 1) + qin.abs() + q.abs()
    val = (1 - z) * h + z * q
    M = z.abs() * Mq + h.abs() + (z * h).abs() + (z * q).abs() + val.abs()
    return val, M


def gate_triples():
    return [e for e in triples() if e.gate]


# ------------------------------------------------------------------------------------------------ rolling launches
def roll_case(mode, Cn, cin, Bn, H, W, residual):
    """Seeded inputs of one codd_conv_roll launch (ops.PackedRoll modes: 0 = 3x3, 1 = 3x3 -> 3x3 (+ the chain input as
    residual), 2 = 1x1 -> 3x3), wide channel scales (the kernel is exact fp32), raw disparities in the first channels."""
    g = _gen(mode, Cn, cin, Bn, H, W, int(residual), 777)
    x = features(g, Bn, cin, H, W, 1e-3, 1e3, True)
    si = x.abs().amax((0, 2, 3)).clamp(min=1e-6)
    k0 = 1 if mode == 2 else 3
    so = _log_uniform(g, Cn, 1e-3, 1e3)
    wa = torch.randn(Cn, cin, k0, k0, generator=g) * so.view(-1, 1, 1, 1) / (si.sqrt().view(1, -1, 1, 1) * math.sqrt(cin * k0 * k0))
    ba = torch.randn(Cn, generator=g) * so
    sb = _log_uniform(g, Cn, 1e-3, 1e3)
    wb = torch.randn(Cn, Cn, 3, 3, generator=g) * sb.view(-1, 1, 1, 1) / (so.sqrt().view(1, -1, 1, 1) * math.sqrt(Cn * 9))
    bb = torch.randn(Cn, generator=g) * sb
    return dict(x=x, wa=wa.contiguous(), ba=ba, wb=wb.contiguous(), bb=bb)


def roll_ref(d, mode, residual, act_a="lrelu", act_b="lrelu"):
    """The two-stage launch as two chained references -> (value, M).  The second stage's M carries the first stage's
    bound: stage B reads a_gpu = a + da with |da| <= c 2^-24 M_a, which moves its sum by at most sum |w_b| |da|, so
    M_b gains  sum |w_b| M_a  (the same tap loop on |w_b| and M_a) before the activation's Lipschitz constant."""
    k0 = d["wa"].shape[2]
    a, Ma = conv_ref(d["x"], d["wa"], d["ba"], pad=(k0 // 2,) * 4, act=act_a)
    if mode == 0:
        return a, Ma
    lin, Ml = conv_lin(a, d["wb"], pad=(1, 1, 1, 1))
    Ml = Ml + conv_lin(Ma, d["wb"].abs(), pad=(1, 1, 1, 1))[0]
    return epilogue(lin, Ml, d["bb"], act_b, d["x"] if residual else None)[:2]
