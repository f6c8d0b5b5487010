"""fp64 restatement of every MODULE of RAFT3D's context network (codd_amd/hrnet.py: the stem, Bottleneck, the
transitions, HRModule, ResizeConcatConv, and ops.context_split behind it; oracle/hrnet.py), the case list, the running
per-element bound and the planted wiring errors, for tests/test_context_net_fp64_reference.py (CPU: the restatement
against the fp32 oracle, the bound against an independent fp32 evaluation, its power, the BatchNorm fold) and
tests/test_gpu_context_net_fp64.py (the product's modules, TEACHER-FORCED: module m runs on the fp32 oracle's own
activation at that point, computed once per case on the host, the same tensor on both sides, never GPU output).

Every module is written ONCE over a small backend.  ``K32`` is the fp32 CPU oracle's own functions (oracle.hrnet._cbn,
F.interpolate, F.relu, torch's +): the modules chained over K32 are bit-equal to oracle.hrnet.hrnet / cnet (tested).
``K64`` carries a pair ``Q(v, E)``: the fp64 value -- conv_fp64's explicit tap loops, BatchNorm UNFOLDED,
(conv - mean) / sqrt(var + 1e-5) * gamma + beta, pointwise_fp64's resize -- and beside it a running bound E >= |fp32
evaluation - v| per ELEMENT, 0 (None) at the module's teacher-forced input.  Nothing in E is taken from GPU output:

  convolution + BatchNorm (hrnet.cbn): with s = gamma / sqrt(var + eps), w' = w s,
        M_pre = sum |w'||x| + |beta| + |mean s| (+ |conv bias s|) + sum |res|,   M = M_pre + |act(v)|
        E_out = |s| conv_lin(E_in, |w|) + sum E_res + conv_fp64.bound(M, "fp32") + FOLD 2^-24 M_pre
                + one rounding 2^-24 |partial sum| per residual addition, in the kernel's order ((conv + acc) + x_i)
  ReLU: Lipschitz 1, E unchanged.  tanh (context_split): E + pointwise_fp64.C["ctx_tanh"] 2^-24 |tanh|.
  resize_bilinear: the same convex combination of E_in, + E of ``out`` / ``extra`` where they are added,
        + pointwise_fp64.C["resize"] 2^-24 M (its M holds the addends), + one rounding per addition ((acc + x_i) + blend).
  1x1 head convolution: conv_lin(E_in, |w|) + conv_fp64.bound(M, "fp32").

FOLD covers what hrnet.packed_cbn rounds in fp32 before any convolution runs (u = 2^-24, first order, relative):
  eps: fl32(1e-5) is off by <= u, so var + eps by <= u; the addition rounds once more: 2 u, halved by the square root: u;
  sqrt to 1 ulp (2 u; a correctly rounded one is u), the division to 1 ulp (2 u):        s~ = s (1 + 5 u)
  w' = fl(w s~): 6 u on every product |w'||x|;   fl(mean s~): 6 u |mean s|;   beta - that: + u (|beta| + |mean s|)
  a convolution with a bias: fl(bias s~) 6 u |bias s|, and one more addition: u |b'|
  => |folded - unfolded| <= 6 u sum|w'||x| + 8 u |mean s| + 2 u |beta| + 7 u |bias s| <= 8 u M_pre.
FOLD = 8.5: the half unit covers the second-order terms (<= 64 u^2 M_pre).  It is derived, not fitted; the reference
test holds the fold's own arithmetic (test_fold_*) on planted BatchNorm channels to it.

There is no discontinuity in this network: no excuse rule, no excluded element.  The oracle's own worst err / E per
module (MEASURED, printed and re-measured by the reference test) says how loose E is; it is asserted only as <= 1.

The bound is a worst-case one: every convolution multiplies E_in by the sum of |w'|, about ten at these weights, where
the errors of a real evaluation add up like a random walk.  One to three convolutions deep it sits 15 .. 100 x above the
oracle's error and far below any wiring error; across a whole HRModule (seven to nine convolutions) it reaches the size
of the activations, and carried through the whole network it is 1e48 x the oracle's error.  Hence the modules
"stageN.m.stepK" and "stageN.m.fuse" (MODULES): the branch steps one by one and the fuse layers alone are what holds
HRModule.run sharply; the whole HRModule and the free-running network are still held to their bounds, for what they say.

VARIANTS are planted wiring errors of the restatement.  Two of them cannot run literally because the shapes do not
fit, and take the nearest form that does: ``transition_from_first`` builds the new branch from ys[0] with the first
C(ys[0]) input channels of the weight and the stride that gives the map the new branch's size;
``down_on_block1`` adds layer1.0's downsample of the first 64 channels of x in layer1.1 in place of x.
``bn_eps0`` moves s by eps / (2 var) <= 5e-6 on the network's own statistics (the filler's running_var >= 1), about
1.5 x a single convolution's bound -- no rigorous bound can see that; the path on which eps matters is var << eps, which
only the planted BatchNorm channels of ``fold_case`` have, so that is where its power is shown."""
import functools
import os

import torch
import torch.nn.functional as F

import conv_fp64 as CV
import pointwise_fp64 as PW
from oracle import hrnet as ohr

F64 = torch.float64
U = CV.U
P = "motion.raft3d.cnet"
H = P + ".0"
FOLD = 8.5
# name -> (B, H, W), multiples of 64 as the product pads them.  T: branch maps 16^2 .. 2^2, every pixel a border pixel,
# branch 3 of width 2 leaves the multi-job group; E: widths 32 / 16 / 8 / 4, four-job groups; B: two different images,
# widths 48 / 24 / 12 / 6 (branch 3 unaligned); A: widths 80 / 40 / 20 / 10, five 16-pixel tiles on branch 0
CASES = {"T": (1, 64, 64), "E": (1, 64, 128), "B": (2, 128, 192), "A": (1, 192, 320)}
STAGE_MODULES = tuple(f"{st}.{m}" for st, cfg in ohr.STAGES.items() for m in range(cfg["num_modules"]))
FUSE_MODULES = tuple(m + ".fuse" for m in STAGE_MODULES)
STEP_MODULES = tuple(f"{m}.step{st}" for m in STAGE_MODULES for st in range(4))
# "stageN.m" is the whole HRModule from its inputs.  The running bound is a worst-case one: it grows by the sum of |w'| --
# about ten -- per convolution, and across the seven to nine convolutions of a whole HRModule it reaches the size of the
# activations themselves (the oracle sits at 1e-6 of it, MEASURED): the whole-module figure is a report, it cannot see a
# wrong branch.  What holds HRModule.run sharply are its parts, one to three convolutions deep:
#   "stageN.m.stepK"  branch step K = 0..3 (conv1 / conv2 of block K // 2 of every branch: one ops.conv2d_multi call) from
#                     the previous step's outputs and, for a conv2, the block's input (trajectory keys "_stageN.m.stepK").
#                     On the device the steps' outputs are captured by wrapping ops.conv2d_multi and each step is held to
#                     its reference from the captured outputs of the step before it (step 0: the module's teacher-forced
#                     input), chosen by the restatement's wiring, not by what the product passed;
#   "stageN.m.fuse"   the fuse layers alone from the last step's outputs: on the device once as an HRModule with no blocks
#                     that shares the real one's fuse_layers (HRModule.run's own fuse code on the oracle's branch outputs)
#                     and once as the whole module's output against the fuse reference of its own captured branch outputs
MODULES = tuple(x for m in ("stem", "layer1.0", "layer1.1", "transition1", "stage2.0", "transition2", "stage3.0", "stage3.1",
                            "stage3.2", "transition3", "stage4.0", "stage4.1", "head", "split")
                for x in ((m,) + tuple(f"{m}.step{st}" for st in range(4)) + (m + ".fuse",) if m in STAGE_MODULES else (m,)))
# module -> the trajectory entries whose tensors (concatenated, in this order) are its input; () = the image
INPUTS = {"stem": (), "layer1.0": ("stem",), "layer1.1": ("layer1.0",), "transition1": ("layer1.1",),
          "stage2.0": ("transition1",), "transition2": ("stage2.0",), "stage3.0": ("stage2.0", "transition2"),
          "stage3.1": ("stage3.0",), "stage3.2": ("stage3.1",), "transition3": ("stage3.2",),
          "stage4.0": ("stage3.2", "transition3"), "stage4.1": ("stage4.0",), "head": ("stage4.1",), "split": ("head",)}
for _m in STAGE_MODULES:  # a conv2 step reads the previous step's outputs and then the block's inputs
    INPUTS.update({_m + ".step0": INPUTS[_m], _m + ".step1": (f"_{_m}.step0",) + INPUTS[_m], _m + ".step2": (f"_{_m}.step1",),
                   _m + ".step3": (f"_{_m}.step2", f"_{_m}.step1"), _m + ".fuse": (f"_{_m}.step3",)})
_CHAIN2 = tuple(m for m in FUSE_MODULES if not m.startswith("stage2"))  # three or more branches
_CONV1 = tuple(m for m in STEP_MODULES if m[-1] in "02")
_CONV2 = tuple(m for m in STEP_MODULES if m[-1] in "13")
# variant -> the modules it touches (bn_eps0: module docstring)
VARIANTS = {
    "no_self_term": FUSE_MODULES, "fuse_align_true": FUSE_MODULES, "head_align_false": ("head",),
    "chain_relu_last": FUSE_MODULES, "chain_no_relu_mid": _CHAIN2, "fuse_relu_missing": FUSE_MODULES,
    "term_dropped_j2": _CHAIN2, "transition_from_first": ("transition2", "transition3"), "down_on_block1": ("layer1.1",),
    "residual_before_bn": ("layer1.0", "layer1.1"), "head_order": ("head",), "split_at_256": ("split",), "bn_eps0": (),
    # the branch steps: the residual of a block dropped; no ReLU after conv1; the two blocks of a branch exchanged; conv1's
    # weights where conv2's belong and the reverse (another branch's weights have another shape: this is the exchange
    # that can run); the residual taken from the block's conv1 output instead of its input; the last column / the last
    # row of branch 0's output wrong (zero: a tile edge not written)
    "block_no_residual": _CONV2, "block_no_relu_mid": _CONV1, "blocks_swapped": STEP_MODULES,
    "conv12_swapped": STEP_MODULES, "residual_from_conv1": _CONV2, "edge_column_zero": STEP_MODULES,
    "edge_row_zero": STEP_MODULES,
}

# worst |stage32 - stage64| / E per module over CASES and all outputs of the sequential fp32 evaluation K32S
# (measure(); tests/test_context_net_fp64_reference.py prints and re-measures it).  A measurement: it says how loose E is
# and is no tolerance.  The oracle's own figures -- F.conv2d sums in an order that follows the host's convolution library
# and thread count, single modules move by up to 2 x from host to host -- are printed beside it and held to <= 1
MEASURED = {
    "stem": 0.00855, "layer1.0": 0.000683, "layer1.1": 0.000459, "transition1": 0.0736, "stage2.0": 6.2e-06,
    "stage2.0.step0": 0.0705, "stage2.0.step1": 0.0633, "stage2.0.step2": 0.0589, "stage2.0.step3": 0.0539,
    "stage2.0.fuse": 0.0638, "transition2": 0.0461, "stage3.0": 1.18e-06, "stage3.0.step0": 0.0675,
    "stage3.0.step1": 0.0479, "stage3.0.step2": 0.057, "stage3.0.step3": 0.0513, "stage3.0.fuse": 0.0336,
    "stage3.1": 1.17e-06, "stage3.1.step0": 0.0611, "stage3.1.step1": 0.049, "stage3.1.step2": 0.0708,
    "stage3.1.step3": 0.046, "stage3.1.fuse": 0.0245, "stage3.2": 1.07e-06, "stage3.2.step0": 0.0481,
    "stage3.2.step1": 0.0545, "stage3.2.step2": 0.0633, "stage3.2.step3": 0.0668, "stage3.2.fuse": 0.031,
    "transition3": 0.0461, "stage4.0": 7.21e-07, "stage4.0.step0": 0.064, "stage4.0.step1": 0.0533,
    "stage4.0.step2": 0.0634, "stage4.0.step3": 0.0603, "stage4.0.fuse": 0.0207, "stage4.1": 7.7e-07,
    "stage4.1.step0": 0.0534, "stage4.1.step1": 0.057, "stage4.1.step2": 0.0714, "stage4.1.step3": 0.0578,
    "stage4.1.fuse": 0.0266, "head": 0.0523, "split": 0.175,
}


# ------------------------------------------------------------------------------------------------ inputs
def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The image [B,3,H,W] fp32: frame b of codd_amd.synth.stereo_sequence is item b."""
    from codd_amd import synth
    B, Hh, W = CASES[name]
    img, _, _ = synth.stereo_sequence(Hh, W, B)
    return img[0].contiguous()


@functools.lru_cache(maxsize=None)
def estimator():
    """(the estimator on the host with the "random" filler at gain 1.4 of the other stage tests, its state dict)"""
    import codd_amd  # noqa: F401
    from codd_amd import configs, synth
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd(iters=2)).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    return est, {k: v.clone() for k, v in est.state_dict().items()}


@functools.lru_cache(maxsize=None)
def weights(dtype):
    return {k: v.to(dtype) for k, v in estimator()[1].items() if k.startswith(P + ".") and v.is_floating_point()}


# ------------------------------------------------------------------------------------------------ the two backends
class Q:
    """An fp64 value and the running bound beside it (None: exactly 0)."""
    __slots__ = ("v", "E")

    def __init__(self, v, E=None):
        self.v, self.E = v, E

    @property
    def shape(self):
        return self.v.shape

    def bound(self):
        return torch.zeros_like(self.v) if self.E is None else self.E


def _esum(*es):
    es = [e for e in es if e is not None]
    return None if not es else functools.reduce(lambda a, b: a + b, es)


class K32:
    """The fp32 CPU oracle's own functions."""
    dtype = torch.float32

    @staticmethod
    def lift(t):
        return t.float()

    @staticmethod
    def cbn(sd, ck, bk, x, stride=1, pad=0, relu=False, res=(), variant=None):
        y = ohr._cbn(sd, ck, bk, x, stride, pad)
        for r in res:
            y = y + r
        return F.relu(y) if relu else y

    @staticmethod
    def conv(sd, key, x, relu=False):
        y = F.conv2d(x, sd[key + ".weight"])
        return F.relu(y) if relu else y

    @staticmethod
    def resize(t, size, ac, acc=None, extra=None):
        v = F.interpolate(t, size=tuple(size), mode="bilinear", align_corners=bool(ac))
        base = acc if extra is None else (extra if acc is None else acc + extra)
        return v if base is None else base + v

    @staticmethod
    def add(a, b):
        return a + b

    @staticmethod
    def edge_zero(y, column):
        y = y.clone()
        if column:
            y[..., -1] = 0
        else:
            y[..., -1, :] = 0
        return y

    relu = staticmethod(F.relu)
    tanh = staticmethod(torch.tanh)

    @staticmethod
    def cat(qs):
        return torch.cat(list(qs), 1)

    @staticmethod
    def chans(q, lo, hi):
        return q[:, lo:hi]


def conv_seq(x, w, stride=1, pad=0):
    """An fp32 convolution with a fixed order of operations: one product at a time, taps outside, channels inside, a
    separate fp32 multiply and add each (torch's element-wise kernels; no BLAS, no thread-dependent order)."""
    O, Cn, kh, kw = w.shape
    Ho, Wo = (x.shape[2] + 2 * pad - kh) // stride + 1, (x.shape[3] + 2 * pad - kw) // stride + 1
    xp = F.pad(x, (pad,) * 4)
    out = torch.zeros(x.shape[0], O, Ho, Wo)
    for ky in range(kh):
        for kx in range(kw):
            sl = xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            for c in range(Cn):
                out += w[:, c, ky, kx].view(1, -1, 1, 1) * sl[:, c:c + 1]
    return out


class K32S(K32):
    """A second fp32 evaluation, independent of the oracle's and of the host's convolution library: conv_seq, BatchNorm written out
    ((y - mean) / sqrt(var + eps) * gamma + beta, unfolded), the rest as K32."""

    @staticmethod
    def cbn(sd, ck, bk, x, stride=1, pad=0, relu=False, res=(), variant=None):
        col = lambda t: t.view(1, -1, 1, 1)
        y = conv_seq(x, sd[ck + ".weight"], stride, pad)
        y = (y - col(sd[bk + ".running_mean"])) / torch.sqrt(col(sd[bk + ".running_var"]) + 1e-5) * col(sd[bk + ".weight"]) \
            + col(sd[bk + ".bias"])
        for r in res:
            y = y + r
        return F.relu(y) if relu else y

    @staticmethod
    def conv(sd, key, x, relu=False):
        y = conv_seq(x, sd[key + ".weight"])
        return F.relu(y) if relu else y


class K64:
    """fp64 values with the running bound (module docstring)."""
    dtype = F64

    @staticmethod
    def lift(t):
        return Q(t.to(F64))

    @staticmethod
    def cbn(sd, ck, bk, x, stride=1, pad=0, relu=False, res=(), variant=None):
        w = sd[ck + ".weight"]
        geo = dict(stride=(stride, stride), pad=(pad,) * 4)
        lin, Ml = CV.conv_lin(x.v, w, **geo)
        res = list(res)
        if variant == "residual_before_bn" and res:
            lin, res = lin + res[0].v, res[1:]
        col = lambda t: t.view(1, -1, 1, 1)
        eps = 0.0 if variant == "bn_eps0" else 1e-5
        s = sd[bk + ".weight"] / torch.sqrt(sd[bk + ".running_var"] + eps)
        beta, ms = sd[bk + ".bias"], sd[bk + ".running_mean"] * s
        v = (lin - col(sd[bk + ".running_mean"])) * col(s) + col(beta)
        M = Ml * col(s.abs()) + col(beta.abs() + ms.abs())
        cb = sd.get(ck + ".bias")
        if cb is not None:
            v, M = v + col(cb * s), M + col((cb * s).abs())
        E = None if x.E is None else CV.conv_lin(x.E, w.abs(), **geo)[0] * col(s.abs())
        rounds = 0.0
        for r in res:
            v, M, E = v + r.v, M + r.v.abs(), _esum(E, r.E)
            rounds = rounds + U * v.abs()
        a = F.relu(v) if relu else v
        return Q(a, _esum(E, CV.bound(M + a.abs(), "fp32") + FOLD * U * M + rounds))

    @staticmethod
    def conv(sd, key, x, relu=False):
        w = sd[key + ".weight"]
        lin, Ml = CV.conv_lin(x.v, w)
        a = F.relu(lin) if relu else lin
        E = None if x.E is None else CV.conv_lin(x.E, w.abs())[0]
        return Q(a, _esum(E, CV.bound(Ml + a.abs(), "fp32")))

    @staticmethod
    def resize(t, size, ac, acc=None, extra=None):
        form = {(False, False): "overwrite", (True, False): "accumulate", (False, True): "extra",
                (True, True): "extra_accumulate"}[(acc is not None, extra is not None)]
        v, M = PW.resize(t.v, tuple(size), ac, form, None if acc is None else acc.v, None if extra is None else extra.v)
        E = None if t.E is None else PW.resize(t.E, tuple(size), ac)[0]
        rounds = 0.0
        if acc is not None and extra is not None:
            rounds = rounds + U * (acc.v + extra.v).abs()
        if form != "overwrite":
            rounds = rounds + U * v.abs()
        E = _esum(E, None if acc is None else acc.E, None if extra is None else extra.E)
        return Q(v, _esum(E, PW.C["resize"] * U * M + rounds))

    @staticmethod
    def add(a, b):
        v = a.v + b.v
        return Q(v, _esum(a.E, b.E, U * v.abs()))

    @staticmethod
    def edge_zero(q, column):
        return Q(K32.edge_zero(q.v, column), q.E)

    @staticmethod
    def relu(q):
        return Q(F.relu(q.v), q.E)

    @staticmethod
    def tanh(q):
        t = torch.tanh(q.v)
        return Q(t, _esum(q.E, PW.C["ctx_tanh"] * U * t.abs()))

    @staticmethod
    def cat(qs):
        qs = list(qs)
        E = None if all(q.E is None for q in qs) else torch.cat([q.bound() for q in qs], 1)
        return Q(torch.cat([q.v for q in qs], 1), E)

    @staticmethod
    def chans(q, lo, hi):
        return Q(q.v[:, lo:hi], None if q.E is None else q.E[:, lo:hi])


# ------------------------------------------------------------------------------------------------ the modules
def m_stem(k, sd, x, variant=None):
    x = k.cbn(sd, H + ".conv1", H + ".bn1", x, 2, 1, True, variant=variant)
    return [k.cbn(sd, H + ".conv2", H + ".bn2", x, 2, 1, True, variant=variant)]


def m_bottleneck(k, sd, b, x, variant=None):
    """layer1.b: b = 0 has the downsample (reference mmseg Bottleneck: bn3(conv3) + identity, then ReLU)."""
    p = f"{H}.layer1.{b}"
    y = k.cbn(sd, p + ".conv1", p + ".bn1", x, relu=True, variant=variant)
    y = k.cbn(sd, p + ".conv2", p + ".bn2", y, 1, 1, True, variant=variant)
    idn = x
    if b == 0:
        idn = k.cbn(sd, p + ".downsample.0", p + ".downsample.1", x, variant=variant)
    elif variant == "down_on_block1":
        q = f"{H}.layer1.0.downsample"
        idn = k.cbn(sd, q + ".0", q + ".1", k.chans(x, 0, 64))
    return [k.cbn(sd, p + ".conv3", p + ".bn3", y, relu=True, res=[idn], variant=variant)]


def m_transition(k, sd, n, ys, variant=None):
    """transition n: 1: both branches of stage 2 from layer1's output; 2 / 3: the new branch from the last one."""
    if n == 1:
        return [k.cbn(sd, H + ".transition1.0.0", H + ".transition1.0.1", ys[0], 1, 1, True, variant=variant),
                k.cbn(sd, H + ".transition1.1.0.0", H + ".transition1.1.0.1", ys[0], 2, 1, True, variant=variant)]
    key = f"{H}.transition{n}.{n}.0"
    if variant == "transition_from_first":
        c0 = ys[0].shape[1]
        sd = dict(sd)
        sd[key + ".0.weight"] = sd[key + ".0.weight"][:, :c0].contiguous()
        return [k.cbn(sd, key + ".0", key + ".1", ys[0], 2 * (ys[0].shape[2] // ys[-1].shape[2]), 1, True)]
    return [k.cbn(sd, key + ".0", key + ".1", ys[-1], 2, 1, True, variant=variant)]


def m_step(k, sd, name, st, prev, blockin=None, variant=None):
    """Branch step ``st`` of HRModule ``name`` (stage2.0 ...): st even = conv1 + BN + ReLU of block st // 2 of every branch
    on ``prev``; st odd = conv2 + BN, + the block's input ``blockin``, ReLU."""
    outs = []
    for i, x in enumerate(prev):
        blk, c = (1 - st // 2 if variant == "blocks_swapped" else st // 2), 1 + st % 2
        if variant == "conv12_swapped":
            c = 3 - c
        p = f"{H}.{name}.branches.{i}.{blk}"
        if st % 2 == 0:
            y = k.cbn(sd, f"{p}.conv{c}", f"{p}.bn{c}", x, 1, 1, variant != "block_no_relu_mid", variant=variant)
        else:
            res = [] if variant == "block_no_residual" else [x if variant == "residual_from_conv1" else blockin[i]]
            y = k.cbn(sd, f"{p}.conv{c}", f"{p}.bn{c}", x, 1, 1, True, res=res, variant=variant)
        if i == 0 and variant in ("edge_column_zero", "edge_row_zero"):
            y = k.edge_zero(y, variant == "edge_column_zero")
        outs.append(y)
    return outs


def m_steps(k, sd, name, xs, variant=None):
    """The four branch steps of HRModule ``name`` chained -> the list of their output lists (the last: the branch outputs)."""
    steps, blockin = [], list(xs)
    for st in range(4):
        steps.append(m_step(k, sd, name, st, steps[-1] if steps else blockin, blockin, variant))
        if st % 2:
            blockin = steps[-1]
    return steps


def m_fuse(k, sd, name, xs, variant=None):
    """The fuse layers of HRModule ``name`` on the branch outputs: out_i = relu(sum_j t_ij) in j order; the additions
    as the product's kernels perform them: (conv + acc) for a down chain's last convolution -- + x_i after it on the
    last branch --, (acc + x_i) + blend for the first up path, acc + blend for the others."""
    p, nb = f"{H}.{name}", len(xs)
    outs = []
    for i in range(nb):
        y, pending = None, None  # pending: x_i, added with the next term
        for j in range(nb):
            if variant == "term_dropped_j2" and i == 0 and j == 2:
                continue
            if j < i:
                t = xs[j]
                for c in range(i - j - 1):
                    q = f"{p}.fuse_layers.{i}.{j}.{c}"
                    t = k.cbn(sd, q + ".0", q + ".1", t, 2, 1, variant != "chain_no_relu_mid", variant=variant)
                q = f"{p}.fuse_layers.{i}.{j}.{i - j - 1}"
                res = [] if y is None else [y]
                if i == nb - 1 and j == i - 1:
                    res = res + [xs[i]]  # the branch's own term rides on its last chain convolution
                if variant == "chain_relu_last":  # (a ReLU between the convolution and the sum)
                    y = k.cbn(sd, q + ".0", q + ".1", t, 2, 1, True)
                    for r in res:
                        y = k.add(y, r)
                else:
                    y = k.cbn(sd, q + ".0", q + ".1", t, 2, 1, res=res, variant=variant)
            elif j == i:
                if i < nb - 1:
                    pending = None if (variant == "no_self_term" and i == 0) else xs[i]
            else:
                q = f"{p}.fuse_layers.{i}.{j}"
                t = k.cbn(sd, q + ".0", q + ".1", xs[j], variant=variant)
                y = k.resize(t, xs[i].shape[2:], variant == "fuse_align_true", acc=y, extra=pending)
                pending = None
        outs.append(y if variant == "fuse_relu_missing" else k.relu(y))
    return outs


def m_head(k, sd, ys, variant=None):
    """ResizeConcatConv: four align_corners=True resizes to branch 1's size, one 270-channel tensor, 1x1 to 512, ReLU."""
    size = ys[1].shape[2:]
    rs = [k.resize(y, size, variant != "head_align_false") for y in ys]
    return [k.conv(sd, P + ".1.convs.0", k.cat(rs[::-1] if variant == "head_order" else rs), True)]


def m_split(k, x, variant=None):
    """ops.context_split: net = tanh(x[:, :128]), inp = relu(x[:, 128:])."""
    at = 256 if variant == "split_at_256" else 128
    full = k.cat([k.tanh(k.chans(x, 0, at)), k.relu(k.chans(x, at, 512))])
    return [k.chans(full, 0, 128), k.chans(full, 128, 512)]


def run_module(k, sd, name, xs, variant=None):
    """Module ``name`` of MODULES on its input list ``xs`` (backend values) -> its output list."""
    if name == "stem":
        return m_stem(k, sd, xs[0], variant)
    if name.startswith("layer1"):
        return m_bottleneck(k, sd, int(name[-1]), xs[0], variant)
    if name.startswith("transition"):
        return m_transition(k, sd, int(name[-1]), xs, variant)
    if name.endswith(".fuse"):
        return m_fuse(k, sd, name[:-5], xs, variant)
    if name in STEP_MODULES:
        st, nb = int(name[-1]), len(xs) // (1 + int(name[-1]) % 2)
        return m_step(k, sd, name[:-6], st, xs[:nb], xs[nb:] or None, variant)
    if name.startswith("stage"):
        return m_fuse(k, sd, name, m_steps(k, sd, name, xs, variant)[-1], variant)
    return m_head(k, sd, xs, variant) if name == "head" else m_split(k, xs[0], variant)


def module_inputs(name, T, image):
    """The fp32 tensors module ``name`` reads: the image, or the outputs in ``T`` (name -> list) of INPUTS[name]."""
    return [image] if not INPUTS[name] else [t for src in INPUTS[name] for t in T[src]]


def evaluate(k, sd, image, T=None, variant=None, modules=MODULES):
    """``modules`` over backend ``k`` -> {name: output list}.  ``T`` None: free running, each module from the previous
    ones' results (K64: the bound accumulates through the whole network).  ``T`` = a trajectory {name: fp32 tensors}:
    TEACHER-FORCED, every module from T's values of its inputs with E = 0."""
    R = {}
    for name in modules:
        if T is None:
            xs = [k.lift(image)] if not INPUTS[name] else [q for src in INPUTS[name] for q in R[src]]
        else:
            xs = [k.lift(t) for t in module_inputs(name, T, image)]
        if name in STAGE_MODULES:
            steps = m_steps(k, sd, name, xs, variant)
            R.update({f"_{name}.step{st}": v for st, v in enumerate(steps)})
            R[name] = m_fuse(k, sd, name, steps[-1], variant)
        elif T is None and (name in STEP_MODULES or name in FUSE_MODULES):  # (free running: the whole module's own parts)
            R[name] = R["_" + name] if name in STEP_MODULES else R[name[:-5]]
        else:
            R[name] = run_module(k, sd, name, xs, variant)
    return R


def oracle_world(name, single_thread=False):
    return _world(name, bool(single_thread))


@functools.lru_cache(maxsize=None)
def _world(name, single_thread):
    """Case ``name`` on the host, computed once: dict(image, T32 = the modules chained over the oracle's functions (the
    oracle's fp32 trajectory), R64 = every module in fp64 from T32's values of its inputs).  ``single_thread``: the
    oracle on ONE host thread (F.conv2d sums in another order there: another fp32 evaluation)."""
    image = inputs(name)
    with torch.no_grad():
        torch.set_num_threads(1) if single_thread else _threads()
        try:
            T32 = evaluate(K32, weights(torch.float32), image)
        finally:
            _threads()
        R64 = evaluate(K64, weights(F64), image, T32)
    return dict(image=image, T32=T32, R64=R64)


@functools.lru_cache(maxsize=None)
def seq_world(name):
    """Case ``name`` under K32S: dict(T32 = its own trajectory, chained from the image, R64 = every module in fp64 from
    that trajectory's values); no convolution library and no thread count enters it (its figures still move with the CPU
    model, test_bound_holds_...'s docstring)."""
    image = inputs(name)
    _threads()
    with torch.no_grad():
        T32 = evaluate(K32S, weights(torch.float32), image)
        R64 = evaluate(K64, weights(F64), image, T32)
    return dict(image=image, T32=T32, R64=R64)


# ------------------------------------------------------------------------------------------------ comparison
def ratio(got, q):
    """|got - q.v| / q.E per element; 0 where the error is 0, inf where E = 0 and it is not, or ``got`` is not finite."""
    err = (got.to(F64) - q.v).abs()
    lim = q.bound()
    r = torch.where(lim > 0, err / lim.clamp(min=1e-300), torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), r)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)


def worst(gots, qs):
    """max err / E over the outputs of one module."""
    assert len(gots) == len(qs) and all(g.shape == q.shape for g, q in zip(gots, qs)), ([g.shape for g in gots], [q.shape for q in qs])
    return max(ratio(g, q).max().item() for g, q in zip(gots, qs))


def measure(names=None):
    """Worst err / E per module -> (table: K32S over the cases, {(case, evaluation, module): figure} with evaluation
    "seq" (K32S), "oracle" (the fp32 oracle on the host's threads) and "oracle/1" (on one thread))."""
    tab, per = {m: 0.0 for m in MODULES}, {}
    for name in (names or CASES):
        for ev, w in (("seq", seq_world(name)), ("oracle", oracle_world(name)), ("oracle/1", oracle_world(name, True))):
            for m in MODULES:
                r = worst(w["T32"][m], w["R64"][m])
                per[(name, ev, m)] = r
                if ev == "seq":
                    tab[m] = max(tab[m], r)
    return tab, per


def power(name, variant, module):
    """max |variant64 - stage64| / E over the outputs of ``module``, both teacher-forced on case ``name``."""
    w = oracle_world(name)
    with torch.no_grad():
        got = evaluate(K64, weights(F64), w["image"], w["T32"], variant, modules=(module,))[module]
    return worst([g.v for g in got], w["R64"][module])


# ------------------------------------------------------------------------------------------------ the BatchNorm fold
FOLD_CHANNELS = ("var_1e-12", "gamma_neg", "gamma_0", "cancel", "plain")


def fold_case(bias, stats=0):
    """One 3x3 convolution 16 -> 8 (``bias``: with a bias) with planted BatchNorm channels, on x [2,16,9,11] = 7 + 0.1 N:
    0: running_var = 1e-12 (s ~ 316 gamma); 1: gamma < 0; 2: gamma = 0; 3: |mean s| ~ 1e3 x the output -- the channel's
    convolution (+ bias) sits at ~1000 away from the zero-padded border and the mean cancels it --; 4 .. 7 ordinary.  ``stats`` = 1: other statistics of
    the same kind (for the fold cache's version key).  -> dict of fp32 tensors under the keys "c.*" / "b.*"."""
    g, gs = torch.Generator().manual_seed(9173 + int(bias)), torch.Generator().manual_seed(577 + stats)
    r = lambda *s: torch.randn(*s, generator=g)
    K = 16 * 9
    x = (7.0 + 0.1 * r(2, 16, 9, 11)).contiguous()
    w = r(8, 16, 3, 3) / K ** 0.5
    cb = 0.3 * r(8)
    target = 500.0 if bias else 1000.0  # what the convolution itself reaches on channel 3
    w[3] = target / (K * 7.0) * (1.0 + 0.01 * r(16, 3, 3))
    cb[3] = 500.0
    r = lambda *s: torch.randn(*s, generator=gs)  # (the convolution and x do not depend on ``stats``)
    gamma, beta = 1.0 + 0.2 * r(8), 0.3 * r(8)
    mean, var = 0.5 * r(8), 1.0 + 0.3 * r(8).abs()
    var[0], gamma[1], gamma[2], mean[3] = 1e-12, -1.3 - 0.1 * stats, 0.0, 1000.0 + stats
    sd = {"c.weight": w.contiguous(), "b.weight": gamma, "b.bias": beta, "b.running_mean": mean, "b.running_var": var}
    if bias:
        sd["c.bias"] = cb
    return dict(x=x, sd=sd)


def fold_ref(case, variant=None):
    """The unfolded fp64 value of the case with its bound (conv_fp64.bound + FOLD) -> Q."""
    sd = {k: v.to(F64) for k, v in case["sd"].items()}
    return K64.cbn(sd, "c", "b", Q(case["x"].to(F64)), 1, 1, variant=variant)


def fold_fp32(sd):
    """hrnet.packed_cbn's arithmetic restated in fp32 -> (w', b')."""
    s = sd["b.weight"] / torch.sqrt(sd["b.running_var"] + 1e-5)
    w = sd["c.weight"] * s.view(-1, 1, 1, 1)
    b = sd["b.bias"] - sd["b.running_mean"] * s
    if "c.bias" in sd:
        b = b + sd["c.bias"] * s
    return w, b


def fold_figure(case):
    """|conv64(x, w') + b' - unfolded fp64| / (2^-24 M_pre) per element, (w', b') = fold_fp32: the fold's roundings
    alone (the convolution of the folded weights is taken in fp64), to stay inside FOLD."""
    sd = case["sd"]
    w, b = fold_fp32(sd)
    got = CV.conv_lin(case["x"], w, pad=(1,) * 4)[0] + b.to(F64).view(1, -1, 1, 1)
    sd64 = {k: v.to(F64) for k, v in sd.items()}
    s = sd64["b.weight"] / torch.sqrt(sd64["b.running_var"] + 1e-5)
    lin, Ml = CV.conv_lin(case["x"], sd64["c.weight"], pad=(1,) * 4)
    col = lambda t: t.view(1, -1, 1, 1)
    ref = (lin - col(sd64["b.running_mean"])) * col(s) + col(sd64["b.bias"])
    M = Ml * col(s.abs()) + col(sd64["b.bias"].abs() + (sd64["b.running_mean"] * s).abs())
    if "c.bias" in sd64:
        ref, M = ref + col(sd64["c.bias"] * s), M + col((sd64["c.bias"] * s).abs())
    return (got - ref).abs() / (U * M).clamp(min=1e-300), ref, M
