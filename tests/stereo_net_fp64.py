"""fp64 restatement of every STAGE of the stereo network (codd_amd/stereo.py: HITUNet.stages, TileInitialization.
init_level, TileUpdate0, TileUpdate, PostTileUpdate, FinalTileUpdate, TilePropagation; reference hitnet.py:75-100), the
case list and the bounds, for tests/test_stereo_net_fp64_reference.py (CPU: the restatement against the fp32 oracle,
the measurement that sets every constant below, the power of the bounds against eleven planted wiring errors) and
tests/test_gpu_stereo_net_fp64.py (the product's trace, ``HITNetMF.stereo_matching(trace=[...])``, TEACHER-FORCED: each
stage in fp64 from the product's own traced inputs of that stage against the product's traced results of it, so that no
error accumulates from stage to stage).

Composed from what the suite already has: conv_fp64's explicit tap loops for convolutions and deconvolutions,
stereo_fusion_fp64.costvol / argmin_check / near_tie_share / tile_warp / hyp_upsample / hyp_select for the four stereo
kernels.  Every stage is written ONCE over a small backend: ``K64`` (fp64: the functions above) and ``K32`` (the fp32
CPU oracle's own functions, oracle/stereo.py: conv, tile_cost_volume_min, tile_warping, upsample_hyp); the stages
chained over K32 are bit-equal to oracle.stereo.stereo_matching (tested), which is what makes ``stage32`` the
oracle's own function.

The bound of a traced quantity q (per channel group, GROUPS below: a slope or a confidence must not hide under the
disparity's scale) is absolute:

    |got - stage64(q)| <= BOUND[q] = 5 x D_q,    D_q = worst |stage32(q) - stage64(q)| over CASES,

both stages from the same inputs, taken along the oracle's fp32 trajectory on the CPU, never from GPU output (at
least 4 x: the margin of the project's other constants, raft_loop_fp64.py:17-23; 5 x leaves the re-measuring test room
on both sides of 4 D <= constant <= 8 D on every host).  D_q = 0 (copies, planted zeros) means: exact.

The two discontinuities.  Arg-min of init_level: the cost volume is evaluated from the tile features handed in
(``tl_tr``: the product's own, or the oracle's) under stereo_fusion_fp64.argmin_check with C["costvol"] -- the pick must
be the reference's first arg-min unless the reference's gap is within 2 x the cost bound; the cost and the descriptor
are then compared AT THE PICK.  Select of TileUpdate: the pick (conf1 > conf0 of the traced ``lastconv`` output) may
differ from the reference's only where the reference's |conf0 - conf1| <= 2 x BOUND[upd:conf]; the hypothesis is then
compared against the reference's other candidate.  Excused tiles per case and rule: at most excuse_cap(tiles)."""
import functools
import os

import torch
import torch.nn.functional as F

import conv_fp64 as CV
import stereo_fusion_fp64 as SF
from oracle import stereo as ost

F64 = torch.float64
P = "stereo"
MAX_DISP = 320
LEVELS = ("16x", "8x", "4x", "2x", "1x")
# name -> (B, H, W): multiples of 64, as the product pads them.  S: 1x2 tiles at 1/16, the 20-disparity search is wider
# than the map (every tile a border tile); B: two different pairs (the U-Net runs a batch of 4, the [:B] / [B:] views
# are live); A: 3x5 tiles at 1/16 (odd counts), a width that is no multiple of the 32-pixel conv column tile or of the
# 60 / 62-column rolling-window strip; W: wider than max_disp -- at W <= 320 the search of EVERY level is at least as wide
# as the map and every candidate beyond it costs the same zero-padded sum |L| as an earlier one, so that whether
# max_disp is divided per level cannot show in any output of S, B or A (6 tiles in a row at 1/16, search 20 < 24)
CASES = {"S": (1, 64, 128), "B": (2, 128, 256), "A": (1, 192, 320), "W": (1, 64, 384)}
# the 16-channel stride-1 layers of A take ops.conv_roll when ops.ROLL_MIN_PIXELS is at most this (case "A-roll"):
# down1's 3x3 and merge2 on the [2,16,96,160] batch (30 720 pixels), merge1 on [2,16,192,320], tile_update6 on [1,16,192,320]
ROLL_PIXELS_A = 2 * 96 * 160
VARIANTS = ("dsc_tl", "pad_left", "max_disp", "up_scale1", "conf_swap", "upd_swap", "cvp_from_cur", "relu_all", "dil1",
            "lr_swap", "final_ch1")
C_BOUND = 5.0


def excuse_cap(tiles):
    """A condition, not a measurement: excused tiles per case and per rule."""
    return max(2, int(1e-3 * tiles))


# D_q: worst |stage32 - stage64| over the cases and the oracle's two thread settings, see measure() (tests/test_stereo_net_fp64_reference.py prints it) ...
MEASURED = {
    "enc0": 1.3e-06, "enc1": 3.62e-06, "enc2": 2.75e-06, "enc3": 1.95e-06, "fea0": 1.41e-06, "fea0_img": 2.09e-06,
    "fea1": 1.13e-06, "fea2": 2.07e-06, "fea3": 3.86e-06, "fea4": 3.13e-06, "init0.tl": 5.97e-07,
    "init0.tr": 5.42e-07, "init0.cost": 2.84e-07, "init0.hyp:d": 0, "init0.hyp:s": 0, "init0.hyp:f": 3.31e-07,
    "init1.tl": 7.01e-07, "init1.tr": 9.85e-07, "init1.cost": 3.78e-07, "init1.hyp:d": 0, "init1.hyp:s": 0,
    "init1.hyp:f": 2.67e-07, "init2.tl": 1.18e-06, "init2.tr": 1.31e-06, "init2.cost": 5.47e-07, "init2.hyp:d": 0,
    "init2.hyp:s": 0, "init2.hyp:f": 4.73e-07, "init3.tl": 2.38e-06, "init3.tr": 2.79e-06, "init3.cost": 1.6e-06,
    "init3.hyp:d": 0, "init3.hyp:s": 0, "init3.hyp:f": 1.08e-06, "init4.tl": 1.78e-06, "init4.tr": 2.21e-06,
    "init4.cost": 1.53e-06, "init4.hyp:d": 0, "init4.hyp:s": 0, "init4.hyp:f": 8.54e-07, "upd0.aug:cvc": 7.53e-06,
    "upd0.upd:d": 1.38e-07, "upd0.upd:s": 1.99e-07, "upd0.upd:f": 2.44e-07, "upd0.hyp:d": 3.33e-07,
    "upd0.hyp:s": 1.99e-07, "upd0.hyp:f": 2.74e-07, "upd1.up:d": 1.67e-06, "upd1.up:s": 0, "upd1.up:f": 0,
    "upd1.aug:cvc": 7.51e-06, "upd1.aug:cvp": 1.75e-05, "upd1.upd:conf": 3.47e-07, "upd1.upd:p.d": 3.3e-07,
    "upd1.upd:p.s": 4.33e-07, "upd1.upd:p.f": 4.53e-07, "upd1.upd:c.d": 2.96e-07, "upd1.upd:c.s": 5.95e-07,
    "upd1.upd:c.f": 4.64e-07, "upd1.hyp:d": 2.2e-06, "upd1.hyp:s": 5.95e-07, "upd1.hyp:f": 4.49e-07,
    "upd2.up:d": 6.06e-06, "upd2.up:s": 0, "upd2.up:f": 0, "upd2.aug:cvc": 1.58e-05, "upd2.aug:cvp": 3.45e-05,
    "upd2.upd:conf": 9.27e-07, "upd2.upd:p.d": 1.12e-06, "upd2.upd:p.s": 1.01e-06, "upd2.upd:p.f": 1.22e-06,
    "upd2.upd:c.d": 9.36e-07, "upd2.upd:c.s": 1.2e-06, "upd2.upd:c.f": 1.47e-06, "upd2.hyp:d": 2.58e-06,
    "upd2.hyp:s": 1.2e-06, "upd2.hyp:f": 1.5e-06, "upd3.up:d": 1.12e-05, "upd3.up:s": 0, "upd3.up:f": 0,
    "upd3.aug:cvc": 1.64e-05, "upd3.aug:cvp": 9.47e-05, "upd3.upd:conf": 2.38e-06, "upd3.upd:p.d": 1.57e-06,
    "upd3.upd:p.s": 1.52e-06, "upd3.upd:p.f": 3.09e-06, "upd3.upd:c.d": 1.86e-06, "upd3.upd:c.s": 2.13e-06,
    "upd3.upd:c.f": 2.95e-06, "upd3.hyp:d": 8.68e-06, "upd3.hyp:s": 2.13e-06, "upd3.hyp:f": 3.02e-06,
    "upd4.up:d": 2.39e-05, "upd4.up:s": 0, "upd4.up:f": 0, "upd4.aug:cvc": 1.34e-05, "upd4.aug:cvp": 0.000128,
    "upd4.upd:conf": 2.81e-06, "upd4.upd:p.d": 2.78e-06, "upd4.upd:p.s": 2.86e-06, "upd4.upd:p.f": 3.75e-06,
    "upd4.upd:c.d": 2.77e-06, "upd4.upd:c.s": 3.27e-06, "upd4.upd:c.f": 3.94e-06, "upd4.hyp:d": 3.15e-05,
    "upd4.hyp:s": 3.14e-06, "upd4.hyp:f": 3.81e-06, "r1:d": 1.68e-05, "r1:s": 7.08e-06, "r1:f": 9.66e-06,
    "up_r1:d": 2.62e-05, "up_r1:s": 0, "up_r1:f": 0, "r05:d": 2.15e-05, "r05:s": 7.51e-06, "r05:f": 8.54e-06,
    "up_r05:d": 2.96e-05, "up_r05:s": 0, "up_r05:f": 0, "pred_disp": 1.7e-05,
}
# ... and the shipped constants: C_BOUND x that, three digits
BOUND = {
    "enc0": 6.5e-06, "enc1": 1.81e-05, "enc2": 1.37e-05, "enc3": 9.75e-06, "fea0": 7.05e-06, "fea0_img": 1.04e-05,
    "fea1": 5.64e-06, "fea2": 1.03e-05, "fea3": 1.93e-05, "fea4": 1.56e-05, "init0.tl": 2.99e-06,
    "init0.tr": 2.71e-06, "init0.cost": 1.42e-06, "init0.hyp:d": 0, "init0.hyp:s": 0, "init0.hyp:f": 1.66e-06,
    "init1.tl": 3.51e-06, "init1.tr": 4.93e-06, "init1.cost": 1.89e-06, "init1.hyp:d": 0, "init1.hyp:s": 0,
    "init1.hyp:f": 1.33e-06, "init2.tl": 5.9e-06, "init2.tr": 6.54e-06, "init2.cost": 2.73e-06, "init2.hyp:d": 0,
    "init2.hyp:s": 0, "init2.hyp:f": 2.36e-06, "init3.tl": 1.19e-05, "init3.tr": 1.4e-05, "init3.cost": 8e-06,
    "init3.hyp:d": 0, "init3.hyp:s": 0, "init3.hyp:f": 5.4e-06, "init4.tl": 8.92e-06, "init4.tr": 1.1e-05,
    "init4.cost": 7.66e-06, "init4.hyp:d": 0, "init4.hyp:s": 0, "init4.hyp:f": 4.27e-06, "upd0.aug:cvc": 3.77e-05,
    "upd0.upd:d": 6.91e-07, "upd0.upd:s": 9.97e-07, "upd0.upd:f": 1.22e-06, "upd0.hyp:d": 1.67e-06,
    "upd0.hyp:s": 9.97e-07, "upd0.hyp:f": 1.37e-06, "upd1.up:d": 8.35e-06, "upd1.up:s": 0, "upd1.up:f": 0,
    "upd1.aug:cvc": 3.76e-05, "upd1.aug:cvp": 8.75e-05, "upd1.upd:conf": 1.73e-06, "upd1.upd:p.d": 1.65e-06,
    "upd1.upd:p.s": 2.17e-06, "upd1.upd:p.f": 2.27e-06, "upd1.upd:c.d": 1.48e-06, "upd1.upd:c.s": 2.98e-06,
    "upd1.upd:c.f": 2.32e-06, "upd1.hyp:d": 1.1e-05, "upd1.hyp:s": 2.98e-06, "upd1.hyp:f": 2.24e-06,
    "upd2.up:d": 3.03e-05, "upd2.up:s": 0, "upd2.up:f": 0, "upd2.aug:cvc": 7.92e-05, "upd2.aug:cvp": 0.000173,
    "upd2.upd:conf": 4.63e-06, "upd2.upd:p.d": 5.62e-06, "upd2.upd:p.s": 5.05e-06, "upd2.upd:p.f": 6.12e-06,
    "upd2.upd:c.d": 4.68e-06, "upd2.upd:c.s": 5.98e-06, "upd2.upd:c.f": 7.36e-06, "upd2.hyp:d": 1.29e-05,
    "upd2.hyp:s": 5.98e-06, "upd2.hyp:f": 7.48e-06, "upd3.up:d": 5.59e-05, "upd3.up:s": 0, "upd3.up:f": 0,
    "upd3.aug:cvc": 8.19e-05, "upd3.aug:cvp": 0.000474, "upd3.upd:conf": 1.19e-05, "upd3.upd:p.d": 7.83e-06,
    "upd3.upd:p.s": 7.62e-06, "upd3.upd:p.f": 1.54e-05, "upd3.upd:c.d": 9.29e-06, "upd3.upd:c.s": 1.06e-05,
    "upd3.upd:c.f": 1.47e-05, "upd3.hyp:d": 4.34e-05, "upd3.hyp:s": 1.06e-05, "upd3.hyp:f": 1.51e-05,
    "upd4.up:d": 0.00012, "upd4.up:s": 0, "upd4.up:f": 0, "upd4.aug:cvc": 6.72e-05, "upd4.aug:cvp": 0.000638,
    "upd4.upd:conf": 1.4e-05, "upd4.upd:p.d": 1.39e-05, "upd4.upd:p.s": 1.43e-05, "upd4.upd:p.f": 1.88e-05,
    "upd4.upd:c.d": 1.39e-05, "upd4.upd:c.s": 1.63e-05, "upd4.upd:c.f": 1.97e-05, "upd4.hyp:d": 0.000158,
    "upd4.hyp:s": 1.57e-05, "upd4.hyp:f": 1.91e-05, "r1:d": 8.4e-05, "r1:s": 3.54e-05, "r1:f": 4.83e-05,
    "up_r1:d": 0.000131, "up_r1:s": 0, "up_r1:f": 0, "r05:d": 0.000107, "r05:s": 3.75e-05, "r05:f": 4.27e-05,
    "up_r05:d": 0.000148, "up_r05:s": 0, "up_r05:f": 0, "pred_disp": 8.49e-05,
}
# the chained fp64 restatement against oracle.stereo.stereo_matching(return_intermediates=True), both free running from
# the same images: one fp32 evaluation of the network against one fp64 evaluation, up to the first arg-min or select
# that the two take differently -- none on these cases: every init disparity and every select agrees.  Measured, worst
# over the cases and levels: U-Net (enc, fea) 5.3e-6; init tl / tr / cost / descriptor 2.0e-5; update hypotheses: disparity
# 3.9e-5, slopes and descriptor 7.4e-6; r1 / r05 and their up-samplings: disparity 9.7e-5, the rest 1.2e-5; pred_disp
# 9.7e-5 (disparities of up to 305).  The level asserted is 4 x that
ORACLE_LEVEL = dict(unet=2.2e-5, init=8.1e-5, upd_d=1.6e-4, upd_sf=3.0e-5, post_d=3.9e-4, post_sf=4.9e-5, pred_disp=3.9e-4)


# ------------------------------------------------------------------------------------------------ inputs
def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(left, right) [B,3,H,W] fp32: frame b of codd_amd.synth.stereo_sequence is item b (the second pair is the first
    one's texture shifted by the sequence's flow, under its own disparity field)."""
    from codd_amd import synth
    B, H, W = CASES[name]
    img, r_img, _ = synth.stereo_sequence(H, W, B)
    return img[0].contiguous(), r_img[0].contiguous()


STEREO_CFG = dict(type="HITNetMF", backbone=dict(type="HITUNet"),
                  initialization=dict(type="TileInitialization", max_disp=MAX_DISP),
                  propagation=dict(type="TilePropagation"))


@functools.lru_cache(maxsize=None)
def estimator():
    """(the stereo-only estimator on the host with the "random" filler at gain 1.4 of the headline tests, its state dict)"""
    import codd_amd  # noqa: F401
    from codd_amd import synth
    from codd_amd.registry import build_estimator
    est = build_estimator(dict(type="ConsistentOnlineDynamicDepth", stereo=STEREO_CFG)).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    return est, {k: v.clone() for k, v in est.state_dict().items()}


@functools.lru_cache(maxsize=None)
def weights(dtype):
    return {k: v.to(dtype) for k, v in estimator()[1].items() if k.startswith(P + ".")}


# ------------------------------------------------------------------------------------------------ the two backends
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class K32:
    """The fp32 CPU oracle's own functions."""
    dtype = torch.float32
    act = staticmethod(ost.lrelu)

    @staticmethod
    def conv(sd, key, x, stride=1, pad=0, dil=1, pad4=None):
        if pad4 is not None:  # (t, l, b, r) zeros in front of an unpadded convolution
            x, pad = F.pad(x, (pad4[1], pad4[3], pad4[0], pad4[2])), 0
        return ost.conv(sd, key, x, stride, pad, dil)

    deconv = staticmethod(ost.deconv2)

    @staticmethod
    def costvol(tl, tr, D):
        cost, d = ost.tile_cost_volume_min(tl, tr, D)
        return dict(cost=cost, arg=d, full=None)

    @staticmethod
    def warp(fl, fr, hyp):
        fea = ost.unshuffle4(fl.abs().sum(1, keepdim=True))
        return torch.cat([fea, ost.tile_warping(hyp[:, :3], fl, fr)], 1)

    @staticmethod
    def upsample(h, scale):
        return ost.upsample_hyp(h, scale, 2)

    @staticmethod
    def select(upd, cur, prv):
        sel = upd[:, :2].argmax(1, keepdim=True).float()  # ties -> 0 (= previous), as oracle.stereo.tile_update
        a, b = ost._relu_d(cur + upd[:, 18:34]), ost._relu_d(prv + upd[:, 2:18])
        return sel * a + (1 - sel) * b, sel > 0


class K64:
    """fp64: conv_fp64's tap loops, stereo_fusion_fp64's kernel references."""
    dtype = F64

    @staticmethod
    def act(v):
        return torch.where(v > 0, v, 0.2 * v)

    @staticmethod
    def conv(sd, key, x, stride=1, pad=0, dil=1, pad4=None):
        w, b = sd[key + ".weight"], sd.get(key + ".bias")
        stride, dil = _pair(stride), _pair(dil)
        p4 = pad4 if pad4 is not None else (_pair(pad)[0], _pair(pad)[1]) * 2
        kh, kw = w.shape[2:]
        out_hw = ((x.shape[2] + p4[0] + p4[2] - dil[0] * (kh - 1) - 1) // stride[0] + 1,
                  (x.shape[3] + p4[1] + p4[3] - dil[1] * (kw - 1) - 1) // stride[1] + 1)
        lin = CV._taps(x.to(F64), w.to(F64), stride, p4, dil, out_hw)
        return lin if b is None else lin + b.to(F64).view(1, -1, 1, 1)

    @staticmethod
    def deconv(sd, key, x):
        lin = CV._deconv_taps(x.to(F64), sd[key + ".weight"].to(F64))
        b = sd.get(key + ".bias")
        return lin if b is None else lin + b.to(F64).view(1, -1, 1, 1)

    @staticmethod
    def costvol(tl, tr, D):
        ref = SF.costvol(tl, tr, D)
        return dict(cost=ref["cost"][:, None], arg=ref["arg"][:, None].to(F64), full=ref)

    @staticmethod
    def warp(fl, fr, hyp):
        return SF.tile_warp(fl, fr, hyp)[0]

    @staticmethod
    def upsample(h, scale):
        return SF.hyp_upsample(h, scale)[0]

    @staticmethod
    def select(upd, cur, prv):
        v, _, sel = SF.hyp_select(upd, cur, prv)
        return v, sel


# ------------------------------------------------------------------------------------------------ the stages
def _relu_d(h, every=False):
    return F.relu(h) if every else torch.cat([F.relu(h[:, :1]), h[:, 1:]], 1)


def _resblock(k, sd, key, x, dil=1):
    t = k.act(k.conv(sd, key + ".0.conv1.0.0", x, 1, dil, dil))
    return k.act(k.conv(sd, key + ".0.conv2.0", t, 1, dil, dil) + x)


def s_enc(k, sd, j, x):
    """Encoder skip j of HITUNet: j = 0: the image -> x0; j = 1..3: x_{j-1} -> x_j (reference backbone.py:69-77)."""
    p = P + ".backbone"
    if j == 0:
        return k.act(k.conv(sd, f"{p}.conv1.0", x, 1, 1))
    t = k.act(k.conv(sd, f"{p}.down{j}.0", x, 2, 1))
    return k.act(k.conv(sd, f"{p}.down{j}.2", t, 1, 1))


def s_fea0(k, sd, x3):
    """Backbone scale 0 (1/16) from the last skip."""
    p = P + ".backbone.down4"
    t = k.act(k.conv(sd, p + ".0.0", x3, 2, 1))
    for key in (".0.2", ".1", ".3"):
        t = k.act(k.conv(sd, p + key, t, 1, 1))
    return t


def s_fea(k, sd, i, prev, skip):
    """Backbone scale i = 1..4 from scale i - 1 and encoder skip 4 - i (reference backbone.py:78-88)."""
    n, p = 5 - i, P + ".backbone"
    u = k.act(k.deconv(sd, f"{p}.up{n}.0", prev))
    t = k.act(k.conv(sd, f"{p}.merge{n}.0", torch.cat((skip, u), 1)))
    t = k.act(k.conv(sd, f"{p}.merge{n}.2", t, 1, 1))
    return k.act(k.conv(sd, f"{p}.merge{n}.4", t, 1, 1))


def s_init(k, sd, lvl, fl, fr, feat, tl_tr=None, pick=None, variant=None):
    """init_level ``lvl`` (reference initialization.py:119-225) -> dict(tl, tr, cost, hyp, full).  ``tl_tr``: the tile
    features that the cost volume and the descriptor are formed from (None: this stage's own); ``pick`` [B,Ht,Wt]
    (K64 only): cost and hypothesis at that disparity instead of the arg-min; full: stereo_fusion_fp64.costvol's dict."""
    name, p = LEVELS[lvl], P + ".tile_init"
    kc = f"{p}.tile_conv{name}"
    tl = k.act(k.conv(sd, kc + ".2", k.act(k.conv(sd, kc + ".0", fl, 4, 0))))
    pad4 = (0, 3, 0, 0) if variant == "pad_left" else (0, 0, 0, 3)
    tr = k.act(k.conv(sd, kc + ".2", k.act(k.conv(sd, kc + ".0", fr, (4, 1), 0, pad4=pad4))))
    a, b = (tl, tr) if tl_tr is None else (tl_tr[0].to(k.dtype), tl_tr[1].to(k.dtype))
    cv = k.costvol(a, b, MAX_DISP if variant == "max_disp" else MAX_DISP // (16 >> lvl))
    cost, d = cv["cost"], cv["arg"]
    if pick is not None:  # (a pick outside the search is a finding of deviations(); here it only must not index past the volume)
        pick = pick.long().clamp(0, cv["full"]["cv"].shape[1] - 1)
        d = pick[:, None].to(k.dtype)
        cost = cv["full"]["cv"].gather(1, pick[:, None])
    f = a if lvl < 2 else feat
    if variant == "dsc_tl" and lvl >= 2:
        f = torch.cat([a, torch.zeros_like(feat[:, 16:])], 1)
    dsc = k.act(k.conv(sd, f"{p}.tile_fea_dscrpt{name}.0", torch.cat([cost, f], 1)))
    z = torch.zeros_like(d)
    return dict(tl=tl, tr=tr, cost=cost, hyp=torch.cat([d, z, z, dsc], 1), full=cv["full"])


def s_update(k, sd, i, fl, fr, hyp, prev=None, variant=None):
    """TileUpdate0 (i = 0) / TileUpdate (i = 1..4), reference propagation.py:124-248 -> dict(aug, upd, hyp) and for
    i >= 1 also up, sel (bool, conf1 > conf0 picks the current hypothesis), cur, prv (both refined candidates)."""
    p = f"{P}.tile_update.tile_update{i}"
    if variant == "lr_swap":
        fl, fr = fr, fl
    w0 = k.warp(fl, fr, hyp)
    cvc = k.act(k.conv(sd, p + ".decrease.0", w0))
    out = {}
    if i == 0:
        aug = torch.cat([hyp, cvc], 1)
    else:
        up = k.upsample(prev, 1.0 if variant == "up_scale1" else 2.0)
        cvp = k.act(k.conv(sd, p + ".decrease.0", w0 if variant == "cvp_from_cur" else k.warp(fl, fr, up)))
        aug = torch.cat([hyp, cvc, up, cvp], 1)
        out["up"] = up
    t = k.act(k.conv(sd, p + ".conv0.0", aug))
    t = _resblock(k, sd, p + ".resblock0", t)
    t = _resblock(k, sd, p + ".resblock1", t)
    upd = k.conv(sd, p + ".lastconv", t, 1, 1)
    out.update(aug=aug, upd=upd)
    if i == 0:
        out["hyp"] = _relu_d(hyp + upd, variant == "relu_all")
        return out
    u = upd
    if variant == "conf_swap":
        u = torch.cat([u[:, 1:2], u[:, 0:1], u[:, 2:]], 1)
    if variant == "upd_swap":
        u = torch.cat([u[:, :2], u[:, 18:34], u[:, 2:18]], 1)
    out["hyp"], out["sel"] = k.select(u, hyp, up)
    out["cur"], out["prv"] = _relu_d(hyp + u[:, 18:34]), _relu_d(up + u[:, 2:18])
    return out


def s_post(k, sd, name, fl, prev, variant=None):
    """PostTileUpdate (tile_update4_1, tile_update5) / FinalTileUpdate (tile_update6: -> [B,1,H,W]), reference
    propagation.py:251-333."""
    p = f"{P}.tile_update.{name}"
    final = name == "tile_update6"
    t = k.act(k.conv(sd, p + ".conv1.0", torch.cat([fl, prev], 1)))
    t = k.act(k.conv(sd, p + ".conv1.2", t, 1, 1))
    for i in range(2 if final else 4):
        t = _resblock(k, sd, f"{p}.resblocks.{i}", t, 3 if (i == 1 and not final and variant != "dil1") else 1)
    t = k.conv(sd, p + ".lastconv", t, 1, 1)
    if final:
        ch = 1 if variant == "final_ch1" else 0
        return F.relu(prev[:, ch:ch + 1] + t)[:, 0:1]
    return _relu_d(prev + t, variant == "relu_all")


def evaluate(k, sd, left, right, T=None, variant=None):
    """Every stage of the network over backend ``k`` -> a flat dict: enc0..3, fea0..4, fea0_img (scale 0 from the images
    alone), init{l}.tl/.tr/.cost/.hyp, upd{l}.aug/.upd/.hyp (l >= 1: .up too), r1, up_r1, r05, up_r05, pred_disp, and
    under a leading "_": _init{l}.full, _upd{l}.sel/.cur/.prv.  ``T`` None: free running (each stage from the previous
    stages' results: the network).  ``T`` a flat dict of the same names (the oracle's trajectory, or the product's
    trace): TEACHER-FORCED -- each stage from T's values of its inputs, the cost volume from T's tile features, cost and
    hypothesis of init at T's pick (K64).  ``variant``: one planted wiring error of VARIANTS."""
    B = left.shape[0]
    x = torch.cat([left, right], 0).to(k.dtype)
    R = {}
    src = R if T is None else T
    g = lambda q: src[q].to(k.dtype)
    L, Rt = (lambda i: g(f"fea{i}")[:B]), (lambda i: g(f"fea{i}")[B:])

    def views(fn, *ts):  # K32: each view through the U-Net on its own, as the oracle runs it (F.conv2d's bits depend on the batch)
        return fn(*ts) if k is not K32 else torch.cat([fn(*(t[:B] for t in ts)), fn(*(t[B:] for t in ts))], 0)

    e = x
    for j in range(4):
        if T is not None:
            e = views(lambda t: s_enc(k, sd, j, t), e)
        R[f"enc{j}"] = views(lambda t: s_enc(k, sd, j, t), x if j == 0 else g(f"enc{j - 1}"))
    R["fea0"] = views(lambda t: s_fea0(k, sd, t), g("enc3"))
    R["fea0_img"] = views(lambda t: s_fea0(k, sd, t), e) if T is not None else R["fea0"]
    for i in range(1, 5):
        R[f"fea{i}"] = views(lambda t, u: s_fea(k, sd, i, t, u), g(f"fea{i - 1}"), g(f"enc{4 - i}"))
    for lvl in range(5):
        forced = T is not None
        o = s_init(k, sd, lvl, L(lvl), Rt(lvl), L(lvl - 2) if lvl >= 2 else None,
                   (T[f"init{lvl}.tl"], T[f"init{lvl}.tr"]) if forced else None,
                   T[f"init{lvl}.hyp"][:, 0] if forced and k is K64 and variant is None else None, variant)
        for q in ("tl", "tr", "cost", "hyp"):
            R[f"init{lvl}.{q}"] = o[q]
        R[f"_init{lvl}.full"] = o["full"]
    for i in range(5):
        o = s_update(k, sd, i, L(i), Rt(i), g(f"init{i}.hyp"), g(f"upd{i - 1}.hyp") if i else None,
                     variant if variant != "lr_swap" or i == 2 else None)
        for q, v in o.items():
            R[("_" if q in ("sel", "cur", "prv") else "") + f"upd{i}.{q}"] = v
    R["r1"] = s_post(k, sd, "tile_update4_1", L(2), g("upd4.hyp"), variant)
    R["up_r1"] = k.upsample(g("r1"), 1.0)
    R["r05"] = s_post(k, sd, "tile_update5", L(3), g("up_r1"), variant)
    R["up_r05"] = k.upsample(g("r05"), 1.0)
    R["pred_disp"] = s_post(k, sd, "tile_update6", L(4), g("up_r05"), variant)
    return R


def oracle_world(name, single_thread=False):
    return _world(name, bool(single_thread))


@functools.lru_cache(maxsize=None)
def _world(name, single_thread):
    """Case ``name`` on the host, computed once: dict(left, right, T32 = the stages chained over the oracle's functions
    (the oracle's fp32 trajectory), R64 = every stage in fp64 from T32's values of its inputs).  ``single_thread``: the
    oracle's trajectory on ONE host thread (F.conv2d sums in another order there: another fp32 evaluation)."""
    left, right = inputs(name)
    with torch.no_grad():
        torch.set_num_threads(1) if single_thread else _threads()
        try:
            T32 = evaluate(K32, weights(torch.float32), left, right)
        finally:
            _threads()
        R64 = evaluate(K64, weights(F64), left, right, T32)
    return dict(left=left, right=right, T32=T32, R64=R64)


# ------------------------------------------------------------------------------------------------ comparison
HYP_GROUPS = (("d", slice(0, 1)), ("s", slice(1, 3)), ("f", slice(3, 16)))


def groups(q, C):
    """The channel groups (suffix, slice) that quantity ``q`` with C channels is normalised by."""
    kind = q.split(".")[-1]
    if kind == "aug":  # the hypothesis slices are compared bit for bit with their producers (GPU test); the cost slices here
        return (("cvc", slice(16, 32)),) + ((("cvp", slice(48, 64)),) if C == 64 else ())
    if kind == "upd" and C == 34:
        return (("conf", slice(0, 2)),) + tuple((f"{w}.{n}", slice(o + s.start, o + s.stop))
                                                 for w, o in (("p", 2), ("c", 18)) for n, s in HYP_GROUPS)
    if C == 16 and kind in ("hyp", "up", "upd", "r1", "up_r1", "r05", "up_r05"):
        return HYP_GROUPS
    return (("", slice(None)),)


def quantities():
    """The traced quantities that a bound is set for, in stage order."""
    qs = [f"enc{j}" for j in range(4)] + ["fea0", "fea0_img"] + [f"fea{i}" for i in range(1, 5)]
    for lvl in range(5):
        qs += [f"init{lvl}.{q}" for q in ("tl", "tr", "cost", "hyp")]
    for i in range(5):
        qs += [f"upd{i}.{q}" for q in (("up",) if i else ()) + ("aug", "upd", "hyp")]
    return qs + ["r1", "up_r1", "r05", "up_r05", "pred_disp"]


def traced_name(q):
    return "fea0" if q == "fea0_img" else q


def select_rule(got, R, i, conf_bound):
    """TileUpdate i's select (module docstring) -> (ref hypothesis with the other candidate on the excused tiles,
    excused count, un-excused count).  ``got``: the flat dict that holds the picks under test (upd{i}.upd)."""
    u = got[f"upd{i}.upd"]
    sel_got = u[:, 1:2] > u[:, 0:1]
    ref_u = R[f"upd{i}.upd"]
    sel_ref = R[f"_upd{i}.sel"]
    diff = sel_got != sel_ref
    near = (ref_u[:, 0:1] - ref_u[:, 1:2]).abs() <= 2 * conf_bound
    ref = torch.where(sel_got, R[f"_upd{i}.cur"], R[f"_upd{i}.prv"])
    return ref, int((diff & near).sum()), int((diff & ~near).sum())


def near_select_count(R, i, conf_bound):
    """The reference alone: tiles whose |conf0 - conf1| lies within 2 x the confidence bound."""
    ref_u = R[f"upd{i}.upd"]
    return int(((ref_u[:, 0] - ref_u[:, 1]).abs() <= 2 * conf_bound).sum())


def deviations(got, R, bound=None):
    """got (a flat dict of fp32 tensors: the oracle's trajectory, or the product's trace) against R = evaluate(K64, ...,
    T=got) -> (dev {"q:group": max |got - ref|}, info).  The init hypothesis' disparity is judged by
    stereo_fusion_fp64.argmin_check (info["argmin"][lvl] = its dict), the select by select_rule (which needs ``bound``,
    default BOUND: info["select"][i] = (excused, un-excused)); a tile that is wrong without excuse counts as inf."""
    bound = BOUND if bound is None else bound
    dev, info = {}, dict(argmin={}, select={})
    for q in quantities():
        ref, x = R[q], got[traced_name(q)].to(F64)
        assert ref.shape == x.shape, (q, ref.shape, x.shape)
        if q.startswith("init") and q.endswith(".hyp"):
            lvl = int(q[4])
            full, d = R[f"_init{lvl}.full"], x[:, 0]
            outside = (d != d.round()) | (d < 0) | (d >= full["cv"].shape[1])
            if outside.any():  # not an integer of the search range at all
                chk = dict(cost=float("inf"), near=0.0, wrong=int(outside.sum()), where=None)
            else:
                chk = SF.argmin_check(full, got[f"init{lvl}.cost"][:, 0], d, SF.C["costvol"])
            info["argmin"][lvl] = chk
            if chk["wrong"] or not torch.equal(ref[:, 0], x[:, 0]):  # (ref[:, 0] is the pick where R was evaluated at it)
                dev[q + ":d"] = float("inf")
        if q.startswith("upd") and q.endswith(".hyp") and q[3] != "0":
            i = int(q[3])
            ref, ex, wrong = select_rule(got, R, i, bound.get(f"upd{i}.upd:conf", 0.0))
            info["select"][i] = (ex, wrong)
            if wrong:
                dev[q + ":d"] = float("inf")
        for gname, sl in groups(q, ref.shape[1]):
            key = q + (":" + gname if gname else "")
            err = (x[:, sl] - ref[:, sl]).abs()
            err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err).max().item()
            dev[key] = max(dev.get(key, 0.0), err)
    return dev, info


def ratios(dev, bound=None):
    """err / bound per key (to be <= 1); 0 / 0 = 0, x / 0 = inf."""
    bound = BOUND if bound is None else bound
    return {k: (0.0 if v == 0 else (v / bound[k] if bound[k] > 0 else float("inf"))) for k, v in dev.items()}


def tiles(name, first=0):
    """The number of tiles of levels first .. 4 of case ``name``, all items."""
    B, H, W = CASES[name]
    return sum(B * (H >> (6 - l)) * (W >> (6 - l)) for l in range(first, 5))


def flatten(trace):
    """The product's trace (list of dicts) -> the flat dict of evaluate's names, tensors on the host."""
    T = {}
    for e in trace:
        st, lvl = e["stage"], e["level"]
        for k, v in e.items():
            if not torch.is_tensor(v):
                continue
            if st in ("enc", "fea"):
                name = f"{st}{lvl}"
            elif st == "init":
                name = f"init{lvl}.{k}"
            elif st == "update":
                name = f"upd{lvl}.{k}"
            else:
                name = st
            assert name not in T, name
            T[name] = v.detach().cpu()
    return T


def measure(names=None):
    """D per key over the cases ``names`` (default: all) -> (D, info per case): the oracle's trajectory T32 against
    every stage in fp64 from T32's values.  The select rule needs the confidence bound, which is itself measured: a first
    pass with bound 0 (every differing select counts as wrong), a second one with C_BOUND x the first pass' confidence D.
    Each case twice: the oracle on the host's threads (at most 16) and on one thread -- the summation order of its
    convolutions follows the thread count (the same bits on 4, 8 and 32 threads, others on 1: single keys move by up to
    1.6 x), and the worst of the two is what a host with any number of threads re-measures within the asserted window."""
    D, infos = {}, {}
    for name in (names or CASES):
        for single in (False, True):
            w = oracle_world(name, single)
            dev, _ = deviations(w["T32"], w["R64"], bound={})
            conf = {k: C_BOUND * v for k, v in dev.items() if k.endswith(":conf")}
            dev, infos[name + (" (1 thread)" if single else "")] = deviations(w["T32"], w["R64"], bound=conf)
            for k, v in dev.items():
                D[k] = max(D.get(k, 0.0), v)
    return D, infos
