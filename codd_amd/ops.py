"""Tensor-level wrappers over the C ABI (include/codd_hip.h).

PyTorch is used for device memory and streams only; every computation below is a call into
libcodd_hip.so.  There is no CPU / eager fallback: tensors must live on a ROCm device.
"""
import collections
import ctypes as C
import functools

import numpy as np
import torch

from . import _abi
from ._abi import ACT, ConvParams, View


class RuntimeState:
    """Mixin of the plug-in modules that keep launch-time objects (side streams, fork helpers, pending prefetches,
    captured frame graphs) in their ``__dict__``: those are neither picklable nor copyable and are rebuilt on demand,
    so they are left out of the module's pickled / deep-copied state."""
    _RUNTIME_KEYS = ("_side", "_pending", "_nowait", "_fk", "_xs", "_runners", "_kside", "_h4c", "_ctx4c", "_fused_now", "_pipe")

    def __getstate__(self):
        state = self.__dict__.copy()
        for k in self._RUNTIME_KEYS:
            state.pop(k, None)
        return state


class Slice:
    """Channels [coff, coff + c) of a contiguous NCHW buffer."""
    __slots__ = ("buf", "coff", "c")

    def __init__(self, buf, coff=0, c=None):
        assert buf.is_contiguous() and buf.dtype == torch.float32
        self.buf, self.coff = buf, coff
        self.c = buf.shape[1] - coff if c is None else c

    @property
    def shape(self):
        return (self.buf.shape[0], self.c) + tuple(self.buf.shape[2:])

    def tensor(self):
        return self.buf[:, self.coff:self.coff + self.c]


def _as_slice(x):
    return x if isinstance(x, Slice) else Slice(x)


def _view(x):
    if x is None:
        return View(None, 0, 0)
    s = _as_slice(x)
    return View(s.buf.data_ptr(), s.buf.shape[1], s.coff)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _require_gpu(t):
    if not t.is_cuda:
        raise _abi.CoddHipError("codd_amd ops run on a ROCm device only (no CPU fallback in the product path)")


# ----------------------------------------------------------------------------------------- conv
class PackedConv:
    """Weights of one Conv2d / ConvTranspose2d(k2,s2) re-laid-out for the MFMA kernel."""

    def __init__(self, weight, bias, deconv=False, cout_keep=None):
        _require_gpu(weight)
        w = weight.detach().float()
        b = None if bias is None else bias.detach().float().contiguous()
        if deconv:  # [Cin, Cout, 2, 2] -> 1x1 conv with 4*Cout outputs, co' = (a*2+b)*Cout + co
            cin, cout = w.shape[:2]
            w = w.permute(2, 3, 1, 0).reshape(4 * cout, cin, 1, 1)
            self.cout = cout
        else:
            if cout_keep is not None:
                w = w[:cout_keep]
                b = None if b is None else b[:cout_keep].contiguous()
            self.cout = w.shape[0]
        w = w.contiguous()
        self.deconv = deconv
        self.cout_eff, self.cin, self.kh, self.kw = w.shape
        self.bias = b
        # 16-channel blocks per workgroup: 64-channel groups only for wide layers that fill them
        # exactly (measured: 96->96 3x3 87 us at mb=2 vs 116 us at mb=4)
        self.mb = 1 if self.cout_eff <= 16 else (4 if (self.cout_eff >= 256 and self.cout_eff % 64 == 0) else 2)
        self._w = w
        self._packs = {}
        self.tuned = {}  # launch shape -> stored launch configuration (decode_cfg)

    def packed(self, ck, mb=None, layout=0):
        """layout 0 / 1: fp32 kernels; 20 + terms (21 | 23): split-bf16 kernel with 1 | 3 product terms."""
        mb = self.mb if mb is None else mb
        if (mb, ck, layout) not in self._packs:
            if layout >= 20:
                wp = _pack_bf16(self._w, self.cout_eff, self.cin, self.kh, self.kw, mb, ck, layout - 20,
                                self.cin * self.kh * self.kw, self.kh * self.kw, 1.0)
            else:
                lib = _abi.load()
                size, pack = ((lib.codd_conv2d_packed_size_quad, lib.codd_conv2d_pack_weights_quad) if layout == 1 else
                              (lib.codd_conv2d_packed_size, lib.codd_conv2d_pack_weights))
                n = size(self.cout_eff, self.cin, self.kh, self.kw, mb, ck)
                if n <= 0:
                    raise _abi.CoddHipError("no packed layout %d for ck=%d mb=%d" % (layout, ck, mb))
                wp = torch.empty(n, device=self._w.device, dtype=torch.float32)
                _abi.check(pack(self._w.data_ptr(), wp.data_ptr(), self.cout_eff, self.cin, self.kh, self.kw, mb, ck,
                                _stream()), "pack_weights")
            self._packs[(mb, ck, layout)] = wp
        return self._packs[(mb, ck, layout)]

    def _pack_key(self, c):
        f = decode_cfg(c, self.mb)
        return (f.mb, f.ck, 20 + f.terms if f.layout == 2 else f.layout)

    def drop_unused_packs(self, keep=None):
        """Free the packed-weight variants that neither a tuned configuration nor ``keep`` refers to (after autotuning)."""
        used = {self._pack_key(c) for c in list(self.tuned.values()) + ([keep] if keep is not None else [])}
        for k in [k for k in self._packs if k not in used]:
            del self._packs[k]


def _pack_bf16(w, cout, cin, kh, kw, mb, ck, terms, co_stride, ci_stride, scale):
    """codd_conv2d_pack_weights_bf16 of the fp32 weights ``w`` ([co][ci][tap] at the given strides) -> a new byte tensor."""
    lib = _abi.load()
    n = lib.codd_conv2d_packed_bytes_bf16(cout, cin, kh, kw, mb, ck, terms)
    if n <= 0:
        raise _abi.CoddHipError("no split-bf16 packed layout for ck=%d mb=%d terms=%d" % (ck, mb, terms))
    wp = torch.empty(n, device=w.device, dtype=torch.uint8)
    _abi.check(lib.codd_conv2d_pack_weights_bf16(w.data_ptr(), wp.data_ptr(), cout, cin, kh, kw, mb, ck, terms, co_stride,
                                                 ci_stride, scale, _stream()), "pack_weights_bf16")
    return wp


# A launch configuration is stored (pc.tuned, TUNE_DB, codd_amd/tuned/mi355x.json, AUTOTUNE_LOG) as a plain tuple:
#   exact fp32   (npb, nw, ck[, mb[, layout]])                     layout 0 | 1, mb defaults to PackedConv.mb
#   split-bf16   (xb, th, ck, mb, 2, pgw, cgw[, terms[, ksplit]])  terms defaults to the launch's, ksplit to 1
# decode_cfg names the fields after codd_conv_params (for layout 2 the header's npb = xb, nw = th); the stored tuples
# themselves are never replaced by decoded ones.
LaunchCfg = collections.namedtuple("LaunchCfg", "npb nw ck mb layout pgw cgw terms ksplit")


def decode_cfg(c, mb=None, terms=None):
    """Named fields of a stored launch configuration ``c``; ``mb`` / ``terms``: the defaults of the short forms
    (PackedConv.mb, the launch's terms).  fp32 configurations have pgw = cgw = terms = ksplit = None."""
    if len(c) > 4 and c[4] == 2:
        if not 7 <= len(c) <= 9:
            raise ValueError("split-bf16 launch configuration of %d fields: %r" % (len(c), tuple(c)))
        return LaunchCfg(c[0], c[1], c[2], c[3], 2, c[5], c[6], c[7] if len(c) > 7 else terms, c[8] if len(c) > 8 else 1)
    if not 3 <= len(c) <= 5 or (len(c) > 4 and c[4] not in (0, 1)):
        raise ValueError("not an exact-fp32 launch configuration: %r" % (tuple(c),))
    return LaunchCfg(c[0], c[1], c[2], c[3] if len(c) > 3 else mb, c[4] if len(c) > 4 else 0, None, None, None, None)


def _set_cfg(p, c, pc=None):
    """Write launch configuration ``c`` into ``p``; with ``pc`` also its packed weights (split-bf16: packed for p.terms;
    exact fp32: p.terms = 0).  Fields of the other family are left as they are."""
    f = decode_cfg(c, None if pc is None else pc.mb, p.terms)
    if f.layout == 2:
        if pc is not None:
            p.wpacked = pc.packed(f.ck, f.mb, 20 + p.terms).data_ptr()
        p.pgw, p.cgw, p.ksplit = f.pgw, f.cgw, f.ksplit
    else:
        if pc is not None:
            p.wpacked = pc.packed(f.ck, f.mb, f.layout).data_ptr()
        p.terms = 0
    p.mb, p.npb, p.nw, p.ck, p.layout = f.mb, f.npb, f.nw, f.ck, f.layout


def _launch_conv(lib, p, stream):
    """Single choke point of every conv launch (bench.py wraps it with HIP events)."""
    return lib.codd_conv2d(C.byref(p), stream)


import os as _os
_FORCE_NW = 0  # (tests: a workgroup height the heuristic may not pick)


def _pick_nw(pc, npb, Hout, Wout, B, ncog):
    """Waves (= 16-pixel tile rows) per workgroup: 4, or 9 where that removes a nearly empty last round.
    The 256 CUs take workgroups round-robin, so a launch lasts about ceil(grid / 256) rounds of nw rows;
    the 72-row GRU maps with 4 channel groups give 576 blocks = 3 rounds x 4 rows with nw = 4 and 256 blocks
    = 1 round x 9 rows with nw = 9 (measured 88 -> 82, 165 -> 153, 133 -> 125 us on the 128/256/196 -> 256
    3x3 layers; tools/time_conv_sweep.py).  Only for the plain 4x16 tile with >= 32 channels per group."""
    if _FORCE_NW:
        return _FORCE_NW if npb == 1 else 4
    if npb != 1 or pc.mb < 2 or Hout * Wout > 16384:
        return 4
    tx = -(-Wout // 16)
    cost = {nw: -(-(-(-Hout // nw) * tx * ncog * B) // 256) * nw for nw in (4, 9)}
    return 9 if cost[9] * 1.2 <= cost[4] else 4


def _conv_cfg(pc, Hout, Wout, B, sy, sx, dy, dx, pl):
    """(npb, nw, ck): tile shape per wave, waves per workgroup and LDS chunk depth.

    Measured on MI355X (tools/time_ops.py): the small 4x16-pixel tile (npb = 1) wins on every
    layer with more than 16 output channels -- the kernel is latency / barrier bound, so more
    resident workgroups beat operand re-use; 16-channel layers prefer 4x32.  The LDS chunk is the deepest
    the library accepts (codd_conv2d_lds_bytes: the register staging of the instantiated kernels) whose LDS
    lets the whole grid be resident at once when possible (a 576-block grid at 2 blocks/CU runs
    a second, nearly empty round: 112 us vs 67 us for 504 blocks)."""
    lib = _abi.load()
    ncog = -(-pc.cout_eff // (16 * pc.mb))
    npb = 2 if pc.cout_eff <= 16 else 1
    nw = _pick_nw(pc, npb, Hout, Wout, B, ncog)
    xb = 2 if npb >= 2 else 1
    th, tw = nw * (npb // xb), 16 * xb
    grid = (-(-Hout // th)) * (-(-Wout // tw)) * ncog * B
    per_cu = min(max(-(-grid // 256), 2 if nw == 4 else 1), 4)
    budget = min(64 * 1024, (160 * 1024) // per_cu - 512)
    # (a dry run: the input size is no part of the launch geometry of layout 0)
    p = _conv_params(pc, B, pc.cin, 0, 0, 0, Hout, Wout, (sy, sx), (pl, pl), (dy, dx))
    ck = min(-(-pc.cin // 4) * 4, 32)
    while ck > 4:
        _set_cfg(p, (npb, nw, ck, pc.mb, 0))
        if 0 <= lib.codd_conv2d_lds_bytes(C.byref(p)) <= budget:
            break
        ck -= 4
    return npb, nw, ck


# Arithmetic of the convolution family (include/codd_hip.h, codd_conv_params.layout / terms):
#   "split" (default)  split-bf16 operands, three bf16 MFMAs per product, fp32 accumulate (fp32-grade: the parity
#                      tests at the benchmarked configurations bound its effect on the disparities)
#   "fp32"             exact-fp32 MFMA kernels (v_mfma_f32_16x16x4_f32)
#   "bf16"             bf16 operands, fp32 accumulate (BASELINE.json configs[4]; reference auto_fp16 hook)
#   "split16"          split-FP16 operands (hi | lo IEEE fp16 planes, three v_mfma_f32_16x16x32_f16 per product): the split
#                      scheme with 22-bit operands, products to ~2^-22 -- fp32's own grade -- at the same MFMA rate as
#                      "split" (16-bit operands, 2^-17); fp16's range applies (|x| <= 65504)
#   "fp16"             IEEE fp16 operands (v_mfma_f32_16x16x32_f16), fp32 accumulate: the reference's own reduced
#                      precision (auto_fp16 IS .half(), model/codd.py:37,128): 11 mantissa bits at bf16's MFMA rate
CONV_PRECISION = "split"  # set through set_conv_precision() / bench.py --precision, never through the environment
_TERMS = dict(split=3, bf16=1, fp16=16, split16=48)  # codd_conv_params.terms (CODD_TERMS_*)


# "bf16" / "fp16" with BF16_STAGE_POLICY on ("bf16mix" / "fp16mix" in bench.py / set_conv_precision): the stages of
# _STAGE_PRECISION keep their exact-fp32 kernels (HITNet, whose output IS the disparity, the context network, Fusion) and
# only RAFT3D's feature encoder and its 16 update iterations -- 85 % of the frame's convolution FLOPs -- run on plain
# bf16 / fp16 operands.
BF16_STAGE_POLICY = False
_HALF_MODES = ("bf16", "fp16")  # one 16-bit operand plane, one MFMA per product
_MODES = ("split", "split16", "fp32", "bf16", "bf16mix", "fp16", "fp16mix")
_SPLIT_MODES = ("split", "split16")  # three MFMAs per product on hi | lo operand planes: the fp32-grade modes


def _split_terms():
    """terms of the all-pairs GEMMs / forced-split re-layouts under the current mode (3 | 48)"""
    return _TERMS["split16"] if CONV_PRECISION == "split16" else 3


def set_conv_precision(mode):
    """-> the previous mode (pass it back to restore).  "bf16mix" / "fp16mix" = "bf16" / "fp16" + the stage policy.
    Range caveat of the fp16 formats ("fp16", "split16", "fp16mix"): IEEE fp16 records saturate to +-inf above 65504 and lo parts
    below ~6e-8 flush to zero; plain "fp16" / "split16" apply to EVERY stage including HITNet (whose channels carry raw
    disparities), "fp16mix" only to RAFT3D's feature encoder and update block (O(1) activations) -- the supported use.  Nothing
    guards against overflow at run time except ``FrameRunner(check_finite=True)`` (debug) and the parity tests."""
    global CONV_PRECISION, BF16_STAGE_POLICY
    if mode not in _MODES:
        raise ValueError("conv precision must be one of %s" % (_MODES,))
    prev = CONV_PRECISION + "mix" if CONV_PRECISION in _HALF_MODES and BF16_STAGE_POLICY else CONV_PRECISION
    CONV_PRECISION, BF16_STAGE_POLICY = (mode[:-3], True) if mode.endswith("mix") else (mode, False)
    return prev


# Stage policy under the default "split" mode.  Measured on MI355X (tools/debug_split_layers.py, headline parity tests):
# a split-bf16 conv is accurate to ~1e-5 of its OUTPUT SCALE.  HITNet's propagation layers carry raw disparities
# (~100 px) in their input channels and emit the disparity itself, so 1e-5 relative is ~1e-3 px absolute -- the whole
# north-star budget -- and its arg-min / arg-max selections flip for ~1.5 % of the pixels; the stereo network
# (7 % of the frame's conv FLOPs) therefore stays on the exact-fp32 kernels, everything else (RAFT3D encoders and the
# 16 update iterations: ~90 % of the FLOPs, O(1) feature scales, smooth outputs) runs split-bf16.
# Round 4: Fusion as well.  Over the configured sequence length (tests/test_gpu_headline_parity.py::
# test_recurrent_sequence_matches_oracle, 16 frames) the split-bf16 error of Fusion's weight path is multiplied by
# |pred_warp - pred_curr| (up to 250 px with the synthetic weights, whose weight-head logits saturate the sigmoid): from
# frame 6 on isolated 4x4 blocks take the other side of a 0 | 1 fusion weight and the all-pixel mean leaves the 1e-3 px
# budget (6.6e-3 ... 1.5e-2 px); with Fusion's ~10 quarter-resolution layers on the exact-fp32 kernels frames 0-13 stay
# at <= 1e-4 px (profiles/r04_sequence_divergence.log).  (`_STAGE_PRECISION["fusion"] = "split"` restores the round-3 policy.)
_STAGE_PRECISION = dict(stereo="fp32", context="fp32", fusion="fp32")


class stage:
    """``with ops.stage("stereo"): ...`` -- conv precision of a pipeline stage (only the "split" default is refined;
    explicit "fp32" / "bf16" modes apply to every stage)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = None
        if self.name in _STAGE_PRECISION and (CONV_PRECISION in _SPLIT_MODES or (CONV_PRECISION in _HALF_MODES and BF16_STAGE_POLICY)):
            to = _STAGE_PRECISION[self.name]
            if to != "split" or CONV_PRECISION == "split":  # (a "split" stage under bf16mix stays bf16)
                self.prev = set_conv_precision(to)

    def __exit__(self, *exc):
        if self.prev is not None:
            set_conv_precision(self.prev)
        return False


# Launch-configuration hint for convolutions that run BESIDE other work on side streams (``with ops.coresident():``):
# only 8-wave workgroups with <= ~106 registers per wave are tried, which leave half of a CU's wave slots and
# registers to the partner kernel (a stand-alone timing would pick 12-wave workgroups that own the CU).
_CORESIDENT = False


class coresident:
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        global _CORESIDENT
        self.prev, _CORESIDENT = _CORESIDENT, self.on
        return self

    def __exit__(self, *exc):
        global _CORESIDENT
        _CORESIDENT = self.prev
        return False


def _small_footprint(cands):
    fs = [decode_cfg(c) for c in cands]
    small = [c for c, f in zip(cands, fs) if f.pgw * f.cgw * f.ksplit == 4 and f.mb // f.cgw <= 2]
    return small or cands


@functools.lru_cache(maxsize=None)
def _b_inst():
    """The split-bf16 kernel instantiations (pgw, cgw, A, B, ksplit) of the library, in the order of CONVB_ALL
    (conv_bf16_kernel.h).  ``ops._B_INST`` reads the same tuple; importing this module loads no library."""
    lib = _abi.load()
    n = lib.codd_conv2d_bf16_instantiations(None, 0)
    flat = (C.c_int * (5 * n))()
    lib.codd_conv2d_bf16_instantiations(flat, n)
    return tuple(tuple(flat[5 * i:5 * i + 5]) for i in range(n))


def __getattr__(name):
    if name == "_B_INST":
        return _b_inst()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


# the tiles (rows, 16-pixel units per row) tried, by pixel units of a workgroup (= pgw * A of an instantiation)
_B_TILES = {10: ((9, 1), (10, 1), (5, 2)), 16: ((8, 2), (16, 1)), 32: ((16, 2),), 8: ((4, 2), (8, 1)), 12: ((12, 1), (6, 2))}
# (round 6 added 96-channel groups (4,2,3,3) / (2,2,5,3) and 20-unit tiles (4,2,5,2) so that the 384-channel gate-input convolution
# -- 288 workgroups = 1.12 dispatch rounds on its 64-channel x 12-unit grid -- could run as ONE round: every single-round
# configuration is SLOWER (33.8 us at 192 / 216 / 240 workgroups against 29.8 us at 288: tools/sweep_update_block.py,
# profiles/r06_sweep_update_block.log), the shipped picks are the optimum of the extended space on all seven update-block
# layers, and the instantiations were removed again.)


def _bf16_candidates(pc, Hout, Wout, B, taps, terms):
    """Launch configurations (xb, th, ck, mb, 2, pgw, cgw, terms, ksplit) of the split-bf16 kernel for this layer, best guess first:
    fewest dispatch rounds over the 256 CUs times work per workgroup, larger channel groups and deeper chunks first."""
    nblk = -(-pc.cout_eff // 16)
    cands = []
    for (pgw, cgw, a, b, ks) in _b_inst():
        mb = b * cgw
        if mb > 1 and mb // 2 >= nblk:  # a channel group at least twice as wide as the layer
            continue
        for (th, xb) in _B_TILES[pgw * a]:
            grid = -(-Hout // th) * -(-Wout // (16 * xb)) * -(-pc.cout_eff // (16 * mb)) * B
            rounds = -(-grid // 256)
            cost = rounds * (pgw * a) * mb
            cands.append((cost, ks if pgw * cgw == 4 else 2, -mb, -th * xb, (xb, th, mb, pgw, cgw, ks)))
    cands.sort()
    cin8 = -(-pc.cin // 8) * 8
    cks = [c for c in ((128, 64, 32, 16, 8) if taps == 1 else (32, 16, 8)) if c <= max(8, cin8)]
    if not cks or cks[0] < min(cin8, 32):
        cks.insert(0, min(cin8, 32))
    out = []
    for _, _, _, _, (xb, th, mb, pgw, cgw, ks) in cands:
        for ck in cks:
            out.append((xb, th, ck, mb, 2, pgw, cgw, terms, ks))
    return out


class SplitTensor:
    """An activation in the split-bf16 conv-input form (include/codd_hip.h, codd_split_bf16): made once by
    ``split_input`` and consumed by any number of convolutions of that activation (same spatial size, padding up to
    the border, channel slices at multiples of 8)."""
    __slots__ = ("buf", "B", "C", "H", "W", "bt", "bl", "hp", "wp", "c8", "terms")

    def __init__(self, buf, B, C, H, W, bt, bl, hp, wp, c8, terms):
        self.buf, self.B, self.C, self.H, self.W = buf, B, C, H, W
        self.bt, self.bl, self.hp, self.wp, self.c8, self.terms = bt, bl, hp, wp, c8, terms


def _split_rows(H):
    """Image rows of a shared split tensor: enough for the row overhang of EVERY tile height of _B_TILES
    (4 ... 16 rows: ceil(H / th) * th <= H + th - 1)."""
    return max(-(-H // th) * th for tiles in _B_TILES.values() for (th, _) in tiles)


def split_input(x, x2=None, border=0, c8=None, hp=None, wp=None, out=None):
    """codd_split_bf16 of (x | x2) with a zero border of ``border`` pixels (int or (top, left)); hp / wp default to
    the size that serves every instantiated tile (4 ... 16 rows, 32-pixel columns) of a stride-1 'same' convolution
    whose padding does not exceed the border.  Returns None outside the split / bf16 precision modes."""
    terms = _TERMS.get(CONV_PRECISION, 0)
    if not terms:
        return None
    lib = _abi.load()
    xs = _as_slice(x)
    _require_gpu(xs.buf)
    B, C0, H, W = xs.shape
    C1 = 0 if x2 is None else _as_slice(x2).c
    if out is not None:  # re-layout into an existing (persistent) tensor of the same geometry
        _abi.check(lib.codd_split_bf16(_view(xs), C0, _view(x2), C1, B, H, W, out.bt, out.bl, out.c8, out.hp, out.wp,
                                       out.terms, out.buf.data_ptr(), _stream()), "codd_split_bf16")
        return out
    bt, bl = (border, border) if isinstance(border, int) else border
    c8 = -(-(C0 + C1) // 32) * 4 if c8 is None else c8  # whole 32-channel chunks
    hp = 2 * bt + _split_rows(H) if hp is None else hp
    wp = 2 * bl + -(-W // 32) * 32 if wp is None else wp
    buf = torch.empty(lib.codd_split_bf16_bytes(B, c8, hp, wp, terms), device=xs.buf.device, dtype=torch.uint8)
    _abi.check(lib.codd_split_bf16(_view(xs), C0, _view(x2), C1, B, H, W, bt, bl, c8, hp, wp, terms, buf.data_ptr(),
                                   _stream()), "codd_split_bf16")
    return SplitTensor(buf, B, C0 + C1, H, W, bt, bl, hp, wp, c8, terms)


_SPLIT_BUFFERS = {}


def split_buffer(key, B, C, H, W, border=0, device=None):
    """A PERSISTENT, zero-initialised SplitTensor for activations that a convolution writes directly in split-bf16
    form (conv2d(..., xs_out=...)): the producer only writes the image interior, so the zero border (and the zero
    channel padding) made here once stays valid for every later frame.  One buffer per call site (``key``) and shape;
    returns None outside the split / bf16 precision modes."""
    terms = _TERMS.get(CONV_PRECISION, 0)
    if not terms:
        return None
    lib = _abi.load()
    bt, bl = (border, border) if isinstance(border, int) else border
    k = (key, B, C, H, W, bt, bl, terms, str(device))
    st = _SPLIT_BUFFERS.get(k)
    if st is None:
        c8 = -(-C // 32) * 4
        hp, wp = 2 * bt + _split_rows(H), 2 * bl + -(-W // 32) * 32
        buf = torch.zeros(lib.codd_split_bf16_bytes(B, c8, hp, wp, terms), device=device, dtype=torch.uint8)
        st = _SPLIT_BUFFERS[k] = SplitTensor(buf, B, C, H, W, bt, bl, hp, wp, c8, terms)
    return st


def _conv_params(pc, B, C0, C1, Hin, Win, Hout, Wout, stride, pad, dil, act="none"):
    """ConvParams of a convolution by ``pc``: geometry, bias, activation; stride / pad (top, left) / dil as (y, x)."""
    p = ConvParams()
    p.C0, p.C1, p.B, p.Hin, p.Win = C0, C1, B, Hin, Win
    p.bias = None if pc.bias is None else pc.bias.data_ptr()
    p.Cout, p.Hout, p.Wout = pc.cout, Hout, Wout
    p.kh, p.kw, p.sy, p.sx = pc.kh, pc.kw, stride[0], stride[1]
    p.pad_t, p.pad_l, p.dil_y, p.dil_x = pad[0], pad[1], dil[0], dil[1]
    p.act = ACT[act]
    p.store_mode = int(pc.deconv)
    return p


def _attach_xs(p, st, coff):
    """Read the conv input from channels [coff, ...) of the SplitTensor ``st``."""
    p.xs, p.xs_c8, p.xs_hp, p.xs_wp = st.buf.data_ptr(), st.c8, st.hp, st.wp
    p.xs_bt, p.xs_bl, p.xs_o8 = st.bt, st.bl, coff // 8


def _attach_xso(p, st, coff):
    """Write the conv output as split records into channels [coff, ...) of the SplitTensor ``st``."""
    p.xso, p.xso_c8, p.xso_hp, p.xso_wp = st.buf.data_ptr(), st.c8, st.hp, st.wp
    p.xso_bt, p.xso_bl, p.xso_o8, p.xso_terms = st.bt, st.bl, coff // 8, st.terms


def _conv_geometry(pc, Hin, Win, stride=1, pad=0, dil=1, pad_tl=None, out_hw=None):
    """-> (sy, sx), (pad top, pad left), (dy, dx), (Hout, Wout, up) of a convolution by ``pc`` of a Hin x Win map.
    stride / pad / dil: an int or a (y, x) pair; ``pad_tl`` = (top, left, bottom, right) for unequal borders; ``out_hw``
    overrides the output map.  A transposed convolution (k2 s2 as a 1x1 with 4 Cout outputs) keeps the input map and
    stores it up = 2 times as large."""
    sy, sx = (stride, stride) if isinstance(stride, int) else stride
    dy, dx = (dil, dil) if isinstance(dil, int) else dil
    if pad_tl is None:
        pt, pl = (pad, pad) if isinstance(pad, int) else pad
        pb, pr = pt, pl
    else:
        pt, pl, pb, pr = pad_tl
    if pc.deconv:
        Hout, Wout = Hin, Win
    elif out_hw is not None:
        Hout, Wout = out_hw
    else:
        Hout = (Hin + pt + pb - dy * (pc.kh - 1) - 1) // sy + 1
        Wout = (Win + pl + pr - dx * (pc.kw - 1) - 1) // sx + 1
    return (sy, sx), (pt, pl), (dy, dx), (Hout, Wout, 2 if pc.deconv else 1)


# A launch shape is looked up under two names: its ``key`` in pc.tuned (this layer object) and its signature string in
# TUNE_DB and the shipped codd_amd/tuned/mi355x.json (any layer of that description).  The strings are the keys of the
# shipped db, so they never change by a byte; tests/conv_fp64.py (parse_sig) and tests/test_conv_launch_config.py (_layer)
# read them back.
#   plain  key  (Hout, Wout, B, sy, sx, dy, dx, pl, two inputs, terms[, "split"][, "co"])
#          sig  [b<terms>|]cout_eff,cin,kh,kw,mb,deconv|Hout,Wout,B,sy,sx,dy,dx,pl,two inputs[|split][|co]
#               "b<terms>|" is absent under the exact-fp32 precision (terms 0); "split": pinned to the split-bf16 kernel
#               (input or output in record form); "co": chosen under ops.coresident()
#   gate   key  ("gate", gate, H, W, B, pad, dil, dil2, terms)
#          sig  g<gate>,b<terms>|cout,cin,kh,kw|H,W,B,pad,dil,dil2
def _plain_key(geom, two, terms, pinned):
    return geom + (two, terms) + (("split",) if pinned else ()) + (("co",) if _CORESIDENT and terms else ())


def _plain_sig(pc, key):
    return ("b%d|" % key[9] if key[9] else "") + "%d,%d,%d,%d,%d,%d|" % (
        pc.cout_eff, pc.cin, pc.kh, pc.kw, pc.mb, int(pc.deconv)) + ",".join(str(int(v)) for v in key[:9]) + "".join(
            "|" + flag for flag in key[10:])


def _gate_key(gate, H, W, B, pad, dil, dil2, terms):
    return ("gate", gate, H, W, B, pad, dil, dil2, terms)


def _gate_sig(pc, key):
    _, gate, H, W, B, pad, dil, dil2, terms = key
    return "g%d,b%d|%d,%d,%d,%d|%d,%d,%d,%d,%d,%d" % (gate, terms, pc.cout, pc.cin, pc.kh, pc.kw, H, W, B, pad, dil, dil2)


# One conv2d / conv_gate call as its chooser and its launch tail see it: the library, the ConvParams ``p`` of the launch,
# the layer, its launch-shape key, geom = the arguments of _conv_cfg after pc, the terms of the precision mode, the fp32
# input (x: a Slice, None when the input exists in record form only; x2), the shared SplitTensor ``xs`` and the record
# output ``xs_out`` with their channel offsets, and small: only the _small_footprint split candidates are tried.
_ConvCall = collections.namedtuple("_ConvCall", "lib p pc key geom terms x x2 xs xs_coff xs_out xs_out_coff small")


def _split_cands(call):
    """The split-bf16 configurations the library accepts for this call, best guess first."""
    Hout, Wout, B = call.geom[:3]
    cands = [c for c in _bf16_candidates(call.pc, Hout, Wout, B, call.pc.kh * call.pc.kw, call.terms)
             if _cfg_ok(call.lib, call.p, c)]
    return _small_footprint(cands) if call.small else cands


def _pinned_cands(call):
    cands = _split_cands(call)
    if not cands:
        raise _abi.CoddHipError("no split-bf16 launch configuration for %sconv %dx%d %d->%d" % (
            "gate " if call.p.gate else "", call.pc.kh, call.pc.kw, call.pc.cin, call.pc.cout))
    return cands


def _heuristic(call):
    return _conv_cfg(call.pc, *call.geom)


def _tune_pinned(call, cands):
    """Time the candidates on the real split input / output tensors (into a scratch ``out``: in-place gates are safe)."""
    keep = None if call.x is None else _make_split(call.lib, call.p, call.x, call.x2, cands)  # noqa: F841
    if call.x is None:
        _attach_xs(call.p, call.xs, call.xs_coff)
    if call.xs_out is not None:
        _attach_xso(call.p, call.xs_out, call.xs_out_coff)
    return _autotune_b(call.lib, call.p, call.pc, cands, None, None)[0]


def _untimed_pinned(call, cands):
    """The configuration this layer was tuned to in its plain form (the signature without "|split") if that is a split
    one, else the first candidate."""
    plain = TUNE_DB.get(_plain_sig(call.pc, call.key[:10])) if _AUTOTUNE and not _CORESIDENT else None
    return tuple(plain) if plain is not None and decode_cfg(plain).layout == 2 else cands[0]


def _tune_choice(call, cands):
    """Measure: the best split-bf16 configuration (incl. its re-layout pass) against the best exact-fp32 one -- small or
    large-map layers can be faster (and are more exact) on the fp32 kernels."""
    lib, p, pc = call.lib, call.p, call.pc
    f32cfg, t32 = _autotune(lib, p, pc, _heuristic(call) + (pc.mb, 0))
    p.terms = call.terms
    bcfg, tb = (None, float("inf"))
    if cands:
        keep = _make_split(lib, p, call.x, call.x2, cands)  # noqa: F841 one split input serving every candidate
        bcfg, tb = _autotune_b(lib, p, pc, cands, call.x, call.x2)
    cfg = bcfg if tb < t32 else f32cfg
    AUTOTUNE_LOG.append(("choice %dx%d %d->%d out %dx%d" % (pc.kh, pc.kw, pc.cin, pc.cout, call.geom[0], call.geom[1]),
                         f32cfg, t32 * 1e3, cfg, min(tb, t32) * 1e3))
    return cfg


# How a launch shape met for the first time gets its configuration (_pick_cfg): the candidates, how they are timed when
# autotuning, the pick when they are not, the signature format, and kept: the pick stays in pc.tuned even when it was
# made untimed while capturing with autotune on.
_Chooser = collections.namedtuple("_Chooser", "candidates tune untimed sig kept")
_PINNED = _Chooser(_pinned_cands, _tune_pinned, _untimed_pinned, _plain_sig, True)  # input or output in record form
_CHOICE = _Chooser(_split_cands, _tune_choice,  # split-bf16 or exact fp32
                   lambda call, cands: cands[0] if cands else _heuristic(call) + (call.pc.mb, 0), _plain_sig, False)
_FP32 = _Chooser(lambda call: [_heuristic(call)],
                 lambda call, cands: _autotune(call.lib, call.p, call.pc, cands[0] + (call.pc.mb, 0))[0],
                 lambda call, cands: cands[0], _plain_sig, False)
_GATE = _Chooser(_pinned_cands, _tune_pinned, lambda call, cands: cands[0], _gate_sig, False)


def _choose(call, how):
    bind = functools.partial
    cfg = _pick_cfg(call.lib, call.p, call.pc, call.key, how.sig(call.pc, call.key), bind(how.candidates, call),
                    bind(how.tune, call), bind(how.untimed, call))
    if how.kept:
        call.pc.tuned[call.key] = cfg
    return cfg


def _launch_split(call, cfg, what="codd_conv2d"):
    """Launch the call on the split-bf16 kernel with configuration ``cfg``: from the shared SplitTensor when it is one of
    this call's input; where there is none, or the library finds that it does not fit this configuration's tiles (rc -1),
    from a private re-layout of the fp32 input -- which an input in record form only does not have."""
    lib, p, pc, xs = call.lib, call.p, call.pc, call.xs
    if call.xs_out is not None:
        _attach_xso(p, call.xs_out, call.xs_out_coff)
    if (xs is not None and xs.terms == call.terms and (xs.B, xs.H, xs.W) == (p.B, p.Hin, p.Win) and call.xs_coff % 8 == 0
            and call.xs_coff + pc.cin <= max(xs.C, 8 * xs.c8 if call.x is None else 0)):
        _attach_xs(p, xs, call.xs_coff)
        _set_cfg(p, cfg, pc)
        rc = _launch_conv(lib, p, _stream())
        if rc == 0:
            return
        if rc != -1 or call.x is None:
            _abi.check(rc, what)
    elif call.x is None:
        raise _abi.CoddHipError("%s: the split input is not one of this convolution's input" % what)
    keep = _make_split(lib, p, call.x, call.x2, [cfg])  # noqa: F841 (alive until the launch below is enqueued)
    _set_cfg(p, cfg, pc)
    _abi.check(_launch_conv(lib, p, _stream()), what)


def conv2d(x, pc, x2=None, stride=1, pad=0, dil=1, act="none", res1=None, res2=None, post=None,
           out=None, pad_tl=None, out_hw=None, xs=None, xs_coff=0, xs_out=None, xs_out_coff=0):
    """act(conv(cat[x, x2]) + bias + res1 + res2) + post  ->  out (tensor or Slice).
    ``xs``: a SplitTensor of the input made by split_input (channels [xs_coff, xs_coff + Cin) of it): used instead of
    a private re-layout when this layer runs on the split-bf16 kernel and the tensor fits its tiles.  ``x`` may be
    None when the input only exists in split form (it was written by a producer's ``xs_out``).
    ``xs_out``: write the result as split-bf16 records into this (persistent, zero-bordered: split_buffer) tensor at
    channel offset ``xs_out_coff`` instead of an fp32 tensor, and return it -- the next convolution then needs no
    re-layout pass.  Both options pin the layer to the split-bf16 kernel."""
    lib = _abi.load()
    pinned = (x is None) or (xs_out is not None)
    if x is None:
        assert xs is not None and x2 is None and xs_coff % 8 == 0
        xsl, src = None, xs.buf
        B, C0, Hin, Win = xs.B, pc.cin, xs.H, xs.W
    else:
        xsl = _as_slice(x)
        src = xsl.buf
        B, C0, Hin, Win = xsl.shape
    _require_gpu(src)
    C1 = 0
    if x2 is not None:
        x2s = _as_slice(x2)
        C1 = x2s.c
        assert x2s.shape[2:] == (Hin, Win)
    assert C0 + C1 == pc.cin, (C0, C1, pc.cin)
    (sy, sx), (pt, pl), (dy, dx), (Hout, Wout, up) = _conv_geometry(pc, Hin, Win, stride, pad, dil, pad_tl, out_hw)
    terms = _TERMS.get(CONV_PRECISION, 0)
    if pinned and not terms:
        raise _abi.CoddHipError("split-form convolution inputs / outputs need the 'split' or 'bf16' conv precision")
    p = _conv_params(pc, B, C0, C1, Hin, Win, Hout, Wout, (sy, sx), (pt, pl), (dy, dx), act)
    p.in0, p.in1 = _view(xsl), _view(x2)
    p.res1, p.res2, p.post = _view(res1), _view(res2), _view(post)
    p.terms = terms
    if xs_out is None:
        if out is None:
            out = torch.empty(B, pc.cout, Hout * up, Wout * up, device=src.device, dtype=torch.float32)
        os_ = _as_slice(out)
        assert os_.shape == (B, pc.cout, Hout * up, Wout * up), (os_.shape, (B, pc.cout, Hout * up, Wout * up))
        p.out, p.out_ctot, p.out_coff = os_.buf.data_ptr(), os_.buf.shape[1], os_.coff
    else:
        assert (xs_out.B, xs_out.H, xs_out.W) == (B, Hout, Wout) and xs_out.terms == terms and xs_out_coff % 8 == 0
        assert xs_out_coff + pc.cout <= 8 * xs_out.c8 and not pc.deconv and res1 is None and res2 is None and post is None
        out = xs_out
    geom = (Hout, Wout, B, sy, sx, dy, dx, pl)
    call = _ConvCall(lib, p, pc, _plain_key(geom, C1 > 0, terms, pinned), geom, terms, xsl, x2, xs, xs_coff, xs_out,
                     xs_out_coff, _CORESIDENT)
    cfg = pc.tuned.get(call.key)
    if cfg is None:
        cfg = _choose(call, _PINNED if pinned else _CHOICE if terms else _FP32)
    if decode_cfg(cfg).layout == 2:  # split-bf16 / bf16 kernel
        _launch_split(call, cfg)
        return out
    _set_cfg(p, cfg, pc)
    heur = (call.key, geom)
    if _DEFERRED is not None and p.layout == 1 and p.npb == 1 and p.nw == 4 and p.mb == 1:
        # inside ``with deferred_convs():`` -- recorded, launched on exit together with its independent neighbours
        _DEFERRED.append((ConvParams.from_buffer_copy(p), (x, x2, res1, res2, post, out), pc, heur))
        return out
    _launch_fp32(lib, p, pc, heur)
    return out


def _pick_cfg(lib, p, pc, key, sig, candidates, tune, untimed=None):
    """Launch configuration of a conv2d / conv_gate launch shape met for the first time (``key`` in pc.tuned, layer
    signature ``sig`` in TUNE_DB): the tune-db entry when this build accepts it; else, autotuning and not capturing,
    tune(candidates()), recorded in TUNE_DB; else untimed(candidates()), by default the first candidate.  The pick is
    kept in pc.tuned, except an untimed one while capturing with autotune on (this launch only, timed later)."""
    if _AUTOTUNE and sig in TUNE_DB and _db_cfg_ok(lib, p, TUNE_DB[sig], sig):
        cfg = pc.tuned[key] = tuple(TUNE_DB[sig])  # same layer signature already timed (this process or a loaded file)
        return cfg
    cands = candidates()
    if _AUTOTUNE and not torch.cuda.is_current_stream_capturing():
        cfg = pc.tuned[key] = TUNE_DB[sig] = tune(cands)
        return cfg
    cfg = cands[0] if untimed is None else untimed(cands)
    if not _AUTOTUNE:
        pc.tuned[key] = cfg
    return cfg


def _launch_fp32(lib, p, pc, heur):
    """Launch one exact-fp32 convolution; a tuned / loaded configuration this build does not support (rc -2, e.g. a tune
    db from another version) falls back to the heuristic configuration for this launch shape, loudly.  Shared by conv2d
    and by deferred_convs' single-launch path."""
    rc = _launch_conv(lib, p, _stream())
    if rc == -2:
        import warnings
        key, geom = heur
        warnings.warn("codd_amd: launch configuration %s rejected for conv %dx%d %d->%d, using the heuristic" % (
            (p.npb, p.nw, p.ck, p.mb, p.layout), pc.kh, pc.kw, pc.cin, pc.cout))
        cfg = pc.tuned[key] = _conv_cfg(pc, *geom)
        _set_cfg(p, cfg, pc)
        rc = _launch_conv(lib, p, _stream())
    _abi.check(rc, "codd_conv2d")


def _db_cfg_ok(lib, p, c, sig):
    """A launch configuration loaded from a tune db must be one THIS build accepts (a db written by another version
    may name tiles that no longer exist): split-bf16 entries are probed with codd_conv2d_check (fp32 entries are
    validated at launch, rc -2 -> heuristic); a rejected entry is dropped with a warning and the layer is tuned /
    given the heuristic as if the db had no entry."""
    try:
        f = decode_cfg(c, terms=p.terms)
    except ValueError:
        f = None
    if f is None or (f.layout == 2 and (not p.terms or f.terms != p.terms or not _cfg_ok(lib, p, c))):
        import warnings
        warnings.warn("codd_amd: tune-db entry %s = %s is not a valid %s configuration of this build; ignored" % (
            sig, tuple(c), "launch" if f is None else "split-bf16"))
        del TUNE_DB[sig]
        return False
    return True


_DEFERRED = None


class deferred_convs:
    """``with ops.deferred_convs(): ...`` -- exact-fp32 convolutions issued inside the block whose launch configuration is
    the multi-job class (quad layout, 4 x 16 tiles, 16 channels per workgroup: csrc/conv_quad_kernel.h) are RECORDED with
    the parameters the single launch would have used and launched on exit, up to four per codd_conv2d_multi launch: the
    same kernel body on the same parameters, i.e. bit-identical results, and one kernel node instead of up to four (every
    node of the frame graph costs ~3.8 us of wall clock, DESIGN.md finding 43).  Convolutions of other classes launch at
    once.  The caller guarantees that the convolutions inside one block do not read one another's results."""

    def __enter__(self):
        global _DEFERRED
        self.prev, _DEFERRED = _DEFERRED, []
        return self

    def __exit__(self, *exc):
        global _DEFERRED
        items, _DEFERRED = _DEFERRED, self.prev
        if exc[0] is not None or not items:
            return False
        lib = _abi.load()
        # one job, or a multi-job launch this build rejects: single launches with conv2d's own fallback
        _launch_multi(lib, items, lambda it: _launch_fp32(lib, it[0], it[2], it[3]), "codd_conv2d_multi (deferred)")
        return False


def _launch_conv_multi(lib, params, n, stream):
    """Single choke point of the multi-job conv launches (bench.py wraps it with HIP events)."""
    return lib.codd_conv2d_multi(params, n, stream)


def _launch_multi(lib, jobs, fallback, what):
    """Launch ``jobs`` -- tuples whose first item is the ConvParams of a convolution of the multi-job class -- up to four
    at a time, in the order given, each group as ONE codd_conv2d_multi; a lone job and every job of a group this build
    rejects (rc -2) go to ``fallback(job)`` instead.  Workgroups are dispatched in job order: inside a group the job with
    the longest per-workgroup chain (most input channels x taps) goes first, so that its chain runs beside the wide,
    shallow jobs instead of after them."""
    for k0 in range(0, len(jobs), 4):
        group = sorted(jobs[k0:k0 + 4], key=lambda j: -((j[0].C0 + j[0].C1) * j[0].kh * j[0].kw))
        rc = -2
        if len(group) > 1:
            arr = (ConvParams * len(group))(*[j[0] for j in group])
            rc = _launch_conv_multi(lib, arr, len(group), _stream())
            if rc not in (0, -2):
                _abi.check(rc, what)
        if rc != 0:
            for j in group:
                fallback(j)


def conv2d_multi(jobs):
    """Independent stride-1/2 convolutions -> list of outputs.  ``jobs``: dicts(x, pc[, stride, pad, act, res1]).  Under the
    exact-fp32 precision the jobs whose rows are 16-byte aligned are launched up to four at a time by ONE
    codd_conv2d_multi (quad layout, 4 x 16 tiles, 16 output channels per workgroup: the launch-bound small layers of
    HRNet's branches); everything else goes through conv2d one by one."""
    lib = _abi.load()
    outs = [None] * len(jobs)
    group = []
    if CONV_PRECISION == "fp32" and len(jobs) > 1:
        group = [idx for idx, j in enumerate(jobs)
                 if (isinstance(j["x"], torch.Tensor) and j["x"].shape[3] % 4 == 0 and j["x"].data_ptr() % 16 == 0
                     and not j["pc"].deconv and j["pc"].cin >= 16 and j.get("stride", 1) in (1, 2))]
        if len(group) % 4 == 1:
            group.pop()  # a lone last job goes through conv2d
    multi = []
    for idx in group:
        j = jobs[idx]
        x, pc = j["x"], j["pc"]
        B, C0, Hin, Win = x.shape
        stride, pad, dil, (Hout, Wout, _) = _conv_geometry(pc, Hin, Win, j.get("stride", 1), j.get("pad", 0))
        out = outs[idx] = torch.empty(B, pc.cout, Hout, Wout, device=x.device, dtype=torch.float32)
        p = _conv_params(pc, B, C0, 0, Hin, Win, Hout, Wout, stride, pad, dil, j.get("act", "none"))
        p.in0, p.res1 = _view(x), _view(j.get("res1"))
        p.out, p.out_ctot, p.out_coff = out.data_ptr(), pc.cout, 0
        _set_cfg(p, (1, 4, 32 if pc.cin > 16 else 16, 1, 1), pc)
        multi.append((p, idx))

    def later(job):  # rejected group: through conv2d below
        outs[job[1]] = None

    _launch_multi(lib, multi, later, "codd_conv2d_multi")
    for idx, j in enumerate(jobs):
        if outs[idx] is None:
            outs[idx] = conv2d(j["x"], j["pc"], stride=j.get("stride", 1), pad=j.get("pad", 0), act=j.get("act", "none"),
                               res1=j.get("res1"))
    return outs


class C4Tensor:
    """A channel-quad fp32 activation [B][C/4][H*W][4] (include/codd_hip.h, codd_conv_params.gate): the private layout of
    the ConvGRU's gate operands -- a lane of the split-bf16 kernel's record-form accumulator holds 4 consecutive
    channels of one pixel, i.e. one 16-byte access here."""
    __slots__ = ("buf", "B", "C", "H", "W")

    def __init__(self, buf, B, C, H, W):
        self.buf, self.B, self.C, self.H, self.W = buf, B, C, H, W

    def view(self, coff=0):
        return _abi.View(self.buf.data_ptr(), self.C, coff)

    def nchw(self):
        """-> a new fp32 NCHW tensor (tests / the hand-over to code outside the update block)."""
        return self.buf.view(self.B, self.C // 4, self.H * self.W, 4).permute(0, 1, 3, 2).reshape(
            self.B, self.C, self.H, self.W).contiguous()


_C4_BUFFERS = {}


def c4_buffer(key, B, C, H, W, device):
    """A persistent C4Tensor per call site (``key``) and shape."""
    assert C % 4 == 0
    k = (key, B, C, H, W, str(device))
    t = _C4_BUFFERS.get(k)
    if t is None:
        t = _C4_BUFFERS[k] = C4Tensor(torch.zeros(B * C * H * W, device=device, dtype=torch.float32), B, C, H, W)
    return t


def to_c4(x, out):
    """fp32 NCHW tensor -> the C4Tensor ``out`` (one strided copy)."""
    B, C, H, W = x.shape
    assert (out.B, out.C, out.H, out.W) == (B, C, H, W)
    out.buf.view(B, C // 4, H * W, 4).copy_(x.reshape(B, C // 4, 4, H * W).permute(0, 1, 3, 2))
    return out


def conv_gate(pc, xs, gate, pad=0, dil=1, dil2=0, out=None, out_coff=0, res1=None, res2=None, post=None, xs_out=None,
              xs_coff=0):
    """A stride-1 'same' convolution of the split tensor ``xs`` on the split-bf16 kernel with a ConvGRU gate epilogue
    (include/codd_hip.h, codd_conv_params.gate / dil2): ``gate`` 1 = plain result into the C4Tensor ``out``;
    2 = z | r*h | q-input of the merged gate-input convolution; 3 = the hidden-state update.  ``dil2``: the weights
    hold two tap sets ([cout, cin, 2*k, k]: dilation dil2 rows first, then dilation dil), both over one input tile.
    out / res1 / res2 / post are C4Tensors, xs_out a SplitTensor."""
    lib = _abi.load()
    terms = _TERMS.get(CONV_PRECISION, 0)
    if not terms:
        raise _abi.CoddHipError("gate-epilogue convolutions need the 'split' or 'bf16' conv precision")
    _require_gpu(xs.buf)
    B, H, W = xs.B, xs.H, xs.W
    p = _conv_params(pc, B, pc.cin, 0, H, W, H, W, (1, 1), (pad, pad), (dil, dil))
    p.dil2, p.gate, p.terms, p.layout = dil2, gate, terms, 2
    p.out, p.out_ctot, p.out_coff = out.buf.data_ptr(), out.C, out_coff
    for name, t in (("res1", res1), ("res2", res2), ("post", post)):
        if t is not None:
            setattr(p, name, t.view())
    # small (gate 1): the z|r convolution runs BESIDE the VALU-only Gauss-Newton builder (BasicUpdateBlock.zr_convs): a
    # stand-alone timing would pick 12-wave workgroups, whose ~450 registers per SIMD leave the builder no room on the
    # same CU; 8-wave workgroups (2 waves per SIMD, ~106 registers each) co-reside with two builder waves per SIMD.
    # Measured in the frame: 93.2-93.5 against 91.7-92.1 frames/s (profiles/r03_ab_runs.log, "zc"); the isolated timing
    # then only chooses among those.
    call = _ConvCall(lib, p, pc, _gate_key(gate, H, W, B, pad, dil, dil2, terms), (H, W, B, 1, 1, dil, dil, pad), terms,
                     None, None, xs, xs_coff, xs_out, 0, gate == 1)
    cfg = pc.tuned.get(call.key)
    if cfg is None:
        cfg = _choose(call, _GATE)
    _launch_split(call, cfg, "codd_conv2d (gate %d)" % gate)
    return out


def _cfg_ok(lib, p, c):
    """Does the library accept split-bf16 configuration ``c`` for the layer described by ``p``? (nothing is launched)"""
    _set_cfg(p, c)
    return lib.codd_conv2d_check(C.byref(p)) == 0


def _split_dims(p, cands):
    """(c8, hp, wp) of a split-bf16 input that serves every configuration in ``cands`` for the conv described by
    ``p`` (include/codd_hip.h, codd_split_bf16): borders (pad_t, pad_l) + the largest tile overhang."""
    cin = p.C0 + p.C1
    c8 = hp = wp = 0
    for c in cands:
        f = decode_cfg(c)
        c8 = max(c8, -(-cin // f.ck) * (f.ck // 8))
        hp = max(hp, p.pad_t + p.Hin, (-(-p.Hout // f.nw) * f.nw - 1) * p.sy + (p.kh - 1) * p.dil_y + 1)
        wp = max(wp, p.pad_l + p.Win, (-(-p.Wout // (16 * f.npb)) * 16 * f.npb - 1) * p.sx + (p.kw - 1) * p.dil_x + 1)
    return c8, hp, wp


def _make_split(lib, p, x, x2, cands, B=None):
    """codd_split_bf16 of the conv input (x | x2) -- B images, default p.B -- sized for every configuration in ``cands``
    of the conv described by ``p`` (borders pad_t / pad_l), attached to ``p``.  Returns the SplitTensor: the caller
    keeps it alive until the conv is enqueued (the caching allocator is stream-ordered)."""
    B = p.B if B is None else B
    c8, hp, wp = _split_dims(p, cands)
    buf = torch.empty(lib.codd_split_bf16_bytes(B, c8, hp, wp, p.terms), device=_as_slice(x).buf.device,
                      dtype=torch.uint8)
    _abi.check(lib.codd_split_bf16(_view(x), p.C0, _view(x2), p.C1, B, p.Hin, p.Win, p.pad_t, p.pad_l, c8, hp, wp,
                                   p.terms, buf.data_ptr(), _stream()), "codd_split_bf16")
    st = SplitTensor(buf, B, p.C0 + p.C1, p.Hin, p.Win, p.pad_t, p.pad_l, hp, wp, c8, p.terms)
    _attach_xs(p, st, 0)
    return st


def _time_cfgs(lib, p, pc, cands, apply, desc):
    """Time the launch configurations ``cands`` of the conv described by ``p`` and keep the fastest.  ``apply(c)`` sets
    ``p`` up for candidate c (what it returns is kept alive while c is timed) or raises CoddHipError to skip it.  The
    launches write into a scratch output: the real one may alias an operand (in-place accumulation "out = conv(x) +
    out"), which repeated launches would accumulate over and over.  The first candidate runs once more first, to warm
    clocks and caches; a candidate's time is the best of two bursts of three launches, and a later candidate must be
    3 % faster to win (ties go to the earlier, heuristic-first candidates).  Frees pc's packed weights of the losers
    (pc may be None) and logs (desc, first candidate, its us | None, winner, us) to AUTOTUNE_LOG.
    -> (winner, ms); (cands[0], inf) when no candidate launches."""
    stream = _stream()
    real_out = p.out
    scratch_out = torch.empty(p.B * p.out_ctot * (4 if p.store_mode else 1) * p.Hout * p.Wout,
                              device="cuda" if pc is None else pc._w.device, dtype=torch.float32)
    p.out = scratch_out.data_ptr()
    torch.cuda.synchronize()  # nothing else on the device while the candidates are timed
    best, best_t, t_first = cands[0], float("inf"), None
    for i, c in enumerate(cands[:1] + cands):
        try:
            keep = apply(c)  # noqa: F841
        except _abi.CoddHipError:
            continue
        if _launch_conv(lib, p, stream) != 0:  # not instantiated / LDS or staging limits: skip
            continue
        t = float("inf")
        for _rep in range(2):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(3):
                _launch_conv(lib, p, stream)
            e.record()
            e.synchronize()
            t = min(t, s.elapsed_time(e) / 3.0)
        if i == 0:
            continue  # warm-up pass
        if i == 1:
            t_first = t
        if AUTOTUNE_TRACE is not None and p.layout == 2:
            cout_eff = p.Cout * (4 if p.store_mode else 1)
            AUTOTUNE_TRACE.append(("b%d g%d k%dx%d d%d/%d %d->%d out %dx%d" % (
                p.terms, p.gate, p.kh, p.kw, p.dil_y, p.dil2, p.C0 + p.C1, p.Cout, p.Hout, p.Wout), c,
                -(-p.Hout // p.nw) * -(-p.Wout // (16 * p.npb)) * -(-cout_eff // (16 * p.mb)) * p.B, t * 1e3))
        if t < best_t * 0.97:
            best, best_t = c, t
    p.out = real_out
    if pc is not None:
        pc.drop_unused_packs(keep=best)
    AUTOTUNE_LOG.append((desc, cands[0], None if t_first is None else t_first * 1e3, best, best_t * 1e3))
    return best, best_t


def _autotune_b(lib, p, pc, cands, xsl, x2):
    """Time every split-bf16 candidate (_time_cfgs) and keep the fastest; returns (configuration, ms) where the time
    includes the layer's own re-layout pass (codd_split_bf16) when ``xsl`` is given."""
    best, best_t = _time_cfgs(lib, p, pc, cands, lambda c: _set_cfg(p, c, pc), "b%d %dx%d k%dx%d %d->%d out %dx%d" % (
        p.terms, p.sy, p.sx, pc.kh, pc.kw, pc.cin, pc.cout, p.Hout, p.Wout))
    if best_t == float("inf"):
        raise _abi.CoddHipError("no split-bf16 launch configuration for conv %dx%d %d->%d" % (pc.kh, pc.kw, pc.cin, pc.cout))
    # the re-layout pass of the winner (private tensor of exactly its size); none when the input exists in split form
    t_split = 0.0
    if xsl is not None:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        _make_split(lib, p, xsl, x2, [best])
        s.record()
        for _ in range(3):
            keep = _make_split(lib, p, xsl, x2, [best])  # noqa: F841
        e.record()
        e.synchronize()
        t_split = s.elapsed_time(e) / 3.0
    return best, best_t + t_split


_AUTOTUNE = False  # enable_autotune()
AUTOTUNE_LOG = []  # (layer description, heuristic cfg, us, chosen cfg, us) of every tuned launch shape
AUTOTUNE_TRACE = None  # dev (tools/sweep_update_block.py): a list collects (layer description, cfg, grid, us) of EVERY split-bf16 candidate timed


TUNE_DB = {}  # layer signature "cout,cin,kh,kw,mb,deconv|launch shape" -> stored launch configuration (decode_cfg)


def save_tune_db(path):
    import json
    with open(path, "w") as f:
        json.dump({k: list(v) for k, v in TUNE_DB.items()}, f, indent=0, sort_keys=True)


def load_tune_db(path=None):
    """path = None: the db shipped with the library (codd_amd/tuned/mi355x.json, tuned on an MI355X)."""
    import json
    if path is None:
        path = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "tuned", "mi355x.json")
    TUNE_DB.update({k: tuple(v) for k, v in json.load(open(path)).items()})


def enable_autotune(flag=True, shipped=True):
    """Measure-don't-guess launch configuration: the first (eager, un-captured) launch of every
    (layer, shape) times the heuristic (npb, nw, ck, mb, layout) against every other configuration the kernels
    are instantiated for and keeps the fastest for the rest of the process (bench.py and the CLI turn this on;
    the tests run the deterministic heuristics).  ``shipped``: start from codd_amd/tuned/mi355x.json (the
    configurations found on an MI355X for the 960x576 workload), so that known layer signatures are not timed
    again.  Different chunk depths / layouts change the fp32 summation order, nothing else."""
    global _AUTOTUNE
    _AUTOTUNE = bool(flag)
    if _AUTOTUNE and shipped and not TUNE_DB:
        try:
            load_tune_db()
        except (OSError, ValueError):
            pass


def _autotune(lib, p, pc, default):
    """-> (configuration, ms): the heuristic exact-fp32 configuration ``default`` (npb, nw, ck, mb, layout) timed against
    every other one the kernels are instantiated for (_time_cfgs)."""
    p.terms = 0
    cin_pad = -(-pc.cin // 4) * 4
    cks = sorted({c for c in (8, 12, 16, 24, 32) if c <= cin_pad} | {min(cin_pad, 32)})
    mbs = [m for m in (1, 2, 4) if m == pc.mb or (16 * m <= max(16, -(-pc.cout_eff // 16) * 16) and pc.cout_eff > 16)]
    cands = [default]
    for mb in mbs:
        for npb in (1, 2, 4):
            for nw in ((4, 9, 2, 8) if npb == 1 else (4,)):
                for ck in cks:
                    if (npb, nw, ck, mb, 0) not in cands:
                        cands.append((npb, nw, ck, mb, 0))
    if p.sx <= 2 and cin_pad >= 16:  # quad layout (ds_read_b128 operands): ck 16 / 32
        for mb in mbs:
            for npb, nw in ((1, 4), (2, 4), (4, 4), (1, 9)):
                for ck in (16, 32):
                    if ck <= max(16, cin_pad):
                        cands.append((npb, nw, ck, mb, 1))
    return _time_cfgs(lib, p, pc, cands, lambda c: _set_cfg(p, c, pc), "%dx%d k%dx%d %d->%d out %dx%d" % (
        p.sy, p.sx, pc.kh, pc.kw, pc.cin, pc.cout, p.Hout, p.Wout))


# ---------------------------------------------------------------------------- rolling-window convolutions
# (csrc/conv_roll.hip, include/codd_hip.h codd_conv_roll): one 3x3, a pair of 3x3 (BasicBlock / merge tail) or a
# 1x1 -> 3x3 pair per launch for HITNet's large 16- / 32-channel maps.  `USE_ROLL` (default on), maps of at
# least ROLL_MIN_PIXELS pixels (below that a 64-column strip grid cannot fill the chip and the tile kernels win).
USE_ROLL = True
ROLL_MIN_PIXELS = 2 * 288 * 480


def use_roll(C, B, Cin_unused, H, W):
    """Rolling-window launch for a C-channel stride-1 layer (pair) on a [B, *, H, W] map?  Measured on MI355X
    (tools/time_roll.py): 16 channels at >= 288x480x2 pixels 1.4-1.8x the tile kernels; the 32-channel class has too
    few 64-column strips on HITNet's half-resolution maps to fill 256 CUs and stays on the tile kernels.  The kernel is
    exact fp32: under the plain bf16 mode (bf16 operands EVERYWHERE, BASELINE.json configs[4]) the layers stay on the bf16
    tile kernels so that the mode's dtype description holds."""
    return (USE_ROLL and CONV_PRECISION in ("split", "split16", "fp32") and C == 16
            and B * H * W >= ROLL_MIN_PIXELS)


class PackedRoll:
    """Weights of one codd_conv_roll launch.  ``stages``: one or two dicts(w [cout,cin,k,k], b | None, act); k = 3
    for every stage except that the FIRST of two may be 1x1 (then cin <= 64).  C = the output channels of every stage
    (16 | 32); ``residual``: add the chain input to the last stage (pair of 3x3 only)."""

    def __init__(self, stages, residual=False):
        lib = _abi.load()
        assert len(stages) in (1, 2)
        w0 = stages[0]["w"]
        _require_gpu(w0)
        ks = [int(st["w"].shape[2]) for st in stages]
        self.C = int(stages[-1]["w"].shape[1]) if len(stages) == 2 else int(w0.shape[1])
        self.cin = int(w0.shape[1])
        self.cout = int(stages[-1]["w"].shape[0])
        if len(stages) == 1:
            self.mode = 0
        else:
            self.mode = 1 if ks[0] == 3 else 2
        assert ks[-1] == 3 and (ks[0] in (1, 3)) and self.C in (16, 32), (ks, self.C)
        assert not residual or self.mode == 1
        self.residual = bool(residual)
        self.acts = [ACT[st.get("act", "none")] for st in stages]
        self.w, self.b = [], []
        for st, k in zip(stages, ks):
            w = st["w"].detach().float().contiguous()
            cout, cin = int(w.shape[0]), int(w.shape[1])
            assert cout <= self.C and (k == 1 or cin == self.C), (cout, cin, self.C)
            n = lib.codd_roll_packed_size(self.C, k, cin)
            if n <= 0:
                raise _abi.CoddHipError("conv_roll: unsupported stage %dx%d %d->%d" % (k, k, cin, cout))
            buf = torch.empty(n, device=w.device, dtype=torch.float32)
            _abi.check(lib.codd_roll_pack_weights(w.data_ptr(), buf.data_ptr(), self.C, cout, cin, k, _stream()), "roll_pack")
            self.w.append(buf)
            b = st.get("b")
            if b is not None:
                bb = torch.zeros(self.C, device=w.device, dtype=torch.float32)
                bb[:cout] = b.detach().float()
                b = bb
            self.b.append(b)


def _roll_rh(B, H, W, mode):
    """Output rows per workgroup: the largest row block that still gives every CU ~3 workgroups (the strips of a
    launch are independent; a row block re-reads `lag` rows of its neighbour and idles for the pipeline fill)."""
    stride = 60 if mode == 1 else 62
    strips = -(-W // stride) * B
    want = 3 * 256
    nrb = max(1, -(-want // strips))
    return max(4, -(-H // nrb))


def conv_roll(x, pr, x2=None, out=None, cout_store=None, rh=None):
    """Run the packed rolling-window launch on (x | x2) -> out [B, cout_store, H, W] (tensor or Slice)."""
    lib = _abi.load()
    xs = _as_slice(x)
    _require_gpu(xs.buf)
    B, C0, H, W = xs.shape
    C1 = 0 if x2 is None else _as_slice(x2).c
    assert C0 + C1 == pr.cin, (C0, C1, pr.cin)
    cs = pr.cout if cout_store is None else cout_store
    if out is None:
        out = torch.empty(B, cs, H, W, device=xs.buf.device, dtype=torch.float32)
    os_ = _as_slice(out)
    assert os_.shape == (B, cs, H, W), (os_.shape, (B, cs, H, W))
    p = _abi.RollParams()
    p.in0, p.in1, p.C0, p.C1, p.B, p.H, p.W = _view(xs), _view(x2), C0, C1, B, H, W
    p.C, p.mode = pr.C, pr.mode
    p.wA, p.bA = pr.w[0].data_ptr(), None if pr.b[0] is None else pr.b[0].data_ptr()
    p.actA = pr.acts[0]
    if pr.mode != 0:
        p.wB, p.bB = pr.w[1].data_ptr(), None if pr.b[1] is None else pr.b[1].data_ptr()
        p.actB = pr.acts[1]
    p.residual = int(pr.residual)
    p.out, p.out_ctot, p.out_coff, p.cout_store = os_.buf.data_ptr(), os_.buf.shape[1], os_.coff, cs
    p.rh = _roll_rh(B, H, W, pr.mode) if rh is None else rh
    _abi.check(_launch_roll(lib, p, _stream()), "codd_conv_roll")
    return out


def _launch_roll(lib, p, stream):
    """Single choke point of every rolling-window launch (bench.py wraps it with HIP events)."""
    return lib.codd_conv_roll(C.byref(p), stream)


# ----------------------------------------------------------------------------------------- stereo
def tile_costvol_argmin(tl, tr, D, cost, hyp):
    """cost: Slice (1 ch) receiving the min cost; hyp: Slice whose channels 0..2 receive (d, 0, 0)."""
    lib = _abi.load()
    _require_gpu(tl)
    B, Cc, Ht, Wt = tl.shape
    cs, hs = _as_slice(cost), _as_slice(hyp)
    _abi.check(lib.codd_tile_costvol_argmin(tl.data_ptr(), tr.data_ptr(), B, Cc, Ht, Wt, tr.shape[3], D,
                                            cs.buf.data_ptr(), cs.buf.shape[1], cs.coff,
                                            hs.buf.data_ptr(), hs.buf.shape[1], hs.coff, 1, _stream()),
               "tile_costvol_argmin")


def tile_warp_cost(fl, fr, hyp0, hyp1=None):
    """-> one or two [B,64,Ht,Wt] tensors ([fea 16 | cv 48])."""
    lib = _abi.load()
    _require_gpu(fl)
    B, Cc, H, W = fl.shape
    Ht, Wt = H // 4, W // 4
    out0 = torch.empty(B, 64, Ht, Wt, device=fl.device, dtype=torch.float32)
    out1 = torch.empty_like(out0) if hyp1 is not None else None
    _abi.check(lib.codd_tile_warp_cost(fl.data_ptr(), fr.data_ptr(), B, Cc, Ht, Wt, _view(hyp0), _view(hyp1),
                                       2 if hyp1 is not None else 1, out0.data_ptr(),
                                       None if out1 is None else out1.data_ptr(), _stream()), "tile_warp_cost")
    return out0, out1


def hyp_upsample(h, scale, out):
    lib = _abi.load()
    hs, os_ = _as_slice(h), _as_slice(out)
    B, _, hh, ww = hs.shape
    _abi.check(lib.codd_hyp_upsample(_view(hs), B, hh, ww, float(scale), os_.buf.data_ptr(), os_.buf.shape[1],
                                     os_.coff, _stream()), "hyp_upsample")
    return out


def hyp_select(upd, cur, prev, out):
    lib = _abi.load()
    B, _, hh, ww = upd.shape
    os_ = _as_slice(out)
    _abi.check(lib.codd_hyp_select(upd.data_ptr(), _view(cur), _view(prev), B, hh, ww, os_.buf.data_ptr(),
                                   os_.buf.shape[1], os_.coff, _stream()), "hyp_select")
    return out


# ----------------------------------------------------------------------------------------- motion
def _f32(*shape, like):
    return torch.empty(*shape, device=like.device, dtype=torch.float32)


def instnorm(x, relu=True, res=None, res_relu=False, xs_out=None, want_fp32=True):
    """InstanceNorm2d(+ReLU).  Plain form: relu(norm(x) + res).  With ``xs_out`` (a split_buffer tensor of the same
    size) the result is written as split-bf16 records -- the next convolution's input -- by the apply pass itself:
    v = norm(x); relu; [+ res; res_relu]; the fp32 tensor is only written (and returned) when ``want_fp32``."""
    lib = _abi.load()
    _require_gpu(x)
    B, Cc, H, W = x.shape
    stats = _f32(128 * B * Cc, like=x)
    if xs_out is not None:
        assert (xs_out.B, xs_out.H, xs_out.W) == (B, H, W) and Cc % 8 == 0 and Cc <= 8 * xs_out.c8
        y = torch.empty_like(x) if want_fp32 else None
        _abi.check(lib.codd_instnorm_xs(x.data_ptr(), B, Cc, H, W, stats.data_ptr(), _ptr(res), int(relu), int(res_relu),
                                        _ptr(y), _xs_view(xs_out), _stream()), "instnorm_xs")
        return y
    assert not res_relu
    y = torch.empty_like(x)
    _abi.check(lib.codd_instnorm(x.data_ptr(), B, Cc, H * W, stats.data_ptr(),
                                 None if res is None else res.data_ptr(), int(relu), y.data_ptr(), _stream()),
               "instnorm")
    return y


# configurations (xb, th, ck, mb, 2, pgw, cgw, 3, ks) tried, in order, for the split-bf16 all-pairs "convolution"
# (1x1, Cout = h*w source pixels, Cin = 128): 64-channel groups, whole 32-channel chunks
_ALLPAIRS_CFGS = ((2, 8, 32, 4, 2, 4, 2, 3, 1), (1, 16, 32, 4, 2, 4, 2, 3, 1), (1, 16, 32, 4, 2, 4, 1, 3, 1), (1, 12, 32, 4, 2, 4, 2, 3, 1),
                  (1, 12, 32, 4, 2, 4, 1, 3, 1), (1, 10, 32, 4, 2, 2, 2, 3, 1), (2, 8, 32, 4, 2, 4, 1, 3, 1),
                  (1, 8, 32, 2, 2, 4, 1, 3, 1), (1, 8, 16, 2, 2, 4, 1, 3, 1))
_ALLPAIRS_PICK = {}  # (D, hh, ww) -> configuration (timed once per shape when autotuning, else the first accepted)


def allpairs_corr_split(f1, f2):
    """The all-pairs pyramid on the split-bf16 convolution kernel (3 bf16 MFMAs per product, fp32 accumulate): level i =
    a 1x1 "convolution" of the i-times pooled f2 (as split records) whose output channels are the h*w source pixels and
    whose weights are f1^T / 16, re-packed every frame.  Level 0 writes 299 MB at 960x576: on the exact-fp32 MFMA kernel
    it was compute-bound at 0.87 TB/s (345 us); here it is write-bound."""
    lib = _abi.load()
    _require_gpu(f1)
    B, D, h, w = f1.shape
    N = h * w
    lv = [_f32(B, N, (h >> i) * (w >> i), like=f1) for i in range(4)]
    srcs = [f2.contiguous()]
    for i in range(1, 4):
        hh, ww = h >> (i - 1), w >> (i - 1)
        nxt = _f32(B, D, hh >> 1, ww >> 1, like=f1)
        _abi.check(lib.codd_avgpool2(srcs[-1].data_ptr(), B * D, hh, ww, nxt.data_ptr(), _stream()), "avgpool2")
        srcs.append(nxt)
    packs = {}
    tune = _AUTOTUNE and not torch.cuda.is_current_stream_capturing()
    for i, src in enumerate(srcs):
        hh, ww = h >> i, w >> i
        p = ConvParams()
        p.C0, p.C1, p.B, p.Hin, p.Win, p.Cout, p.Hout, p.Wout = D, 0, 1, hh, ww, N, hh, ww
        p.kh = p.kw = p.sy = p.sx = p.dil_y = p.dil_x = 1
        p.terms, p.out_ctot = _split_terms(), N
        key = (D, hh, ww)
        cfg = _ALLPAIRS_PICK.get(key)
        if cfg is None:
            ok = [c for c in _ALLPAIRS_CFGS if _cfg_ok(lib, p, c)]
            if not ok:
                raise _abi.CoddHipError("all-pairs: no split-bf16 configuration for a %dx%d map" % (hh, ww))
            # the timing may only choose among configurations that give THE SAME BITS (tile shape and wave grid do not
            # change a sum, the chunk depth does): a pick that depended on the box would make the pyramid -- and with it
            # every selection downstream -- differ from lease to lease
            if any(decode_cfg(c).ck == 32 for c in ok):
                ok = [c for c in ok if decode_cfg(c).ck == 32]
            cfg = _allpairs_tune(lib, p, ok, f1[0], N, D) if tune else ok[0]
            if tune:
                _ALLPAIRS_PICK[key] = cfg  # (un-tuned picks are not remembered: a later eager call may still time them)
        f = decode_cfg(cfg)
        xs = _make_split(lib, p, src, None, [cfg], B=B)
        for b in range(B):
            if (f.mb, f.ck, b) not in packs:  # weights[co = n1][ci = d] = f1[b, d, n1] / 16 for this (mb, ck)
                packs[(f.mb, f.ck, b)] = _pack_bf16(f1[b], N, D, 1, 1, f.mb, f.ck, p.terms, 1, N, 1.0 / 16.0)
            p.wpacked = packs[(f.mb, f.ck, b)].data_ptr()
            p.out = lv[i][b].data_ptr()
            p.xs = xs.buf.data_ptr() + b * (xs.buf.numel() // B)
            _set_cfg(p, cfg)
            _abi.check(_launch_conv(lib, p, _stream()), "allpairs conv")
    return lv


def _allpairs_tune(lib, p, cands, f1b, N, D):
    """Time the accepted all-pairs configurations on this level's shape (_time_cfgs; own split input / weights per
    candidate)."""
    src = torch.zeros(1, D, p.Hin, p.Win, device=f1b.device)

    def apply(c):
        f = decode_cfg(c)
        xs = _make_split(lib, p, src, None, [c])
        wp = _pack_bf16(f1b, N, D, 1, 1, f.mb, f.ck, p.terms, 1, N, 1.0 / 16.0)
        p.wpacked = wp.data_ptr()
        _set_cfg(p, c)
        return xs, wp

    return _time_cfgs(lib, p, None, cands, apply, "allpairs %dx%d" % (p.Hin, p.Win))[0]


def allpairs_corr(f1, f2, split=None):
    """-> 4 pyramid levels [B, h*w, (h>>i)*(w>>i)] (reference blocks/corr.py:28-45).  ``split`` (default: the "split"
    conv precision is active): the GEMMs run on the split-bf16 kernel (allpairs_corr_split), else on exact-fp32 MFMA."""
    if split is None:
        split = CONV_PRECISION in _SPLIT_MODES
    if split:
        return allpairs_corr_split(f1, f2)
    lib = _abi.load()
    _require_gpu(f1)
    B, D, h, w = f1.shape
    lv = [_f32(B, h * w, (h >> i) * (w >> i), like=f1) for i in range(4)]
    scratch = _f32(lib.codd_allpairs_corr_scratch(B, D, h, w), like=f1)
    _abi.check(lib.codd_allpairs_corr(f1.data_ptr(), f2.data_ptr(), B, D, h, w, lv[0].data_ptr(), lv[1].data_ptr(),
                                      lv[2].data_ptr(), lv[3].data_ptr(), scratch.data_ptr(), _stream()),
               "allpairs_corr")
    return lv


def corr_lookup(pyr, coords, h, w, out=None):
    """coords [B,h,w,>=2] (x,y,...) -> [B,196,h,w]."""
    lib = _abi.load()
    B = coords.shape[0]
    if out is None:
        out = _f32(B, 196, h, w, like=coords)
    _abi.check(lib.codd_corr_lookup(pyr[0].data_ptr(), pyr[1].data_ptr(), pyr[2].data_ptr(), pyr[3].data_ptr(),
                                    coords.data_ptr(), coords.shape[-1], B, h, w, out.data_ptr(), _stream()),
               "corr_lookup")
    return out


def raft_geometry(T, d1, d2, K8):
    lib = _abi.load()
    B, h, w, _ = T.shape
    xyz = _f32(B, h, w, 3, like=T)
    minfo = _f32(B, 9, h, w, like=T)
    _abi.check(lib.codd_raft_geometry(T.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, h, w, *K8, xyz.data_ptr(),
                                      minfo.data_ptr(), _stream()), "raft_geometry")
    return xyz, minfo


def raft_geometry_lookup(T, d1, d2, K8, pyr, minfo_xs=None, corr_xs=None):
    """raft_geometry + corr_lookup in one launch -> (xyz [B,h,w,3], minfo [B,9,h,w], corr [B,196,h,w]).
    With ``minfo_xs`` / ``corr_xs`` (split_buffer tensors of 9 / 196 channels) the two tensor results are written
    directly as split-bf16 records -- the encoder convolutions' input form -- and (xyz, None, None) is returned."""
    lib = _abi.load()
    B, h, w, _ = T.shape
    if corr_xs is not None:
        xyz = _f32(B, h, w, 3, like=T)
        _abi.check(lib.codd_raft_geometry_lookup_xs(T.data_ptr(), d1.data_ptr(), d2.data_ptr(), pyr[0].data_ptr(),
                                                    pyr[1].data_ptr(), pyr[2].data_ptr(), pyr[3].data_ptr(), B, h, w,
                                                    *K8, xyz.data_ptr(), _xs_view(minfo_xs), _xs_view(corr_xs),
                                                    _stream()), "raft_geometry_lookup_xs")
        return xyz, None, None
    xyz, minfo, out = _f32(B, h, w, 3, like=T), _f32(B, 9, h, w, like=T), _f32(B, 196, h, w, like=T)
    _abi.check(lib.codd_raft_geometry_lookup(T.data_ptr(), d1.data_ptr(), d2.data_ptr(), pyr[0].data_ptr(),
                                             pyr[1].data_ptr(), pyr[2].data_ptr(), pyr[3].data_ptr(), B, h, w, *K8,
                                             xyz.data_ptr(), minfo.data_ptr(), out.data_ptr(), _stream()),
               "raft_geometry_lookup")
    return xyz, minfo, out


def se3_gn_step(T, ae, xyz, delta, weight, d1, K8, radius=32, lm=1e-4, ep=10.0):
    """In-place Gauss-Newton update of the SE3 field T [B,h,w,7]."""
    lib = _abi.load()
    B, h, w, _ = T.shape
    scratch = _f32(lib.codd_se3_gn_scratch(B, h, w, radius), like=T)
    _abi.check(lib.codd_se3_gn_step(T.data_ptr(), ae.data_ptr(), ae.shape[1], xyz.data_ptr(), delta.data_ptr(),
                                    weight.data_ptr(), d1.data_ptr(), B, h, w, *K8, radius, lm, ep,
                                    scratch.data_ptr(), _stream()), "se3_gn_step")
    return T


def se3_gn_step_heads(T, hidden_xs, head_w, head_b, xyz, d1, K8, radius=32, lm=1e-4, ep=10.0):
    """se3_gn_step with the ae / delta / weight 1x1 heads computed inside the record-packing kernel from the hidden
    channels in split form (``hidden_xs``: 768 channels); returns the confidence weights [B,3,h,w]."""
    lib = _abi.load()
    B, h, w, _ = T.shape
    scratch = _f32(lib.codd_se3_gn_scratch(B, h, w, radius), like=T)
    wout = _f32(B, 3, h, w, like=T)
    _abi.check(lib.codd_se3_gn_step_heads(T.data_ptr(), _xs_view(hidden_xs), head_w.data_ptr(), head_b.data_ptr(),
                                          xyz.data_ptr(), d1.data_ptr(), B, h, w, *K8, radius, lm, ep, wout.data_ptr(),
                                          scratch.data_ptr(), _stream()), "se3_gn_step_heads")
    return wout


def cvx_upsample(data, mask, mode):
    """mode 0: [B,h,w,D] -> [B,8h,8w,D]; 1: SE3 field [B,h,w,7]; 2: [B,D,h,w] -> [B,D,8h,8w]."""
    lib = _abi.load()
    if mode == 2:
        B, D, h, w = data.shape
        out = _f32(B, D, 8 * h, 8 * w, like=data)
    else:
        B, h, w, D = data.shape
        out = _f32(B, 8 * h, 8 * w, D, like=data)
    _abi.check(lib.codd_cvx_upsample(data.data_ptr(), mask.data_ptr(), B, h, w, D, mode, out.data_ptr(), _stream()),
               "cvx_upsample")
    return out


def cvx_upsample_se3_weight(T, weight, mask):
    """cvx_upsample(T, mask, 1) and cvx_upsample(weight, mask, 2) in one launch (the mask is read once)."""
    lib = _abi.load()
    B, h, w, _ = T.shape
    To, wo = _f32(B, 8 * h, 8 * w, 7, like=T), _f32(B, 3, 8 * h, 8 * w, like=T)
    _abi.check(lib.codd_cvx_upsample_se3_weight(T.data_ptr(), weight.data_ptr(), mask.data_ptr(), B, h, w, To.data_ptr(),
                                                wo.data_ptr(), _stream()), "cvx_upsample_se3_weight")
    return To, wo


def disp_to_depth(disp, bf):
    lib = _abi.load()
    out = torch.empty_like(disp)
    _abi.check(lib.codd_disp_to_depth(disp.data_ptr(), disp.numel(), float(bf), out.data_ptr(), _stream()),
               "disp_to_depth")
    return out


def subsample(x, oy, ox, step):
    """x[:, oy::step, ox::step] of a contiguous [B, H, W] map as a kernel of this library."""
    lib = _abi.load()
    _require_gpu(x)
    B, H, W = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32
    out = torch.empty(B, -(-(H - oy) // step), -(-(W - ox) // step), device=x.device, dtype=torch.float32)
    _abi.check(lib.codd_subsample(x.data_ptr(), B, H, W, oy, ox, step, out.data_ptr(), _stream()), "subsample")
    return out


def batch_pair(a, b):
    """torch.cat([a, b], 0) of two contiguous fp32 tensors of one shape as ONE copy kernel of this library (other dtypes:
    torch.cat, as before round 4)."""
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype != torch.float32:
        return torch.cat([a, b], 0)
    out = torch.empty((2 * a.shape[0],) + tuple(a.shape[1:]), device=a.device, dtype=torch.float32)
    copy_many([(out[:a.shape[0]], a.contiguous()), (out[a.shape[0]:], b.contiguous())])
    return out


def splat(T, depth, featA, featB, with_flow, H, W, oy, ox, ds, K, radius, bf=0.0):
    """T [B,HT,WT,7], depth [B,HT,WT] sampled at (oy+ds*y, ox+ds*x) -> (out [B,C,H,W], z [B,1,H,W])."""
    lib = _abi.load()
    B, HT, WT, _ = T.shape
    CA = 0 if featA is None else featA.shape[1]
    CB = 0 if featB is None else featB.shape[1]
    Cc = CA + (3 if with_flow else 0) + CB
    out = _f32(B, Cc, H, W, like=T)
    z = _f32(B, 1, H, W, like=T)
    scratch = torch.empty(lib.codd_splat_scratch(B, H, W, float(radius)), device=T.device, dtype=torch.int32)
    _abi.check(lib.codd_splat(T.data_ptr(), depth.data_ptr(), HT, WT, oy, ox, ds,
                              None if featA is None else featA.data_ptr(), CA,
                              None if featB is None else featB.data_ptr(), CB, int(with_flow), B, H, W, *K,
                              float(radius), float(bf), out.data_ptr(), z.data_ptr(), scratch.data_ptr(), _stream()),
               "splat")
    return out, z


def induced_flow(T, depth, K):
    lib = _abi.load()
    B, H, W, _ = T.shape
    out = _f32(B, H, W, 3, like=T)
    _abi.check(lib.codd_induced_flow(T.data_ptr(), depth.data_ptr(), B, H, W, *K, out.data_ptr(), _stream()),
               "induced_flow")
    return out


def context_split(x):
    lib = _abi.load()
    B, _, h, w = x.shape
    net, inp = _f32(B, 128, h, w, like=x), _f32(B, 384, h, w, like=x)
    _abi.check(lib.codd_context_split(x.data_ptr(), B, h * w, net.data_ptr(), inp.data_ptr(), _stream()),
               "context_split")
    return net, inp


def se3_identity(B, h, w, device):
    lib = _abi.load()
    T = torch.empty(B, h, w, 7, device=device, dtype=torch.float32)
    _abi.check(lib.codd_se3_identity(T.data_ptr(), B * h * w, _stream()), "se3_identity")
    return T


def resize_bilinear(x, size, align_corners, out=None, accumulate=False, relu=False, extra=None):
    """``extra`` (contiguous [B, C, Ho, Wo]; ``out`` then a whole tensor): out = relu?((out + extra) + blend) with
    ``accumulate``, (extra + blend) without -- an add_relu launch folded in with its rounding."""
    lib = _abi.load()
    B, Cc, Hi, Wi = x.shape
    Ho, Wo = size
    if out is None:
        out = _f32(B, Cc, Ho, Wo, like=x)
    os_ = _as_slice(out)
    if extra is not None:
        assert extra.is_contiguous() and tuple(extra.shape) == (B, Cc, Ho, Wo) and os_.buf.shape[1] == Cc and os_.coff == 0
        _abi.check(lib.codd_resize_bilinear_add(x.data_ptr(), B, Cc, Hi, Wi, Ho, Wo, int(align_corners), os_.buf.data_ptr(),
                                                os_.buf.shape[1], os_.coff, int(accumulate), int(relu), extra.data_ptr(),
                                                _stream()), "resize_bilinear_add")
        return out
    _abi.check(lib.codd_resize_bilinear(x.data_ptr(), B, Cc, Hi, Wi, Ho, Wo, int(align_corners), os_.buf.data_ptr(),
                                        os_.buf.shape[1], os_.coff, int(accumulate), int(relu), _stream()),
               "resize_bilinear")
    return out


def add_relu(a, b=None, relu=True, out=None):
    lib = _abi.load()
    if out is None:
        out = torch.empty_like(a)
    _abi.check(lib.codd_add_relu(a.data_ptr(), None if b is None else b.data_ptr(), a.numel(), int(relu),
                                 out.data_ptr(), _stream()), "add_relu")
    return out


def copy_many(pairs):
    """dst.copy_(src) for up to 8 (dst, src) pairs of contiguous fp32 tensors in one kernel launch (a kernel node under
    graph capture: see runtime.FrameRunner._capture); pairs that do not meet the 16-byte rules fall back to one
    codd_copy launch each (a kernel node under capture like the fast path; 32-bit words moved as integers: bit-exact,
    unlike an add of 0.f, which turns -0.0 into +0.0)."""
    import ctypes as C
    lib = _abi.load()
    fast = []
    for d, s in pairs:
        assert d.numel() == s.numel() and d.is_contiguous() and s.is_contiguous()
        if s.numel() == 0:  # (an empty tensor's pointer may be NULL, which the entry points reject)
            continue
        if s.numel() % 4 == 0 and s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0:
            fast.append((d, s))
        else:
            _abi.check(lib.codd_copy(s.data_ptr(), d.data_ptr(), s.numel(), _stream()), "copy")
    for i in range(0, len(fast), 8):
        chunk = fast[i:i + 8]
        n = len(chunk)
        srcs = (C.c_void_p * n)(*[s.data_ptr() for _, s in chunk])
        dsts = (C.c_void_p * n)(*[d.data_ptr() for d, _ in chunk])
        cnt = (C.c_longlong * n)(*[s.numel() for _, s in chunk])
        _abi.check(lib.codd_copy_many(srcs, dsts, cnt, n, _stream()), "copy_many")


def gru_gate_zr(t1, t2, inp, cor, mot, h):
    lib = _abi.load()
    B, _, hh, ww = h.shape
    zr, rh = _f32(B, 256, hh, ww, like=h), torch.empty_like(h)
    _abi.check(lib.codd_gru_gate_zr(t1.data_ptr(), t2.data_ptr(), inp.data_ptr(), _ptr(cor), _ptr(mot),
                                    h.data_ptr(), B, hh * ww, zr.data_ptr(), rh.data_ptr(), _stream()), "gru_gate_zr")
    return zr, rh


def _ptr(t):
    return None if t is None else t.data_ptr()


def _xs_view(st, coff=0):
    return _abi.XsView(st.buf.data_ptr(), st.c8, st.hp, st.wp, st.bt, st.bl, coff // 8, st.terms)


def gru_gate_zr_xs(t1, t2, inp, cor, mot, h, rh_xs):
    """gru_gate_zr writing r*h straight into the q convolutions' split-bf16 input (``rh_xs``: split_buffer) and only
    z as fp32: no fp32 r*h tensor, no re-layout launch.  Returns z [B,128,h,w]."""
    lib = _abi.load()
    B, _, hh, ww = h.shape
    z = torch.empty_like(h)
    _abi.check(lib.codd_gru_gate_zr_xs(t1.data_ptr(), t2.data_ptr(), inp.data_ptr(), _ptr(cor), _ptr(mot),
                                       h.data_ptr(), B, hh, ww, z.data_ptr(), _xs_view(rh_xs), _stream()),
               "gru_gate_zr_xs")
    return z


def gru_gate_q_xs(t1, t2, inp, cor, mot, z, h, h_xs):
    """gru_gate_q with ``z`` as returned by gru_gate_zr_xs; the new hidden state is returned as fp32 AND written as
    split records into ``h_xs`` (the input of the head convolution and of the next update's z|r convolutions)."""
    lib = _abi.load()
    B, _, hh, ww = h.shape
    ho = torch.empty_like(h)
    _abi.check(lib.codd_gru_gate_q_xs(t1.data_ptr(), t2.data_ptr(), inp.data_ptr(), _ptr(cor), _ptr(mot),
                                      z.data_ptr(), h.data_ptr(), B, hh, ww, ho.data_ptr(), _xs_view(h_xs), _stream()),
               "gru_gate_q_xs")
    return ho


def gru_gate_q(t1, t2, inp, cor, mot, zr, h):
    lib = _abi.load()
    B, _, hh, ww = h.shape
    ho = torch.empty_like(h)
    _abi.check(lib.codd_gru_gate_q(t1.data_ptr(), t2.data_ptr(), inp.data_ptr(), _ptr(cor), _ptr(mot),
                                   zr.data_ptr(), h.data_ptr(), B, hh * ww, ho.data_ptr(), _stream()), "gru_gate_q")
    return ho


class Fork:
    """Fork / join of independent launch chains over side HIP streams (parallel branches of the
    captured frame graph).  Discipline: every branch starts by waiting on the caller's stream, only
    the caller's stream consumes branch outputs, and ``join`` makes it wait for every branch used
    since the last join -- so the stream-tagged block re-use of the caching allocator stays safe."""

    serial = False  # debugging / per-launch timing: run every branch on the caller's stream

    def __init__(self, device, n):
        self.dev = device
        self.streams = [torch.cuda.Stream(device=device) for _ in range(n)]
        self.used = []
        self.inline = False  # this fork only: run the branches on the caller's stream (A/B switches of call sites)

    def run(self, i, fn, *a, **k):
        if Fork.serial or self.inline:
            return fn(*a, **k)
        cur = torch.cuda.current_stream(self.dev)
        s = self.streams[i]
        if s not in self.used:
            s.wait_stream(cur)
            self.used.append(s)
        with torch.cuda.stream(s):
            return fn(*a, **k)

    def join(self):
        cur = torch.cuda.current_stream(self.dev)
        for s in self.used:
            cur.wait_stream(s)
        self.used = []

    def prefork(self, origin=None):
        """Bring every branch stream into the caller's ORIGIN stream's dependency graph (default: the current stream)
        before the branches are first used from a stream that is itself a fork.  Under hipGraph capture (ROCm 7.2) a
        stream whose FIRST captured operation is a wait on an already-forked stream crashes hipGraphInstantiate; a
        stream that joined the capture through the origin stream can wait on forked streams freely."""
        if Fork.serial:
            return
        cur = torch.cuda.current_stream(self.dev) if origin is None else origin
        for s in self.streams:
            s.wait_stream(cur)


# ----------------------------------------------------------------------------------------- fusion
def fusion_cues_lr(pred_curr, pred_warp, feat_curr, feat_warp, fea_l, fea_r, dsub, patch=3, ds=4):
    """-> corr_feat [B, 3 patch^2 + 4, H/ds, W/ds]; writes (pc, pw) sub-sampled into the 2-channel Slice ``dsub``."""
    lib = _abi.load()
    B, _, H, W = pred_curr.shape
    corr = _f32(B, 3 * patch * patch + 4, H // ds, W // ds, like=pred_curr)
    ds_ = _as_slice(dsub)
    _abi.check(lib.codd_fusion_cues_lr(pred_curr.data_ptr(), pred_warp.data_ptr(), feat_curr.data_ptr(),
                                       feat_warp.data_ptr(), fea_l.data_ptr(), fea_r.data_ptr(), B, H, W, patch, ds,
                                       feat_curr.shape[1], fea_l.shape[1], corr.data_ptr(), ds_.buf.data_ptr(),
                                       ds_.buf.shape[1], ds_.coff, _stream()), "fusion_cues_lr")
    return corr


def fusion_cues_fr(pred_curr, pred_warp, flow_warp, conf_warp, patch=3):
    lib = _abi.load()
    B, _, H, W = pred_curr.shape
    out = _f32(B, 3 * patch * patch + 5, H, W, like=pred_curr)
    _abi.check(lib.codd_fusion_cues_fr(pred_curr.data_ptr(), pred_warp.data_ptr(), flow_warp.data_ptr(),
                                       conf_warp.data_ptr(), B, H, W, patch, out.data_ptr(), _stream()), "fusion_cues_fr")
    return out


def fusion_forget(pred_curr, pred_warp, flow_warp, conf_warp, weff, patch=3):
    """cues -> forget head -> sigmoid in one launch (codd_fusion_forget); ``weff`` = the merged head
    [W_eff 9 x nc | beta 9 | c0] (fusion.Fusion.forget_matrix).  -> wr [B,1,H,W]."""
    lib = _abi.load()
    B, _, H, W = pred_curr.shape
    assert weff.numel() == 9 * (3 * patch * patch + 5) + 10 and weff.is_contiguous()
    wr = torch.empty_like(pred_curr)
    _abi.check(lib.codd_fusion_forget(pred_curr.data_ptr(), pred_warp.data_ptr(), flow_warp.data_ptr(),
                                      conf_warp.data_ptr(), B, H, W, patch, weff.data_ptr(), wr.data_ptr(), _stream()),
               "fusion_forget")
    return wr


def fusion_blend(pred_curr, pred_warp, wf_lr, wr, ds=4):
    lib = _abi.load()
    B, _, H, W = pred_curr.shape
    fused, wf, wro = torch.empty_like(pred_curr), torch.empty_like(pred_curr), torch.empty_like(pred_curr)
    _abi.check(lib.codd_fusion_blend(pred_curr.data_ptr(), pred_warp.data_ptr(), wf_lr.data_ptr(), wr.data_ptr(),
                                     B, H, W, ds, fused.data_ptr(), wf.data_ptr(), wro.data_ptr(), _stream()),
               "fusion_blend")
    return fused, wf, wro


def timestamp(buf, idx):
    """(diagnostics) buf[idx] (int64, device) = device wall clock (100 MHz) when this launch runs on the current stream."""
    lib = _abi.load()
    _require_gpu(buf)
    _abi.check(lib.codd_timestamp(buf.data_ptr() + 8 * idx, _stream()), "timestamp")


def disp_metrics(pred, gt, crop_hw, lo, hi, thr, meters, scratch=None):
    """Accumulate EPE / threshold-rate of one frame into ``meters`` ([3] fp64 on the device)."""
    lib = _abi.load()
    _require_gpu(pred)
    B, _, H, W = pred.shape
    _same_hw(pred, gt)
    if scratch is None:
        scratch = torch.empty(3 * 128 * B, device=pred.device, dtype=torch.float64)
    _abi.check(lib.codd_disp_metrics(pred.data_ptr(), gt.data_ptr(), B, H, W, crop_hw[0], crop_hw[1], float(lo),
                                     float(hi), float(thr), scratch.data_ptr(), meters.data_ptr(), _stream()),
               "disp_metrics")
    return meters


def tepe_metrics(pred, gt, pred_prev, gt_prev, flow_prev, crop_hw, lo, hi, bf, meters, scratch=None, gt_mask=None,
                 gt2_prev=None):
    """Accumulate the temporal metrics of one frame pair into ``meters`` ([7] fp64 on the device).  ``gt_mask``: the map
    the current frame's validity is computed from (default ``gt``); ``gt2_prev``: second-frame ground-truth disparity in
    the previous frame's coordinates, replacing the flow-warped ground truth (include/codd_hip.h)."""
    lib = _abi.load()
    _require_gpu(pred)
    B, _, H, W = pred.shape
    _same_hw(pred, gt, pred_prev, gt_prev, flow_prev, gt_mask, gt2_prev)
    if scratch is None:
        scratch = torch.empty(6 * 128 * B, device=pred.device, dtype=torch.float64)
    _abi.check(lib.codd_tepe_metrics(pred.data_ptr(), gt.data_ptr(), pred_prev.data_ptr(), gt_prev.data_ptr(),
                                     flow_prev.data_ptr(), None if gt_mask is None else gt_mask.data_ptr(),
                                     None if gt2_prev is None else gt2_prev.data_ptr(),
                                     B, H, W, crop_hw[0], crop_hw[1], float(lo), float(hi),
                                     float(bf), scratch.data_ptr(), meters.data_ptr(), _stream()), "tepe_metrics")
    return meters


def _same_hw(ref, *ts):
    """GT / flow maps handed to the metric kernels must be padded like the prediction: the kernels index them with
    the prediction's strides (a smaller tensor would be read out of bounds)."""
    for t in ts:
        if t is not None and tuple(t.shape[-2:]) != tuple(ref.shape[-2:]):
            raise ValueError("metric inputs must share the prediction's padded size %s, got %s" % (
                tuple(ref.shape[-2:]), tuple(t.shape[-2:])))


def sceneflow_metrics(Ts, pred_prev, gt_disp_prev, gt_flow_prev, gt_disp_change, gt_flow_occ, crop_hw, lo, hi, bf, K,
                      meters, scratch=None):
    """Accumulate the five scene-flow sums of one frame pair into ``meters`` ([5] fp64 on the device)."""
    lib = _abi.load()
    _require_gpu(pred_prev)
    B, _, H, W = pred_prev.shape
    _same_hw(pred_prev, gt_disp_prev, gt_flow_prev, gt_disp_change, gt_flow_occ)
    if tuple(Ts.shape) != (B, H, W, 7):
        raise ValueError("Ts must be [B,H,W,7] at the prediction's padded size")
    occ = None if gt_flow_occ is None else gt_flow_occ.to(torch.uint8).contiguous()
    if scratch is None:
        scratch = torch.empty(5 * 128 * B, device=pred_prev.device, dtype=torch.float64)
    _abi.check(lib.codd_sceneflow_metrics(Ts.contiguous().data_ptr(), pred_prev.data_ptr(), gt_disp_prev.data_ptr(),
                                          gt_flow_prev.data_ptr(), gt_disp_change.data_ptr(),
                                          None if occ is None else occ.data_ptr(), B, H, W, crop_hw[0], crop_hw[1],
                                          float(lo), float(hi), float(bf), *[float(v) for v in K], scratch.data_ptr(),
                                          meters.data_ptr(), _stream()), "sceneflow_metrics")
    return meters


IMAGENET_MEAN = (123.675, 116.28, 103.53)  # reference configs/datasets/custom.py:9
IMAGENET_STD = (58.395, 57.12, 57.375)


def preprocess(img_u8, bgr=True, mean=IMAGENET_MEAN, std=IMAGENET_STD, divisor=64):
    """uint8 [h,w,3] device image -> normalised, reflect-padded fp32 [1,3,H,W] (H, W multiples of 64)."""
    lib = _abi.load()
    _require_gpu(img_u8)
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous()
    h, w = img_u8.shape[:2]
    H, W = -(-h // divisor) * divisor, -(-w // divisor) * divisor
    out = torch.empty(1, 3, H, W, device=img_u8.device, dtype=torch.float32)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    _abi.check(lib.codd_preprocess(img_u8.data_ptr(), h, w, int(bgr), m, s, H, W, out.data_ptr(), _stream()),
               "preprocess")
    return out


def _ingest_args(left_u8, right_u8, out_left, out_right, src_ok, maps, map_shape, mean, std):
    """What the ingest wrappers share: the asserts on the source views (``src_ok``: shape or size of one) and on the output
    buffers, the four map pointers (None where a view has no maps) and the mean / std arrays -> (H, W, pointers, mean, std)."""
    for t in (left_u8, right_u8):
        assert t.dtype == torch.uint8 and src_ok(t) and t.is_contiguous() and t.is_cuda
    H, W = out_left.shape[-2:]
    for t in (out_left, out_right):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda and t.numel() == 3 * H * W
    ptrs = []
    for pair in (maps or (None, None)):
        for m in (pair or (None, None)):
            if m is not None:
                assert m.dtype == torch.float32 and tuple(m.shape) == tuple(map_shape) and m.is_contiguous() and m.is_cuda
            ptrs.append(None if m is None else m.data_ptr())
    return H, W, ptrs, (C.c_float * 3)(*mean), (C.c_float * 3)(*std)


def ingest_pair(left_u8, right_u8, out_left, out_right, bgr=True, maps=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """Both views of one frame in one launch: uint8 [h,w,3] device images -> normalised, reflect-padded fp32 written
    into the caller's [..,3,H,W] buffers (nothing is allocated).  ``maps``: None or ((lmx, lmy), (rmx, rmy)), fp32
    [h,w] device rectification maps per view (either pair may be None).  Without maps the result is bit-identical to
    ``preprocess`` of each view."""
    lib = _abi.load()
    _require_gpu(left_u8)
    h, w = left_u8.shape[:2]
    H, W, ptrs, m, s = _ingest_args(left_u8, right_u8, out_left, out_right, lambda t: tuple(t.shape) == (h, w, 3), maps, (h, w),
                                    mean, std)
    _abi.check(lib.codd_ingest_pair(left_u8.data_ptr(), right_u8.data_ptr(), h, w, int(bgr), m, s, *ptrs, H, W,
                                    out_left.data_ptr(), out_right.data_ptr(), _stream()), "ingest_pair")


FRAME_FORMATS = dict(mono8=1, yuyv=2, uyvy=3, nv12=4, bayer_rggb=5, bayer_grbg=6, bayer_gbrg=7,
                     bayer_bggr=8)  # CODD_FMT_* of include/codd_hip.h
YUV_MATRICES = dict(bt601=0, bt709=1, jpeg=2)  # CODD_YUV_*


def frame_bytes(fmt, h, w, pitch=None):
    """Bytes of one view of a raw ``fmt`` frame (codd_frame_bytes); ValueError for an invalid combination."""
    if fmt not in FRAME_FORMATS:
        raise ValueError(f"pixel format: one of {tuple(FRAME_FORMATS)} expected, got {fmt!r}")
    n = _abi.load().codd_frame_bytes(FRAME_FORMATS[fmt], int(h), int(w), int(pitch or 0))
    if n < 0:
        raise ValueError(f"{fmt}: invalid size {h}x{w} or pitch {pitch} (see codd_ingest_frames in include/codd_hip.h)")
    return n


def ingest_frames(left_u8, right_u8, out_left, out_right, fmt, shape, yuv="bt601", pitch=None, maps=None,
                  mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """``ingest_pair`` on raw camera frames: both views, flat or shaped uint8 device tensors of exactly
    ``frame_bytes(fmt, h, w, pitch)`` in format ``fmt`` (a key of FRAME_FORMATS), are decoded to RGB inside the launch
    (never in memory) and written normalised, rectified and reflect-padded into the caller's [..,3,H,W] buffers --
    the bits ``ingest_pair`` gives on the decoded images.  ``shape``: (h, w); ``yuv``: a key of YUV_MATRICES (ignored
    for mono and Bayer); ``pitch``: bytes per source row, None = tight; ``maps`` as ``ingest_pair``."""
    lib = _abi.load()
    _require_gpu(left_u8)
    h, w = int(shape[0]), int(shape[1])
    nbytes = frame_bytes(fmt, h, w, pitch)
    if yuv not in YUV_MATRICES:
        raise ValueError(f"yuv: one of {tuple(YUV_MATRICES)} expected, got {yuv!r}")
    H, W, ptrs, m, s = _ingest_args(left_u8, right_u8, out_left, out_right, lambda t: t.numel() == nbytes, maps, (h, w), mean, std)
    _abi.check(lib.codd_ingest_frames(left_u8.data_ptr(), right_u8.data_ptr(), FRAME_FORMATS[fmt], YUV_MATRICES[yuv], h, w,
                                      int(pitch or 0), m, s, *ptrs, H, W, out_left.data_ptr(), out_right.data_ptr(),
                                      _stream()), "ingest_frames")


CALIB_MODELS = dict(brown=0, fisheye=1)  # CODD_CALIB_* of include/codd_hip.h
CALIB_FORMATS = dict(rgb8=0, **FRAME_FORMATS)  # CODD_FMT_RGB8 next to the raw formats


def calib_structs(rect):
    """The two ``codd_calib_view`` structs of a ``calibration.Rectification`` -- or of a pair ``(left, right)`` of
    ``calibration.RectifiedView``s, either of which may be None (a view without calibration) -- as a tuple that
    ``rectify_maps`` and ``ingest_calibrated`` also take in place of ``rect``.  No device call."""
    if isinstance(rect, tuple) and len(rect) == 2 and all(v is None or isinstance(v, _abi.CalibView) for v in rect):
        return rect
    views = rect.views if hasattr(rect, "views") else tuple(rect)
    if len(views) != 2:
        raise ValueError("rect: a Rectification or a pair (left view, right view) expected")
    out = []
    for v in views:
        if v is None:
            out.append(None)
            continue
        s = _abi.CalibView()
        s.R[:] = [float(x) for row in v.R for x in row]
        s.f, s.cx, s.cy = float(v.P[0]), float(v.P[2]), float(v.P[3])
        s.K[:] = v.camera.K
        s.dist[:] = v.camera.dist8
        s.model = CALIB_MODELS[v.camera.model]
        out.append(s)
    return tuple(out)


def rectify_maps(rect, shape, device):
    """The rectifying maps of ``rect`` (as ``calib_structs`` takes it) for a rectified image of ``shape`` (h, w), computed
    on ``device``: ``((lmx, lmy), (rmx, rmy))``, fp32 [h,w] each -- what ``ingest_pair`` / ``ingest_frames`` take as
    ``maps`` and what ``cv2.remap`` takes; a view without calibration gives None in place of its pair."""
    lib = _abi.load()
    device = torch.device(device)
    if device.type != "cuda":
        raise _abi.CoddHipError("codd_amd ops run on ROCm devices only (no CPU fallback in the product path)")
    views = calib_structs(rect)
    h, w = int(shape[0]), int(shape[1])
    with torch.cuda.device(device):
        maps = tuple(None if v is None else tuple(torch.empty(h, w, dtype=torch.float32, device=device) for _ in range(2))
                     for v in views)
        ptrs = [None if p is None else m.data_ptr() for p in maps for m in (p or (None, None))]
        _abi.check(lib.codd_rectify_maps(*(None if v is None else C.byref(v) for v in views), h, w, *ptrs, _stream()),
                   "rectify_maps")
    return maps


def ingest_calibrated(left_u8, right_u8, out_left, out_right, rect, fmt, src_shape, shape, bgr=False, yuv="bt601",
                      pitch=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """``ingest_pair`` (``fmt`` "rgb8", with ``bgr``) and ``ingest_frames`` (a key of FRAME_FORMATS) in one launch that
    rectifies from a calibration: both views, uint8 device tensors of a ``src_shape`` = (hs, ws) frame in format ``fmt``
    (``pitch``: bytes per source row, None = tight), are sampled at the positions the map function of ``rect`` (as
    ``calib_structs`` takes it) gives for a rectified image of ``shape`` = (h, w), and written normalised and
    reflect-padded into the caller's [..,3,H,W] buffers -- the bits ``ingest_pair`` / ``ingest_frames`` give with the maps
    of ``rectify_maps(rect, shape)``, which are never in memory here.  A view without calibration takes the map-free
    path (then ``src_shape`` must equal ``shape``)."""
    lib = _abi.load()
    _require_gpu(left_u8)
    if fmt not in CALIB_FORMATS:
        raise ValueError(f"pixel format: one of {tuple(CALIB_FORMATS)} expected, got {fmt!r}")
    if yuv not in YUV_MATRICES:
        raise ValueError(f"yuv: one of {tuple(YUV_MATRICES)} expected, got {yuv!r}")
    hs, ws = int(src_shape[0]), int(src_shape[1])
    h, w = int(shape[0]), int(shape[1])
    if fmt == "rgb8":
        if hs <= 0 or ws <= 0 or (pitch is not None and int(pitch) < 3 * ws):
            raise ValueError(f"rgb8: invalid size {hs}x{ws} or pitch {pitch}")
        nbytes = hs * (3 * ws if pitch is None else int(pitch))
    else:
        nbytes = frame_bytes(fmt, hs, ws, pitch)
    views = calib_structs(rect)
    H, W, _, m, s = _ingest_args(left_u8, right_u8, out_left, out_right, lambda t: t.numel() == nbytes, None, None, mean, std)
    _abi.check(lib.codd_ingest_calibrated(left_u8.data_ptr(), right_u8.data_ptr(), CALIB_FORMATS[fmt], int(bool(bgr)),
                                          YUV_MATRICES[yuv], hs, ws, int(pitch or 0),
                                          *(None if v is None else C.byref(v) for v in views), h, w, m, s, H, W,
                                          out_left.data_ptr(), out_right.data_ptr(), _stream()), "ingest_calibrated")


EXPORT_MODES = dict(disp=0, depth=1, disp_u16=2)  # CODD_EXPORT_* of include/codd_hip.h


def export_depth(disp, out, mode="disp", calib=1.0):
    """The frame's padded disparity [1,1,H,W] -> the cropped [h,w] result in ``out`` (fp32, or uint16 for
    ``disp_u16``; caller-owned device staging buffer).  ``depth`` is calib / disp."""
    lib = _abi.load()
    _require_gpu(disp)
    H, W = disp.shape[-2:]
    h, w = out.shape
    assert disp.dtype == torch.float32 and disp.is_contiguous() and disp.numel() == H * W
    # (uint16 results may live in an int16 tensor: same bytes, and every torch build copies int16)
    assert out.is_cuda and out.is_contiguous() and out.dtype in ((torch.uint16, torch.int16) if mode == "disp_u16" else (torch.float32,))
    _abi.check(lib.codd_export_depth(disp.data_ptr(), H, W, h, w, EXPORT_MODES[mode], float(calib), out.data_ptr(),
                                     _stream()), "export_depth")
    return out


MOTION_MODES = dict(flow2d=0, flow_dd=1, sceneflow=2)  # CODD_MOTION_* of include/codd_hip.h
MOTION_CHANNELS = dict(flow2d=2, flow_dd=3, sceneflow=3)


def export_motion(T, disp_cur, depth_prev, out, mode, K, bf, scale=1.0, crop=None):
    """One launch per frame: the up-sampled SE3 field ``T`` [1,H,W,7] (or None: the frame has no field) and the
    previous frame's depth ``depth_prev`` [H,W] -> per-pixel motion of the cropped image in ``out`` [h,w,C] (fp32,
    caller-owned; untouched when T is None), on the previous frame's grid, NaN where a point is not in front of the
    camera; then depth_prev[:h,:w] becomes ``disp_to_depth(disp_cur, bf)[:h,:w]`` for the next frame.  ``mode``:
    'flow2d' (C=2, pixels), 'flow_dd' (C=3, flow + disparity change in pixels), 'sceneflow' (C=3, scale * (X1 - X0)).
    ``out`` may be None when T is None (only the roll runs); ``crop`` = (h, w) then says which part is rolled."""
    lib = _abi.load()
    _require_gpu(disp_cur)
    H, W = disp_cur.shape[-2:]
    if out is None:
        assert T is None and crop is not None
        h, w = int(crop[0]), int(crop[1])
    else:
        h, w, ch = out.shape
        assert ch == MOTION_CHANNELS[mode] and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    for t in (disp_cur, depth_prev):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == H * W
    if T is not None:
        assert T.dtype == torch.float32 and T.is_cuda and T.is_contiguous() and T.numel() == H * W * 7 and T.shape[-1] == 7
    _abi.check(lib.codd_export_motion(None if T is None else T.data_ptr(), disp_cur.data_ptr(), depth_prev.data_ptr(),
                                      H, W, h, w, MOTION_MODES[mode], *[float(v) for v in K], float(bf), float(scale),
                                      None if out is None else out.data_ptr(), _stream()), "export_motion")
    return out


def ego_motion_scratch(h, w):
    """Bytes of scratch ``ego_motion`` needs for an h x w crop (codd_ego_motion_scratch)."""
    n = int(_abi.load().codd_ego_motion_scratch(int(h), int(w)))
    if n <= 0:
        raise ValueError(f"ego_motion_scratch: positive (h, w) expected, got {(h, w)}")
    return n


def ego_motion(T, depth_prev, K, crop, record, moving, residual=None, scale=1.0, iters=5, delta_px=1.0, tau_px=2.0,
               min_valid=16, scratch=None):
    """The camera's rigid motion between the previous and the current frame, fitted robustly to the SE3 field ``T``
    [1,H,W,7] over the ``crop`` (h, w) of the previous frame's depth ``depth_prev`` [H,W] (read only), and the pixels
    that moved on their own (include/codd_hip.h, codd_ego_motion).  Outputs are caller-owned device tensors: ``record``
    fp32 [16] (scale * t, q_xyzw, ok, valid, inliers, rms_px, steps), ``moving`` uint8 [h,w] (0 static, 1 moving, 255
    invalid), ``residual`` fp32 [h,w] or None.  ``scratch``: a uint8 tensor of ``ego_motion_scratch(h, w)`` bytes;
    allocated here when None.  iters + 1 launches on the current stream, no host synchronisation."""
    lib = _abi.load()
    _require_gpu(T)
    H, W = depth_prev.shape[-2:]
    h, w = int(crop[0]), int(crop[1])
    assert T.dtype == torch.float32 and T.is_cuda and T.is_contiguous() and T.numel() == H * W * 7 and T.shape[-1] == 7
    assert depth_prev.dtype == torch.float32 and depth_prev.is_cuda and depth_prev.is_contiguous() and depth_prev.numel() == H * W
    assert record.dtype == torch.float32 and record.is_cuda and record.is_contiguous() and record.numel() == 16
    assert moving.dtype == torch.uint8 and moving.is_cuda and moving.is_contiguous() and tuple(moving.shape) == (h, w)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.is_cuda and residual.is_contiguous() and tuple(residual.shape) == (h, w)
    if scratch is None:
        scratch = torch.empty(ego_motion_scratch(h, w), dtype=torch.uint8, device=T.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_ego_motion(T.data_ptr(), depth_prev.data_ptr(), H, W, h, w, *[float(v) for v in K], float(scale),
                                   int(iters), float(delta_px), float(tau_px), int(min_valid), scratch.data_ptr(),
                                   scratch.numel(), record.data_ptr(), moving.data_ptr(),
                                   None if residual is None else residual.data_ptr(), _stream()), "ego_motion")
    return record


CONF_OUT_OF_VIEW, CONF_OCCLUDED, CONF_MISMATCH, CONF_INVALID = 1, 2, 4, 128  # CODD_CONF_* of include/codd_hip.h


def export_confidence(disp, flags, residual=None, left=None, right=None, crop=None, occ_px=1.0, tau=24.0, std=IMAGENET_STD):
    """One launch per frame: which pixels of the padded disparity ``disp`` [H,W] (or [1,1,H,W]) to trust, inside the
    ``crop`` (h, w) (default: the shape of ``flags``).  ``flags`` uint8 [h,w] (caller-owned) gets the CONF_* bits:
    OUT_OF_VIEW (the match falls left of the right image), OCCLUDED (another pixel of the row lands on the same right
    column with a disparity more than ``occ_px`` larger), INVALID (disparity not finite or not > 0) and, with the
    normalised images ``left`` / ``right`` [3,H,W] (or [1,3,H,W]; as preprocess / ingest_pair wrote them with ``std``),
    MISMATCH (the photometric residual exceeds ``tau`` grey levels); ``residual`` fp32 [h,w] or None gets that residual,
    NaN where invalid or out of view (include/codd_hip.h, codd_export_confidence)."""
    lib = _abi.load()
    _require_gpu(disp)
    H, W = disp.shape[-2:]
    h, w = (int(crop[0]), int(crop[1])) if crop is not None else tuple(flags.shape)
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    assert flags.dtype == torch.uint8 and flags.is_cuda and flags.is_contiguous() and tuple(flags.shape) == (h, w)
    assert (left is None) == (right is None), "left and right are given together or not at all"
    for t in (left, right):
        if t is not None:
            assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == 3 * H * W
            assert tuple(t.shape[-3:]) == (3, H, W)
    if residual is not None:
        assert left is not None, "residual needs the images"
        assert residual.dtype == torch.float32 and residual.is_cuda and residual.is_contiguous() and tuple(residual.shape) == (h, w)
    s = (C.c_float * 3)(*std) if left is not None else None
    _abi.check(lib.codd_export_confidence(disp.data_ptr(), None if left is None else left.data_ptr(),
                                          None if right is None else right.data_ptr(), H, W, h, w, s, float(occ_px),
                                          float(tau), flags.data_ptr(), None if residual is None else residual.data_ptr(),
                                          _stream()), "export_confidence")
    return flags


def epipolar_scratch(h, w):
    """Bytes of scratch ``epipolar_check`` needs for an h x w crop (codd_epipolar_scratch)."""
    n = int(_abi.load().codd_epipolar_scratch(int(h), int(w)))
    if n <= 0:
        raise ValueError(f"epipolar_scratch: positive (h, w) with h w < 2^31 expected, got {(h, w)}")
    return n


def epipolar_check(disp, left, right, K, shape, record, dy_map=None, scratch=None, range_px=2, step=2, tau=24.0,
                   min_curv=0.5, iters=4, delta_px=0.25, min_valid=256, std=IMAGENET_STD):
    """Is the rig still rectified?  Per measured pixel (every ``step``-th column and row) of the ``shape`` (h, w) crop the
    row offset ``dy`` at which the normalised ``right`` image [3,H,W] (or [1,3,H,W]) really matches ``left`` under the padded
    disparity ``disp`` [H,W] (or [1,1,H,W]) -- ``L(x, y) ~ R(x - d, y + dy)``, searched over ``-range_px .. range_px`` rows
    -- and a robust fit ``dy = fy (c0 (1 + yn^2) + c1 xr yn + c2 xr + c3 yn)`` of that map with ``K`` = (fx, fy, cx, cy): a
    rotation of the right view by (-c0, c1, c2) radians and a focal error c3 (include/codd_hip.h, codd_epipolar_check).
    Outputs are caller-owned device tensors: ``record`` float64 [32] (c, ok, measurable, inliers, rms of dy, rms of the
    inliers' residual, steps, the last step's A and b); ``dy_map`` fp32 [h,w] or None, NaN where nothing was measured.
    ``scratch``: a uint8 tensor of ``epipolar_scratch(h, w)`` bytes; allocated here when None.  2 + iters launches on the
    current stream, no host synchronisation."""
    lib = _abi.load()
    _require_gpu(disp)
    H, W = disp.shape[-2:]
    h, w = int(shape[0]), int(shape[1])
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    for t in (left, right):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == 3 * H * W
        assert tuple(t.shape[-3:]) == (3, H, W)
    assert record.dtype == torch.float64 and record.is_cuda and record.is_contiguous() and record.numel() == 32
    if dy_map is not None:
        assert dy_map.dtype == torch.float32 and dy_map.is_cuda and dy_map.is_contiguous() and tuple(dy_map.shape) == (h, w)
    if scratch is None:
        scratch = torch.empty(epipolar_scratch(h, w), dtype=torch.uint8, device=disp.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_epipolar_check(disp.data_ptr(), left.data_ptr(), right.data_ptr(), H, W, h, w, (C.c_float * 3)(*std),
                                       *[float(v) for v in K], int(range_px), int(step), float(tau), float(min_curv),
                                       int(iters), float(delta_px), int(min_valid), scratch.data_ptr(), scratch.numel(),
                                       record.data_ptr(), None if dy_map is None else dy_map.data_ptr(), _stream()),
               "epipolar_check")
    return record


GROUND_FLOOR, GROUND_OBSTACLE, GROUND_OVERHEAD, GROUND_BELOW, GROUND_INVALID = 0, 1, 2, 3, 255  # CODD_GROUND_* of the header
GROUND_PARAMS = dict(step=2, iters=8, delta_px=0.25, delta0_px=4.0, asym=4.0, min_valid=256, max_tilt_deg=45.0, tol_px=0.5,
                     ground_tol=0.05, clearance=2.0, cell=0.1)


def ground_scratch(h, w, grid=None):
    """Bytes of scratch ``ground_plane`` needs for an h x w crop and a ``grid`` (gh, gw) or None (codd_ground_scratch)."""
    gh, gw = (0, 0) if grid is None else (int(grid[0]), int(grid[1]))
    n = int(_abi.load().codd_ground_scratch(int(h), int(w), gh, gw))
    if n <= 0:
        raise ValueError(f"ground_scratch: positive (h, w) with h w < 2^31 and a grid of None or positive (gh, gw) with "
                         f"gh gw < 2^30 expected, got {(h, w)}, {grid}")
    return n


def ground_plane(disp, K, calib, crop, record, labels, height=None, grid_count=None, grid_height=None, scratch=None,
                 seed=None, up=(0.0, -1.0, 0.0), **par):
    """Where is the floor?  A robust fit of one plane ``d = c0 (x - cx) + c1 (y - cy) + c2`` to the ``crop`` (h, w) of the
    padded disparity ``disp`` [H,W] (or [1,1,H,W]) with ``K`` = (fx, fy, cx, cy) and ``calib`` = fx * baseline, per pixel the
    height above that plane and a label (GROUND_*), and a top-down grid of the floor and obstacle pixels
    (include/codd_hip.h, codd_ground_plane).  Outputs are caller-owned device tensors: ``record`` float64 [32] (c, ok, fit
    pixels, inliers, rms, steps, normal, camera height, tilt, the last step's A and b, the forward axis); ``labels`` uint8
    [h,w]; ``height`` fp32 [h,w] or None; ``grid_count`` int32 [2,gh,gw] and ``grid_height`` fp32 [gh,gw], both or
    neither.  ``seed``: three coefficients to start from (``live.ground_seed``) or None; ``up``: the unit up vector in
    camera coordinates; ``par`` overrides ``GROUND_PARAMS``.  ``scratch``: a uint8 tensor of ``ground_scratch`` bytes;
    allocated here when None.  iters + 1 launches on the current stream, no host synchronisation."""
    lib = _abi.load()
    _require_gpu(disp)
    unknown = set(par) - set(GROUND_PARAMS)
    if unknown:
        raise TypeError(f"ground_plane: unknown parameters {sorted(unknown)}; known: {tuple(GROUND_PARAMS)}")
    p = dict(GROUND_PARAMS, **par)
    H, W = disp.shape[-2:]
    h, w = int(crop[0]), int(crop[1])
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    assert record.dtype == torch.float64 and record.is_cuda and record.is_contiguous() and record.numel() == 32
    assert labels.dtype == torch.uint8 and labels.is_cuda and labels.is_contiguous() and tuple(labels.shape) == (h, w)
    if height is not None:
        assert height.dtype == torch.float32 and height.is_cuda and height.is_contiguous() and tuple(height.shape) == (h, w)
    assert (grid_count is None) == (grid_height is None), "grid_count and grid_height: both or neither"
    gh = gw = 0
    if grid_count is not None:
        gh, gw = (int(v) for v in grid_height.shape)
        assert grid_height.dtype == torch.float32 and grid_height.is_cuda and grid_height.is_contiguous()
        assert grid_count.dtype == torch.int32 and grid_count.is_cuda and grid_count.is_contiguous()
        assert tuple(grid_count.shape) == (2, gh, gw)
    if scratch is None:
        scratch = torch.empty(ground_scratch(h, w, (gh, gw) if gh else None), dtype=torch.uint8, device=disp.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    sd = None if seed is None else (C.c_double * 3)(*[float(v) for v in seed])
    _abi.check(lib.codd_ground_plane(disp.data_ptr(), H, W, h, w, *[float(v) for v in K], float(calib), sd,
                                     (C.c_float * 3)(*[float(v) for v in up]), int(p["step"]), int(p["iters"]),
                                     float(p["delta_px"]), float(p["delta0_px"]), float(p["asym"]), int(p["min_valid"]),
                                     float(p["max_tilt_deg"]), float(p["tol_px"]), float(p["ground_tol"]),
                                     float(p["clearance"]), float(p["cell"]), gh, gw, scratch.data_ptr(), scratch.numel(),
                                     record.data_ptr(), labels.data_ptr(), None if height is None else height.data_ptr(),
                                     None if grid_count is None else grid_count.data_ptr(),
                                     None if grid_height is None else grid_height.data_ptr(), _stream()), "ground_plane")
    return record


OBJECT_PARAMS = dict(select=1 << GROUND_OBSTACLE, gap_px=1.0, gap_rel=0.05, min_pixels=64, min_height=0.15, max_objects=256)
OBJECT_MAX = 4096  # the largest max_objects (include/codd_hip.h)


def objects_scratch(h, w, max_objects=OBJECT_PARAMS["max_objects"]):
    """Bytes of scratch ``objects`` needs for an h x w crop (codd_objects_scratch)."""
    n = int(_abi.load().codd_objects_scratch(int(h), int(w), int(max_objects)))
    if n <= 0:
        raise ValueError(f"objects_scratch: positive (h, w) with h w < 2^31 and max_objects in [1, {OBJECT_MAX}] expected, "
                         f"got {(h, w)}, {max_objects}")
    return n


def objects(disp, K, calib, crop, labels, ground_record, count, obj_i, obj_f, ids=None, scratch=None, **par):
    """What are the obstacles?  The connected components (4-neighbours whose disparities differ by at most
    max(gap_px, gap_rel * the smaller one)) of the pixels of the ``crop`` (h, w) of the padded disparity ``disp`` [H,W] (or
    [1,1,H,W]) whose label in ``labels`` uint8 [h,w] is in the bit set ``select``, and one table row for each of the first
    ``max_objects`` components, in raster order of their first pixel, with at least ``min_pixels`` pixels and a top at
    least ``min_height`` above the floor (include/codd_hip.h, codd_objects).  ``labels`` and ``ground_record`` (float64
    [32]) are the device tensors ``ground_plane`` wrote, ``K`` and ``calib`` the ones it took.  Outputs are caller-owned
    device tensors: ``count`` int32 [4] (objects, passing components, components, foreground pixels); ``obj_i`` int32
    [max_objects,8] (pixels, x0, y0, x1, y1, near_x, near_y, key); ``obj_f`` fp32 [max_objects,8] (gx_min, gx_max, gz_min,
    gz_max, hgt_min, hgt_max, d_min, d_max), rows past the objects zero; ``ids`` uint16 [h,w] or None (the object number
    of every pixel, 0xFFFF for none).  ``par`` overrides ``OBJECT_PARAMS`` (``max_objects`` is the tables' row count).
    ``scratch``: a uint8 tensor of ``objects_scratch`` bytes; allocated here when None.  7 launches on the current
    stream (6 without ``ids``), no host synchronisation."""
    lib = _abi.load()
    _require_gpu(disp)
    unknown = set(par) - set(OBJECT_PARAMS)
    if unknown:
        raise TypeError(f"objects: unknown parameters {sorted(unknown)}; known: {tuple(OBJECT_PARAMS)}")
    H, W = disp.shape[-2:]
    h, w = int(crop[0]), int(crop[1])
    assert obj_i.dim() == 2, "obj_i: [max_objects,8] expected"
    p = dict(OBJECT_PARAMS, max_objects=int(obj_i.shape[0]))
    p.update(par)
    m = int(p["max_objects"])
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    assert labels.dtype == torch.uint8 and labels.is_cuda and labels.is_contiguous() and tuple(labels.shape) == (h, w)
    assert ground_record.dtype == torch.float64 and ground_record.is_cuda and ground_record.is_contiguous()
    assert ground_record.numel() == 32
    assert count.dtype == torch.int32 and count.is_cuda and count.is_contiguous() and count.numel() == 4
    assert obj_i.dtype == torch.int32 and obj_i.is_cuda and obj_i.is_contiguous() and tuple(obj_i.shape) == (m, 8)
    assert obj_f.dtype == torch.float32 and obj_f.is_cuda and obj_f.is_contiguous() and tuple(obj_f.shape) == (m, 8)
    if ids is not None:
        assert ids.dtype == torch.uint16 and ids.is_cuda and ids.is_contiguous() and tuple(ids.shape) == (h, w)
    if scratch is None:
        scratch = torch.empty(objects_scratch(h, w, m), dtype=torch.uint8, device=disp.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_objects(disp.data_ptr(), H, W, h, w, *[float(v) for v in K], float(calib), labels.data_ptr(),
                                ground_record.data_ptr(), int(p["select"]), float(p["gap_px"]), float(p["gap_rel"]),
                                int(p["min_pixels"]), float(p["min_height"]), m, scratch.data_ptr(), scratch.numel(),
                                count.data_ptr(), obj_i.data_ptr(), obj_f.data_ptr(),
                                None if ids is None else ids.data_ptr(), _stream()), "objects")
    return count


TRACK_PARAMS = dict(min_votes=16)
TRACK_MAX = 1024  # CODD_TRACK_MAX_OBJECTS of include/codd_hip.h


def _track_sizes(h, w, max_objects, what):
    h, w, m = int(h), int(w), int(max_objects)
    if h <= 0 or w <= 0 or h * w >= 2 ** 31 or not 1 <= m <= TRACK_MAX:
        raise ValueError(f"{what}: positive (h, w) with h w < 2^31 and max_objects in [1, {TRACK_MAX}] expected, "
                         f"got {(h, w)}, {max_objects}")
    return h, w, m


def track_state_bytes(h, w, max_objects=256):
    """Bytes of the persistent state ``track_objects`` keeps for an h x w crop (codd_track_state_bytes)."""
    return int(_abi.load().codd_track_state_bytes(*_track_sizes(h, w, max_objects, "track_state_bytes")))


def track_scratch(h, w, max_objects=256):
    """Bytes of scratch ``track_objects`` needs for an h x w crop (codd_track_scratch)."""
    return int(_abi.load().codd_track_scratch(*_track_sizes(h, w, max_objects, "track_scratch")))


def track_objects(T, depth_prev, K, crop, ids, count, state, trk_count, trk_i, trk_f, scratch=None, ego_record=None,
                  moving=None, scale=1.0, fresh=False, min_votes=16, max_objects=256):
    """Which object of this frame is which object of the last one, and how did it move?  Every pixel of a previous object
    (the id map in ``state``) is carried by the SE3 field ``T`` [1,H,W,7] (None: the frame has no field and every object
    starts a track) over the ``crop`` (h, w) of the previous frame's depth ``depth_prev`` [H,W] (read only; call this
    before ``export_motion`` rolls it) onto ``ids`` uint16 [h,w] and ``count`` int32 [4], the device outputs of this
    frame's ``objects``, and votes; mutual best matches with at least ``min_votes`` votes keep their track id
    (include/codd_hip.h, codd_track_objects).  ``ego_record`` fp32 [16] and ``moving`` uint8 [h,w] (both optional) are the
    device outputs of ``ego_motion``.  ``state``: a uint8 tensor of ``track_state_bytes`` bytes the caller keeps between
    calls; ``fresh`` True ignores its contents (the first frame of a sequence).  Outputs are caller-owned device tensors:
    ``trk_count`` int32 [4] (n, continued, started, ended); ``trk_i`` int32 [max_objects,8] (track, age, prev, votes,
    pixels, moving, own_pixels, 0); ``trk_f`` fp32 [max_objects,8] (Dx, Dy, Dz, Ox, Oy, Oz, 0, 0), the mean displacement of
    the object's pixels and what is left of it after the camera's motion, NaN where undefined; rows past the objects
    zero.  ``scratch``: a uint8 tensor of ``track_scratch`` bytes; allocated here when None.  4 launches on the current
    stream, no host synchronisation."""
    h, w, m = _track_sizes(crop[0], crop[1], max_objects, "track_objects")
    if not (isinstance(min_votes, int) and not isinstance(min_votes, bool) and min_votes >= 1):
        raise ValueError(f"track_objects: an integer min_votes >= 1 expected, got {min_votes!r}")
    if T is not None and depth_prev is None:
        raise ValueError("track_objects: T needs depth_prev")
    _require_gpu(ids)
    lib = _abi.load()
    H, W = (h, w) if depth_prev is None else depth_prev.shape[-2:]
    if T is not None:
        assert T.dtype == torch.float32 and T.is_cuda and T.is_contiguous() and T.numel() == H * W * 7 and T.shape[-1] == 7
    if depth_prev is not None:
        assert depth_prev.dtype == torch.float32 and depth_prev.is_cuda and depth_prev.is_contiguous() and depth_prev.numel() == H * W
    assert ids.dtype == torch.uint16 and ids.is_cuda and ids.is_contiguous() and tuple(ids.shape) == (h, w)
    assert count.dtype == torch.int32 and count.is_cuda and count.is_contiguous() and count.numel() == 4
    assert trk_count.dtype == torch.int32 and trk_count.is_cuda and trk_count.is_contiguous() and trk_count.numel() == 4
    assert trk_i.dtype == torch.int32 and trk_i.is_cuda and trk_i.is_contiguous() and tuple(trk_i.shape) == (m, 8)
    assert trk_f.dtype == torch.float32 and trk_f.is_cuda and trk_f.is_contiguous() and tuple(trk_f.shape) == (m, 8)
    if ego_record is not None:
        assert ego_record.dtype == torch.float32 and ego_record.is_cuda and ego_record.is_contiguous() and ego_record.numel() == 16
    if moving is not None:
        assert moving.dtype == torch.uint8 and moving.is_cuda and moving.is_contiguous() and tuple(moving.shape) == (h, w)
    assert state.dtype == torch.uint8 and state.is_cuda and state.is_contiguous()
    if scratch is None:
        scratch = torch.empty(track_scratch(h, w, m), dtype=torch.uint8, device=ids.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_track_objects(None if T is None else T.data_ptr(), None if depth_prev is None else depth_prev.data_ptr(),
                                      H, W, h, w, *[float(v) for v in K], float(scale), ids.data_ptr(), count.data_ptr(),
                                      None if ego_record is None else ego_record.data_ptr(),
                                      None if moving is None else moving.data_ptr(), int(min_votes), m, int(bool(fresh)),
                                      state.data_ptr(), state.numel(), scratch.data_ptr(), scratch.numel(),
                                      trk_count.data_ptr(), trk_i.data_ptr(), trk_f.data_ptr(), _stream()), "track_objects")
    return trk_count


SCAN_PARAMS = dict(range_min=0.0, range_max=12.8, select=1 << GROUND_OBSTACLE, min_pixels=8)
SCAN_MAX_BEAMS, SCAN_MAX_BINS, SCAN_MAX_CELLS = 2048, 1024, 2 ** 20  # the limits of codd_range_scan (include/codd_hip.h)


def scan_edges(beams, angle_min, angle_max):
    """The beam-edge table of ``range_scan``: numpy fp32 [beams+1,2] = (sin a_i, cos a_i) with a_i = angle_min + (angle_max -
    angle_min) * i / beams in float64 (radians from the grid's forward axis, positive to the right), sine and cosine taken
    in float64 and rounded once.  ValueError outside 1 <= beams <= ``SCAN_MAX_BEAMS`` and -pi/2 <= angle_min < angle_max
    <= pi/2 (no device call)."""
    if not (isinstance(beams, (int, np.integer)) and not isinstance(beams, bool) and 1 <= beams <= SCAN_MAX_BEAMS):
        raise ValueError(f"scan_edges: an integer beams in [1, {SCAN_MAX_BEAMS}] expected, got {beams!r}")
    lo, hi = float(angle_min), float(angle_max)
    if not (-np.pi / 2 <= lo < hi <= np.pi / 2):  # (NaN compares false)
        raise ValueError(f"scan_edges: -pi/2 <= angle_min < angle_max <= pi/2 expected, got {angle_min!r}, {angle_max!r}")
    a = lo + (hi - lo) * np.arange(int(beams) + 1, dtype=np.float64) / float(beams)
    return np.stack([np.sin(a), np.cos(a)], 1).astype(np.float32)


def range_scan_scratch(beams, bins):
    """Bytes of scratch ``range_scan`` needs (codd_range_scan_scratch)."""
    n = int(_abi.load().codd_range_scan_scratch(int(beams), int(bins)))
    if n <= 0:
        raise ValueError(f"range_scan_scratch: beams in [1, {SCAN_MAX_BEAMS}], bins in [1, {SCAN_MAX_BINS}] and beams bins <= "
                         f"2^20 expected, got {beams}, {bins}")
    return n


def range_scan(disp, K, calib, crop, labels, ground_record, edges, count, scan_i, scan_f, ids=None, scratch=None, **par):
    """How far can I go?  Every floor pixel and every pixel whose label is in the bit set ``select`` (the obstacles) of the
    ``crop`` (h, w) of the padded disparity ``disp`` [H,W] (or [1,1,H,W]) is projected onto the floor -- the frame of
    ``objects``' extents -- and binned by bearing, between the beam edges ``edges`` (device fp32 [beams+1,2]: ``scan_edges``),
    and by range, in ``bins`` = ``par["bins"]`` bins up to ``range_max``; per beam, the nearest bin with at least
    ``min_pixels`` obstacle pixels is the hit (include/codd_hip.h, codd_range_scan).  ``labels`` and ``ground_record`` are the
    device tensors ``ground_plane`` wrote, ``K`` and ``calib`` the ones it took; ``ids`` uint16 [h,w] or None: the id map
    ``objects`` wrote.  Outputs are caller-owned device tensors: ``count`` int32 [4] (hit, clear, unknown beams, obstacle
    pixels binned); ``scan_f`` fp32 [beams,4] (range: +inf clear, NaN unknown; free range; gx, gz of the hit); ``scan_i``
    int32 [beams,4] (raster index of the hit pixel, object, obstacle pixels of the hit bin, floor pixels before it; -1 for
    no pixel / no object).  ``par`` overrides ``SCAN_PARAMS`` and gives ``bins`` (default 128).  ``scratch``: a uint8 tensor
    of ``range_scan_scratch`` bytes; allocated here when None.  3 launches on the current stream, no host
    synchronisation."""
    lib = _abi.load()
    _require_gpu(disp)
    unknown = set(par) - set(SCAN_PARAMS) - {"bins"}
    if unknown:
        raise TypeError(f"range_scan: unknown parameters {sorted(unknown)}; known: {tuple(SCAN_PARAMS) + ('bins',)}")
    p = dict(SCAN_PARAMS, bins=128)
    p.update(par)
    H, W = disp.shape[-2:]
    h, w = int(crop[0]), int(crop[1])
    assert scan_i.dim() == 2, "scan_i: [beams,4] expected"
    beams, bins = int(scan_i.shape[0]), int(p["bins"])
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    assert labels.dtype == torch.uint8 and labels.is_cuda and labels.is_contiguous() and tuple(labels.shape) == (h, w)
    assert ground_record.dtype == torch.float64 and ground_record.is_cuda and ground_record.is_contiguous()
    assert ground_record.numel() == 32
    assert edges.dtype == torch.float32 and edges.is_cuda and edges.is_contiguous() and tuple(edges.shape) == (beams + 1, 2)
    assert count.dtype == torch.int32 and count.is_cuda and count.is_contiguous() and count.numel() == 4
    assert scan_i.dtype == torch.int32 and scan_i.is_cuda and scan_i.is_contiguous() and tuple(scan_i.shape) == (beams, 4)
    assert scan_f.dtype == torch.float32 and scan_f.is_cuda and scan_f.is_contiguous() and tuple(scan_f.shape) == (beams, 4)
    if ids is not None:
        assert ids.dtype == torch.uint16 and ids.is_cuda and ids.is_contiguous() and tuple(ids.shape) == (h, w)
    if scratch is None:
        scratch = torch.empty(range_scan_scratch(beams, bins), dtype=torch.uint8, device=disp.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_range_scan(disp.data_ptr(), H, W, h, w, *[float(v) for v in K], float(calib), labels.data_ptr(),
                                   ground_record.data_ptr(), None if ids is None else ids.data_ptr(), edges.data_ptr(),
                                   beams, bins, float(p["range_min"]), float(p["range_max"]), int(p["select"]),
                                   int(p["min_pixels"]), scratch.data_ptr(), scratch.numel(), count.data_ptr(),
                                   scan_i.data_ptr(), scan_f.data_ptr(), _stream()), "range_scan")
    return count


MAP_RESET, MAP_HOLD = 0, 1  # CODD_MAP_RESET, CODD_MAP_HOLD of include/codd_hip.h
MAP_MAX_SIDE, MAP_MAX_CELLS = 4096, 2 ** 22  # the limits of codd_local_map
# The increments and levels are chosen by reasoning, not measured on real footage: an occupied observation weighs twice a
# free one (a missed obstacle costs more than a detour); two occupied observations make a cell occupied, so one frame of
# stereo speckle does not; two free ones make it free; the clamps bound how long stale evidence outlives the scene (a cell
# saturated at 64 takes 34 free frames to count as free, one saturated at -32 ten occupied frames to count as occupied).
MAP_PARAMS = dict(cell=0.1, range_min=0.0, range_max=12.8, select=1 << GROUND_OBSTACLE, min_pixels=4, l_occ=4, l_free=2,
                  l_min=-32, l_max=64, decay=0, occ_level=8, free_level=-4, lost=MAP_RESET)


def local_map_scratch(gh, gw):
    """Bytes of scratch ``local_map`` needs (codd_local_map_scratch)."""
    n = int(_abi.load().codd_local_map_scratch(int(gh), int(gw)))
    if n <= 0:
        raise ValueError(f"local_map_scratch: gh, gw in [1, {MAP_MAX_SIDE}] and gh gw <= 2^22 expected, got {gh}, {gw}")
    return n


def local_map(disp, K, calib, crop, labels, ground_record, ego_record, state, logodds, age, map_out, age_out, record, fresh=False,
              scratch=None, **par):
    """What is around me, and what was?  One frame into the rolling occupancy map (include/codd_hip.h, codd_local_map).
    ``disp`` [H,W] (or [1,1,H,W]), ``K``, ``calib``, ``crop`` (h, w), ``labels`` and ``ground_record`` as ``objects`` takes
    them; ``ego_record``: the device fp32 [16] ``ego_motion`` wrote for this frame, or None for a frame without a field;
    ``fresh``: the first frame of a sequence.  Persistent, caller-owned device tensors, zeroed once and then left to this
    call: ``state`` float64 [32], ``logodds`` int16 [gh,gw] and ``age`` uint8 [gh,gw] (toroidal storage).  Outputs,
    caller-owned device tensors: ``map_out`` int16 [gh,gw] and ``age_out`` uint8 [gh,gw] (the unrolled window, [j,i] = world
    cell (ix0 + i, iz0 + j)) and ``record`` float64 [16].  ``par`` overrides ``MAP_PARAMS``.  ``scratch``: a uint8 tensor of
    ``local_map_scratch`` bytes; allocated here when None.  4 launches on the current stream, no host synchronisation."""
    lib = _abi.load()
    _require_gpu(disp)
    unknown = set(par) - set(MAP_PARAMS)
    if unknown:
        raise TypeError(f"local_map: unknown parameters {sorted(unknown)}; known: {tuple(MAP_PARAMS)}")
    p = dict(MAP_PARAMS)
    p.update(par)
    H, W = disp.shape[-2:]
    h, w = int(crop[0]), int(crop[1])
    assert logodds.dim() == 2, "logodds: [gh,gw] expected"
    gh, gw = int(logodds.shape[0]), int(logodds.shape[1])
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    assert labels.dtype == torch.uint8 and labels.is_cuda and labels.is_contiguous() and tuple(labels.shape) == (h, w)
    assert ground_record.dtype == torch.float64 and ground_record.is_cuda and ground_record.is_contiguous()
    assert ground_record.numel() == 32
    if ego_record is not None:
        assert ego_record.dtype == torch.float32 and ego_record.is_cuda and ego_record.is_contiguous() and ego_record.numel() == 16
    assert state.dtype == torch.float64 and state.is_cuda and state.is_contiguous() and state.numel() == 32
    assert record.dtype == torch.float64 and record.is_cuda and record.is_contiguous() and record.numel() == 16
    for t, dt in ((logodds, torch.int16), (map_out, torch.int16), (age, torch.uint8), (age_out, torch.uint8)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (gh, gw)
    if scratch is None:
        scratch = torch.empty(local_map_scratch(gh, gw), dtype=torch.uint8, device=disp.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_local_map(disp.data_ptr(), H, W, h, w, *[float(v) for v in K], float(calib), labels.data_ptr(),
                                  ground_record.data_ptr(), None if ego_record is None else ego_record.data_ptr(),
                                  1 if fresh else 0, gh, gw, float(p["cell"]), float(p["range_min"]), float(p["range_max"]),
                                  int(p["select"]), int(p["min_pixels"]), int(p["l_occ"]), int(p["l_free"]), int(p["l_min"]),
                                  int(p["l_max"]), int(p["decay"]), int(p["occ_level"]), int(p["free_level"]), int(p["lost"]),
                                  state.data_ptr(), logodds.data_ptr(), age.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                  map_out.data_ptr(), age_out.data_ptr(), record.data_ptr(), _stream()), "local_map")
    return record


# CODD_HEIGHT_* of include/codd_hip.h: the bits of the flags, the byte of an unknown cell, the sentinels of the layers and
# the largest quantised height or threshold
HEIGHT_STEP, HEIGHT_HEADROOM, HEIGHT_HOLE, HEIGHT_UNKNOWN = 1, 2, 4, 255
HEIGHT_NONE, HEIGHT_NO_CEIL, HEIGHT_Q_MAX = -32768, 32767, 32000
# Chosen by reasoning, not measured on real footage: 5 mm resolves a kerb well below stereo's depth noise at a few metres
# and covers +-160 m of int16; every surface label is mapped, the overhead ones go to their own layer; four pixels as the
# map's; alpha 128 halves the distance to each new observation, so one frame of speckle moves a cell half way and two
# agreeing frames most of it; a platform that climbs 10 cm and drops 10 cm; a robot 1 m tall.
HEIGHT_PARAMS = dict(h_res=0.005, select=(1 << GROUND_FLOOR) | (1 << GROUND_OBSTACLE) | (1 << GROUND_BELOW), min_pixels=4,
                     alpha=128, max_step=0.10, robot_height=1.0, max_drop=0.10)


def height_map_scratch(gh, gw):
    """Bytes of scratch ``height_map`` needs (codd_height_map_scratch)."""
    n = int(_abi.load().codd_height_map_scratch(int(gh), int(gw)))
    if n <= 0:
        raise ValueError(f"height_map_scratch: gh, gw in [1, {MAP_MAX_SIDE}] and gh gw <= 2^22 expected, got {gh}, {gw}")
    return n


def height_thresholds(h_res, max_step, robot_height, max_drop):
    """(max_step_q, robot_height_q, max_drop_q): the thresholds in units of ``h_res``, (int)rint(v / h_res) in fp64.
    ValueError for a non-finite or non-positive ``h_res`` and for a threshold outside [0, ``HEIGHT_Q_MAX``] units."""
    h_res = float(h_res)
    if not (np.isfinite(h_res) and h_res > 0):
        raise ValueError(f"height_map: a finite h_res > 0 expected, got {h_res!r}")
    out = []
    for name, v in (("max_step", max_step), ("robot_height", robot_height), ("max_drop", max_drop)):
        q = np.rint(np.float64(v) / np.float64(h_res))
        if not (np.isfinite(q) and 0 <= q <= HEIGHT_Q_MAX):
            raise ValueError(f"height_map: {name} / h_res in [0, {HEIGHT_Q_MAX}] expected, got {v!r} / {h_res!r}")
        out.append(int(q))
    return tuple(out)


def height_map(disp, K, calib, crop, labels, ground_record, state, top, bot, ceil, hage, top_out, bot_out, ceil_out, hage_out,
               step_out, flags_out, record, cell=MAP_PARAMS["cell"], range_min=MAP_PARAMS["range_min"],
               range_max=MAP_PARAMS["range_max"], scratch=None, **par):
    """How high is it, and do I fit?  One frame into the rolling elevation layer on ``local_map``'s window
    (include/codd_hip.h, codd_height_map).  Call it exactly once after every ``local_map`` call on ``state``, with the
    ``cell``, ``range_min`` and ``range_max`` that call was given.  ``disp``, ``K``, ``calib``, ``crop``, ``labels`` and
    ``ground_record`` as ``local_map`` takes them; ``state``: the float64 [32] ``local_map`` left (read only).  Persistent,
    caller-owned device tensors, toroidal as ``logodds``, their contents before the first call irrelevant: ``top``, ``bot``,
    ``ceil`` int16 [gh,gw] and ``hage`` uint8 [gh,gw].  Outputs, caller-owned device tensors: ``top_out``, ``bot_out``,
    ``ceil_out`` int16, ``hage_out`` uint8, ``step_out`` uint16 and ``flags_out`` uint8 [gh,gw] (the unrolled window) and
    ``record`` float64 [16].  ``par`` overrides ``HEIGHT_PARAMS`` (``select`` a bit set of labels without the overhead bit;
    the thresholds in the unit of ``h_res``, quantised here by ``height_thresholds``).  ``scratch``: a uint8 tensor of
    ``height_map_scratch`` bytes; allocated here when None.  4 launches on the current stream, no host synchronisation."""
    lib = _abi.load()
    _require_gpu(disp)
    unknown = set(par) - set(HEIGHT_PARAMS)
    if unknown:
        raise TypeError(f"height_map: unknown parameters {sorted(unknown)}; known: {tuple(HEIGHT_PARAMS)}")
    p = dict(HEIGHT_PARAMS)
    p.update(par)
    if not 0 <= int(p["select"]) < 2 ** 32:
        raise ValueError(f"height_map: select: a set of label bits below 32 expected, got {p['select']!r}")
    step_q, robot_q, drop_q = height_thresholds(p["h_res"], p["max_step"], p["robot_height"], p["max_drop"])
    H, W = disp.shape[-2:]
    h, w = int(crop[0]), int(crop[1])
    assert top.dim() == 2, "top: [gh,gw] expected"
    gh, gw = int(top.shape[0]), int(top.shape[1])
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    assert labels.dtype == torch.uint8 and labels.is_cuda and labels.is_contiguous() and tuple(labels.shape) == (h, w)
    assert ground_record.dtype == torch.float64 and ground_record.is_cuda and ground_record.is_contiguous()
    assert ground_record.numel() == 32
    assert state.dtype == torch.float64 and state.is_cuda and state.is_contiguous() and state.numel() == 32
    assert record.dtype == torch.float64 and record.is_cuda and record.is_contiguous() and record.numel() == 16
    for t, dt in ((top, torch.int16), (bot, torch.int16), (ceil, torch.int16), (hage, torch.uint8), (top_out, torch.int16),
                  (bot_out, torch.int16), (ceil_out, torch.int16), (hage_out, torch.uint8), (step_out, torch.uint16),
                  (flags_out, torch.uint8)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (gh, gw)
    if scratch is None:
        scratch = torch.empty(height_map_scratch(gh, gw), dtype=torch.uint8, device=disp.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_height_map(disp.data_ptr(), H, W, h, w, *[float(v) for v in K], float(calib), labels.data_ptr(),
                                   ground_record.data_ptr(), state.data_ptr(), gh, gw, float(cell), float(range_min),
                                   float(range_max), float(p["h_res"]), int(p["select"]), int(p["min_pixels"]), int(p["alpha"]),
                                   step_q, robot_q, drop_q, top.data_ptr(), bot.data_ptr(), ceil.data_ptr(), hage.data_ptr(),
                                   scratch.data_ptr(), scratch.numel(), top_out.data_ptr(), bot_out.data_ptr(),
                                   ceil_out.data_ptr(), hage_out.data_ptr(), step_out.data_ptr(), flags_out.data_ptr(),
                                   record.data_ptr(), _stream()), "height_map")
    return record


# CODD_COST_* of include/codd_hip.h: the cost values of ROS costmap_2d, the dist2 of a cell farther than R from every
# obstacle, and the largest R
COST_LETHAL, COST_INSCRIBED, COST_NO_INFO, COST_FAR, COST_MAX_R = 254, 253, 255, 0x7fffffff, 128


def cost_lut(cell, robot_radius, inflation_radius, scaling):
    """(R, lut): the table ``cost_map`` takes, uint8 [R R + 2], the cost by squared distance in cells.  R = max(1,
    ceil(inflation_radius / cell)) (ValueError above ``COST_MAX_R``).  For n in 0 .. R R, with dist = sqrt(n) cell: 254 for
    n == 0, 253 for dist <= robot_radius, max(1, int(252 exp(-scaling (dist - robot_radius)))) for dist <=
    inflation_radius (ROS costmap_2d's inflation layer), 0 otherwise; lut[R R + 1] = 0 (farther than R).  numpy float64 on
    the host, no device call."""
    cell, robot_radius, inflation_radius, scaling = float(cell), float(robot_radius), float(inflation_radius), float(scaling)
    if not (np.isfinite([cell, robot_radius, inflation_radius, scaling]).all() and cell > 0 and inflation_radius > 0
            and 0 <= robot_radius <= inflation_radius and scaling >= 0):
        raise ValueError(f"cost_lut: finite cell > 0, 0 <= robot_radius <= inflation_radius, inflation_radius > 0 and scaling >= 0 "
                         f"expected, got {cell!r}, {robot_radius!r}, {inflation_radius!r}, {scaling!r}")
    R = max(1, int(np.ceil(inflation_radius / cell)))
    if R > COST_MAX_R:
        raise ValueError(f"cost_lut: ceil(inflation_radius / cell) <= {COST_MAX_R} expected, got {R}")
    dist = np.sqrt(np.arange(R * R + 1, dtype=np.float64)) * cell
    decay = np.maximum(1, (252.0 * np.exp(-scaling * np.maximum(dist - robot_radius, 0.0))).astype(np.int64))  # (truncated)
    lut = np.zeros(R * R + 2, np.uint8)
    lut[:-1] = np.where(dist <= robot_radius, COST_INSCRIBED, np.where(dist <= inflation_radius, decay, 0))
    lut[0] = COST_LETHAL
    return R, lut


def cost_map_scratch(gh, gw, R):
    """Bytes of scratch ``cost_map`` needs (codd_cost_map_scratch)."""
    n = int(_abi.load().codd_cost_map_scratch(int(gh), int(gw), int(R)))
    if n <= 0:
        raise ValueError(f"cost_map_scratch: gh, gw in [1, {MAP_MAX_SIDE}], gh gw <= 2^22 and R in [1, {COST_MAX_R}] expected, got "
                         f"{gh}, {gw}, {R}")
    return n


def cost_map(map, age, lut, R, start, dist2, nearest, cost, reach, record, occ_level=MAP_PARAMS["occ_level"],
             free_level=MAP_PARAMS["free_level"], seed_r2=0, through_unknown=False, scratch=None):
    """Where can I go?  Clearance, inflated cost, reachable cells and frontiers of one occupancy map (include/codd_hip.h,
    codd_cost_map).  ``map`` int16 [gh,gw] and ``age`` uint8 [gh,gw]: the ``map_out`` and ``age_out`` of ``local_map``;
    ``lut`` uint8 [R R + 2] on the device (``cost_lut``); ``start`` = (start_i, start_j), the robot's cell (column, row).
    Outputs, caller-owned device tensors: ``dist2`` int32 [gh,gw], ``nearest`` int32 [gh,gw] or None, ``cost`` and ``reach``
    uint8 [gh,gw], ``record`` float64 [16].  ``scratch``: a uint8 tensor of ``cost_map_scratch`` bytes; allocated here when
    None.  Five launches on the current stream, no host synchronisation."""
    lib = _abi.load()
    _require_gpu(map)
    assert map.dim() == 2, "map: [gh,gw] expected"
    gh, gw = int(map.shape[0]), int(map.shape[1])
    R = int(R)
    assert map.dtype == torch.int16 and map.is_cuda and map.is_contiguous()
    assert lut.dtype == torch.uint8 and lut.is_cuda and lut.is_contiguous() and lut.numel() == R * R + 2
    assert record.dtype == torch.float64 and record.is_cuda and record.is_contiguous() and record.numel() == 16
    for t, dt in ((age, torch.uint8), (dist2, torch.int32), (cost, torch.uint8), (reach, torch.uint8)) + (
            () if nearest is None else ((nearest, torch.int32),)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (gh, gw)
    if scratch is None:
        scratch = torch.empty(cost_map_scratch(gh, gw, R), dtype=torch.uint8, device=map.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_cost_map(map.data_ptr(), age.data_ptr(), gh, gw, int(occ_level), int(free_level), R, lut.data_ptr(),
                                 int(start[0]), int(start[1]), int(seed_r2), 1 if through_unknown else 0, scratch.data_ptr(),
                                 scratch.numel(), dist2.data_ptr(), None if nearest is None else nearest.data_ptr(),
                                 cost.data_ptr(), reach.data_ptr(), record.data_ptr(), _stream()), "cost_map")
    return record


# CODD_PLAN_* of include/codd_hip.h: the potential of a cell no path leaves, the largest window, the goal modes
PLAN_UNREACHED, PLAN_MAX_CELLS = 0xffffffff, 25600
PLAN_GOAL_CELL, PLAN_GOAL_WORLD, PLAN_GOAL_FRONTIER = 0, 1, 2


def _plan_shape_ok(gh, gw):
    return gh >= 1 and gw >= 1 and gh * gw <= PLAN_MAX_CELLS


def plan_scratch(gh, gw):
    """Bytes of scratch ``plan`` needs (codd_plan_scratch)."""
    n = int(_abi.load().codd_plan_scratch(int(gh), int(gw)))
    if n <= 0:
        raise ValueError(f"plan_scratch: gh, gw >= 1 and gh gw <= {PLAN_MAX_CELLS} expected, got {gh}, {gw}")
    return n


def plan_goal(goal):
    """``goal`` of ``plan`` -> (mode, goal_i, goal_j, goal_x, goal_z): "frontier", ("cell", i, j) or ("world", x, z).
    ValueError otherwise; no device call."""
    if isinstance(goal, str) and goal == "frontier":
        return PLAN_GOAL_FRONTIER, 0, 0, 0.0, 0.0
    try:
        kind, a, b = goal
        if kind == "cell" and not isinstance(a, (bool, float)) and not isinstance(b, (bool, float)):
            return PLAN_GOAL_CELL, int(a), int(b), 0.0, 0.0
        if kind == "world" and not isinstance(a, bool) and not isinstance(b, bool):
            return PLAN_GOAL_WORLD, 0, 0, float(a), float(b)
    except (TypeError, ValueError):
        pass
    raise ValueError(f'plan: goal "frontier", ("cell", i, j) or ("world", x, z) expected, got {goal!r}')


def plan(cost, reach, start, potential, path, record, *, dir=None, goal="frontier", cost_record=None, map_record=None,
         cell=None, goal_r2=0, neutral=50, factor=205, unknown_cost=128, scratch=None):
    """Which way do I go?  The navigation function and the path to a goal on one cost map (include/codd_hip.h, codd_plan).
    ``cost`` and ``reach`` uint8 [gh,gw]: the outputs of ``cost_map``; ``start`` = (start_i, start_j) as given to it.
    ``goal``: "frontier" (the nearest frontier: ``cost_record``, the record of ``cost_map``, is read on the device),
    ("cell", i, j), or ("world", x, z) in the map frame (``map_record``, the record of ``local_map``, is read on the
    device, and ``cell`` is the map's cell size).  ``goal_r2``: the squared radius in cells of the goal set.  A cell costs
    ``neutral`` + ``factor`` c / 256 per unit of length, c its cost byte or ``unknown_cost`` for 255.  Outputs,
    caller-owned device tensors: ``potential`` int32 [gh,gw] holding the uint32 bits (``PLAN_UNREACHED``: no path),
    ``dir`` uint8 [gh,gw] or None, ``path`` int32 [max_path] (raster indices, -1 behind the last), ``record`` float64 [16].
    ``scratch``: a uint8 tensor of ``plan_scratch`` bytes; allocated here when None.  ValueError for what the entry rejects,
    before any device call.  One launch of one workgroup on the current stream, no host synchronisation."""
    mode, goal_i, goal_j, goal_x, goal_z = plan_goal(goal)
    if cost.dim() != 2:
        raise ValueError("plan: cost [gh,gw] expected")
    gh, gw = int(cost.shape[0]), int(cost.shape[1])
    if not _plan_shape_ok(gh, gw):
        raise ValueError(f"plan: gh, gw >= 1 and gh gw <= {PLAN_MAX_CELLS} expected, got {gh}, {gw}")
    start_i, start_j = int(start[0]), int(start[1])
    if not (0 <= start_i < gw and 0 <= start_j < gh):
        raise ValueError(f"plan: start (i, j) inside the {gh} x {gw} window expected, got {tuple(start)!r}")
    goal_r2, neutral, factor, unknown_cost = int(goal_r2), int(neutral), int(factor), int(unknown_cost)
    if goal_r2 < 0 or goal_r2 >= 2 ** 31:
        raise ValueError(f"plan: 0 <= goal_r2 < 2^31 expected, got {goal_r2}")
    if not (1 <= neutral <= 255 and 0 <= factor <= 1024 and 0 <= unknown_cost <= 254):
        raise ValueError(f"plan: neutral in [1, 255], factor in [0, 1024] and unknown_cost in [0, 254] expected, got {neutral}, "
                         f"{factor}, {unknown_cost}")
    if mode == PLAN_GOAL_CELL and not (0 <= goal_i < gw and 0 <= goal_j < gh):
        raise ValueError(f"plan: a goal cell (i, j) inside the {gh} x {gw} window expected, got {goal_i}, {goal_j}")
    if mode == PLAN_GOAL_FRONTIER and cost_record is None:
        raise ValueError('plan: goal "frontier" reads cost_record, the record of cost_map')
    c32 = 0.0
    if mode == PLAN_GOAL_WORLD:
        if map_record is None or cell is None:
            raise ValueError('plan: a ("world", x, z) goal reads map_record, the record of local_map, and needs cell')
        c32 = float(np.float32(cell))  # (the entry takes a float)
        if not (np.isfinite([c32, goal_x, goal_z]).all() and c32 > 0 and abs(goal_x / c32) < 2 ** 30 and abs(goal_z / c32) < 2 ** 30):
            raise ValueError(f"plan: finite cell > 0 and a finite goal with |goal / cell| < 2^30 expected, got {cell!r}, {goal_x!r}, "
                             f"{goal_z!r}")
    if path.dim() != 1 or path.numel() < 1 or path.numel() >= 2 ** 31:
        raise ValueError("plan: path int32 [max_path] with max_path >= 1 expected")
    lib = _abi.load()
    _require_gpu(cost)
    assert cost.dtype == torch.uint8 and cost.is_cuda and cost.is_contiguous()
    assert reach.dtype == torch.uint8 and reach.is_cuda and reach.is_contiguous() and tuple(reach.shape) == (gh, gw)
    assert potential.dtype == torch.int32 and potential.is_cuda and potential.is_contiguous() and tuple(potential.shape) == (gh, gw)
    assert dir is None or (dir.dtype == torch.uint8 and dir.is_cuda and dir.is_contiguous() and tuple(dir.shape) == (gh, gw))
    assert path.dtype == torch.int32 and path.is_cuda and path.is_contiguous()
    for t in (record,) + tuple(r for r in (cost_record, map_record) if r is not None):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.numel() == 16
    if scratch is None:
        scratch = torch.empty(plan_scratch(gh, gw), dtype=torch.uint8, device=cost.device)
    assert scratch.dtype == torch.uint8 and scratch.is_cuda and scratch.is_contiguous()
    _abi.check(lib.codd_plan(cost.data_ptr(), reach.data_ptr(),
                             cost_record.data_ptr() if mode == PLAN_GOAL_FRONTIER else None,
                             map_record.data_ptr() if mode == PLAN_GOAL_WORLD else None, gh, gw, start_i, start_j, mode, goal_i,
                             goal_j, goal_x, goal_z, c32, goal_r2, neutral, factor, unknown_cost, int(path.numel()),
                             scratch.data_ptr(), scratch.numel(), potential.data_ptr(), None if dir is None else dir.data_ptr(),
                             path.data_ptr(), record.data_ptr(), _stream()), "plan")
    return record


ALIGN_MAX_FOOTPRINT = 4  # CODD_ALIGN_MAX_FOOTPRINT of include/codd_hip.h


def align_view(target, rect=None):
    """The ``codd_align_view`` struct of a ``calibration.AlignTarget``: its pose taken from the rectified left camera of
    ``rect`` (a ``calibration.Rectification``; None: the target's pose already refers to the grid of the disparity), its
    camera, and ``r2_max`` = ``calibration.fold_radius2`` of that camera.  No device call."""
    from . import calibration
    R, T = target.pose_from(rect)
    s = _abi.AlignView()
    s.R[:] = [float(x) for row in R for x in row]
    s.T[:] = [float(x) for x in T]
    s.K[:] = target.camera.K
    s.dist[:] = target.camera.dist8
    s.r2_max = calibration.fold_radius2(target.camera)
    s.model = CALIB_MODELS[target.camera.model]
    return s


def align_depth(disp, shape, intrinsics, calib, view, target_size, footprint, depth_out, uv_out=None):
    """A fill and one launch per frame: the padded disparity ``disp`` [H,W] (or [1,1,H,W]) of the rectified left camera with
    ``intrinsics`` (f', f', cx', cy') and ``calib`` = f' * baseline, read inside ``shape`` = (h, w), forward-warped into the
    camera ``view`` (``align_view``) of ``target_size`` = (ht, wt): ``depth_out`` fp32 [ht,wt] (caller-owned) gets the depth
    of the nearest surface that lands on each target pixel, in the unit of ``calib``, +inf where nothing lands; each
    source pixel covers the ``footprint`` x ``footprint`` (1 .. 4) target pixels nearest to its position.  ``uv_out`` fp32
    [h,w,2] or None gets that position (sx, sy), NaN where the pixel has no valid disparity or does not project
    (include/codd_hip.h, codd_align_depth)."""
    lib = _abi.load()
    _require_gpu(disp)
    H, W = disp.shape[-2:]
    h, w = int(shape[0]), int(shape[1])
    ht, wt = int(target_size[0]), int(target_size[1])
    f, fy, cx, cy = (float(v) for v in intrinsics)
    if f != fy:
        raise ValueError(f"intrinsics: the rectified camera has one focal length (f', f', cx', cy'), got {tuple(intrinsics)}")
    assert disp.dtype == torch.float32 and disp.is_cuda and disp.is_contiguous() and disp.numel() == H * W
    assert depth_out.dtype == torch.float32 and depth_out.is_cuda and depth_out.is_contiguous() and tuple(depth_out.shape) == (ht, wt)
    if uv_out is not None:
        assert uv_out.dtype == torch.float32 and uv_out.is_cuda and uv_out.is_contiguous() and tuple(uv_out.shape) == (h, w, 2)
    _abi.check(lib.codd_align_depth(disp.data_ptr(), H, W, h, w, f, cx, cy, float(calib), C.byref(view), ht, wt,
                                    int(footprint), depth_out.data_ptr(), None if uv_out is None else uv_out.data_ptr(),
                                    _stream()), "align_depth")
    return depth_out


def fusion_select(mode, cur, warp, gt=None, K=0.5):
    """mode 'kalman' / 'gt' (ablation fusions).  cur, warp [B,1,H,W]; gt [B,1,hg,wg]."""
    lib = _abi.load()
    _require_gpu(cur)
    B, _, H, W = cur.shape
    out = torch.empty_like(cur)
    hg, wg = (gt.shape[-2], gt.shape[-1]) if gt is not None else (0, 0)
    _abi.check(lib.codd_fusion_select(0 if mode == "kalman" else 1, cur.data_ptr(), warp.data_ptr(),
                                      gt.data_ptr() if gt is not None else None, B, H, W, hg, wg, float(K),
                                      out.data_ptr(), _stream()), "fusion_select")
    return out


def gt_motion(img_prev, feat_prev, disp_prev, gt_flow, gt_disp_change, gt_flow_occ):
    """-> [img_warp, feat_warp, conf, disp_warp [B,1,H,W], flow3] (GTMotion ablation)."""
    lib = _abi.load()
    _require_gpu(img_prev)
    B, _, H, W = img_prev.shape
    hg, wg = gt_flow.shape[-2:]
    occ = gt_flow_occ.to(torch.uint8).contiguous()
    img_w, feat_w = torch.empty_like(img_prev), torch.empty_like(feat_prev)
    conf, flow3 = torch.empty_like(img_prev), torch.empty_like(img_prev)
    disp_w = torch.empty(B, 1, H, W, device=img_prev.device, dtype=torch.float32)
    _abi.check(lib.codd_gt_motion(img_prev.data_ptr(), disp_prev.data_ptr(), feat_prev.data_ptr(), feat_prev.shape[1],
                                  gt_flow.data_ptr(), gt_disp_change.data_ptr(), occ.data_ptr(), B, H, W, hg, wg,
                                  img_w.data_ptr(), feat_w.data_ptr(), conf.data_ptr(), disp_w.data_ptr(),
                                  flow3.data_ptr(), _stream()), "gt_motion")
    return [img_w, feat_w, conf, disp_w, flow3]
