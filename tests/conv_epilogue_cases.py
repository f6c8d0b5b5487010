"""The launches whose output bits tests/golden/conv_epilogue_bits.json records (sha256 of the fp32 output bytes), shared
by the generator tools/parent_bits.py --cases conv_epilogue and by tests/test_gpu_conv_epilogue_bits.py:

* ``sweep/<sig>|<cfg>``: every exact-fp32 entry (configuration not of layout 2) of conv_fp64.sweep(), launched exactly
  as tests/test_gpu_conv_fp64.py::_launch does (its setup is documented there);
* ``multi/<n>``: the four jobs of test_gpu_conv_fp64._multi_jobs() as ONE codd_conv2d_multi launch;
* ``hand/<case>/<H>x<W>/l<layout>``: four hand-made layers at a 9 x 21 output (Wout & 3 != 0) and a 10 x 24 one, on the
  classic (layout 0) and, where its rows are 16-byte aligned, the quad (layout 1) kernel, 4 x 16 tiles, B = 2:
  cout = 18 (a channel tail inside the second 16-block), two inputs, the transposed-convolution store, and
  res1 + res2 + post together with relu_ch0.  launch(), which runs them, also runs the layers of
  tests/conv_epilogue_vec_cases.py (other sizes, configurations and seeds).
The recorded bits are those of the library BEFORE the epilogue was restructured: the restructured one only moves loads
ahead of stores, every output element keeps its order of operations."""
import functools

import torch

import conv_fp64 as V
from parent_bits import DEV, digest, forced

NAME = "conv_epilogue"
SOURCES = ("codd_amd/csrc/conv_kernel.h", "codd_amd/csrc/conv_quad_kernel.h")
SENTINEL = -7.25


def _fp64_tests():
    """The module tests/test_gpu_conv_fp64: the launch of the sweep and of the multi jobs is the test file's own.  (Imported
    where a launch needs it: the key list needs neither it nor the library.)"""
    import test_gpu_conv_fp64 as T
    return T


# ------------------------------------------------------------------------------------------------ the db sweep
def is_fp32_family(cfg):
    return not (len(cfg) > 4 and cfg[4] == 2)


def sweep_key(e):
    return "sweep/%s|%s" % (e.sig, ",".join(str(int(v)) for v in e.cfg))


def sweep_entries():
    """{Layer: [(key, Entry, Geom, act, operands)]} of the exact-fp32 entries of the db sweep, in its order."""
    out = {}
    for L, items in V.sweep().items():
        mine = [(sweep_key(e), e, geom, act, operands) for (e, geom, act, operands) in items if is_fp32_family(e.cfg)]
        if mine:
            out[L] = mine
    return out


@functools.lru_cache(maxsize=8)
def _case(geom, wide, act, operands):
    return V.make_case(geom, wide, act, operands), {}


def sweep_digests(items):
    """``items``: the entries of one layer, a value of sweep_entries()."""
    T, out = _fp64_tests(), {}
    for (key, e, geom, act, operands) in items:
        case, holder = _case(geom, V.MODE_OF_TERMS[e.terms] in V.WIDE_MODES, act, operands)
        out[key] = digest(T._launch(case, holder, e.cfg, e.terms, co=e.co))
    return out


# ------------------------------------------------------------------------------------------------ the multi launch
class _Patch:
    """The two calls of pytest's monkeypatch that test_gpu_conv_fp64._multi_run makes (for the generator)."""

    @staticmethod
    def setattr(obj, name, value):
        setattr(obj, name, value)


def multi_keys():
    return ["multi/%d" % n for n in range(4)]


def multi_digests(monkeypatch=None):
    from codd_amd import ops
    T = _fp64_tests()
    prev = ops.set_conv_precision("fp32")
    try:
        outs = T._multi_run(T._multi_jobs(), monkeypatch or _Patch)
    finally:
        ops.set_conv_precision(prev)
    assert len(outs) == 4
    return {k: digest(o) for k, o in zip(multi_keys(), outs)}


# ------------------------------------------------------------------------------------------------ hand-made cases
HAND_SIZES = ((9, 21), (10, 24))
HAND = {  # name -> (cin, cout, kernel, C1 of the second input, deconv, act, operands)
    "cout18": (16, 18, 3, 0, False, "lrelu", ("res1",)),
    "two_inputs": (16, 16, 3, 5, False, "tanh", ("post",)),
    "deconv": (16, 6, 1, 0, True, "relu", ()),
    "all_operands_relu_ch0": (16, 32, 3, 0, False, "relu_ch0", ("res1", "res2", "post")),
}


def geometry(layer, H, W, layout):
    """(Hin, Win, (pad t, l, b, r)) of a hand-made ``layer`` (a value of HAND), or None where the quad kernel cannot run
    it (its input rows are a multiple of 4 floats: a 3x3 layer gets the widest input that is a multiple of 4 columns and
    the right padding that gives the output width, the transposed convolution has Win = Wout)."""
    k, deconv = layer[2], layer[4]
    if deconv:
        return None if (layout == 1 and W % 4) else (H, W, (0, 0, 0, 0))
    assert k == 3
    if layout == 1 and W % 4:
        Win = W - W % 4
        return (H, Win, (1, 1, 1, W + 1 - Win))
    return (H, W, (1, 1, 1, 1))


def _inputs(layer, H, W, layout, seed, bias=True):
    cin, cout, k, C1, deconv, act, operands = layer
    Hin, Win, pad = geometry(layer, H, W, layout)
    g = torch.Generator().manual_seed(seed)
    up = 2 if deconv else 1
    d = dict(x=torch.randn(V.B, cin, Hin, Win, generator=g),
             w=(torch.randn(cin, cout, 2, 2, generator=g) if deconv else torch.randn(cout, cin, k, k, generator=g)) / (cin * k * k) ** 0.5,
             bias=torch.randn(cout, generator=g) if bias else None)
    for o in ("res1", "res2", "post"):
        d[o] = torch.randn(V.B, cout, H * up, W * up, generator=g) if o in operands else None
    return d, (Hin, Win, pad)


def _guarded(shape, fill, off):
    """A contiguous tensor of ``shape`` that starts ``off`` floats into a flat sentinel-filled allocation (off = 1: 4
    bytes past a 16-byte boundary), and the allocation."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 8,), SENTINEL, device=DEV)
    t = flat[off:off + n].view(shape)
    assert t.is_contiguous() and flat.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 4 * off
    t.fill_(fill)
    return t, flat


def launch(layer, H, W, npb, nw, layout, seed, bias=True, in_place=False, misalign=False):
    """One launch of a hand-made ``layer`` (a value of HAND, inputs seeded with ``seed``) on the configuration (npb, nw,
    ck 16, mb, layout) -> the output on the host.  The first input is a Slice of a sentinel-filled buffer, the output a
    Slice at channel 3 of a sentinel-filled buffer pre-filled with NaN; the buffer's other channels must come back
    untouched.  ``in_place``: res1 IS the output Slice (pre-filled with res1's values).  ``misalign``: the output buffer,
    res1 and post each start one float into a flat sentinel-filled allocation (4 bytes off a 16-byte boundary; the input
    stays aligned); the floats in front of and behind each of them must come back untouched, and res1 and post unchanged.
    (The views are dense NCHW, as the library requires: between two channel planes of a view there is no room for a
    sentinel, so what surrounds the planes is guarded -- the floats around every allocation and the sentinel channels on
    both sides of the output Slice in every batch item -- and a write that leaves its plane inside the Slice shows in the
    bit comparison with the aligned launch.)"""
    from codd_amd import ops
    from codd_amd.ops import Slice
    cin, cout, k, C1, deconv, act, operands = layer
    d, (Hin, Win, pad) = _inputs(layer, H, W, layout, seed, bias)
    B, C0, up = V.B, cin - C1, 2 if deconv else 1
    off = 1 if misalign else 0
    xbuf = torch.full((B, C0 + 8, Hin, Win), SENTINEL, device=DEV)
    xbuf[:, 6:6 + C0] = d["x"][:, :C0].to(DEV)
    x2 = d["x"][:, C0:].contiguous().to(DEV) if C1 else None
    pc = ops.PackedConv(d["w"].to(DEV), None if d["bias"] is None else d["bias"].to(DEV), deconv=deconv)
    obuf, oflat = _guarded((B, cout + 5, H * up, W * up), SENTINEL, off)
    obuf[:, 3:3 + cout] = float("nan")
    out = Slice(obuf, 3, cout)
    guards = [(oflat, off)]
    opnd = {}
    for o in ("res1", "res2", "post"):
        opnd[o] = None
        if d[o] is not None:
            o_off = off if o in ("res1", "post") else 0
            t, flat = _guarded(tuple(d[o].shape), 0.0, o_off)
            t.copy_(d[o].to(DEV))
            opnd[o] = t
            guards.append((flat, o_off))
    if in_place:
        assert opnd["res1"] is not None
        obuf[:, 3:3 + cout] = opnd["res1"]
        opnd["res1"] = out
    prev = ops.set_conv_precision("fp32")
    try:
        forced(pc, (H, W, B, 1, 1, 1, 1, pad[1], C1 > 0, 0), (npb, nw, 16, pc.mb, layout),
               lambda: ops.conv2d(Slice(xbuf, 6, C0), pc, x2=x2, pad_tl=pad, act=act, res1=opnd["res1"], res2=opnd["res2"],
                                  post=opnd["post"], out=out, out_hw=None if deconv else (H, W)))
    finally:
        ops.set_conv_precision(prev)
    host = obuf.cpu()
    assert bool((host[:, :3] == SENTINEL).all()) and bool((host[:, 3 + cout:] == SENTINEL).all()), "sentinel channels"
    for flat, g_off in guards:
        f = flat.cpu()
        n = f.numel() - 8
        assert bool((f[:g_off] == SENTINEL).all()) and bool((f[g_off + n:] == SENTINEL).all()), "sentinel floats around an allocation"
    for o in ("res1", "res2", "post"):
        if isinstance(opnd[o], torch.Tensor):
            assert torch.equal(opnd[o].cpu().view(torch.int32), d[o].view(torch.int32)), "operand %s changed" % o
    return host[:, 3:3 + cout].contiguous()


def hand_keys():
    return ["hand/%s/%dx%d/l%d" % (name, H, W, layout) for name in HAND for (H, W) in HAND_SIZES for layout in (0, 1)
            if geometry(HAND[name], H, W, layout) is not None]


def hand_launch(name, H, W, layout, in_place=False):
    """launch() of a layer of HAND on the configuration (npb 1, nw 4, ck 16, mb, layout)."""
    return launch(HAND[name], H, W, 1, 4, layout, 7 + 1000 * list(HAND).index(name) + 10 * W + layout, in_place=in_place)


def hand_digests():
    out = {}
    for key in hand_keys():
        _, name, hw, lay = key.split("/")
        H, W = (int(v) for v in hw.split("x"))
        out[key] = digest(hand_launch(name, H, W, int(lay[1:])))
    return out


# ------------------------------------------------------------------------------------------------ all of it
def groups():
    """[(group id, keys, function -> {key: digest})] in the fixture's order."""
    return ([("sweep/" + V.layer_id(L), [k for (k, *_) in items], functools.partial(sweep_digests, items))
             for L, items in sweep_entries().items()] +
            [("multi", multi_keys(), multi_digests), ("hand", hand_keys(), hand_digests)])
