"""The launches whose output bits tests/golden/conv_epilogue_bits.json records (sha256 of the fp32 output bytes), shared
by the generator tools/conv_epilogue_bits.py and by tests/test_gpu_conv_epilogue_bits.py:

* ``sweep/<sig>|<cfg>``: every exact-fp32 entry (configuration not of layout 2) of conv_fp64.sweep(), launched exactly
  as tests/test_gpu_conv_fp64.py::_launch does (its setup is documented there);
* ``multi/<n>``: the four jobs of test_gpu_conv_fp64._multi_jobs() as ONE codd_conv2d_multi launch;
* ``hand/<case>/<H>x<W>/l<layout>``: four hand-made layers at a 9 x 21 output (Wout & 3 != 0) and a 10 x 24 one, on the
  classic (layout 0) and, where its rows are 16-byte aligned, the quad (layout 1) kernel, 4 x 16 tiles, B = 2:
  cout = 18 (a channel tail inside the second 16-block), two inputs, the transposed-convolution store, and
  res1 + res2 + post together with relu_ch0.
The recorded bits are those of the library BEFORE the epilogue was restructured: the restructured one only moves loads
ahead of stores, every output element keeps its order of operations."""
import functools
import hashlib
import warnings

import torch

import conv_fp64 as V

DEV = "cuda:0"
SENTINEL = -7.25


def digest(t):
    """sha256 of the bytes of a host fp32 tensor (NaN payloads included)."""
    t = t.contiguous()
    assert t.dtype == torch.float32 and t.device.type == "cpu"
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


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


def sweep_digest(T, e, geom, act, operands):
    """``T``: the module tests/test_gpu_conv_fp64 (its _launch runs the entry)."""
    case, holder = _case(geom, V.MODE_OF_TERMS[e.terms] in V.WIDE_MODES, act, operands)
    return digest(T._launch(case, holder, e.cfg, e.terms, co=e.co))


# ------------------------------------------------------------------------------------------------ the multi launch
class _Patch:
    """The two calls of pytest's monkeypatch that test_gpu_conv_fp64._multi_run makes (for the generator)."""

    @staticmethod
    def setattr(obj, name, value):
        setattr(obj, name, value)


def multi_keys():
    return ["multi/%d" % n for n in range(4)]


def multi_digests(T, monkeypatch=None):
    from codd_amd import ops
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


def hand_geometry(name, H, W, layout):
    """(Hin, Win, (pad t, l, b, r)) of a hand-made case, or None where the quad kernel cannot run it (its input rows
    are a multiple of 4 floats: the 3x3 layers get a right padding of 2 on a 20-column input for the 21-column output,
    the transposed convolution has Win = Wout)."""
    k, deconv = HAND[name][2], HAND[name][4]
    if deconv:
        return None if (layout == 1 and W % 4) else (H, W, (0, 0, 0, 0))
    assert k == 3
    if layout == 1 and W % 4:
        return (H, W - 1, (1, 1, 1, 2))
    return (H, W, (1, 1, 1, 1))


def hand_keys():
    return ["hand/%s/%dx%d/l%d" % (name, H, W, layout) for name in HAND for (H, W) in HAND_SIZES for layout in (0, 1)
            if hand_geometry(name, H, W, layout) is not None]


def _hand_inputs(name, H, W, layout):
    cin, cout, k, C1, deconv, act, operands = HAND[name]
    Hin, Win, pad = hand_geometry(name, H, W, layout)
    g = torch.Generator().manual_seed(7 + 1000 * list(HAND).index(name) + 10 * W + layout)
    up = 2 if deconv else 1
    d = dict(x=torch.randn(V.B, cin, Hin, Win, generator=g),
             w=(torch.randn(cin, cout, 2, 2, generator=g) if deconv else torch.randn(cout, cin, k, k, generator=g)) / (cin * k * k) ** 0.5,
             bias=torch.randn(cout, generator=g))
    for o in ("res1", "res2", "post"):
        d[o] = torch.randn(V.B, cout, H * up, W * up, generator=g) if o in operands else None
    return d, (Hin, Win, pad)


def hand_launch(name, H, W, layout, in_place=False):
    """One hand-made launch on the configuration (npb 1, nw 4, ck 16, mb, layout) -> the output on the host.  The first
    input is a Slice of a sentinel-filled buffer, the output a Slice at channel 3 of a sentinel-filled buffer whose
    other channels must come back untouched.  ``in_place``: res1 IS the output Slice (pre-filled with res1's values)."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    cin, cout, k, C1, deconv, act, operands = HAND[name]
    d, (Hin, Win, pad) = _hand_inputs(name, H, W, layout)
    C0, up = cin - C1, 2 if deconv else 1
    xbuf = torch.full((V.B, C0 + 8, Hin, Win), SENTINEL, device=DEV)
    xbuf[:, 6:6 + C0] = d["x"][:, :C0].to(DEV)
    x2 = d["x"][:, C0:].contiguous().to(DEV) if C1 else None
    pc = ops.PackedConv(d["w"].to(DEV), d["bias"].to(DEV), deconv=deconv)
    obuf = torch.full((V.B, cout + 5, H * up, W * up), SENTINEL, device=DEV)
    obuf[:, 3:3 + cout] = float("nan")
    out = Slice(obuf, 3, cout)
    dev = lambda t: None if t is None else t.to(DEV)
    res1 = dev(d["res1"])
    if in_place:
        assert res1 is not None
        obuf[:, 3:3 + cout] = res1
        res1 = out
    cfg = (1, 4, 16, pc.mb, layout)
    key = (H, W, V.B, 1, 1, 1, 1, pad[1], C1 > 0, 0)
    prev = ops.set_conv_precision("fp32")
    try:
        pc.tuned[key] = cfg
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ops.conv2d(Slice(xbuf, 6, C0), pc, x2=x2, pad_tl=pad, act=act, res1=res1, res2=dev(d["res2"]), post=dev(d["post"]),
                       out=out, out_hw=None if deconv else (H, W))
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision(prev)
    assert dict(pc.tuned) == {key: cfg} and not caught, (dict(pc.tuned), [str(w.message) for w in caught])
    host = obuf.cpu()
    assert bool((host[:, :3] == SENTINEL).all()) and bool((host[:, 3 + cout:] == SENTINEL).all()), "sentinel channels"
    return host[:, 3:3 + cout].contiguous()


def hand_digests():
    out = {}
    for key in hand_keys():
        _, name, hw, lay = key.split("/")
        H, W = (int(v) for v in hw.split("x"))
        out[key] = digest(hand_launch(name, H, W, int(lay[1:])))
    return out


def all_keys():
    return [k for items in sweep_entries().values() for (k, *_) in items] + multi_keys() + hand_keys()
