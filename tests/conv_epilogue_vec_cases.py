"""The launches whose output bits tests/golden/conv_epilogue_vec_bits.json records (sha256 of the fp32 output bytes), shared
by the generator tools/conv_epilogue_vec_bits.py and by tests/test_gpu_conv_epilogue_vec_bits.py.  They reach the decisions
of the vector epilogue (conv_kernel.h conv_epilogue: a lane holds four consecutive pixels of one channel; 16-byte accesses
where ConvK.evec allows, 4-byte accesses under a per-pixel predicate elsewhere) that tests/conv_epilogue_cases.py does not:

* ``vec/<layer>/<H>x<W>/n<npb>w<nw>/l<layout>``: five hand-made layers (the four of conv_epilogue_cases.HAND and one without
  a bias) at B = 2 on seven output sizes and seven launch configurations:
    9 x 20   the second 16-block of a row is valid for exactly one lane group (pixels 16..19)
    5 x 4, 9 x 12   narrower than one block
    6 x 36   the second 32-wide tile is valid for one quad
    9 x 22, 9 x 21   Wout % 4 != 0: 4-byte path with a partial quad
    7 x 30   the product's coarse width (4-byte path)
  (npb, nw) = (1, 4), (2, 4), (4, 4) on the classic (layout 0) and the quad (layout 1) kernel -- 4 x 16, 4 x 32 (two blocks
  along x) and 8 x 32 (two rows per wave) tiles -- and (1, 9) on the quad kernel; ck = 16, mb follows cout.  The quad kernel
  runs where its input rows are 16-byte aligned: a 3 x 3 layer gets the widest input that is a multiple of 4 columns and
  the right padding that gives the output width, the transposed convolution (Win = Wout) only where Wout % 4 == 0.
* ``multi/<n>``: ONE codd_conv2d_multi launch of a 9 x 20 job (Wout % 4 == 0) and a 7 x 22 job (Wout % 4 != 0): the flag
  is per job.
The recorded bits are those of the library BEFORE the MFMA operands were swapped and the epilogue rewritten: every output
element is still C + sum_k w x over the same k in the same order and ((acc + bias) + res1) + res2 -> act -> + post."""
import warnings

import torch

import conv_epilogue_cases as E
from conv_epilogue_cases import DEV, SENTINEL, digest  # noqa: F401

B = E.V.B
SIZES = ((9, 20), (5, 4), (9, 12), (6, 36), (9, 22), (9, 21), (7, 30))
CONFIGS = ((1, 4, 0), (1, 4, 1), (2, 4, 0), (2, 4, 1), (4, 4, 0), (4, 4, 1), (1, 9, 1))  # (npb, nw, layout)
LAYERS = dict(E.HAND)  # name -> (cin, cout, kernel, C1 of the second input, deconv, act, operands)
LAYERS["no_bias"] = (16, 16, 3, 0, False, "lrelu", ("res1",))
NO_BIAS = ("no_bias",)


def geometry(name, H, W, layout):
    """(Hin, Win, (pad t, l, b, r)) or None where the quad kernel cannot run the case (its input rows are a multiple of 4
    floats)."""
    k, deconv = LAYERS[name][2], LAYERS[name][4]
    if deconv:
        return None if (layout == 1 and W % 4) else (H, W, (0, 0, 0, 0))
    assert k == 3
    if layout == 1 and W % 4:
        Win = W - W % 4
        return (H, Win, (1, 1, 1, W + 1 - Win))
    return (H, W, (1, 1, 1, 1))


def key_of(name, H, W, npb, nw, layout):
    return "vec/%s/%dx%d/n%dw%d/l%d" % (name, H, W, npb, nw, layout)


def cases():
    """[(key, name, H, W, npb, nw, layout)] in the fixture's order."""
    return [(key_of(name, H, W, npb, nw, layout), name, H, W, npb, nw, layout) for name in LAYERS for (H, W) in SIZES
            for (npb, nw, layout) in CONFIGS if geometry(name, H, W, layout) is not None]


def _inputs(name, H, W, layout):
    cin, cout, k, C1, deconv, act, operands = LAYERS[name]
    Hin, Win, pad = geometry(name, H, W, layout)
    g = torch.Generator().manual_seed(11 + 1000 * list(LAYERS).index(name) + 10 * W + H + 7 * layout)
    up = 2 if deconv else 1
    d = dict(x=torch.randn(B, cin, Hin, Win, generator=g),
             w=(torch.randn(cin, cout, 2, 2, generator=g) if deconv else torch.randn(cout, cin, k, k, generator=g)) / (cin * k * k) ** 0.5,
             bias=None if name in NO_BIAS else torch.randn(cout, generator=g))
    for o in ("res1", "res2", "post"):
        d[o] = torch.randn(B, cout, H * up, W * up, generator=g) if o in operands else None
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


def launch(name, H, W, npb, nw, layout, in_place=False, misalign=False):
    """One launch on the configuration (npb, nw, ck 16, mb, layout) -> the output on the host.  The first input is a Slice
    of a sentinel-filled buffer, the output a Slice at channel 3 of a sentinel-filled buffer pre-filled with NaN; the
    buffer's other channels must come back untouched.  ``in_place``: res1 IS the output Slice (pre-filled with res1's
    values).  ``misalign``: the output buffer, res1 and post each start one float into a flat sentinel-filled allocation
    (4 bytes off a 16-byte boundary; the input stays aligned); the floats in front of and behind each of them must come
    back untouched, and res1 and post unchanged.  (The views are dense NCHW, as the library requires: between two channel
    planes of a view there is no room for a sentinel, so what surrounds the planes is guarded -- the floats around every
    allocation and the sentinel channels on both sides of the output Slice in every batch item -- and a write that leaves
    its plane inside the Slice shows in the bit comparison with the aligned launch.)"""
    from codd_amd import ops
    from codd_amd.ops import Slice
    cin, cout, k, C1, deconv, act, operands = LAYERS[name]
    d, (Hin, Win, pad) = _inputs(name, H, W, layout)
    C0, up = cin - C1, 2 if deconv else 1
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
    cfg = (npb, nw, 16, pc.mb, layout)
    key = (H, W, B, 1, 1, 1, 1, pad[1], C1 > 0, 0)
    prev = ops.set_conv_precision("fp32")
    try:
        pc.tuned[key] = cfg
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ops.conv2d(Slice(xbuf, 6, C0), pc, x2=x2, pad_tl=pad, act=act, res1=opnd["res1"], res2=opnd["res2"], post=opnd["post"],
                       out=out, out_hw=None if deconv else (H, W))
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision(prev)
    assert dict(pc.tuned) == {key: cfg} and not caught, (dict(pc.tuned), [str(w.message) for w in caught])
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


def case_digests():
    return {key: digest(launch(*rest)) for (key, *rest) in cases()}


# ------------------------------------------------------------------------------------------------ the multi launch
def multi_keys():
    return ["multi/0", "multi/1"]


def multi_launch():
    """A 3 x 3 16 -> 16 layer with res1 at a 9 x 20 output and a stride-2 3 x 3 16 -> 16 layer at 7 x 22 (from 14 x 44),
    issued inside ``ops.deferred_convs()`` and so launched as ONE accepted codd_conv2d_multi -> the two outputs on the host.
    Each output is a Slice at channel 3 of a sentinel-filled buffer, pre-filled with NaN; the other channels must come back
    untouched."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    g = torch.Generator().manual_seed(4242)
    rnd = lambda *s: torch.randn(*s, generator=g)
    w0, b0, x0, r0 = rnd(16, 16, 3, 3) / 12.0, rnd(16), rnd(B, 16, 9, 20), rnd(B, 16, 9, 20)
    w1, b1, x1 = rnd(16, 16, 3, 3) / 12.0, rnd(16), rnd(B, 16, 14, 44)
    jobs = [dict(x=x0.to(DEV), pc=ops.PackedConv(w0.to(DEV), b0.to(DEV)), stride=1, act="relu", res1=r0.to(DEV), hw=(9, 20)),
            dict(x=x1.to(DEV), pc=ops.PackedConv(w1.to(DEV), b1.to(DEV)), stride=2, act="lrelu", res1=None, hw=(7, 22))]
    rcs, real = [], ops._launch_conv_multi

    def spy(lib, params, n, stream):
        rcs.append((n, real(lib, params, n, stream)))
        return rcs[-1][1]

    bufs = []
    prev = ops.set_conv_precision("fp32")
    ops._launch_conv_multi = spy
    try:
        with ops.deferred_convs():
            for j in jobs:
                H, W = j["hw"]
                obuf = torch.full((B, 16 + 5, H, W), SENTINEL, device=DEV)
                obuf[:, 3:3 + 16] = float("nan")
                bufs.append(obuf)
                j["pc"].tuned[(H, W, B, j["stride"], j["stride"], 1, 1, 1, False, 0)] = (1, 4, 16, 1, 1)
                ops.conv2d(j["x"], j["pc"], stride=j["stride"], pad=1, act=j["act"], res1=j["res1"], out=Slice(obuf, 3, 16))
        torch.cuda.synchronize()
    finally:
        ops._launch_conv_multi = real
        ops.set_conv_precision(prev)
    assert rcs == [(2, 0)], rcs
    outs = []
    for obuf in bufs:
        host = obuf.cpu()
        assert bool((host[:, :3] == SENTINEL).all()) and bool((host[:, 3 + 16:] == SENTINEL).all()), "sentinel channels"
        outs.append(host[:, 3:3 + 16].contiguous())
    assert tuple(outs[0].shape) == (B, 16, 9, 20) and tuple(outs[1].shape) == (B, 16, 7, 22)
    return outs


def multi_digests():
    return {k: digest(o) for k, o in zip(multi_keys(), multi_launch())}


def all_keys():
    return [c[0] for c in cases()] + multi_keys()
