"""The launches whose output bits tests/golden/conv_epilogue_vec_bits.json records (sha256 of the fp32 output bytes), shared
by the generator tools/parent_bits.py --cases conv_epilogue_vec and by tests/test_gpu_conv_epilogue_vec_bits.py.  They
reach the decisions of the vector epilogue (conv_kernel.h conv_epilogue: a lane holds four consecutive pixels of one
channel; 16-byte accesses where ConvK.evec allows, 4-byte accesses under a per-pixel predicate elsewhere) that
tests/conv_epilogue_cases.py does not:

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
import torch

import conv_epilogue_cases as E
from conv_epilogue_cases import SENTINEL
from parent_bits import DEV, digest, forced  # noqa: F401

NAME = "conv_epilogue_vec"
SOURCES = E.SOURCES
B = E.V.B
SIZES = ((9, 20), (5, 4), (9, 12), (6, 36), (9, 22), (9, 21), (7, 30))
CONFIGS = ((1, 4, 0), (1, 4, 1), (2, 4, 0), (2, 4, 1), (4, 4, 0), (4, 4, 1), (1, 9, 1))  # (npb, nw, layout)
LAYERS = dict(E.HAND)  # name -> (cin, cout, kernel, C1 of the second input, deconv, act, operands)
LAYERS["no_bias"] = (16, 16, 3, 0, False, "lrelu", ("res1",))
NO_BIAS = ("no_bias",)


def geometry(name, H, W, layout):
    """(Hin, Win, (pad t, l, b, r)) or None where the quad kernel cannot run the case (conv_epilogue_cases.geometry)."""
    return E.geometry(LAYERS[name], H, W, layout)


def key_of(name, H, W, npb, nw, layout):
    return "vec/%s/%dx%d/n%dw%d/l%d" % (name, H, W, npb, nw, layout)


def cases():
    """[(key, name, H, W, npb, nw, layout)] in the fixture's order."""
    return [(key_of(name, H, W, npb, nw, layout), name, H, W, npb, nw, layout) for name in LAYERS for (H, W) in SIZES
            for (npb, nw, layout) in CONFIGS if geometry(name, H, W, layout) is not None]


def launch(name, H, W, npb, nw, layout, in_place=False, misalign=False):
    """conv_epilogue_cases.launch of a layer of LAYERS -> the output on the host."""
    return E.launch(LAYERS[name], H, W, npb, nw, layout, 11 + 1000 * list(LAYERS).index(name) + 10 * W + H + 7 * layout,
                    bias=name not in NO_BIAS, in_place=in_place, misalign=misalign)


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
                forced(j["pc"], (H, W, B, j["stride"], j["stride"], 1, 1, 1, False, 0), (1, 4, 16, 1, 1),
                       lambda: ops.conv2d(j["x"], j["pc"], stride=j["stride"], pad=1, act=j["act"], res1=j["res1"],
                                          out=Slice(obuf, 3, 16)))
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


def groups():
    """[(group id, keys, function -> {key: digest})] in the fixture's order."""
    return [("cases", [c[0] for c in cases()], case_digests), ("multi", multi_keys(), multi_digests)]
