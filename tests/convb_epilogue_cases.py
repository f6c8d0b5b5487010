"""The launches whose output bits tests/golden/convb_epilogue_bits.json records (sha256 of the bytes the launch wrote),
shared by the generator tools/parent_bits.py --cases convb_epilogue and by tests/test_gpu_convb_epilogue_bits.py: the
epilogues of the split-bf16 convolution kernel (conv_bf16_kernel.h) on every instantiated wave grid X(PGW, CGW, A, B, KS) of CONVB_ALL, in
the four operand formats (terms 1, 3, 16, 48), at B = 2 on three maps:

    9 x 21   partial tiles in both axes; the second 16-pixel unit of a row is valid for 5 lanes
    10 x 24  Wout % 4 == 0 (the 16-byte path of the fp32 epilogue); the second unit is valid for a single lane group pair
    7 x 30   the product's coarse width (4-byte path); one tile row, the last pixel units of tall tiles hold no pixel

Every layer is a 3 x 3 'same' convolution of 32 channels (ck = 16: two chunks, so the k-split kernels have their exchange
room in the ring), tiles 32 pixels wide and PGW * A / 2 rows high.  Key ``<X>/<H>x<W>/t<terms>/<case>``:

  rec_*   record output (xs_out), no gate: cout 64 | 18 (the per-element bias path and the zeroed octet padding), with and
          without bias, relu | none, written at channel offset 8 | 0 into a record tensor with border 1 | 0 | 4.  The digest
          is the WHOLE record tensor; its interior octets are pre-filled with 0x5A bytes so an unwritten record shows.
  g1, g2_G16, g2_G32, g3, g3_inplace   the gate epilogues: gate 2 with G = 16 (3G = 48 does not fill a 64-channel group;
          a wave with B = 4 meets z, r*h, q-input and an empty block) and G = 32; gate 3 into a tensor of its own (a
          slice at channel 4 between sentinel channels) and with out = post.  Digest: the channel-quad output tensor
          (sentinel channels included) and the record tensor.
  f32_*   fp32 output (OUTF == 0): res1 + res2 + post with relu_ch0 on 18 channels, res1 = the output Slice, and the
          transposed store (k-split grids cannot run that 1 x 1 layer: no exchange room; they have no such case).
Hazards: every operand and the bias hold one NaN and one -0.
``bias_off4`` (no digest): a bias 4 bytes off a 16-byte boundary must be refused with CODD_EINVAL."""
import functools

import torch

from parent_bits import DEV, digest, forced

NAME = "convb_epilogue"
SOURCES = ("codd_amd/csrc/conv_bf16_kernel.h",)
B = 2
CIN = 32
SENTINEL = 12345.0
SIZES = ((9, 21), (10, 24), (7, 30))
TERMS = (1, 3, 16, 48)
MODE_OF_TERMS = {1: "bf16", 3: "split", 16: "fp16", 48: "split16"}
# X(PGW, CGW, A, B, KS) of CONVB_ALL (conv_bf16_kernel.h), in its order
CONVB_ALL = ((2, 2, 5, 2, 1), (4, 1, 4, 4, 1), (4, 1, 4, 2, 1), (4, 1, 4, 1, 1), (4, 1, 8, 1, 1), (4, 1, 2, 2, 1), (4, 1, 2, 1, 1),
             (4, 1, 3, 4, 1), (4, 1, 3, 2, 1), (2, 2, 5, 2, 2), (4, 1, 4, 2, 2), (4, 1, 3, 2, 2), (4, 1, 3, 4, 2), (4, 2, 4, 2, 1),
             (4, 2, 3, 2, 1), (8, 1, 4, 4, 1))
REC = {  # name -> (cout, bias, act, border, channel offset)
    "rec_c64_bias_relu_b1": (64, True, "relu", 1, 8),
    "rec_c64_nobias_none_b0": (64, False, "none", 0, 0),
    "rec_c18_bias_none_b4": (18, True, "none", 4, 8),
    "rec_c18_nobias_relu_b1": (18, False, "relu", 1, 8),
}
GATES = ("g1", "g2_G16", "g2_G32", "g3", "g3_inplace")
F32 = ("f32_all_relu_ch0", "f32_res1_is_out", "f32_deconv")


def xname(X):
    return "x%d_%d_%d_%d_k%d" % X


def header_convb_all():
    """The expansion of CONVB_ALL parsed from conv_bf16_kernel.h: [(PGW, CGW, A, B, KS)] in its order."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "codd_amd", "csrc", "conv_bf16_kernel.h")).read()
    groups = dict(re.findall(r"#define CONVB_GROUP_(\w)\(X\) (.*)", src))
    listed = re.search(r"#define CONVB_ALL\(X\)(.*?)\n#define", src, re.S).group(1)
    return [tuple(int(v) for v in x) for gname in re.findall(r"CONVB_GROUP_(\w)\(X\)", listed)
            for x in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+)\)", groups[gname])]


def cfg_of(X, terms):
    """The stored launch configuration (xb, th, ck, mb, 2, pgw, cgw, terms, ksplit) that runs instantiation X: tiles of
    th x 32 pixels = PGW * A pixel units, mb = B * CGW channel blocks."""
    pgw, cgw, a, b, ks = X
    assert (pgw * a) % 2 == 0
    return (2, pgw * a // 2, 16, b * cgw, 2, pgw, cgw, terms, ks)


def case_names(X):
    return list(REC) + list(GATES) + [n for n in F32 if not (n == "f32_deconv" and X[4] == 2)]


def key_of(X, H, W, terms, name):
    return "%s/%dx%d/t%d/%s" % (xname(X), H, W, terms, name)


def cases():
    """[(key, X, H, W, terms, name)] in the fixture's order."""
    return [(key_of(X, H, W, t, n), X, H, W, t, n) for X in CONVB_ALL for (H, W) in SIZES for t in TERMS for n in case_names(X)]


def _hazards(t):
    """One NaN and one -0 in a tensor (first batch item, away from the corner)."""
    flat = t.view(-1)
    flat[flat.numel() // 3] = float("nan")
    flat[flat.numel() // 3 + 1] = -0.0
    return t


@functools.lru_cache(maxsize=4)
def inputs(H, W):
    """Seeded host tensors of one map: the input, weights and biases per cout, operands per channel count."""
    g = torch.Generator().manual_seed(77000 + 100 * H + W)
    rnd = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=rnd(B, CIN, H, W))
    for cout in (18, 32, 48, 64, 96):
        d["w", cout] = rnd(cout, CIN, 3, 3) / (CIN * 9) ** 0.5
        bias = rnd(cout)
        bias[5], bias[9] = float("nan"), -0.0
        d["b", cout] = bias
    d["wT"] = rnd(CIN, 18, 2, 2) / CIN ** 0.5
    for c in (16, 18, 32, 48, 64, 96):
        for o in ("res1", "res2", "post"):
            d[o, c] = _hazards(rnd(B, c, H, W))
    d["h", 32] = _hazards(torch.tanh(rnd(B, 32, H, W)))
    d["h", 16] = _hazards(torch.tanh(rnd(B, 16, H, W)))
    d["zq", 64] = _hazards(torch.sigmoid(rnd(B, 64, H, W)))
    return d


def _record_tensor(C, H, W, border, coff, terms):
    """A zeroed SplitTensor as ops.split_buffer makes them, with room for C channels from channel ``coff`` on; the image
    interior of the octets the launch writes is pre-filled with 0x5A bytes."""
    from codd_amd import _abi, ops
    c8 = -(-(coff + C) // 32) * 4
    hp, wp = 2 * border + ops._split_rows(H), 2 * border + -(-W // 32) * 32
    planes = 2 if terms in (3, 48) else 1
    buf = torch.zeros(_abi.load().codd_split_bf16_bytes(B, c8, hp, wp, terms), device=DEV, dtype=torch.uint8)
    assert buf.numel() == B * planes * c8 * hp * wp * 16
    v = buf.view(B, planes, c8, hp, wp, 16)
    v[:, :, coff // 8:-(-(coff + C) // 8), border:border + H, border:border + W] = 0x5A
    return ops.SplitTensor(buf, B, coff + C, H, W, border, border, hp, wp, c8, terms)


def _c4(t, pad=0):
    """The C4Tensor holding ``t`` [B,C,H,W] in channels [pad, pad + C) between ``pad`` sentinel channels on both sides."""
    from codd_amd import ops
    Bn, Cn, H, W = t.shape
    full = torch.full((Bn, Cn + 2 * pad, H, W), SENTINEL)
    full[:, pad:pad + Cn] = t
    c4 = ops.C4Tensor(torch.empty(Bn * (Cn + 2 * pad) * H * W, device=DEV), Bn, Cn + 2 * pad, H, W)
    return ops.to_c4(full.to(DEV), c4)


def launch(X, H, W, terms, name, bias_off4=False):
    """One launch of instantiation X -> the digest of what it wrote."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    d, cfg = inputs(H, W), cfg_of(X, terms)
    prev = ops.set_conv_precision(MODE_OF_TERMS[terms])
    try:
        if name in REC:
            cout, has_bias, act, border, coff = REC[name]
            bias = d["b", cout].to(DEV) if has_bias else None
            pc = ops.PackedConv(d["w", cout].to(DEV), bias)
            if bias_off4:
                flat = torch.zeros(cout + 8, device=DEV)
                flat[1:1 + cout] = d["b", cout].to(DEV)
                pc.bias = flat[1:1 + cout]
                assert pc.bias.data_ptr() % 16 == 4
            rec = _record_tensor(cout, H, W, border, coff, terms)
            key = (H, W, B, 1, 1, 1, 1, 1, False, terms, "split")
            forced(pc, key, cfg, lambda: ops.conv2d(d["x"].to(DEV), pc, pad=1, act=act, xs_out=rec, xs_out_coff=coff))
            return digest(rec.buf)
        if name in GATES:
            gate = int(name[1])
            G = 16 if name == "g2_G16" else 32
            cout = {1: 2 * G, 2: 3 * G, 3: G}[gate]
            pc = ops.PackedConv(d["w", cout].to(DEV), d["b", cout].to(DEV))
            xs = ops.split_input(d["x"].to(DEV), border=1)
            key = ("gate", gate, H, W, B, 1, 1, 0, terms)
            if gate == 1:
                out = _c4(torch.full((B, cout, H, W), float("nan")), 4)
                forced(pc, key, cfg, lambda: ops.conv_gate(pc, xs, 1, pad=1, out=out, out_coff=4))
                return digest(out.buf)
            rec = _record_tensor(G, H, W, 1, 0, terms)
            if gate == 2:
                out = _c4(torch.full((B, 2 * G, H, W), float("nan")), 4)
                ctx, t12, h = _c4(d["res1", 3 * G]), _c4(d["res2", 2 * G]), _c4(d["h", G])
                forced(pc, key, cfg, lambda: ops.conv_gate(pc, xs, 2, pad=1, out=out, out_coff=4, res1=ctx, res2=t12, post=h,
                                                            xs_out=rec))
                assert digest(ctx.buf, t12.buf, h.buf) == digest(_c4(d["res1", 3 * G]).buf, _c4(d["res2", 2 * G]).buf, _c4(d["h", G]).buf), "operand changed"
                return digest(out.buf, rec.buf)
            zq, h = _c4(d["zq", 2 * G]), _c4(d["h", G])
            if name == "g3_inplace":
                forced(pc, key, cfg, lambda: ops.conv_gate(pc, xs, 3, pad=1, out=h, res1=zq, post=h, xs_out=rec))
                return digest(h.buf, rec.buf)
            out = _c4(torch.full((B, G, H, W), float("nan")), 4)
            forced(pc, key, cfg, lambda: ops.conv_gate(pc, xs, 3, pad=1, out=out, out_coff=4, res1=zq, post=h, xs_out=rec))
            host = out.nchw().cpu()
            assert bool((host[:, :4] == SENTINEL).all()) and bool((host[:, 4 + G:] == SENTINEL).all()), "sentinel channels"
            return digest(host[:, 4:4 + G], rec.buf)
        deconv = name == "f32_deconv"
        cout, up = 18, 2 if deconv else 1
        pc = ops.PackedConv((d["wT"] if deconv else d["w", cout]).to(DEV), d["b", cout].to(DEV), deconv=deconv)
        obuf = torch.full((B, cout + 5, H * up, W * up), SENTINEL, device=DEV)
        obuf[:, 3:3 + cout] = float("nan")
        out = Slice(obuf, 3, cout)
        opnd = dict(res1=None, res2=None, post=None)
        if name == "f32_all_relu_ch0":
            opnd = {o: d[o, cout].to(DEV) for o in opnd}
        elif name == "f32_res1_is_out":
            obuf[:, 3:3 + cout] = d["res1", cout].to(DEV)
            opnd["res1"] = out
        pad = 0 if deconv else 1
        key = (H, W, B, 1, 1, 1, 1, pad, False, terms)
        forced(pc, key, cfg, lambda: ops.conv2d(d["x"].to(DEV), pc, pad=pad, act="none" if deconv else "relu_ch0", out=out, **opnd))
        host = obuf.cpu()
        assert bool((host[:, :3] == SENTINEL).all()) and bool((host[:, 3 + cout:] == SENTINEL).all()), "sentinel channels"
        return digest(host[:, 3:3 + cout])
    finally:
        ops.set_conv_precision(prev)


def case_digests(mine):
    """``mine``: entries of cases()."""
    return {key: launch(*rest) for (key, *rest) in mine}


def groups():
    """[(group id, keys, function -> {key: digest})] in the fixture's order: one group per instantiation X.  (The fixture
    lists an instantiation's maps outside its operand formats, so the (X, terms) unit of the test is no contiguous run
    of keys and cannot be a group.)"""
    every = cases()
    by_x = [(X, [c for c in every if c[1] == X]) for X in CONVB_ALL]
    return [(xname(X), [c[0] for c in mine], functools.partial(case_digests, mine)) for (X, mine) in by_x]
