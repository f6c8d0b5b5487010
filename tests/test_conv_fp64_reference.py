"""CPU checks of tests/conv_fp64.py, the fp64 reference of the convolution family: the reference is pinned against
torch's own fp64 convolutions for every geometry feature, the record codec by hand-computed bit patterns, ``c`` is
re-measured (two plain fp32 evaluations stay within a quarter of every bound), the operand bounds ``e_mode`` hold for an
emulation of every record format on every case of the db sweep, each wrong variant of a convolution exceeds the GPU
bound at least 2 x somewhere, and the coverage of the shipped tune db is stated as data."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_fp64 as V
from oracle import fusion as of

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _sweep():
    return V.sweep()


def _layer(want):
    return next(v[0] for L, v in _sweep().items() if want(L))


# ------------------------------------------------------------------------------------------------ the db
def test_signature_parser_and_triple_count():
    entries = V.load_db()
    assert len(entries) >= 1000
    e = V.parse_sig("b3|576,256,1,1,4,0|72,120,2,1,1,1,1,0,0|split|co", (1, 9, 32, 4, 2, 2, 2, 3, 1))
    assert (e.terms, e.cout_eff, e.cin, e.kh, e.mb, e.H, e.W, e.B, e.split, e.co) == (3, 576, 256, 1, 4, 72, 120, 2, True, True)
    e = V.parse_sig("64,3,7,7,2,0|256,320,1,2,2,1,1,3,0", (1, 8, 4, 2, 0))
    assert (e.terms, e.gate, e.cin, e.kh, e.sy, e.sx, e.pl, e.two, e.split) == (0, 0, 3, 7, 2, 2, 3, 0, False)
    e = V.parse_sig("g2,b16|384,384,1,1|48,160,1,0,1,0", (1, 8, 32, 2, 2, 4, 1, 16, 1))
    assert (e.gate, e.terms, e.cout_eff, e.cin, e.H, e.W, e.pl, e.dy, e.dil2) == (2, 16, 384, 384, 48, 160, 0, 1, 0)
    n = len(V.triples(entries))
    assert n >= 500, n  # (548 today: a db format change cannot empty the list)
    assert sum(len(v) for v in _sweep().values()) == len(V.plain_triples()) >= 400


def test_every_split_configuration_of_the_sweep_is_accepted_at_its_small_map():
    """The dry run of the library (codd_conv2d_check) takes every stored layout-2 configuration at the map of
    ``geometry``: no GPU launch of the sweep can fall back for a reason known here."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    n = 0
    for v in _sweep().values():
        for (e, g, _, _) in v:
            th, tw = V.tile_of(e.cfg)
            assert g.Hout == th + 3 and tw + 2 <= g.Wout <= tw + 9 < 2 * tw, (e.sig, g)  # two tiles, a ragged second one
            if not (len(e.cfg) > 4 and e.cfg[4] == 2):
                assert g.Win % 4 == 0 or e.cfg[4:5] != (1,), (e.sig, g)
                continue
            L, p = g.layer, _abi.ConvParams()
            p.terms, p.C0, p.B, p.Hout, p.Wout, p.Hin, p.Win = e.terms, L.cin, V.B, g.Hout, g.Wout, g.Hin, g.Win
            p.Cout, p.store_mode = (L.cout_eff // 4, 1) if L.deconv else (L.cout_eff, 0)
            p.kh, p.kw, p.sy, p.sx, p.pad_t, p.pad_l, p.dil_y, p.dil_x = L.kh, L.kw, L.sy, L.sx, g.pad[0], g.pad[1], L.dy, L.dx
            ops._set_cfg(p, e.cfg)
            assert lib.codd_conv2d_check(ctypes.byref(p)) == 0, (e.sig, e.cfg, g)
            n += 1
    assert n >= 50, n  # (83 today)


# What the shipped db reaches, asserted from the parsed db and ops._B_INST.  fp32: the (npb, nw, mb, layout) classes;
# layout 2: the (pgw, cgw, A, B, ksplit) instantiations (A = ceil(tile units / pgw), B = mb / cgw) with the terms and the
# epilogue kinds (plain, record output, gate 1 / 2 / 3) they are reached in.  NOT_REACHED is the rest, as data.
FP32_CLASSES = [(1, 2, 4, 0), (1, 4, 1, 0), (1, 4, 1, 1), (1, 4, 2, 0), (1, 4, 2, 1), (1, 4, 4, 0), (1, 4, 4, 1), (1, 8, 1, 0),
                (1, 8, 2, 0), (1, 8, 4, 0), (1, 9, 1, 1), (1, 9, 2, 0), (1, 9, 2, 1), (1, 9, 4, 1), (2, 4, 1, 0), (2, 4, 1, 1),
                (2, 4, 2, 0), (2, 4, 2, 1)]
NOT_REACHED = {
    "layout-2 instantiations": [],  # every entry of ops._B_INST is in some shipped entry
    "terms": [48],  # split16 has no db entries: the GPU sweep re-encodes the b3 configurations with terms 48
    # the exact-fp32 kernels also instantiate npb = 4 and nw = 2 / 8 / 9 with mb / layout combinations beyond
    # FP32_CLASSES; test_gpu_stereo_ops.py keeps covering those through the heuristic and hand-picked configurations
    "fp32": "every (npb, nw, mb, layout) outside FP32_CLASSES",
}


def test_coverage_of_the_shipped_db():
    from codd_amd import ops
    fp32, inst, kinds = set(), set(), set()
    for e in V.triples():
        c = e.cfg
        if len(c) > 4 and c[4] == 2:
            inst.add((c[5], c[6], -(-c[1] * c[0] // c[5]), c[3] // c[6], c[8] if len(c) > 8 else 1))
            kinds.add((e.terms, "gate %d" % e.gate if e.gate else ("record output" if e.split else "plain")))
        else:
            assert not e.gate and not e.split, e.sig
            fp32.add((c[0], c[1], c[3] if len(c) > 3 else e.mb, c[4] if len(c) > 4 else 0))
    assert sorted(fp32) == FP32_CLASSES
    assert inst <= set(ops._B_INST) and sorted(set(ops._B_INST) - inst) == NOT_REACHED["layout-2 instantiations"]
    assert kinds == {(t, k) for t in (1, 3, 16) for k in ("plain", "record output", "gate 1", "gate 2", "gate 3")}
    assert {e.cfg[8] for e in V.triples() if len(e.cfg) > 8} == {1, 2}  # both k-split depths
    n = (len(V.plain_triples()), len(V.split_triples()), len(V.gate_triples()))
    assert min(n) > 0 and sum(n) == len(V.triples()), n  # (432 + 92 + 24 today: every triple has a reference here; the GPU module runs the 432)


# ------------------------------------------------------------------------------------------------ reference pins
def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize("k,stride,pad,dil", [(3, (1, 1), (1, 1, 1, 1), (1, 1)), (3, (2, 2), (1, 1, 1, 1), (1, 1)),
                                              (3, (1, 1), (4, 4, 4, 4), (4, 4)), (3, (1, 1), (3, 3, 3, 3), (3, 3)),
                                              (7, (2, 2), (3, 3, 3, 3), (1, 1)), (4, (4, 1), (0, 0, 0, 3), (1, 1)),
                                              (4, (2, 2), (1, 1, 1, 1), (1, 1)), (1, (2, 2), (0, 0, 0, 0), (1, 1)),
                                              (3, (2, 1), (2, 0, 1, 3), (1, 2))])
def test_reference_matches_torch_fp64_convolution(k, stride, pad, dil):
    x, x2, w, b = _rnd(2, 5, 13, 18), _rnd(2, 3, 13, 18, seed=1), _rnd(6, 8, k, k, seed=2), _rnd(6, seed=3)
    pt, pl, pb, pr = pad
    want = F.conv2d(F.pad(torch.cat([x, x2], 1), (pl, pr, pt, pb)), w, b, stride, 0, dil)
    got, M = V.conv_ref(x, w, b, x2, stride, pad, dil)
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-13 * M.max()
    wantM = F.conv2d(F.pad(torch.cat([x, x2], 1).abs(), (pl, pr, pt, pb)), w.abs(), b.abs(), stride, 0, dil)
    assert (M - wantM - got.abs()).abs().max() <= 1e-13 * M.max()  # (M = L * M_pre + |act(v)|)
    oh = (want.shape[2] - 1, want.shape[3] - 2)  # out_hw smaller than the natural size: the top-left part
    got2, _ = V.conv_ref(x, w, b, x2, stride, pad, dil, out_hw=oh)
    assert torch.equal(got2, got[:, :, :oh[0], :oh[1]])


def test_reference_matches_torch_fp64_transposed_convolution():
    x, w, b = _rnd(2, 5, 7, 9), _rnd(5, 6, 2, 2, seed=1), _rnd(6, seed=2)
    want = F.conv_transpose2d(x, w, b, stride=2)
    got, M = V.conv_ref(x, w, b, deconv=True)
    assert got.shape == want.shape and (got - want).abs().max() <= 1e-13 * M.max()


def test_operand_order_and_activations():
    x, w, b = _rnd(2, 4, 6, 7), _rnd(5, 4, 3, 3, seed=1), _rnd(5, seed=2)
    r1, r2, post = _rnd(2, 5, 6, 7, seed=3), _rnd(2, 5, 6, 7, seed=4), _rnd(2, 5, 6, 7, seed=5)
    pre = F.conv2d(x, w * 4, b, 1, 1) + r1 + r2
    acts = dict(none=lambda v: v, lrelu=lambda v: F.leaky_relu(v, 0.2), relu=torch.relu, sigmoid=torch.sigmoid,
                tanh=torch.tanh, mish=of.mish,
                relu_ch0=lambda v: torch.cat([torch.relu(v[:, :1]), v[:, 1:]], 1))
    assert set(acts) == set(V.ACTS)
    for name, fn in acts.items():
        got, M = V.conv_ref(x, w * 4, b, None, (1, 1), (1, 1, 1, 1), (1, 1), None, name, r1, r2, post)
        want = fn(pre) + post
        assert (got - want).abs().max() <= 1e-13 * M.max(), name
        assert (M >= got.abs() * (1 - 1e-12)).all(), name


def test_mish_lipschitz_constant():
    v = torch.linspace(-30, 30, 600001, dtype=F64)
    sp = F.softplus(v, threshold=700.0)
    d = torch.tanh(sp) + v * torch.sigmoid(v) * (1 - torch.tanh(sp) ** 2)
    top = d.abs().max().item()
    assert 1.0883 < top <= V.MISH_LIPSCHITZ < 1.09, top
    # far from 0 mish is the identity (v > 20, the kernels' branch) or 0; mish64 has no overflow at either end
    far = V.mish64(torch.tensor([-800.0, -95.0, 25.0, 95.0, 800.0], dtype=F64))
    assert far[0] == 0 and -1e-38 < far[1] < 0 and far[2] == 25 and far[3] == 95 and far[4] == 800


# ------------------------------------------------------------------------------------------------ record codec
def _bits16(t):
    return [v & 0xFFFF for v in t.view(torch.int16).tolist()]


def _f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def test_codec_bit_patterns():
    # bf16: 1 + 2^-8 is a tie between 0x3F80 and 0x3F81 -> even (0x3F80), lo = 2^-8 = 0x3B80; 1 + 3 * 2^-8 ties to
    # 0x3F82, lo = -2^-8 = 0xBB80; -0 stays -0 with lo = +0 (x - hi = -0 - -0 = +0)
    x = _f32([0x3F808000, 0x3F818000, 0x80000000, 0x3F800001])
    hi, lo = V.encode(x, 3)
    assert _bits16(hi) == [0x3F80, 0x3F82, 0x8000, 0x3F80]
    assert _bits16(lo) == [0x3B80, 0xBB80, 0x0000, 0x3400]  # (2^-23 = 0x3400 in bf16)
    assert V.encode(x, 1)[1] is None and _bits16(V.encode(x, 1)[0]) == _bits16(hi)
    # fp16: 1 + 2^-11 ties to 0x3C00 (lo = 2^-11 = 0x1000); 1 + 3 * 2^-11 ties to 0x3C02 (lo = -2^-11 = 0x9000);
    # 1 + 2^-20: lo = 2^-20 is an fp16 subnormal (0x0010); 65504 is the largest finite; 65520 is the tie that rounds
    # to +inf (hi = 0x7C00, lo = 65520 - inf = -inf = 0xFC00); -0
    x = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -20, 65504.0, 65520.0, -0.0, 65519.996])
    hi, lo = V.encode(x, 48)
    assert _bits16(hi) == [0x3C00, 0x3C02, 0x3C00, 0x7BFF, 0x7C00, 0x8000, 0x7BFF]
    assert _bits16(lo) == [0x1000, 0x9000, 0x0010, 0x0000, 0xFC00, 0x0000, 0x4C00]  # (65504 + 16 - 2^-8: lo ties to 16)
    assert V.encode(x, 16)[1] is None


def test_codec_residuals_and_buffer_layout():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(20000, generator=g) * torch.exp(torch.rand(20000, generator=g) * 12 - 6)
    # p significant bits (bf16 8, fp16 11): hi is within 2^-p |x|; lo = RNE(x - hi) with |x - hi| < 2^(e-p) for x in
    # [2^e, 2^(e+1)), so its own rounding is within 2^(e-2p-1) <= 2^-(2p+1) |x|: 2^-17 |x| for split-bf16 (reached just
    # above a power of two, e.g. x = 1 + 2^-8 + 2^-16 + 2^-17: hi = 1 + 2^-7, lo = RNE(-2^-8 + 3 * 2^-17) = -2^-8, 0.996 * 2^-17 |x| off;
    # the 2^-18 |x| sometimes quoted is a typical figure, not a bound).  fp16 is held to the 2^-22 |x| of its users.
    for terms, u2 in ((3, 2.0 ** -17), (48, 2.0 ** -22)):
        hi, lo = V.encode(x, terms)
        keep = x.abs() > 2.0 ** -14 * 2.0 ** 11 if terms == 48 else torch.ones_like(x, dtype=torch.bool)  # lo normal
        assert ((x.double() - V.decode(hi, lo)).abs() <= u2 * x.double().abs())[keep].all()
        hi1 = V.encode(x, 1 if terms == 3 else 16)[0]
        assert ((x.double() - V.decode(hi1)).abs() <= (2.0 ** -8 if terms == 3 else 2.0 ** -11) * x.double().abs())[
            x.abs() > 2.0 ** -14].all()
    a, b = torch.randn(2, 5, 3, 4, generator=g), torch.randn(2, 6, 3, 4, generator=g)
    r = V.records(a, b, 1, 2, 2, 6, 9, 3)
    assert r.shape == (2, 2, 2, 6, 9, 8)
    full = torch.cat([a, b], 1)
    hi, lo = V.encode(full, 3)
    assert r[1, 0, 1, 1 + 2, 2 + 3, 2].item() == hi[1, 10, 2, 3].view(torch.int16).item()
    assert r[0, 1, 0, 1 + 0, 2 + 0, 7].item() == lo[0, 7, 0, 0].view(torch.int16).item()
    assert (r[:, :, :, 0] == 0).all() and (r[:, :, :, :, :2] == 0).all() and (r[:, :, 1, :, :, 3:] == 0).all()
    assert (r[:, :, :, 4:] == 0).all() and (r[:, :, :, :, 6:] == 0).all()


# ------------------------------------------------------------------------------------------------ c
def _sequential_fp32(case, ck=16):
    """The linear part one product at a time in fp32, separate multiply and add, in the k order conv.hip documents:
    chunk (``ck`` channels), tap, channel.  (Pessimistic against the kernels' fma / MFMA.)"""
    L, gm = case.geom.layer, case.geom
    x = case.x if case.x2 is None else torch.cat([case.x, case.x2], 1)
    if L.deconv:
        w = case.w.permute(2, 3, 1, 0).reshape(-1, L.cin, 1, 1)
        Ho, Wo = gm.Hin, gm.Win
    else:
        w, (Ho, Wo) = case.w, (gm.Hout, gm.Wout)
    pt, pl = gm.pad[:2]
    need_h, need_w = (Ho - 1) * L.sy + L.dy * (L.kh - 1) + 1, (Wo - 1) * L.sx + L.dx * (L.kw - 1) + 1
    xp = torch.zeros(x.shape[0], L.cin, max(need_h, pt + x.shape[2]), max(need_w, pl + x.shape[3]))
    xp[:, :, pt:pt + x.shape[2], pl:pl + x.shape[3]] = x
    acc = torch.zeros(x.shape[0], w.shape[0], Ho, Wo)
    for c0 in range(0, L.cin, ck):
        for ky in range(L.kh):
            for kx in range(L.kw):
                sl = xp[:, :, ky * L.dy:ky * L.dy + (Ho - 1) * L.sy + 1:L.sy, kx * L.dx:kx * L.dx + (Wo - 1) * L.sx + 1:L.sx]
                for c in range(c0, min(c0 + ck, L.cin)):
                    acc = acc + w[:, c, ky, kx].view(1, -1, 1, 1) * sl[:, c:c + 1]
    if L.deconv:
        cout = L.cout_eff // 4
        out = torch.zeros(x.shape[0], cout, 2 * Ho, 2 * Wo)
        for a in range(2):
            for b in range(2):
                out[:, :, a::2, b::2] = acc[:, (a * 2 + b) * cout:(a * 2 + b + 1) * cout]
        acc = out
    return acc


def _torch_fp32(case):
    L, gm = case.geom.layer, case.geom
    x = case.x if case.x2 is None else torch.cat([case.x, case.x2], 1)
    if L.deconv:
        return F.conv_transpose2d(x, case.w, None, stride=2)
    pt, pl, pb, pr = gm.pad
    out = F.conv2d(F.pad(x, (pl, pr + L.sx, pt, pb + L.sy)), case.w, None, (L.sy, L.sx), 0, (L.dy, L.dx))
    return out[:, :, :gm.Hout, :gm.Wout]


def test_measured_c():
    """MEASURED is what these inputs give, C is 4 x its worst (two digits, rounded up), and both fp32 evaluations stay
    within a quarter of every bound, on the linear part (the tightest magnitude: M without the epilogue's terms)."""
    worst = {"torch_fp32": 0.0, "sequential_fp32": 0.0}
    for (e, g, act, operands) in V.c_cases():
        for wide in (True, False):
            case = V.make_case(g, wide)
            L = g.layer
            lin, M = V.conv_lin(case.x if case.x2 is None else torch.cat([case.x, case.x2], 1), case.w, (L.sy, L.sx),
                                g.pad, (L.dy, L.dx), (g.Hout, g.Wout), bool(L.deconv))
            for name, fn in (("torch_fp32", _torch_fp32), ("sequential_fp32", _sequential_fp32)):
                r = ((fn(case).to(F64) - lin).abs() / (V.U * M).clamp(min=1e-300)).max().item()
                print(f"{V.layer_id(L)} wide={wide} {name}: {r:.3g}")
                worst[name] = max(worst[name], r)
                assert r <= V.C / 4, (V.layer_id(L), name, r)
    print("measured:", worst)
    # one-sided: torch's fp32 CPU convolution depends on the build, its blocking and the thread count, so another machine
    # may measure less; more than MEASURED (or than C / 4) means MEASURED and C are to be re-derived
    for k, v in worst.items():
        assert v <= 1.02 * V.MEASURED[k], (k, v, V.MEASURED[k])
        assert V.C >= 4 * v, (k, v, V.C)
    top = 4 * max(V.MEASURED.values())
    assert top <= V.C < top * 1.1 + 1, (top, V.C)


# ------------------------------------------------------------------------------------------------ operand bounds
EMULATED = {}  # mode -> worst err / (e_mode M) of the emulation


@functools.lru_cache(maxsize=None)
def _reference_cases():
    """One (Geom, wide) per distinct reference of the GPU sweep, by mode."""
    out = {}
    for v in _sweep().values():
        for (e, g, _, _) in v:
            modes = [V.MODE_OF_TERMS[e.terms]] + (["split16"] if e.terms == 3 and len(e.cfg) > 4 and e.cfg[4] == 2 else [])
            for m in modes:
                if m != "fp32" and len(e.cfg) > 4 and e.cfg[4] == 2:
                    out.setdefault((g.layer, m), g)  # one map per (layer, mode): the operand error does not depend on the tile
    return out


@pytest.mark.parametrize("mode", ["split", "bf16", "fp16", "split16"])
def test_emulated_record_formats_stay_inside_e_mode(mode):
    """Operands rounded by the codec, hi*hi (+ hi*lo + lo*hi) summed in fp64: the reference's own distance from what an
    exact-accumulation MFMA kernel of that format computes is at most e_mode * sum |w||x| on EVERY element of every
    layer the sweep runs in that mode (wide channel scales for split / bf16, 0.25 .. 4 for the fp16 formats)."""
    terms = {v: k for k, v in V.MODE_OF_TERMS.items()}[mode]
    worst, at, n = 0.0, None, 0
    for (L, m), g in _reference_cases().items():
        if m != mode:
            continue
        case = V.make_case(g, mode in V.WIDE_MODES)
        x = case.x if case.x2 is None else torch.cat([case.x, case.x2], 1)
        kw = dict(stride=(L.sy, L.sx), pad=g.pad, dil=(L.dy, L.dx), out_hw=(g.Hout, g.Wout), deconv=bool(L.deconv))
        lin, M = V.conv_lin(x, case.w, **kw)
        lim = V.E_MODE[mode] * M + (V.f16_floor(x, case.w, **kw) if mode in ("fp16", "split16") else 0.0)
        r = ((V.conv_lin_emulated(x, case.w, terms, **kw) - lin).abs() / lim.clamp(min=1e-300)).max().item()
        if r > worst:
            worst, at = r, V.layer_id(L)
        n += 1
    EMULATED[mode] = worst
    print(f"{mode}: worst emulation error {worst:.3g} of e_mode M at {at} over {n} layers")
    assert n >= 5 and worst <= 1.0, (mode, worst, at)


# ------------------------------------------------------------------------------------------------ power
def _power_case(want, act="none", operands=(), wide=True):
    e, g, _, _ = _layer(want)
    case = V.make_case(g, wide, act, operands)
    ref, M = V.case_ref(case)
    return case, ref, M


def _excess(name, got, ref, M, mode="fp32", floor=None):
    r = V.ratio(got, ref, M, mode, floor)
    r = r[torch.isfinite(r)].max().item() if torch.isfinite(r).any() else float("inf")
    print(f"power: {name}: worst err / bound {r:.3g} ({mode})")
    assert r >= 2.0, (name, r)
    return r


def _variant(case, **over):
    """conv_ref of ``case`` with some of its arguments replaced."""
    L, gm = case.geom.layer, case.geom
    a = dict(x=case.x, w=case.w, bias=case.bias, x2=case.x2, stride=(L.sy, L.sx), pad=gm.pad, dil=(L.dy, L.dx),
             out_hw=(gm.Hout, gm.Wout), act=case.act, res1=case.res1, res2=case.res2, post=case.post, deconv=bool(L.deconv))
    a.update(over)
    return V.conv_ref(**a)[0]


def test_power_geometry_variants():
    is33 = lambda L: (L.kh, L.sy, L.dy, L.cin, L.two) == (3, 1, 1, 128, 0) and L.cout_eff == 128
    case, ref, M = _power_case(is33, "lrelu", ("res1", "res2", "post"))
    w = case.w.clone()
    w[:, :, 0, 0], w[:, :, 0, 1] = case.w[:, :, 0, 1], case.w[:, :, 0, 0]
    _excess("a tap shifted by one", _variant(case, w=w), ref, M)
    # border clamp instead of zero padding: replicate-pad by hand, then convolve unpadded
    pt, pl, pb, pr = case.geom.pad
    xr = F.pad(case.x, (pl, pr, pt, pb), mode="replicate")
    _excess("border clamp instead of zero padding", _variant(case, x=xr, pad=(0, 0, 0, 0)), ref, M)
    x = case.x.clone()
    x[:, 16:32] = 0
    _excess("one 16-channel chunk dropped", _variant(case, x=x), ref, M)
    _excess("bias omitted", _variant(case, bias=None), ref, M)
    _excess("res2 omitted", _variant(case, res2=None), ref, M)
    pre_post = _variant(case, res1=case.res1 + case.post, post=None)
    _excess("post added before the activation", pre_post, ref, M)
    x = torch.cat([case.x[:1], case.x[:1]])
    _excess("batch item 1 convolving item 0", _variant(case, x=x), ref, M)
    # (no shipped layer has pad_t != pad_l -- the bottom / right padding is implied by out_hw --, so the same layer
    # with the padding (t, l) = (2, 1))
    ref21, M21 = V.conv_ref(case.x, case.w, pad=(2, 1, 0, 1), out_hw=(case.geom.Hout, case.geom.Wout))
    _excess("pad_t / pad_l exchanged", V.conv_ref(case.x, case.w, pad=(1, 2, 1, 0), out_hw=(case.geom.Hout, case.geom.Wout))[0],
            ref21, M21)
    # a dilated layer read at dilation 1 (with its padding)
    case, ref, M = _power_case(lambda L: L.dy == 4)
    _excess("dilation ignored", _variant(case, dil=(1, 1), pad=(1, 1, 1, 1)), ref, M)


def test_power_channel_variants():
    case, ref, M = _power_case(lambda L: L.cin % 8 != 0 and L.cin > 8 and not L.two and L.kh == 3)
    x = case.x.clone()
    x[:, case.x.shape[1] // 8 * 8:] = 0
    _excess("the last channel octet of a cin % 8 != 0 layer dropped", _variant(case, x=x), ref, M)
    case, ref, M = _power_case(lambda L: L.two and L.kh == 3)
    full = torch.cat([case.x, case.x2], 1)
    _excess("the second input's channels read from offset 0", _variant(case, x2=full[:, :case.C1].contiguous()), ref, M)
    case, ref, M = _power_case(lambda L: L.kh == 3 and L.sy == 1 and L.cout_eff <= 32 and not L.two, "relu_ch0", ("res1",))
    wrong = _variant(case, act="none")
    wrong[:, 1:2] = torch.relu(wrong[:, 1:2])
    _excess("relu_ch0 applied to channel 1", wrong, ref, M)
    case, ref, M = _power_case(lambda L: L.deconv)
    _excess("deconvolution quadrants a, b exchanged", _variant(case, w=case.w.transpose(2, 3).contiguous()), ref, M)


def test_power_record_variants():
    """A dropped lo*hi term and a zero lo plane are visible against the SPLIT bounds (they are the bf16-grade errors)."""
    e, g, _, _ = _layer(lambda L: (L.kh, L.sy, L.dy, L.cin, L.two) == (3, 1, 1, 128, 0) and L.cout_eff == 128)
    L = g.layer
    kw = dict(stride=(L.sy, L.sx), pad=g.pad, dil=(L.dy, L.dx), out_hw=(g.Hout, g.Wout))
    for mode, terms, wide in (("split", 3, True), ("split16", 48, False)):
        case = V.make_case(g, wide)
        lin, M = V.conv_lin(case.x, case.w, **kw)
        fl = V.f16_floor(case.x, case.w, **kw)
        _excess(f"the lo*hi term dropped ({mode})", V.conv_lin_emulated(case.x, case.w, terms, drop=("lohi",), **kw), lin, M, mode, fl)
        _excess(f"a zero lo plane ({mode})", V.conv_lin_emulated(case.x, case.w, terms, drop=("lohi", "hilo"), **kw), lin, M, mode, fl)


# ------------------------------------------------------------------------------------------------ gate epilogues
def _gate_chain(d, **wrong):
    """The three gate references chained in fp64 (each fed the previous one's VALUE) -> (h', M of the last stage)."""
    t12 = wrong.get("t12", V.gate1_ref(d["h"], d["wzr"], d["bzr"], dil2=wrong.get("dil2", 1))[0])
    r2 = V.gate2_ref(d["enc"], d["wm"], d["bm"], d["ctx"], t12, wrong.get("h_for_r", d["h"]))
    z = r2["z"][0]
    return V.gate3_ref(r2["rh"][0], d["wq"], d["bq"], 1 - z if wrong.get("swap_z") else z, r2["qin"][0], d["h"])


def test_gate_references_chain_to_the_oracle_conv_gru():
    """gate 1 -> 2 -> 3 as BasicUpdateBlock chains them equals oracle.motion.conv_gru in fp64 (inputs ctx + the merged
    1x1 convolution of enc), and the dual tap sets equal the sum of the two convolutions."""
    from oracle import motion as om
    d = {k: v.to(F64) for k, v in V.gate_inputs(9, 13).items()}
    G = V.GATE_G
    sd = {}
    for i, n in enumerate(("z", "r")):
        sd[f"g.conv{n}1.weight"], sd[f"g.conv{n}2.weight"] = d["wzr"][i * G:(i + 1) * G, :, :3], d["wzr"][i * G:(i + 1) * G, :, 3:]
        sd[f"g.conv{n}1.bias"], sd[f"g.conv{n}2.bias"] = d["bzr"][i * G:(i + 1) * G], torch.zeros(G, dtype=F64)
    sd["g.convq1.weight"], sd["g.convq2.weight"] = d["wq"][:, :, :3], d["wq"][:, :, 3:]
    sd["g.convq1.bias"], sd["g.convq2.bias"] = d["bq"], torch.zeros(G, dtype=F64)
    want = om.conv_gru(sd, "g", d["h"], d["ctx"], F.conv2d(d["enc"], d["wm"], d["bm"]))
    got, M = _gate_chain(d)
    assert (got - want).abs().max() <= 1e-12 and (M >= got.abs()).all()
    lin, _ = V.dual_lin(d["h"], d["wzr"], 4, 1)
    assert (lin - F.conv2d(d["h"], d["wzr"][:, :, :3], None, 1, 1, 1) - F.conv2d(d["h"], d["wzr"][:, :, 3:], None, 1, 4, 4)).abs().max() <= 1e-12


def test_power_gate_variants():
    d = V.gate_inputs(9, 13)
    ref, M = _gate_chain(d)
    _excess("dil2 rows read at dil", V.gate1_ref(d["h"], d["wzr"], d["bzr"], dil2=4)[0], *V.gate1_ref(d["h"], d["wzr"], d["bzr"]))
    qin_as_h = V.gate2_ref(d["enc"], d["wm"], d["bm"], d["ctx"], V.gate1_ref(d["h"], d["wzr"], d["bzr"])[0], d["h"])["qin"][0]
    _excess("gate 2's r multiplied by the q-input instead of h", _gate_chain(d, h_for_r=qin_as_h)[0], ref, M)
    _excess("gate 3 with z and 1 - z exchanged", _gate_chain(d, swap_z=True)[0], ref, M)


# ------------------------------------------------------------------------------------------------ rolling launches
def _roll_chain(d, mode, residual, dtype):
    x = d["x"].to(dtype)
    t = F.leaky_relu(F.conv2d(x, d["wa"].to(dtype), d["ba"].to(dtype), padding=d["wa"].shape[2] // 2), 0.2)
    if mode:
        t = F.conv2d(t, d["wb"].to(dtype), d["bb"].to(dtype), padding=1) + (x if residual else 0)
        t = torch.relu(t) if residual else F.leaky_relu(t, 0.2)
    return t


@pytest.mark.parametrize("mode,residual", [(0, False), (1, False), (1, True), (2, False)])
def test_rolling_reference_is_two_chained_convolutions(mode, residual):
    d = V.roll_case(mode, 16, 40 if mode == 2 else 16, 2, 9, 63, residual)
    got, M = V.roll_ref(d, mode, residual, "lrelu", "relu" if residual else "lrelu")
    assert (got - _roll_chain(d, mode, residual, F64)).abs().max() <= 1e-13 * M.max() and (M >= got.abs()).all()
    # the same chain in fp32 stays within a quarter of the bound
    assert V.ratio(_roll_chain(d, mode, residual, torch.float32), got, M, "fp32").max().item() <= 0.25


def test_power_rolling_seam():
    """A second stage that sees zero instead of the first stage's value in the row above a row-block seam."""
    d = V.roll_case(1, 16, 16, 2, 9, 63, False)
    ref, M = V.roll_ref(d, 1, False)
    a = V.conv_ref(d["x"], d["wa"], d["ba"], pad=(1, 1, 1, 1), act="lrelu")[0]
    a[:, :, 3] = 0  # the row above the seam at rh = 4
    wrong = V.epilogue(*V.conv_lin(a, d["wb"], pad=(1, 1, 1, 1)), d["bb"], "lrelu")[0]
    wrong[:, :, :4] = ref[:, :, :4]  # (only the block below the seam is affected)
    _excess("rolling: zero above a row-block seam", wrong, ref, M)


# ------------------------------------------------------------------------------------------------ dry runs
def test_record_chain_and_gate_configurations_are_accepted_at_their_small_maps():
    """codd_conv2d_check (no device: the pointers are placeholders) takes every |split configuration with the record
    input / output tensors the GPU module builds, and every gate configuration with its channel-quad operands."""
    from codd_amd import _abi, ops
    lib, PTR, rows = _abi.load(), 0x10000, ops._split_rows
    wide = lambda W: -(-W // 32) * 32
    for L, v in V.sweep(V.split_triples()).items():
        for (e, g, _, _) in v:
            p = _abi.ConvParams()
            p.terms, p.C0, p.B, p.Hout, p.Wout, p.Hin, p.Win, p.Cout = e.terms, L.cin, V.B, g.Hout, g.Wout, g.Hin, g.Win, L.cout_eff
            p.kh, p.kw, p.sy, p.sx, p.pad_t, p.pad_l, p.dil_y, p.dil_x = L.kh, L.kw, L.sy, L.sx, g.pad[0], g.pad[1], L.dy, L.dx
            p.out, p.out_ctot, p.wpacked = PTR, L.cout_eff, PTR
            bt, bl = g.pad[:2]
            p.xs, p.xs_c8, p.xs_hp, p.xs_wp, p.xs_bt, p.xs_bl = PTR, -(-L.cin // 32) * 4, 2 * bt + rows(g.Hin), 2 * bl + wide(g.Win), bt, bl
            p.xso, p.xso_c8, p.xso_hp, p.xso_wp = PTR, -(-(8 + L.cout_eff) // 32) * 4, 2 + rows(g.Hout), 2 + wide(g.Wout)
            p.xso_bt, p.xso_bl, p.xso_o8, p.xso_terms = 1, 1, 1, e.terms
            ops._set_cfg(p, e.cfg)
            assert lib.codd_conv2d_check(ctypes.byref(p)) == 0, (e.sig, e.cfg, g)
    G = V.GATE_G
    shapes = {1: (2 * G, G, 6, 3, 4, 4, 1, 2 * G), 2: (3 * G, 3 * G, 1, 1, 0, 1, 0, 2 * G), 3: (G, G, 6, 3, 4, 4, 1, G)}
    for e in V.gate_triples():
        cout, cin, kh, kw, pad, dil, dil2, octot = shapes[e.gate]
        assert (e.cout_eff, e.cin, e.kh, e.kw, e.pl, e.dy, e.dil2) == (cout, cin, kh, kw, pad, dil, dil2), e.sig
        for H, W in ((e.cfg[1] + 3, 16 * e.cfg[0] + 5), (19, 37)):  # its own smallest map and the chain's largest
            p = _abi.ConvParams()
            p.terms, p.C0, p.B, p.Hout, p.Wout, p.Hin, p.Win, p.Cout = e.terms, cin, V.B, H, W, H, W, cout
            p.kh, p.kw, p.sy, p.sx, p.pad_t, p.pad_l, p.dil_y, p.dil_x = kh, kw, 1, 1, pad, pad, dil, dil
            p.dil2, p.gate, p.layout, p.out, p.out_ctot, p.wpacked = dil2, e.gate, 2, PTR, octot, PTR
            p.xs, p.xs_c8, p.xs_hp, p.xs_wp, p.xs_bt, p.xs_bl = PTR, -(-cin // 32) * 4, 2 * pad + rows(H), 2 * pad + wide(W), pad, pad
            if e.gate == 2:
                p.res1, p.res2, p.post = _abi.View(PTR, 3 * G, 0), _abi.View(PTR, 2 * G, 0), _abi.View(PTR, G, 0)
            if e.gate == 3:
                p.res1, p.post = _abi.View(PTR, 2 * G, 0), _abi.View(PTR, G, 0)
            if e.gate > 1:
                p.xso, p.xso_c8, p.xso_hp, p.xso_wp = PTR, G // 8, 8 + rows(H), 8 + wide(W)
                p.xso_bt, p.xso_bl, p.xso_o8, p.xso_terms = 4, 4, 0, e.terms
            ops._set_cfg(p, e.cfg)
            assert lib.codd_conv2d_check(ctypes.byref(p)) == 0, (e.sig, e.cfg, H, W)
