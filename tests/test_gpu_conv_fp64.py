"""The convolution kernels (conv.hip, conv_kernel.h, conv_quad_kernel.h, conv_bf16*.h/.hip) and the record converter
codd_split_bf16 against the fp64 reference of tests/conv_fp64.py.  Bound per output element:
|gpu - ref64| <= (e_mode + c 2^-24) M (+ the fp16 formats' floor); its origin and power: tests/test_conv_fp64_reference.py.

* every entry of the shipped tune db (its 548 distinct (layer, geometry, configuration) triples: 432 plain / co-resident,
  92 |split record chains through xs= / xs_out=, 24 gate epilogues through ops.conv_gate, chained g1 -> g2 -> g3 on one
  hidden state) runs on ITS STORED configuration -- forced through pc.tuned, asserted after the launch, no fallback warning --
  at the smallest map with two tiles in each direction and a ragged second one, B = 2, its real channels, kernel,
  stride, dilation and padding, inputs whose channel scales span 1e-3 .. 1e3 (0.25 .. 4 for the fp16 formats), the seven
  activations (saturated pre-activations planted) and the res1 / res2 / post combinations cycling over the layers; the
  b3 layout-2 configurations run once more as split16 (terms 48);
* codd_split_bf16 bit for bit against the torch codec over the whole buffer;
* ops.conv_roll (modes 0 / 1 / 2, C = 16 / 32) against the two-stage reference across strip and row-block seams;
* four shipped jobs of the multi-job class through ops.deferred_convs: one launch, bit-equal to the single launches;
* two launches give the same bits and a batch item does not depend on its neighbour, per kernel family: fp32 classic,
  quad, strided, split with ksplit 1 and 2, bf16, fp16, record output, multi, roll, and the gate chain with gate 3 on
  its ksplit-1 and ksplit-2 configurations (in place);
* a NaN / +inf input gives non-finite outputs exactly where the fp64 reference has them, per kernel family and
  activation, through the gate chain, one job of a multi launch and the rolling stages.
Outputs are Slices of a sentinel-filled wider buffer, pre-filled with NaN; the other channels must come back untouched."""
import contextlib
import functools
import os
import warnings

import pytest
import torch

import conv_fp64 as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SUMMARY = {}  # (family, layer) -> worst err / bound
LAUNCHES = [0]
SENTINEL = -7.25
SWEEP = V.sweep()
TERMS = {v: k for k, v in V.MODE_OF_TERMS.items()}


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _is_b(cfg):
    return len(cfg) > 4 and cfg[4] == 2


def _family(cfg, terms):
    """The kernel family a (configuration, terms of the launch) runs on, and the mode of its bound."""
    if _is_b(cfg):
        return "layout2 %s ks%d" % (V.MODE_OF_TERMS[terms], cfg[8] if len(cfg) > 8 else 1), V.MODE_OF_TERMS[terms]
    return ("fp32 quad" if len(cfg) > 4 and cfg[4] == 1 else "fp32 classic"), "fp32"


@functools.lru_cache(maxsize=6)
def _reference(geom, wide, act, operands):
    """(case, ref64, M, fp16 floor, PackedConv holder) of one reference, shared by the configurations and precisions
    that run at this map."""
    _threads()
    case = V.make_case(geom, wide, act, operands)
    ref, M = V.case_ref(case)
    return case, ref, M, V.case_f16_floor(case), {}


def _packed(case, holder):
    from codd_amd import ops
    if "pc" not in holder:
        holder["pc"] = ops.PackedConv(case.w.to(DEV), case.bias.to(DEV), deconv=bool(case.geom.layer.deconv))
    return holder["pc"]


def _record_buffer(Bn, C, H, W, bt, bl, terms, coff):
    """A zeroed SplitTensor as ops.split_buffer makes them (its own allocation: nothing persists between tests), with
    room for ``C`` channels from channel ``coff`` on."""
    from codd_amd import _abi, ops
    c8 = -(-(coff + C) // 32) * 4
    hp, wp = 2 * bt + ops._split_rows(H), 2 * bl + -(-W // 32) * 32
    buf = torch.zeros(_abi.load().codd_split_bf16_bytes(Bn, c8, hp, wp, terms), device=DEV, dtype=torch.uint8)
    return ops.SplitTensor(buf, Bn, coff + C, H, W, bt, bl, hp, wp, c8, terms)


def _decode_records(st, coff, C):
    """-> the image [B,C,H,W] (fp64) the records of ``st`` hold in channels [coff, coff + C); everything else in the
    buffer -- borders, channel padding, the channels below ``coff`` -- must still be zero."""
    planes = 2 if st.terms in (3, 48) else 1
    raw = st.buf.cpu().view(torch.int16).view(st.B, planes, st.c8, st.hp, st.wp, 8).clone()
    img = raw.view(V.rec_dtype(st.terms)).permute(0, 1, 2, 5, 3, 4).reshape(st.B, planes, 8 * st.c8, st.hp, st.wp)
    val = img.to(F64).sum(1)[:, coff:coff + C, st.bt:st.bt + st.H, st.bl:st.bl + st.W].contiguous()
    rest = raw.permute(0, 1, 2, 5, 3, 4).reshape(st.B, planes, 8 * st.c8, st.hp, st.wp).clone()
    rest[:, :, coff:coff + C, st.bt:st.bt + st.H, st.bl:st.bl + st.W] = 0
    assert not rest.any(), "record borders / channel padding written"
    return val


def _launch(case, holder, cfg, terms, co=False, items=None, x=None, force=None):
    """ops.conv2d of ``case`` on the stored configuration ``cfg`` under the precision of ``terms`` -> the output
    [B,cout,H,W] on the host.  The first input is a Slice at channel ``case.coff`` of a sentinel-filled buffer, the
    output a NaN-filled Slice at channel 3 of a sentinel-filled buffer whose other channels must stay untouched.
    ``items``: run only these batch items (fresh allocations); ``x``: replace the concatenated input.
    ``force``: the |split forms -- "xso": the output goes as records into channels [8, 8 + cout) of a zeroed record
    tensor (returned decoded); "xs": the input only exists as records (split_input with the layer's padding as border)."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    L, gm = case.geom.layer, case.geom
    sel = (lambda t: t) if items is None else (lambda t: None if t is None else t[items].clone())
    xin = torch.cat([case.x, case.x2], 1) if (x is None and case.x2 is not None) else (case.x if x is None else x)
    x0, x1 = sel(xin[:, :case.C0]), (sel(xin[:, case.C0:]) if case.C1 else None)
    Bn = x0.shape[0]
    xbuf = torch.full((Bn, case.C0 + case.coff + 2, gm.Hin, gm.Win), SENTINEL, device=DEV)
    xbuf[:, case.coff:case.coff + case.C0] = x0.to(DEV)
    pc = _packed(case, holder)
    up = 2 if L.deconv else 1
    obuf = torch.full((Bn, pc.cout + 5, gm.Hout * up, gm.Wout * up), SENTINEL, device=DEV)
    obuf[:, 3:3 + pc.cout] = float("nan")
    dev = lambda t: None if t is None else sel(t).to(DEV)
    key = (gm.Hout, gm.Wout, Bn, L.sy, L.sx, L.dy, L.dx, gm.pad[1], case.C1 > 0, terms) + (("split",) if force else ()) + (
        ("co",) if co and terms else ())
    prev = ops.set_conv_precision(V.MODE_OF_TERMS[terms])
    try:
        pc.tuned.clear()
        pc.tuned[key] = tuple(cfg)
        with warnings.catch_warnings(record=True) as caught, (ops.coresident() if co else contextlib.nullcontext()):
            warnings.simplefilter("always")
            xin0, more = Slice(xbuf, case.coff, case.C0), {}
            if force == "xso":
                rec = _record_buffer(Bn, pc.cout, gm.Hout, gm.Wout, 1, 1, terms, 8)
                more = dict(xs_out=rec, xs_out_coff=8)
            else:
                more = dict(out=Slice(obuf, 3, pc.cout))
            if force == "xs":
                assert x1 is None
                more["xs"], xin0 = ops.split_input(xin0, border=gm.pad[:2]), None
            ops.conv2d(xin0, pc, x2=None if x1 is None else x1.to(DEV), stride=(L.sy, L.sx),
                       pad_tl=gm.pad, dil=(L.dy, L.dx), act=case.act, res1=dev(case.res1), res2=dev(case.res2),
                       post=dev(case.post), out_hw=None if L.deconv else (gm.Hout, gm.Wout), **more)
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision(prev)
    LAUNCHES[0] += 1
    # the launch ran on the stored configuration: the key still holds it, nothing was added, no fallback warning fired
    assert dict(pc.tuned) == {key: tuple(cfg)}, (dict(pc.tuned), key, cfg)
    assert not caught, [str(w.message) for w in caught]
    if force == "xso":
        return _decode_records(rec, 8, pc.cout)
    host = obuf.cpu()
    assert bool((host[:, :3] == SENTINEL).all()) and bool((host[:, 3 + pc.cout:] == SENTINEL).all()), "sentinel channels"
    return host[:, 3:3 + pc.cout].contiguous()


def _floor(floor, mode, extra=None):
    """The additive part of a bound: the fp16 formats' floor (only theirs) + ``extra``."""
    fl = floor if mode in ("fp16", "split16") else None
    return fl if extra is None else (extra if fl is None else fl + extra)


def _check(got, ref, M, floor, mode, what, extra=None):
    r = V.ratio(got, ref, M, mode, _floor(floor, mode, extra))
    v, at = r.reshape(-1).max(0)
    loc = tuple(int(i) for i in torch.unravel_index(at, r.shape))
    assert v.item() <= 1.0, (what, "worst err / bound %.3g at %s: got %r ref %r M %r" % (
        v.item(), loc, got[loc].item(), ref[loc].item(), M[loc].item()))
    return v.item()


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. the db sweep
@pytest.mark.parametrize("L", list(SWEEP), ids=V.layer_id)
def test_every_shipped_configuration(L):
    for (e, geom, act, operands) in SWEEP[L]:
        runs = [(e.cfg, e.terms)]
        if e.terms == 3 and _is_b(e.cfg):  # the same tile / wave grid / k-split on split-fp16 operands
            runs.append((e.cfg[:7] + (48,) + e.cfg[8:], 48))
        for cfg, terms in runs:
            fam, mode = _family(cfg, terms)
            case, ref, M, floor, holder = _reference(geom, V.MODE_OF_TERMS[terms] in V.WIDE_MODES, act, operands)
            got = _launch(case, holder, cfg, terms, co=e.co)
            worst = _check(got, ref, M, floor, mode, (e.sig, cfg, terms, act, operands))
            k = (fam + (" co" if e.co else ""), V.layer_id(L))
            SUMMARY[k] = max(SUMMARY.get(k, 0.0), worst)


SPLIT_SWEEP = V.sweep(V.split_triples())


@pytest.mark.parametrize("L", list(SPLIT_SWEEP), ids=V.layer_id)
def test_every_shipped_record_chain_configuration(L):
    """The |split entries: (a) the output written as records (xs_out; a plain convolution without operands, as the
    library requires), decoded and held to the conv bound plus the record's own residual, borders and channel padding
    still zero; (b) for one-input layers also the input read from records made by split_input (xs), fp32 output with
    the layer's operands."""
    for (e, geom, act, operands) in SPLIT_SWEEP[L]:
        fam, mode = _family(e.cfg, e.terms)
        wide = mode in V.WIDE_MODES
        act_o = "relu" if act == "relu_ch0" else act
        case, ref, M, floor, holder = _reference(geom, wide, act_o, ())
        got = _launch(case, holder, e.cfg, e.terms, co=e.co, force="xso")
        worst = _check(got, ref, M, floor, mode, (e.sig, e.cfg, "xs_out", act_o), extra=V.record_floor(ref, e.terms))
        if not L.two:
            case, ref, M, floor, holder = _reference(geom, wide, act, operands)
            got = _launch(case, holder, e.cfg, e.terms, co=e.co, force="xs")
            worst = max(worst, _check(got, ref, M, floor, mode, (e.sig, e.cfg, "xs", act, operands)))
        k = (fam + " records" + (" co" if e.co else ""), V.layer_id(L))
        SUMMARY[k] = max(SUMMARY.get(k, 0.0), worst)


# ------------------------------------------------------------------------------------------------ 2. the converter
def _codec_values(g, f16, *shape):
    """fp32 values over the format's range with planted ties to even, -0, exact record values, values whose lo part is
    subnormal (fp16) and the largest finite fp16; no fp32 subnormals, nothing above 65504."""
    lo, hi = (-7.0, 2.0) if f16 else (-20.0, 20.0)
    x = torch.randn(*shape, generator=g) * 10.0 ** (torch.rand(*shape, generator=g) * (hi - lo) + lo)
    if f16:
        x = x.clamp(-60000.0, 60000.0)
    plant = ([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -20, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, 3 * 2.0 ** -25]
             if f16 else [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -23, 3.0e38, -1.0e-30])
    flat = x.view(-1)
    flat[:len(plant) + 2] = torch.tensor(plant + [-0.0, 0.0])
    flat[-len(plant):] = -torch.tensor(plant)
    return x


@pytest.mark.parametrize("terms", [3, 1, 16, 48])
@pytest.mark.parametrize("border,extra", [((0, 0), 0), ((1, 1), 0), ((4, 3), 5)], ids=["b00", "b11", "b43_wide"])
def test_split_bf16_bit_for_bit(terms, border, extra):
    """One input (a Slice at channel offset 6) and two inputs (C0 = 24, C1 = 18: octet 24..31 straddles both), B = 2,
    hp / wp as needed or ``extra`` larger, the buffer pre-filled with 0xFF bytes and passed as ``out=`` (the
    persistent-tensor path): every byte equals the torch codec's -- records, zero borders, zero channel padding."""
    from codd_amd import _abi, ops
    from codd_amd.ops import Slice
    lib = _abi.load()
    g = torch.Generator().manual_seed(1000 * terms + 10 * border[0] + extra)
    Bn, H, W, (bt, bl) = 2, 11, 21, border
    prev = ops.set_conv_precision(V.MODE_OF_TERMS[terms])
    try:
        for C0, C1 in ((24, 18), (13, 0)):
            x0 = _codec_values(g, terms in (16, 48), Bn, C0, H, W)
            x1 = _codec_values(g, terms in (16, 48), Bn, C1, H, W) if C1 else None
            buf0 = torch.full((Bn, C0 + 9, H, W), SENTINEL, device=DEV)
            buf0[:, 6:6 + C0] = x0.to(DEV)
            c8 = -(-(C0 + C1) // 8) + (1 if extra else 0)
            hp, wp = H + 2 * bt + extra, W + 2 * bl + extra
            nbytes = lib.codd_split_bf16_bytes(Bn, c8, hp, wp, terms)
            raw = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
            st = ops.SplitTensor(raw, Bn, C0 + C1, H, W, bt, bl, hp, wp, c8, terms)
            assert ops.split_input(Slice(buf0, 6, C0), None if x1 is None else x1.to(DEV), out=st) is st
            torch.cuda.synchronize()
            want = V.records(x0, x1, bt, bl, c8, hp, wp, terms)
            got = raw.cpu().view(torch.int16).view(want.shape)
            assert nbytes == want.numel() * 2
            bad = (got != want).nonzero()
            assert bad.numel() == 0, (terms, border, (C0, C1), "first mismatch [b, plane, octet, y, x, i]", bad[0].tolist(),
                                      hex(got[tuple(bad[0])].item() & 0xFFFF), hex(want[tuple(bad[0])].item() & 0xFFFF))
            if not extra:  # the allocating path with its default (larger) geometry agrees on the image
                st2 = ops.split_input(Slice(buf0, 6, C0), None if x1 is None else x1.to(DEV), border=border)
                want2 = V.records(x0, x1, st2.bt, st2.bl, st2.c8, st2.hp, st2.wp, terms)
                assert torch.equal(st2.buf.cpu().view(torch.int16).view(want2.shape), want2)
    finally:
        ops.set_conv_precision(prev)


# ------------------------------------------------------------------------------------------------ families
def _pick(want, small=True):
    """The sweep entry of a kernel family with the least work (3x3, stride 1 preferred by ``want``)."""
    cands = [(L.cout_eff * L.cin * L.kh * L.kw, i, item) for i, (L, v) in enumerate(SWEEP.items()) for item in v if want(item[0], L)]
    return min(cands)[2]


FAMILIES = {  # (the record-output family: "split ks1" launched with force="xso" where a test says so)
    "fp32 classic": lambda e, L: e.terms == 0 and not _is_b(e.cfg) and (len(e.cfg) < 5 or e.cfg[4] == 0) and L.kh == 3 and L.sy == 1 and L.cin >= 16 and L.cout_eff >= 8,
    "fp32 quad": lambda e, L: e.terms == 0 and len(e.cfg) > 4 and e.cfg[4] == 1 and L.kh == 3 and L.sy == 1 and L.cin >= 16 and L.cout_eff >= 8,
    "fp32 quad two inputs": lambda e, L: e.terms == 0 and len(e.cfg) > 4 and e.cfg[4] == 1 and L.two and L.kh == 3 and L.cout_eff >= 8,
    "fp32 strided": lambda e, L: e.terms == 0 and L.sy == 2 and L.kh == 3 and L.cout_eff >= 8,
    "split ks1": lambda e, L: e.terms == 3 and _is_b(e.cfg) and (len(e.cfg) < 9 or e.cfg[8] == 1) and L.kh == 3 and L.cout_eff >= 8,
    "split ks2": lambda e, L: e.terms == 3 and _is_b(e.cfg) and len(e.cfg) > 8 and e.cfg[8] == 2 and L.kh == 3,
    "bf16": lambda e, L: e.terms == 1 and _is_b(e.cfg) and L.kh == 3,
    "fp16": lambda e, L: e.terms == 16 and _is_b(e.cfg) and L.kh == 3,
}


def test_family_picks_exist():
    for name, want in FAMILIES.items():
        e, geom, _, _ = _pick(want)
        assert geom.Hout > 0, name


# ------------------------------------------------------------------------------------------------ 5. saturation
@pytest.mark.parametrize("family", ["fp32 classic", "fp32 quad", "split ks1", "split ks2", "bf16", "fp16"])
def test_saturated_activations(family):
    """sigmoid / tanh / mish with planted pre-activations beyond +-20 and +-90 (asserted), held to the same bound."""
    e, geom, _, _ = _pick(FAMILIES[family])
    fam, mode = _family(e.cfg, e.terms)
    for act in ("sigmoid", "tanh", "mish"):
        case, ref, M, floor, holder = _reference(geom, mode in V.WIDE_MODES, act, ("res1",))
        L = geom.layer
        pre = V.epilogue(*V.conv_lin(case.x if case.x2 is None else torch.cat([case.x, case.x2], 1), case.w, (L.sy, L.sx), geom.pad,
                                     (L.dy, L.dx), (geom.Hout, geom.Wout)), case.bias, "none", case.res1)[2]
        assert pre.max() > 90 and pre.min() < -90 and ((pre.abs() > 20) & (pre.abs() < 90)).any()
        got = _launch(case, holder, e.cfg, e.terms, co=e.co)
        k = (fam + " " + act, V.layer_id(L))
        SUMMARY[k] = max(SUMMARY.get(k, 0.0), _check(got, ref, M, floor, mode, (family, act, e.sig)))


# ------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("family", list(FAMILIES))
def test_same_bits_twice_and_items_are_independent(family):
    e, geom, _, _ = _pick(FAMILIES[family])
    _, mode = _family(e.cfg, e.terms)
    case, ref, M, floor, holder = _reference(geom, mode in V.WIDE_MODES, "lrelu", ("res1", "post"))
    a = _launch(case, holder, e.cfg, e.terms, co=e.co)
    b = _launch(case, holder, e.cfg, e.terms, co=e.co)
    assert _bits(a, b), family
    for item in range(V.B):
        one = _launch(case, holder, e.cfg, e.terms, co=e.co, items=slice(item, item + 1))
        assert _bits(one, a[item:item + 1]), (family, item)


# ------------------------------------------------------------------------------------------------ 7. non-finite
@pytest.mark.parametrize("family", list(FAMILIES))
def test_non_finite_inputs_reach_the_output_exactly_where_the_reference_has_them(family):
    """One NaN in one pixel and channel of item 0 and one +inf elsewhere: the output is non-finite exactly where the
    fp64 reference is (the tap footprint of that pixel in every output channel), through every activation, res1 and
    post, and nowhere else -- item 1 and the sentinel channels included; the finite rest stays inside the bound.  (The
    kind may differ: a split record turns inf into inf, NaN.)  ReLU computed as fmaxf(v, 0) turned the NaN into 0."""
    e, geom, _, _ = _pick(FAMILIES[family])
    _, mode = _family(e.cfg, e.terms)
    L = geom.layer
    for act in V.ACTS:
        operands = ("res1", "post") if act != "mish" else ()
        case, _, _, floor, holder = _reference(geom, mode in V.WIDE_MODES, act, operands)
        x = (case.x if case.x2 is None else torch.cat([case.x, case.x2], 1)).clone()
        x[0, L.cin // 2, geom.Hin // 2, geom.Win // 2] = float("nan")
        x[0, L.cin - 1, 1, geom.Win - 2] = float("inf")
        # a two-plane record of +inf is (inf, inf - inf = NaN): for the split formats the reference sees a NaN there
        # (after a ReLU the footprint of -inf is 0, that of NaN stays NaN)
        xr = torch.where(torch.isinf(x), torch.full_like(x, float("nan")), x) if mode in ("split", "split16") else x
        lin, Mlin = V.conv_lin(xr, case.w, (L.sy, L.sx), geom.pad, (L.dy, L.dx), (geom.Hout, geom.Wout))
        ref, M, _ = V.epilogue(lin, Mlin, case.bias, act, case.res1, case.res2, case.post)
        want = ~torch.isfinite(ref)
        assert want[0].any() and not want[1].any() and not want.all()
        got = _launch(case, holder, e.cfg, e.terms, co=e.co, x=x)
        bad = (~torch.isfinite(got)) != want
        assert not bad.any(), (family, act, "non-finite mask differs at", bad.nonzero()[:4].tolist(),
                               "got", got[bad][:4].tolist(), "ref", ref[bad][:4].tolist())
        keep = ~want
        r = V.ratio(torch.where(keep, got.to(F64), ref), ref, torch.where(keep, M, torch.ones_like(M)), mode,
                    _floor(floor, mode))
        assert r[keep].max().item() <= 1.0, (family, act, r[keep].max().item())


# ------------------------------------------------------------------------------------------------ gates
def _gate_cfgs(terms):
    """{gate: [stored configurations]} of the db's gate triples for these terms."""
    out = {1: [], 2: [], 3: []}
    for e in V.gate_triples():
        if e.terms == terms and e.cfg not in out[e.gate]:
            assert (e.kh, e.kw, e.pl, e.dy, e.dil2) == ((1, 1, 0, 1, 0) if e.gate == 2 else (6, 3, 4, 4, 1)), e.sig
            out[e.gate].append(e.cfg)
    return out


def _c4(t=None, shape=None):
    """A C4Tensor of its own: holding ``t`` [B,C,H,W], or NaN-filled of ``shape``."""
    from codd_amd import ops
    Bn, Cn, H, W = shape if t is None else t.shape
    c4 = ops.C4Tensor(torch.full((Bn * Cn * H * W,), float("nan"), device=DEV), Bn, Cn, H, W)
    return c4 if t is None else ops.to_c4(t.to(DEV), c4)


def _gate_launch(pc, xs, gate, cfg, terms, **kw):
    from codd_amd import ops
    pad, dil, dil2 = (0, 1, 0) if gate == 2 else (4, 4, 1)
    key = ("gate", gate, xs.H, xs.W, xs.B, pad, dil, dil2, terms)
    pc.tuned.clear()
    pc.tuned[key] = tuple(cfg)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ops.conv_gate(pc, xs, gate, pad=pad, dil=dil, dil2=dil2, **kw)
    torch.cuda.synchronize()
    LAUNCHES[0] += 1
    assert dict(pc.tuned) == {key: tuple(cfg)} and not caught, (dict(pc.tuned), key, cfg, [str(w.message) for w in caught])


class _Mod:
    """Stands in for an nn.Conv2d as codd_amd.motion.packed_dual reads it."""

    def __init__(self, w, b):
        self.weight, self.bias = w.contiguous().to(DEV), b.to(DEV)


def _dual_pc(w, b, blocks):
    """The product's PackedConv of dual tap sets (motion.packed_dual) from the reference's [cout, cin, 2k, k] weight:
    per block of GATE_G output channels conv*1 = rows [0, k) (small dilation, carries the bias), conv*2 = rows [k, 2k)."""
    from codd_amd.motion import packed_dual
    G, k = V.GATE_G, w.shape[3]
    pairs = tuple((_Mod(w[n * G:(n + 1) * G, :, :k], b[n * G:(n + 1) * G]), _Mod(w[n * G:(n + 1) * G, :, k:], torch.zeros(G)))
                  for n in range(blocks))
    return packed_dual(pairs), pairs  # (the pairs own packed_dual's cache: keep them alive)


def _gate_chain(d, cfgs, terms, items=None):
    """g1 -> g2 -> g3 on one hidden state through ops.conv_gate on the stored configurations ``cfgs`` (gate 3 in place:
    out = post = h4) -> what the device holds after each launch, on the host: t12, zq, rh (decoded records), h1 (the
    new hidden state, fp32) and h1_rec (its records); record borders / channel padding asserted zero, the operands of
    gate 2 asserted untouched.  ``items``: run these batch items only (fresh allocations)."""
    from codd_amd import ops
    G = V.GATE_G
    sel = (lambda v: v) if items is None else (lambda v: v[items].clone())
    h, ctx, enc = sel(d["h"]), sel(d["ctx"]), sel(d["enc"])
    Bn, _, H, W = h.shape
    c1, c2, c3 = cfgs
    pzr, keep1 = _dual_pc(d["wzr"], d["bzr"], 2)
    pq, keep3 = _dual_pc(d["wq"], d["bq"], 1)
    ns = ops.split_input(h.to(DEV), border=4)
    t12 = _c4(shape=(Bn, 2 * G, H, W))
    _gate_launch(pzr, ns, 1, c1, terms, out=t12)
    out = {"t12": t12.nchw().cpu()}
    es = ops.split_input(enc.to(DEV), border=0)
    h4, ctx4 = _c4(h), _c4(ctx)
    zq = _c4(shape=(Bn, 2 * G, H, W))
    rs = _record_buffer(Bn, G, H, W, 4, 4, terms, 0)
    _gate_launch(ops.PackedConv(d["wm"].to(DEV), d["bm"].to(DEV)), es, 2, c2, terms, out=zq, res1=ctx4, res2=t12, post=h4, xs_out=rs)
    out["zq"], out["rh"] = zq.nchw().cpu(), _decode_records(rs, 0, G)
    assert _bits(t12.nchw().cpu(), out["t12"]) and _bits(h4.nchw().cpu(), h)  # operands untouched
    hb = _record_buffer(Bn, G, H, W, 4, 4, terms, 0)
    _gate_launch(pq, rs, 3, c3, terms, out=h4, res1=zq, post=h4, xs_out=hb)
    out["h1"], out["h1_rec"] = h4.nchw().cpu(), _decode_records(hb, 0, G)
    return out


def _same(a, b):
    """Two chain results hold the same bits (NaN payloads included)."""
    return all(_bits(a[k], b[k]) for k in a)


def _gate_map(cfgs):
    return max(c[1] for c in cfgs) + 3, 16 * max(c[0] for c in cfgs) + 5


@pytest.mark.parametrize("terms", [3, 1, 16])
def test_every_shipped_gate_configuration_chained(terms):
    """The g1 / g2 / g3 entries through ops.conv_gate with motion.packed_dual on their stored configurations, chained on
    one hidden state as BasicUpdateBlock chains them (gate 3 in place: out = post), each launch against the fp64
    reference of ITS operands as the device holds them (conv_fp64, gate epilogues).  Record outputs: the conv bound + the
    record's own residual, borders and channel padding still zero.  The planted pre-activations of z, r and q reach beyond
    +-20 and +-90 (asserted on the reference)."""
    from codd_amd import ops
    _threads()
    mode, G = V.MODE_OF_TERMS[terms], V.GATE_G
    cfgs = _gate_cfgs(terms)
    assert all(cfgs[g] for g in (1, 2, 3))
    prev = ops.set_conv_precision(mode)
    try:
        for i in range(max(len(v) for v in cfgs.values())):
            c = tuple(cfgs[g][i % len(cfgs[g])] for g in (1, 2, 3))
            H, W = _gate_map(c)
            d = V.gate_inputs(H, W)
            kw = dict(stride=(1, 1), pad=(4, 4, 4, 4), dil=(4, 4))
            fl = lambda x, w: V.f16_floor(x, w[:, :, :3], pad=(1, 1, 1, 1)) + V.f16_floor(x, w[:, :, 3:], **kw)
            dev = _gate_chain(d, c, terms)
            ref, M = V.gate1_ref(d["h"], d["wzr"], d["bzr"])
            worst = {"g1": _check(dev["t12"], ref, M, fl(d["h"], d["wzr"]), mode, ("g1", c[0]))}
            r2 = V.gate2_ref(d["enc"], d["wm"], d["bm"], d["ctx"], dev["t12"], d["h"])
            f2 = V.f16_floor(d["enc"], d["wm"])
            worst["g2 z"] = _check(dev["zq"][:, :G], *r2["z"], 0.25 * f2[:, :G], mode, ("g2 z", c[1]))
            worst["g2 q-input"] = _check(dev["zq"][:, G:], *r2["qin"], f2[:, 2 * G:], mode, ("g2 qin", c[1]))
            worst["g2 r*h records"] = _check(dev["rh"], *r2["rh"], 0.25 * f2[:, G:2 * G] * d["h"].abs().to(F64), mode, ("g2 rh", c[1]),
                                            extra=V.record_floor(r2["rh"][0], terms))
            ref, M = V.gate3_ref(dev["rh"], d["wq"], d["bq"], dev["zq"][:, :G], dev["zq"][:, G:], d["h"])
            f3 = dev["zq"][:, :G].abs().to(F64) * fl(dev["rh"], d["wq"])
            worst["g3 h'"] = _check(dev["h1"], ref, M, f3, mode, ("g3", c[2]))
            worst["g3 h' records"] = _check(dev["h1_rec"], ref, M, f3, mode, ("g3 records", c[2]), extra=V.record_floor(ref, terms))
            # saturation is reached: the pre-activations of z and r (s + t12) and of q
            s = V.conv_lin(d["enc"], d["wm"])[0] + d["bm"].to(F64).view(1, -1, 1, 1) + d["ctx"].to(F64)
            pre_q = V.dual_lin(dev["rh"], d["wq"], 4, 1)[0] + d["bq"].to(F64).view(1, -1, 1, 1) + dev["zq"][:, G:].to(F64)
            for name, pre in (("z", s[:, :G] + dev["t12"][:, :G]), ("r", s[:, G:2 * G] + dev["t12"][:, G:]), ("q", pre_q)):
                assert pre.max() > 90 and pre.min() < -90 and ((pre.abs() > 20) & (pre.abs() < 90)).any(), name
            for k, v in worst.items():
                key = ("gate %s %s" % (mode, k), "%dx%d" % (H, W))
                SUMMARY[key] = max(SUMMARY.get(key, 0.0), v)
    finally:
        ops.set_conv_precision(prev)


def _ks(cfg):
    return cfg[8] if len(cfg) > 8 else 1


@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("ksplit", [1, 2])
def test_gate_chain_twice_and_items_are_independent(terms, ksplit):
    """Each gate on a stored configuration, gate 3 on its stored ksplit-1 / ksplit-2 one (gates 1 and 2 have ksplit-1 entries
    only: the first / the last of them): two chains give the same bits in every output (t12, z | q-input, r*h records, the
    in-place h' and its records), and item b of the B = 2 chain equals the B = 1 chain of that item in fresh allocations.
    The k-split exchange through LDS and the in-place update are where a race would show as a changed bit."""
    from codd_amd import ops
    cfgs = _gate_cfgs(terms)
    g3 = [c for c in cfgs[3] if _ks(c) == ksplit]
    assert g3 and all(_ks(c) == 1 for c in cfgs[1] + cfgs[2])
    c = (cfgs[1][0 if ksplit == 1 else -1], cfgs[2][0 if ksplit == 1 else -1], g3[0])
    d = V.gate_inputs(*_gate_map(c))
    prev = ops.set_conv_precision(V.MODE_OF_TERMS[terms])
    try:
        a, b = _gate_chain(d, c, terms), _gate_chain(d, c, terms)
        assert _same(a, b)
        for item in range(V.B):
            one = _gate_chain(d, c, terms, items=slice(item, item + 1))
            assert _same(one, {k: v[item:item + 1] for k, v in a.items()}), item
    finally:
        ops.set_conv_precision(prev)


@pytest.mark.parametrize("terms", [3, 1])
def test_gate_chain_non_finite(terms):
    """A NaN planted in one pixel and channel of h and a +inf in one of enc, item 0, through g1 -> g2 -> g3: every output
    is non-finite exactly where the fp64 reference of that launch (from the operands the device holds) is, item 1 and
    the records' borders stay clean.  (Two-plane records turn the +inf into inf, NaN: the reference then sees a NaN.)"""
    from codd_amd import ops
    G = V.GATE_G
    cfgs = _gate_cfgs(terms)
    c = (cfgs[1][0], cfgs[2][0], [k for k in cfgs[3] if _ks(k) == 2][0])
    H, W = _gate_map(c)
    d = V.gate_inputs(H, W)
    d["h"][0, 37, H // 2, W // 2] = float("nan")
    d["enc"][0, 200, 1, W - 2] = float("inf")
    enc_r = torch.where(torch.isinf(d["enc"]), torch.full_like(d["enc"], float("nan")), d["enc"]) if terms == 3 else d["enc"]
    prev = ops.set_conv_precision(V.MODE_OF_TERMS[terms])
    try:
        dev = _gate_chain(d, c, terms)
    finally:
        ops.set_conv_precision(prev)
    r2 = V.gate2_ref(enc_r, d["wm"], d["bm"], d["ctx"], dev["t12"], d["h"])
    want = {"t12": V.gate1_ref(d["h"], d["wzr"], d["bzr"])[0], "zq": torch.cat([r2["z"][0], r2["qin"][0]], 1), "rh": r2["rh"][0]}
    want["h1"] = V.gate3_ref(dev["rh"], d["wq"], d["bq"], dev["zq"][:, :G], dev["zq"][:, G:], d["h"])[0]
    want["h1_rec"] = want["h1"]
    for k, ref in want.items():
        nf = ~torch.isfinite(ref)
        assert nf[0].any() and not nf[1].any() and not nf.all(), k
        bad = (~torch.isfinite(dev[k])) != nf
        assert not bad.any(), (k, bad.nonzero()[:4].tolist(), dev[k][bad][:4].tolist(), ref[bad][:4].tolist())


# ------------------------------------------------------------------------------------------------ 3. multi-launch
def _multi_jobs():
    """Four shipped jobs of the multi-job class (quad layout, npb = 1, nw = 4, mb = 1) of different layers, the two with
    the longest k chains among them, on different maps: job i gets 2 i more rows and 4 i more columns than its tile's
    smallest map."""
    jobs, seen = [], set()
    for L, v in SWEEP.items():
        for (e, geom, act, operands) in v:
            c = e.cfg
            if (e.terms == 0 and len(c) == 5 and (c[0], c[1], c[3], c[4]) == (1, 4, 1, 1) and not L.two and L.sy == 1
                    and (geom.Hout, geom.Wout, L.cin) not in seen):
                seen.add((geom.Hout, geom.Wout, L.cin))
                jobs.append((e, geom, act, tuple(o for o in operands if o == "res1")))
                break
    jobs = sorted(jobs, key=lambda j: -j[1].layer.cin * j[1].layer.kh)[:2] + jobs[:2]
    assert len({id(j) for j in jobs}) == 4, len(jobs)
    grow = lambda gm, i: gm._replace(Hin=gm.Hin + 2 * i, Hout=gm.Hout + 2 * i, Win=gm.Win + 4 * i, Wout=gm.Wout + 4 * i)
    return [(e, grow(gm, i), act, operands) for i, (e, gm, act, operands) in enumerate(jobs)]


def _multi_run(jobs, monkeypatch, items=None, xs=None):
    """The jobs inside one ``ops.deferred_convs()`` block (precision fp32) -> their outputs on the host; asserts that
    they went out as ONE accepted codd_conv2d_multi launch of four jobs.  ``items``: these batch items only (fresh
    allocations); ``xs``: {job index: replacement input}."""
    from codd_amd import ops
    rcs, real = [], ops._launch_conv_multi
    monkeypatch.setattr(ops, "_launch_conv_multi", lambda lib, params, n, stream: rcs.append((n, real(lib, params, n, stream))) or rcs[-1][1])
    sel = (lambda v: v) if items is None else (lambda v: None if v is None else v[items].clone())
    keep = []
    try:
        with ops.deferred_convs():
            for n, (e, geom, act, operands) in enumerate(jobs):
                case, _, _, _, holder = _reference(geom, True, act, operands)
                L, pc = geom.layer, _packed(case, holder)
                x = sel(case.x if xs is None or n not in xs else xs[n])
                t = [x.to(DEV), None if case.res1 is None else sel(case.res1).to(DEV),
                     torch.full((x.shape[0], pc.cout, geom.Hout, geom.Wout), float("nan"), device=DEV)]
                pc.tuned.clear()
                pc.tuned[(geom.Hout, geom.Wout, x.shape[0], L.sy, L.sx, L.dy, L.dx, geom.pad[1], False, 0)] = tuple(e.cfg)
                ops.conv2d(t[0], pc, stride=(L.sy, L.sx), pad_tl=geom.pad, dil=(L.dy, L.dx), act=act, res1=t[1], out=t[2],
                           out_hw=(geom.Hout, geom.Wout))
                keep.append(t)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(ops, "_launch_conv_multi", real)
    assert rcs == [(4, 0)], rcs
    LAUNCHES[0] += 1
    return [t[2].cpu() for t in keep]


def test_deferred_multi_launch_equals_the_single_launches(monkeypatch):
    """Four shipped jobs of the multi-job class of different layers and maps inside ``ops.deferred_convs()``: ONE accepted
    codd_conv2d_multi launch (asserted), bit-equal to the single launches and inside the bound; a second multi launch
    gives the same bits; item b of it equals the B = 1 multi launch of that item."""
    from codd_amd import ops
    jobs = _multi_jobs()
    prev = ops.set_conv_precision("fp32")
    try:
        single = [_launch(_reference(geom, True, act, operands)[0], _reference(geom, True, act, operands)[4], e.cfg, 0)
                  for (e, geom, act, operands) in jobs]
        multi, again = _multi_run(jobs, monkeypatch), _multi_run(jobs, monkeypatch)
        ones = [_multi_run(jobs, monkeypatch, items=slice(b, b + 1)) for b in range(V.B)]
        for n, (e, geom, act, operands) in enumerate(jobs):
            _, ref, M, _, _ = _reference(geom, True, act, operands)
            assert _bits(multi[n], single[n]) and _bits(again[n], multi[n]), e.sig
            for b in range(V.B):
                assert _bits(ones[b][n], multi[n][b:b + 1]), (e.sig, b)
            SUMMARY[("fp32 quad multi", V.layer_id(V.layer_of(e)))] = _check(multi[n], ref, M, None, "fp32", ("multi", e.sig))
    finally:
        ops.set_conv_precision(prev)


def test_deferred_multi_launch_keeps_a_nan_in_its_job(monkeypatch):
    """A NaN and a +inf in item 0 of ONE job's input: that job's output is non-finite exactly where the fp64 reference
    is, item 1 clean; the three other jobs of the launch keep every bit."""
    from codd_amd import ops
    jobs = _multi_jobs()
    prev = ops.set_conv_precision("fp32")
    try:
        clean = _multi_run(jobs, monkeypatch)
        e, geom, act, operands = jobs[0]
        case = _reference(geom, True, act, operands)[0]
        L = geom.layer
        x = case.x.clone()
        x[0, L.cin // 2, geom.Hin // 2, geom.Win // 2] = float("nan")
        x[0, L.cin - 1, 1, geom.Win - 2] = float("inf")
        got = _multi_run(jobs, monkeypatch, xs={0: x})
        ref = V.conv_ref(x, case.w, case.bias, None, (L.sy, L.sx), geom.pad, (L.dy, L.dx), (geom.Hout, geom.Wout), act, case.res1)[0]
        want = ~torch.isfinite(ref)
        assert want[0].any() and not want[1].any() and torch.equal(~torch.isfinite(got[0]), want)
        assert all(_bits(got[n], clean[n]) for n in (1, 2, 3))
    finally:
        ops.set_conv_precision(prev)


# ------------------------------------------------------------------------------------------------ 4. rolling launches
ROLL_RH = 4


@pytest.mark.parametrize("mode,Cn", [(m, c) for m in (0, 1, 2) for c in (16, 32)], ids=lambda v: str(v))
def test_rolling_launches(mode, Cn):
    """ops.conv_roll against the two-stage reference at the smallest maps that cross a strip seam (the 60 / 62-column
    strip stride: W in 1, 61, 63, 125) and a row-block seam (H in 1, rh, rh + 1, 2 rh + 1), B = 2, residual on and
    off (mode 1), two sources (mode 2, and a Slice pair in the others), output into a Slice of a sentinel-filled
    buffer; two row-block heights give the same bits, and a batch item does not depend on its neighbour."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    _threads()
    rh = ROLL_RH
    sizes = [(H, W) for H in (1, rh, rh + 1, 2 * rh + 1) for W in (1, 61, 63, 125)]
    worst = 0.0
    for i, (H, W) in enumerate(sizes):
        residual = mode == 1 and i % 2 == 0
        cin = Cn if mode != 2 else (24, 40, 64, 16)[i % 4]
        c0 = cin if (mode != 2 and i % 3) else (cin - 8 if mode != 2 else cin // 2 + 4)
        act_b = "relu" if residual else "lrelu"
        d = V.roll_case(mode, Cn, cin, V.B, H, W, residual)
        ref, M = V.roll_ref(d, mode, residual, "lrelu", act_b)
        st = [dict(w=d["wa"].to(DEV), b=d["ba"].to(DEV), act="lrelu")]
        if mode:
            st.append(dict(w=d["wb"].to(DEV), b=d["bb"].to(DEV), act=act_b))
        pr = ops.PackedRoll(st, residual=residual)
        xd = torch.full((V.B, cin + 3, H, W), SENTINEL, device=DEV)
        xd[:, 2:2 + cin] = d["x"].to(DEV)
        outs = []
        for r in (rh, rh // 2 + 1):
            out = torch.full((V.B, Cn + 5, H, W), SENTINEL, device=DEV)
            out[:, 3:3 + Cn] = float("nan")
            ops.conv_roll(Slice(xd, 2, c0), pr, x2=Slice(xd, 2 + c0, cin - c0) if c0 < cin else None, out=Slice(out, 3, Cn), rh=r)
            torch.cuda.synchronize()
            LAUNCHES[0] += 1
            host = out.cpu()
            assert bool((host[:, :3] == SENTINEL).all()) and bool((host[:, 3 + Cn:] == SENTINEL).all())
            outs.append(host[:, 3:3 + Cn].contiguous())
        assert _bits(outs[0], outs[1]), (mode, Cn, H, W)
        for b in range(V.B):  # item b of the B = 2 launch equals the B = 1 launch of that item (fresh allocations)
            one = torch.full((1, Cn, H, W), float("nan"), device=DEV)
            x1 = d["x"][b:b + 1].to(DEV)
            ops.conv_roll(x1[:, :c0].contiguous(), pr, x2=x1[:, c0:].contiguous() if c0 < cin else None, out=one, rh=rh)
            assert _bits(one.cpu(), outs[0][b:b + 1]), (mode, Cn, H, W, b)
        worst = max(worst, _check(outs[0], ref, M, None, "fp32", ("roll", mode, Cn, cin, c0, H, W, residual)))
    SUMMARY[("roll mode %d" % mode, "C%d" % Cn)] = worst


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rolling_launches_keep_a_nan(mode):
    """One NaN and one +inf in item 0 through ops.conv_roll with a ReLU in every stage (roll_act; relu_ch0 in mode 0):
    non-finite exactly where the chained fp64 reference is, item 1 and the sentinel channels clean."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    Cn, cin, H, W = 16, (40 if mode == 2 else 16), 2 * ROLL_RH + 1, 63
    residual = mode == 1
    acts = ("relu_ch0", None) if mode == 0 else ("relu", "relu")
    d = V.roll_case(mode, Cn, cin, V.B, H, W, residual)
    d["x"][0, cin // 2, ROLL_RH, 60] = float("nan")  # beside the strip seam, on the row-block seam
    d["x"][0, cin - 1, 1, 3] = float("inf")
    ref, M = V.roll_ref(d, mode, residual, *acts)
    want = ~torch.isfinite(ref)
    assert want[0].any() and not want[1].any() and not want.all()
    st = [dict(w=d["wa"].to(DEV), b=d["ba"].to(DEV), act=acts[0])]
    if mode:
        st.append(dict(w=d["wb"].to(DEV), b=d["bb"].to(DEV), act=acts[1]))
    out = torch.full((V.B, Cn + 5, H, W), SENTINEL, device=DEV)
    out[:, 3:3 + Cn] = float("nan")
    ops.conv_roll(d["x"].to(DEV), ops.PackedRoll(st, residual=residual), out=Slice(out, 3, Cn), rh=ROLL_RH)
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool((host[:, :3] == SENTINEL).all()) and bool((host[:, 3 + Cn:] == SENTINEL).all())
    got = host[:, 3:3 + Cn]
    bad = (~torch.isfinite(got)) != want
    assert not bad.any(), (mode, bad.nonzero()[:4].tolist(), got[bad][:4].tolist(), ref[bad][:4].tolist())
    keep = ~want
    r = V.ratio(torch.where(keep, got.to(F64), ref), ref, torch.where(keep, M, torch.ones_like(M)), "fp32")
    assert r[keep].max().item() <= 1.0, (mode, r[keep].max().item())


def test_record_output_twice_and_with_a_nan():
    """The record-output family (xs_out): two launches give the same records, a batch item does not depend on its
    neighbour, and a NaN input gives NaN records exactly on the reference's footprint (ReLU epilogue)."""
    e, geom, _, _ = next(item for L, v in SPLIT_SWEEP.items() if L.kh == 3 and L.dy == 1 for item in v if item[0].terms == 3)
    case, ref, M, floor, holder = _reference(geom, True, "relu", ())
    a = _launch(case, holder, e.cfg, e.terms, co=e.co, force="xso")
    b = _launch(case, holder, e.cfg, e.terms, co=e.co, force="xso")
    assert torch.equal(a, b)
    for item in range(V.B):
        assert torch.equal(_launch(case, holder, e.cfg, e.terms, co=e.co, force="xso", items=slice(item, item + 1)), a[item:item + 1])
    L = geom.layer
    x = case.x.clone()
    x[0, L.cin // 2, geom.Hin // 2, geom.Win // 2] = float("nan")
    want = ~torch.isfinite(V.conv_ref(x, case.w, case.bias, pad=geom.pad, dil=(L.dy, L.dx), out_hw=(geom.Hout, geom.Wout), act="relu")[0])
    got = _launch(case, holder, e.cfg, e.terms, co=e.co, force="xso", x=x)
    assert want[0].any() and not want[1].any() and torch.equal(~torch.isfinite(got), want)


# ------------------------------------------------------------------------------------------------ summary
def test_zz_summary():
    """Printed under -s: worst err / bound per (kernel family, layer) of this run (the table of DESIGN.md finding 69)."""
    fam = {}
    for (f, layer), v in SUMMARY.items():
        if v > fam.get(f, (0.0, ""))[0] or f not in fam:
            fam[f] = (v, layer)
    print("\nlaunches on stored configurations: %d" % LAUNCHES[0])
    for f in sorted(fam):
        print("%-28s worst err / bound %.3f at %s" % (f, fam[f][0], fam[f][1]))
    assert all(v <= 1.0 for v in SUMMARY.values())
