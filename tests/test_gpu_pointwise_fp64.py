"""The pointwise HIP kernels that the other fp64 modules leave out -- the stand-alone GRU gates and codd_context_split
(csrc/motion.hip), the resize / add / copy helpers (csrc/context.hip, ops.batch_pair), the three metric kernels and the
two ablation kernels (csrc/fusion.hip) -- against the fp64 references of tests/pointwise_fp64.py.  Bound per output
element: |gpu - ref64| <= c 2^-24 M (pointwise_fp64.C; its origin and power: tests/test_pointwise_fp64_reference.py);
copies, selections, masks and counts exact.  Also: every output element is written (outputs pre-filled with NaN; slice
outputs sit in a sentinel-filled wider buffer whose other channels must come back untouched bit for bit), a batch item
does not depend on its neighbour, two launches give the same bits, a NaN / inf input gives non-finite outputs exactly
where the fp64 reference has them, the nearest warp follows the documented rounding rule on tie-free, 1/64-px and
all-half-integer flows, a batch of B frames equals B calls, and every launch path the wrappers can take is in the case
list (test_every_launch_path_is_in_the_case_list)."""
import functools
import os

import pytest
import torch

import pointwise_fp64 as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
ids = dict(ids=P.case_id)
SUMMARY = {}  # (kernel figure, case) -> worst err / bound
SENTINEL = -7.25
NAN = float("nan")


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _items(x, b):
    return x[b:b + 1].clone()  # (a fresh, aligned allocation)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _note(kernel, case, res):
    """Record worst err / bound per figure of ``res`` ({key of C: err / (2^-24 M)}; "count" / "select": 0 or inf) and
    assert the bound."""
    exact = {k: res.pop(k) for k in ("count", "select") if k in res}
    assert all(v == 0.0 for v in exact.values()), (kernel, case, exact)
    for k, v in res.items():
        SUMMARY[(f"{kernel} {k}", P.case_id(case))] = v / P.C[k.split(":")[0]]
    P.within(res, 1.0, (kernel, case))


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _same_nonfinite(got, ref, what, strict=True):
    """got is non-finite exactly where the fp64 reference is; strict: NaN where it is NaN, inf where it is inf."""
    assert torch.equal(torch.isfinite(got.cpu()), torch.isfinite(ref)), what
    if strict:
        assert torch.equal(torch.isnan(got.cpu()), torch.isnan(ref)), what


# ------------------------------------------------------------------------------------------------ launch paths
NBLK, NTHR = 128, 256  # the metric kernels' grid


def test_every_launch_path_is_in_the_case_list():
    """From the wrapper-visible launch decisions: the metric kernels' stride loop runs once with idle blocks, once with a
    ragged tail and a second time with a ragged tail, at B = 1 and B = 2; the gates with cor / mot and without; the
    resize with ``extra`` and ``accumulate`` in all four combinations; copy_many's vector path, its word-copy fallback
    (size and alignment) and a second chunk; two x-blocks of fusion_select, gt_motion (full: 256 columns per block,
    features: 64) -- and b > 0 for each."""
    trips = {(-(-(h * w) // (NBLK * NTHR)), (h * w) % (NBLK * NTHR) != 0, B > 1) for (B, H, W, h, w) in P.METRIC_CASES}
    assert {(1, True, False), (2, True, True), (1, True, True)} <= trips
    assert any(h * w < NTHR for (_, _, _, h, w) in P.METRIC_CASES) and any((H, W) == (h, w) for (_, H, W, h, w) in P.METRIC_CASES)
    assert {"overwrite", "accumulate", "extra", "extra_accumulate", "relu"} == set(P.RESIZE_FORMS)
    assert {c[6] for c in P.RESIZE_CASES} == {0, 1} and any(c[0] > 1 for c in P.RESIZE_CASES)
    assert any(c[4] == 1 for c in P.RESIZE_CASES) and any(c[5] == 1 for c in P.RESIZE_CASES) and any(c[2] == 1 for c in P.RESIZE_CASES)
    paths = set()
    for n_pairs in COPY_COUNTS:
        pairs = _copy_pairs(n_pairs, device="cpu")
        fast = [s.numel() % 4 == 0 and s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0 for d, s in pairs if s.numel()]
        paths |= {"fast"} if any(fast) else set()
        paths |= {"fallback"} if not all(fast) else set()
        paths |= {"second chunk"} if sum(fast) > 8 else set()
        paths |= {"empty"} if any(s.numel() == 0 for _, s in pairs) else set()
    assert paths == {"fast", "fallback", "second chunk", "empty"}, paths
    assert any(W > 256 and B == 1 for (B, H, W, hg, wg) in P.SELECT_CASES) and any(B > 1 and (hg, wg) != (H, W) for (B, H, W, hg, wg) in P.SELECT_CASES)
    assert any(W > 256 and W // 4 > 64 for (B, Cc, H, W, hg, wg) in P.GT_MOTION_CASES)
    assert any(B > 1 and hg < H and (H // 4 - 1) * 4 + 2 >= hg for (B, Cc, H, W, hg, wg) in P.GT_MOTION_CASES)
    assert any((B * 128 * h * w) % 256 for (B, h, w) in P.GATE_CASES) and any((B * 16 * h * w) % 256 for (B, h, w) in P.GATE_CASES)


# ------------------------------------------------------------------------------------------------ GRU gates
def _gate_zr(lib, d, summed, B, hw):
    from codd_amd import _abi
    zr, rh = _nan(*d["t1"].shape), _nan(*d["h"].shape)
    cor, mot = (None, None) if summed else (d["cor"].data_ptr(), d["mot"].data_ptr())
    _abi.check(lib.codd_gru_gate_zr(d["t1"].data_ptr(), d["t2"].data_ptr(), d["inp"].data_ptr(), cor, mot, d["h"].data_ptr(),
                                    B, hw, zr.data_ptr(), rh.data_ptr(), _stream()), "gru_gate_zr")
    return zr, rh


def _gate_q(lib, d, zr, summed, B, hw):
    from codd_amd import _abi
    ho = _nan(*d["h"].shape)
    cor, mot = (None, None) if summed else (d["cor"].data_ptr(), d["mot"].data_ptr())
    _abi.check(lib.codd_gru_gate_q(d["q1"].data_ptr(), d["q2"].data_ptr(), d["inp"].data_ptr(), cor, mot, zr.data_ptr(),
                                   d["h"].data_ptr(), B, hw, ho.data_ptr(), _stream()), "gru_gate_q")
    return ho


def _device_records(st):
    """The whole record buffer of a SplitTensor as int16 [B][plane][octet][hp][wp][8] on the host."""
    planes = 2 if st.terms in (3, 48) else 1
    n = st.B * planes * st.c8 * st.hp * st.wp * 8
    return st.buf.view(torch.int16)[:n].view(st.B, planes, st.c8, st.hp, st.wp, 8).cpu()


@pytest.mark.parametrize("summed", [False, True], ids=["cor_mot", "summed"])
@pytest.mark.parametrize("case", P.GATE_CASES, **ids)
def test_gru_gates_against_fp64(case, summed):
    """codd_gru_gate_zr / codd_gru_gate_q (outputs pre-filled with NaN) within their bounds, with cor / mot and with
    both NULL, on pre-activations planted beyond +-20 and +-90; two launches and batch items bit for bit; the _xs forms
    (split_buffer with a border of 4; once a view at o8 > 0 of a wider record tensor) give the plain kernels' fp32 bits
    and exactly the records of those bits, zero border included."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    _threads()
    B, h, w = case
    d = P.gate_inputs(B, h, w)
    dd = _dev(d)
    zr, rh = _gate_zr(lib, dd, summed, B, h * w)
    ho = _gate_q(lib, dd, zr, summed, B, h * w)
    assert torch.isfinite(zr).all() and torch.isfinite(rh).all() and torch.isfinite(ho).all()
    ref = P.gate_zr(d, summed)
    res = {k: P.fig(f"{P.case_id(case)} {k}", g.cpu(), *ref[k]) for k, g in (("gate_z", zr), ("gate_rh", rh))}
    res["gate_q"] = P.fig(f"{P.case_id(case)} gate_q", ho.cpu(), *P.gate_q(d, zr.cpu(), summed))
    _note("gates " + ("summed" if summed else "cor_mot"), case, res)
    z2, r2 = _gate_zr(lib, dd, summed, B, h * w)
    assert _bits(zr, z2) and _bits(rh, r2) and _bits(ho, _gate_q(lib, dd, zr, summed, B, h * w))
    cm = (None, None) if summed else (dd["cor"], dd["mot"])
    wz, wr = ops.gru_gate_zr(dd["t1"], dd["t2"], dd["inp"], cm[0], cm[1], dd["h"])
    assert _bits(wz, zr) and _bits(wr, rh) and _bits(ops.gru_gate_q(dd["q1"], dd["q2"], dd["inp"], cm[0], cm[1], zr, dd["h"]), ho)
    if B > 1:
        for b in range(B):
            di = {k: _items(v, b) for k, v in dd.items()}
            zi, ri = _gate_zr(lib, di, summed, 1, h * w)
            assert _bits(zi, zr[b:b + 1]) and _bits(ri, rh[b:b + 1]) and _bits(_gate_q(lib, di, zi, summed, 1, h * w), ho[b:b + 1])
    # the record-writing forms
    rs = ops.split_buffer(("pw64", "rh", summed), B, 128, h, w, 4, DEV)
    hs = ops.split_buffer(("pw64", "h", summed), B, 128, h, w, 4, DEV)
    rs.buf.zero_(), hs.buf.zero_()
    z = ops.gru_gate_zr_xs(dd["t1"], dd["t2"], dd["inp"], cm[0], cm[1], dd["h"], rs)
    assert _bits(z, zr[:, :128])
    hx = ops.gru_gate_q_xs(dd["q1"], dd["q2"], dd["inp"], cm[0], cm[1], z, dd["h"], hs)
    assert _bits(hx, ho)
    for st, val in ((rs, rh), (hs, ho)):
        assert torch.equal(_device_records(st), P.records(val.cpu(), None, st.bt, st.bl, st.c8, st.hp, st.wp, st.terms))
    if case == P.GATE_CASES[1] and not summed:  # a view with o8 > 0: channels [128, 256) of a 256-channel record tensor
        wide = ops.split_buffer(("pw64", "wide"), B, 256, h, w, 4, DEV)
        wide.buf.zero_()
        view = _abi.XsView(wide.buf.data_ptr(), wide.c8, wide.hp, wide.wp, wide.bt, wide.bl, 16, wide.terms)
        zz = _nan(B, 128, h, w)
        _abi.check(lib.codd_gru_gate_zr_xs(dd["t1"].data_ptr(), dd["t2"].data_ptr(), dd["inp"].data_ptr(), dd["cor"].data_ptr(),
                                           dd["mot"].data_ptr(), dd["h"].data_ptr(), B, h, w, zz.data_ptr(), view, _stream()), "zr_xs")
        both = torch.cat([torch.zeros_like(rh), rh], 1).cpu()
        assert _bits(zz, zr[:, :128])
        assert torch.equal(_device_records(wide), P.records(both, None, wide.bt, wide.bl, wide.c8, wide.hp, wide.wp, wide.terms))


def test_gru_gates_non_finite():
    """A NaN, a +inf and a -inf planted in one input at a time: zr, r h and h' are non-finite exactly where the fp64
    reference is (an infinite pre-activation saturates the gate: finite)."""
    from codd_amd import _abi
    lib = _abi.load()
    B, h, w = P.GATE_CASES[1]
    d0 = P.gate_inputs(B, h, w)
    for key in ("t1", "t2", "inp", "cor", "mot", "h", "q1"):
        for val in (NAN, float("inf"), float("-inf")):
            d = {k: v.clone() for k, v in d0.items()}
            for c in (3, 130) if d[key].shape[1] > 130 else (3,):
                d[key][B - 1, c, h // 2, w // 2] = val
            if key == "inp":
                d[key][0, 300, 1, 1] = val
            dd = _dev(d)
            zr, rh = _gate_zr(lib, dd, False, B, h * w)
            ho = _gate_q(lib, dd, zr, False, B, h * w)
            ref = P.gate_zr(d)
            _same_nonfinite(zr, ref["gate_z"][0], (key, val, "zr"))
            _same_nonfinite(rh, ref["gate_rh"][0], (key, val, "rh"))
            _same_nonfinite(ho, P.gate_q(d, zr.cpu())[0], (key, val, "h'"))


# ------------------------------------------------------------------------------------------------ context helpers
def _resize_run(ops, xd, case, form, out0, extra):
    """One form of ops.resize_bilinear -> (result [B,C,Ho,Wo], sentinel buffer or None)."""
    from codd_amd.ops import Slice
    B, Cc, Hi, Wi, Ho, Wo, ac = case
    acc = form in ("accumulate", "extra_accumulate")
    if form in ("extra", "extra_accumulate"):
        out = out0.to(DEV).clone() if acc else _nan(B, Cc, Ho, Wo)
        return ops.resize_bilinear(xd, (Ho, Wo), ac, out=out, accumulate=acc, extra=extra.to(DEV)), None
    buf = torch.full((B, Cc + 3, Ho, Wo), SENTINEL, device=DEV)
    buf[:, 1:1 + Cc] = out0.to(DEV) if acc else NAN
    ops.resize_bilinear(xd, (Ho, Wo), ac, out=Slice(buf, 1, Cc), accumulate=acc, relu=form == "relu")
    return buf[:, 1:1 + Cc], buf


@pytest.mark.parametrize("case", P.RESIZE_CASES, **ids)
def test_resize_bilinear_against_fp64(case):
    """ops.resize_bilinear in its five forms (overwrite, accumulate on a pre-filled output, relu -- those into a Slice at
    channel 1 of a sentinel-filled wider buffer -- and ``extra`` with and without accumulate on a whole tensor) against
    the fp64 blend at the exact source coordinate; both align_corners modes, integer and non-integer ratios, down-scaling,
    Ho / Wo / Hi == 1."""
    from codd_amd import ops
    _threads()
    B, Cc, Hi, Wi, Ho, Wo, ac = case
    x, out0, extra = P.resize_inputs(case)
    xd = x.to(DEV)
    top = 0.0
    for form in P.RESIZE_FORMS:
        got, buf = _resize_run(ops, xd, case, form, out0, extra)
        assert torch.isfinite(got).all(), form
        if buf is not None:
            assert bool((buf[:, :1] == SENTINEL).all()) and bool((buf[:, 1 + Cc:] == SENTINEL).all()), form
        top = max(top, P.fig(f"{P.case_id(case)} resize {form}", got.cpu(), *P.resize(x, (Ho, Wo), ac, form, out0, extra)))
        assert _bits(got, _resize_run(ops, xd, case, form, out0, extra)[0]), form
        if B > 1:
            for b in range(B):
                gi = _resize_run(ops, _items(xd, b), (1,) + case[1:], form, out0[b:b + 1], extra[b:b + 1])[0]
                assert _bits(gi, got[b:b + 1]), (form, b)
    _note("resize", case, {"resize": top})


def test_resize_and_add_relu_keep_a_nan_through_the_relu():
    """torch.relu keeps a NaN (fmaxf(NaN, 0) is 0): a NaN / inf tap, accumulator or ``extra`` element gives a non-finite
    output exactly where the fp64 reference has one, in every form, ReLU included."""
    from codd_amd import ops
    case = P.RESIZE_CASES[5]
    B, Cc, Hi, Wi, Ho, Wo, ac = case
    x0, out0, extra0 = P.resize_inputs(case)
    for val in (NAN, float("inf"), float("-inf")):
        for which in ("x", "out0", "extra"):
            x, out_, extra = x0.clone(), out0.clone(), extra0.clone()
            dict(x=x, out0=out_, extra=extra)[which][0, 1, 2, 3] = val
            for form in P.RESIZE_FORMS + ("accumulate_relu",):
                if form == "accumulate_relu":
                    buf = out_.to(DEV).clone()
                    got = ops.resize_bilinear(x.to(DEV), (Ho, Wo), ac, out=buf, accumulate=True, relu=True)
                    ref = torch.relu(P.resize(x, (Ho, Wo), ac, "accumulate", out_, extra)[0])
                else:
                    got = _resize_run(ops, x.to(DEV), case, form, out_, extra)[0]
                    ref = P.resize(x, (Ho, Wo), ac, form, out_, extra)[0]
                # (an infinite tap met with a weight that is 0 at the exact coordinate only: NaN here, inf there)
                _same_nonfinite(got, ref, (val, which, form), strict=not (which == "x" and val == val))
    a, b = torch.randn(300), torch.randn(300)
    a[7], a[8], b[8], a[9], b[10] = NAN, float("inf"), float("-inf"), float("-inf"), NAN
    for relu in (False, True):
        _same_nonfinite(ops.add_relu(a.to(DEV), b.to(DEV), relu=relu), P.add_relu(a, b, relu)[0], ("add_relu", relu))
        _same_nonfinite(ops.add_relu(a.to(DEV), None, relu=relu), P.add_relu(a, None, relu)[0], ("add_relu b=None", relu))


@pytest.mark.parametrize("n", P.ADD_RELU_N)
def test_add_relu_against_fp64(n):
    """ops.add_relu at n = 1, 255, 257 and a product branch: with and without relu, b = None, and in place as hrnet.py
    calls it (out is b; out is a); the elements around the output untouched."""
    from codd_amd import ops
    g = P._gen(91, n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    top = 0.0
    for relu in (False, True):
        ref, Mg = P.add_relu(a, b, relu)
        buf = torch.full((n + 8,), SENTINEL, device=DEV)
        buf[4:4 + n] = NAN
        got = ops.add_relu(ad, bd, relu=relu, out=buf[4:4 + n])
        assert bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + n:] == SENTINEL).all())
        top = max(top, P.fig(f"add_relu n={n} relu={relu}", got.cpu(), ref, Mg))
        assert _bits(got, ops.add_relu(ad, bd, relu=relu))
        ia, ib = ad.clone(), bd.clone()
        assert _bits(ops.add_relu(ad, ib, relu=relu, out=ib), got) and _bits(ops.add_relu(ia, bd, relu=relu, out=ia), got)
        ref1, M1 = P.add_relu(a, None, relu)
        assert P.fig("add_relu b=None", ops.add_relu(ad, None, relu=relu, out=_nan(n)).cpu(), ref1, M1) == 0.0
    _note("add_relu", (n,), {"add_relu": top})


@pytest.mark.parametrize("case", P.SPLIT_CASES, **ids)
def test_context_split_against_fp64(case):
    """codd_context_split (outputs pre-filled with NaN): net = tanh within its bound (+-100 planted), inp = relu exact;
    batch items and two launches bit for bit; a NaN stays a NaN in both halves, +-inf gives +-1 / inf / 0."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    B, h, w = case
    x = P.split_input(B, h, w)

    def run(xd, Bn):
        net, inp = _nan(Bn, 128, h, w), _nan(Bn, 384, h, w)
        _abi.check(lib.codd_context_split(xd.data_ptr(), Bn, h * w, net.data_ptr(), inp.data_ptr(), _stream()), "context_split")
        return net, inp

    xd = x.to(DEV)
    net, inp = run(xd, B)
    (rn, Mn), (ri, Mi) = P.context_split(x)
    assert torch.isfinite(net).all() and torch.isfinite(inp).all()
    _note("context_split", case, {"ctx_tanh": P.fig("tanh", net.cpu(), rn, Mn), "select": P.fig("relu", inp.cpu(), ri, Mi)})
    wn, wi = ops.context_split(xd)
    assert _bits(wn, net) and _bits(wi, inp)
    for b in range(B):
        nb, ib = run(_items(xd, b), 1)
        assert _bits(nb, net[b:b + 1]) and _bits(ib, inp[b:b + 1])
    xn = x.clone()
    for c, val in ((5, NAN), (6, float("inf")), (7, float("-inf")), (200, NAN), (201, float("inf")), (202, float("-inf"))):
        xn[B - 1, c, h - 1, 0] = val
    net, inp = run(xn.to(DEV), B)
    (rn, _), (ri, _) = P.context_split(xn)
    _same_nonfinite(net, rn, "tanh half")
    _same_nonfinite(inp, ri, "relu half")


COPY_COUNTS = (1, 2, 8, 9, 12)


def _copy_pairs(n_pairs, device=DEV):
    """(dst, src) pairs for ops.copy_many: sizes 4 and 1028; with 8 and 12 pairs one of 0 elements in the middle; with 12
    one whose size is no multiple of 4 and one whose source is a 4-byte-shifted view (9 aligned pairs remain); every destination is a window [8, 8 + n) of
    its own sentinel-filled buffer; contents hold -0.0, NaNs with payloads, +-inf and denormals."""
    pairs = []
    for i in range(n_pairs):
        n = (4, 1028)[i % 2]
        if n_pairs == 12 and i == 3:
            n = 1027
        if n_pairs in (8, 12) and i == n_pairs // 2:
            n = 0
        src = P.special_words(n + 1, tag=51 + i).to(device)
        src = src[1:] if (n_pairs == 12 and i == 5) else src[:n]
        pairs.append((torch.full((n + 16,), SENTINEL, device=device)[8:8 + n], src[:n]))
    return pairs


@pytest.mark.parametrize("n_pairs", COPY_COUNTS)
def test_copy_many_is_a_copy_bit_for_bit(n_pairs):
    """ops.copy_many with 1, 2, 8, 9 and 12 pairs (9 aligned pairs: two launches): every destination equals its
    source as int32 bits -- -0.0, NaN payloads, +-inf and denormals included, on the vector path and on the word-copy
    fallback (a size that is no multiple of 4; a 4-byte-shifted source) -- and the words around it keep the sentinel."""
    from codd_amd import ops
    pairs = _copy_pairs(n_pairs)
    ops.copy_many(pairs)
    for i, (dst, src) in enumerate(pairs):
        assert torch.equal(dst.view(torch.int32), src.view(torch.int32)), (n_pairs, i, dst.numel())
        whole = dst._base if dst._base is not None else dst
        assert bool((whole[:8] == SENTINEL).all()) and bool((whole[8 + dst.numel():] == SENTINEL).all()), (n_pairs, i)


def test_batch_pair_equals_torch_cat_bit_for_bit():
    from codd_amd import ops
    for shape in ((1, 3, 5, 7), (2, 3, 8, 8), (1, 1, 1, 1)):
        n = 1
        for s in shape:
            n *= s
        a, b = P.special_words(n, tag=57).view(shape).to(DEV), P.special_words(n, tag=58).view(shape).to(DEV)
        assert _bits(ops.batch_pair(a, b), torch.cat([a, b], 0)), shape
        ah, bh = a.nan_to_num().clamp(-100, 100).half(), b.nan_to_num().clamp(-100, 100).half()
        assert torch.equal(ops.batch_pair(ah, bh), torch.cat([ah, bh], 0))


# ------------------------------------------------------------------------------------------------ metrics
@functools.lru_cache(None)
def _mcase(case, kind="float", empty_item=None):
    _threads()
    return P.metrics_case(case, kind, empty_item)


def _kinds(case):
    return ("float", "float", "float") if case[2] >= 1000 else P.FLOW_KINDS  # (KITTI size: one reference, added thrice)


def _disp(ops, dd, meters, frame=1):
    h, w = dd["case"][3:]
    return ops.disp_metrics(dd["pred%d" % frame], dd["gt%d" % frame], (h, w), P.LO, P.HI, P.THR, meters)


def _tepe(ops, dd, meters, use_mask=False, use_gt2=False):
    h, w = dd["case"][3:]
    gt1 = torch.zeros_like(dd["gt1"]) if use_mask else dd["gt1"]
    return ops.tepe_metrics(dd["pred1"], gt1, dd["pred0"], dd["gt0"], dd["flow"], (h, w), P.LO, P.HI, P.BF, meters,
                            gt_mask=P.dummy_mask(dd) if use_mask else None, gt2_prev=dd["gt2"] if use_gt2 else None)


def _sf(ops, dd, meters, use_occ=True):
    h, w = dd["case"][3:]
    return ops.sceneflow_metrics(dd["Ts"], dd["pred0"], dd["gt0"], dd["flow"], dd["dchange"], dd["occ"] if use_occ else None,
                                 (h, w), P.LO, P.HI, P.BF, dd["K"], meters)


def _accumulate(rows, Ms, start):
    """Meters after adding the items of ``rows`` (a list of [B,k]) in order to ``start`` -> (value, M)."""
    v, M = start.clone(), torch.zeros_like(start)
    for r, m in zip(rows, Ms):
        for b in range(r.shape[0]):
            v, M = v + r[b], M + m[b]
    return v, M


@pytest.mark.parametrize("case", P.METRIC_CASES, **ids)
def test_metric_kernels_against_fp64(case):
    """codd_disp_metrics, codd_tepe_metrics (with and without gt_mask = the KITTI dummy, with and without gt2_prev) and
    codd_sceneflow_metrics (with and without occ), accumulated over three successive calls -- tie-free, 1/64-px and
    all-half-integer flows: the warp's rounding rule -- into meters that start non-zero: means within their bounds,
    counts exact with no excluded pixel; a second run gives the same bits."""
    from codd_amd import ops
    _threads()
    kinds = _kinds(case)
    cases = {k: _mcase(case, k) for k in set(kinds)}
    devs = {k: _dev(d) for k, d in cases.items()}
    name = P.case_id(case)
    runs = [("disp", 3, lambda dd, m: _disp(ops, dd, m), lambda d: P.disp_metrics(d))]
    for um, ug in P.TEPE_VARIANTS:
        runs.append((f"tepe mask={um} gt2={ug}", 7, functools.partial(lambda dd, m, um, ug: _tepe(ops, dd, m, um, ug), um=um, ug=ug),
                     functools.partial(lambda d, um, ug: P.tepe_metrics(d, um, ug), um=um, ug=ug)))
    for uo in (False, True):
        runs.append((f"sceneflow occ={uo}", 5, functools.partial(lambda dd, m, uo: _sf(ops, dd, m, uo), uo=uo),
                     functools.partial(lambda d, uo: P.sceneflow_metrics(d, uo), uo=uo)))
    for what, k, launch, ref in runs:
        start = torch.arange(1, k + 1, dtype=F64) * 0.375
        got = []
        for _ in range(2):
            meters = start.to(DEV)
            for k_ in kinds:
                launch(devs[k_], meters)
            got.append(meters.cpu())
        assert torch.equal(got[0], got[1]), what
        refs = {k_: ref(d) for k_, d in cases.items()}
        want, Mw = _accumulate([refs[k_][0] for k_ in kinds], [refs[k_][1] for k_ in kinds], start)
        print(f"{name} {what}: meters {got[0].tolist()}")
        _note(what, case, P.meter_figures(what.split()[0], got[0], want, Mw, name))


@pytest.mark.parametrize("case", [c for c in P.METRIC_CASES if c[0] > 1], **ids)
def test_metric_batch_is_B_frames_in_index_order(case):
    """One call at B = 2 equals two calls at B = 1 on the items in turn: bit for bit for disp and tepe (one mean per
    item), to the fp64 rounding of the sums for scene flow; an item whose ground truth is all invalid moves neither the
    means nor the count (flow magnitude, a mean over the crop, counts every item)."""
    from codd_amd import ops
    for empty in (None, 0, 1):
        d = _mcase(case, "q64", empty)
        dd = _dev(d)
        items = [_dev(P.metrics_item(d, b)) for b in range(case[0])]
        for what, k, launch in (("disp", 3, _disp), ("tepe", 7, _tepe), ("sceneflow", 5, _sf)):
            start = torch.arange(1, k + 1, dtype=F64) * 0.375
            whole = launch(ops, dd, start.to(DEV)).cpu()
            parts = start.to(DEV)
            for it in items:
                launch(ops, it, parts)
            if what == "sceneflow":
                assert (whole - parts.cpu()).abs().max() <= 2.0 ** -46 * whole.abs().max(), (what, empty)
            else:
                assert torch.equal(whole, parts.cpu()), (what, empty, whole, parts)
            if empty is not None:
                alone = launch(ops, items[1 - empty], start.to(DEV)).cpu()
                keep = {"disp": [0, 1, 2], "tepe": [0, 1, 2, 3, 4], "sceneflow": [0, 1, 2, 3, 4]}[what]
                if what == "sceneflow":
                    assert (whole[keep] - alone[keep]).abs().max() <= 2.0 ** -46 * whole.abs().max(), (what, empty)
                else:
                    assert torch.equal(whole[keep], alone[keep]), (what, empty)
                r = {"disp": P.disp_metrics, "tepe": P.tepe_metrics, "sceneflow": P.sceneflow_metrics}[what](d)
                _note(f"{what} empty item {empty}", case, P.meter_figures(what, whole, *_accumulate([r[0]], [r[1]], start)))


def test_metric_kernels_non_finite():
    """A NaN prediction inside the mask makes the affected meters NaN, as the fp64 reference (and torch.clip in the
    restatement) has them -- the scene-flow depth clamp included; a NaN outside the crop or at an invalid ground-truth
    pixel changes no bit."""
    from codd_amd import ops
    case = P.METRIC_CASES[0]
    B, H, W, h, w = case
    d0 = _mcase(case)
    fns = (("disp", 3, _disp, P.disp_metrics), ("tepe", 7, _tepe, P.tepe_metrics), ("sceneflow", 5, _sf, P.sceneflow_metrics))
    clean = {what: launch(ops, _dev(d0), torch.zeros(k, dtype=F64, device=DEV)).cpu() for what, k, launch, _ in fns}
    s = P.sceneflow_elems(d0)["mask"][0] & P.tepe_elems(d0)["mask"][0, 0] & P.disp_elems(d0)[0][0, 0]
    cand = torch.nonzero(s & ~P._crop(d0["plant"], h, w)[0, 0])
    y, x = [int(v) for v in cand[len(cand) // 2]]
    for key in ("pred0", "pred1"):
        d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d0.items()}
        d[key][0, 0, y, x] = NAN
        hit = 0
        for what, k, launch, ref in fns:
            got = launch(ops, _dev(d), torch.zeros(k, dtype=F64, device=DEV)).cpu()
            want, Mw = ref(d)
            want, Mw = want.sum(0), Mw.sum(0)
            bad = torch.isnan(want)
            assert torch.equal(torch.isnan(got), bad), (key, what, got, want)
            hit += int(bad.sum())
            zero = torch.zeros((), dtype=F64)
            _note(f"{what} NaN {key}", case, P.meter_figures(what, torch.where(bad, zero, got), torch.where(bad, zero, want),
                                                              torch.where(bad, zero, Mw)))
        assert hit >= 1, key
    d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d0.items()}
    assert d["gt0"][0, 0, 6, 10] == 0 and d["gt1"][0, 0, 6, 10] == 0 and H > h
    for key in ("pred0", "pred1"):
        d[key][0, 0, 6, 10] = NAN
        d[key][0, 0, H - 1, W - 1] = NAN
        d[key][0, 0, 2, W - 1] = NAN
    for what, k, launch, _ in fns:
        assert torch.equal(launch(ops, _dev(d), torch.zeros(k, dtype=F64, device=DEV)).cpu(), clean[what]), what


def test_metric_kernels_reject_an_empty_crop():
    """h < 1 or w < 1 (and a crop larger than the map) is CODD_EINVAL for all three entry points; the meters stay."""
    from codd_amd import _abi, ops
    dd = _dev(_mcase(P.METRIC_CASES[0]))
    H, W = dd["case"][1:3]
    for what, k, launch in (("disp", 3, _disp), ("tepe", 7, _tepe), ("sceneflow", 5, _sf)):
        for crop in ((0, 5), (5, 0), (-1, 5), (H + 1, 5), (5, W + 1)):
            meters = torch.full((k,), 0.5, dtype=F64, device=DEV)
            bad = dict(dd, case=dd["case"][:3] + crop)
            with pytest.raises(_abi.CoddHipError):
                launch(ops, bad, meters)
            assert bool((meters == 0.5).all()), (what, crop)


# ------------------------------------------------------------------------------------------------ ablation kernels
@pytest.mark.parametrize("case", P.SELECT_CASES, **ids)
def test_fusion_select_against_fp64(case):
    """codd_fusion_select, both modes, K = 0.5 and 0.25 (output pre-filled with NaN): a passed-through estimate carries
    its source's bits (warp == 0, -0.0, < 0, |warp - cur| == 1, d == +-1, gt == 0 and a NaN gt planted), the Kalman
    blend and the GT average are within their bounds; batch items and two launches bit for bit."""
    from codd_amd import _abi
    lib = _abi.load()
    B, H, W, hg, wg = case

    def run(mode, cur, warp, gt, K, Bn):
        out = _nan(Bn, 1, H, W)
        _abi.check(lib.codd_fusion_select(mode, cur.data_ptr(), warp.data_ptr(), gt.data_ptr(), Bn, H, W, hg, wg, K,
                                          out.data_ptr(), _stream()), "fusion_select")
        return out

    for K in (0.5, 0.25):
        cur, warp, gt = P.select_inputs(case, K)
        cd, wd, gd = cur.to(DEV), warp.to(DEV), gt.to(DEV)
        for mode, name, key in ((0, "kalman", "kalman"), (1, "gt", "gt_avg")):
            got = run(mode, cd, wd, gd, K, B)
            ref, Mg, blended = P.fusion_select(name, cur, warp, gt, K)
            assert torch.isfinite(got).all() and 0.05 < blended.double().mean() < 0.98
            assert _bits(got.cpu()[~blended], ref[~blended].float()), (name, K)  # (a pass-through: its source's bits)
            _note(f"fusion_select {name} K={K}", case, {key: P.fig(f"{name} K={K}", got.cpu(), ref, Mg)})
            assert _bits(got, run(mode, cd, wd, gd, K, B))
            for b in range(B):
                assert _bits(run(mode, _items(cd, b), _items(wd, b), _items(gd, b), K, 1), got[b:b + 1])


@pytest.mark.parametrize("kind", P.FLOW_KINDS)
@pytest.mark.parametrize("case", P.GT_MOTION_CASES, **ids)
def test_gt_motion_is_exact(case, kind):
    """codd_gt_motion (all five outputs pre-filled with NaN) on tie-free, 1/64-px and all-half-integer flows, occlusion
    bytes 0 / 1 / 255, a flow smaller than the map: every output equals the reference under the documented rounding
    rule bit for bit (disp - dchange = the fp64 difference rounded to fp32; conf all ones; flow3 = the zero-padded
    inputs); batch items and two launches bit for bit."""
    from codd_amd import _abi
    lib = _abi.load()
    B, Cc, H, W, hg, wg = case
    a = P.gt_motion_inputs(case, kind)

    def run(t, Bn):
        img, feat, disp, fl, dch, occ = t
        outs = [_nan(Bn, 3, H, W), _nan(Bn, Cc, H // 4, W // 4), _nan(Bn, 3, H, W), _nan(Bn, 1, H, W), _nan(Bn, 3, H, W)]
        _abi.check(lib.codd_gt_motion(img.data_ptr(), disp.data_ptr(), feat.data_ptr(), Cc, fl.data_ptr(), dch.data_ptr(),
                                      occ.data_ptr(), Bn, H, W, hg, wg, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                      outs[3].data_ptr(), outs[4].data_ptr(), _stream()), "gt_motion")
        return outs

    ad = [t.to(DEV).contiguous() for t in a]
    got = run(ad, B)
    ref = P.gt_motion(*a)
    names = ("img_warp", "feat_warp", "conf", "disp_warp", "flow3")
    for n, g, r in zip(names, got, ref):
        assert torch.equal(g.cpu(), r), (n, int((g.cpu() != r).sum()))
    assert 0.02 < (ref[0] == 0).double().mean() < 0.9  # (occluded / out-of-view pixels are there, and so are the others)
    for g, g2 in zip(got, run(ad, B)):
        assert _bits(g, g2)
    for b in range(B):
        for g, gi in zip(got, run([_items(t, b) for t in ad], 1)):
            assert _bits(gi, g[b:b + 1])
    SUMMARY[(f"gt_motion {kind} (exact)", P.case_id(case))] = 0.0


def test_zz_summary():
    """Worst err / bound per kernel figure over the cases that ran (printed; every entry was asserted <= 1 above)."""
    by = {}
    for (what, case), v in SUMMARY.items():
        if v >= by.get(what, (-1.0, ""))[0]:
            by[what] = (v, case)
    for what in sorted(by):
        print(f"SUMMARY {what}: worst err / bound {by[what][0]:.3g} at {by[what][1]}")
    assert all(v <= 1.0 for v, _ in by.values())
