"""The HIP kernels of csrc/stereo.hip (tile cost volume + arg-min, slanted-plane warp costs, plane up-sampling, hypothesis
selection) and csrc/fusion.hip (quarter- and full-resolution cues, the fused forget branch, the blend) against the fp64
references of tests/stereo_fusion_fp64.py at the product's shapes, B = 2, odd sizes and planted edge inputs.  Bound per
output element: |gpu - ref64| <= c 2^-24 M (stereo_fusion_fp64.C; its origin and power:
tests/test_stereo_fusion_fp64_reference.py); the arg-min under the near-tie rule of stereo_fusion_fp64.argmin_check;
selections and masks exact.  Also: every output element is written (outputs pre-filled with NaN; slice outputs sit in a
sentinel-filled wider buffer whose other channels must come back untouched bit for bit), a batch item does not depend on
its neighbour, two launches give the same bits, two hypothesis sets equal two single-set launches, a NaN / +inf input
gives non-finite outputs exactly where the fp64 reference has them, and every launch path the wrappers can take is in
the case list (test_every_launch_path_is_in_the_case_list)."""
import functools
import os

import pytest
import torch

import stereo_fusion_fp64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
ids = dict(ids=S.case_id)
SUMMARY = {}  # (kernel figure, case) -> worst err / bound
SENTINEL = -7.25


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _items(x, b):
    return x[b:b + 1].clone()  # (a fresh, aligned allocation)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _note(kernel, case, res):
    """Record worst err / bound per figure of ``res`` ({key of C: err / (2^-24 M)}) and assert the bound."""
    for k, v in res.items():
        SUMMARY[(f"{kernel} {k}", S.case_id(case))] = v / S.C[k.split(":")[0]]
    S.within(res, 1.0, (kernel, case))


def _host(B, ctot, h, w, coff, c):
    """A sentinel-filled [B,ctot,h,w] buffer whose channels [coff, coff + c) are NaN -> (buffer, Slice of those channels)."""
    from codd_amd.ops import Slice
    buf = torch.full((B, ctot, h, w), SENTINEL, device=DEV)
    buf[:, coff:coff + c] = float("nan")
    return buf, Slice(buf, coff, c)


def _untouched(buf, coff, c):
    """Every channel outside [coff, coff + c) still holds the sentinel's bits."""
    rest = torch.cat([buf[:, :coff], buf[:, coff + c:]], 1)
    return bool((rest == SENTINEL).all())


def _embed(t, ctot, coff):
    """t [B,c,h,w] as a Slice at channel ``coff`` of a sentinel-filled ``ctot``-channel buffer on the device."""
    from codd_amd.ops import Slice
    B, c, h, w = t.shape
    buf = torch.full((B, ctot, h, w), SENTINEL, device=DEV)
    buf[:, coff:coff + c] = t.to(DEV)
    return Slice(buf, coff, c)


# ------------------------------------------------------------------------------------------------ launch paths
def _warp_path(case):
    """The launch decision of codd_tile_warp_cost, recomputed: (staging, threads per workgroup)."""
    B, Cc, Ht, Wt, shift = case
    lds = Cc * 4 * Wt * 4
    if lds > 96 * 1024:
        return "unstaged by size", 64
    if shift:
        return "unstaged by alignment", 64
    return ("staged opt-in" if lds > 64 * 1024 else "staged"), (256 if Wt > 128 else 128 if Wt > 64 else 64)


def test_every_launch_path_is_in_the_case_list():
    """From the wrapper-visible launch decisions: the scalar (D % 4 != 0) and the vector cost-volume kernel; the warp
    kernel staged within 64 KB, staged with the opt-in above it, unstaged by size and unstaged by alignment, with 64-,
    128- and 256-thread workgroups; P = 3 and P = 5 of cues_lr (8 x 33 x 64 and 4 x 81 x 64 partial sums: 67 584 and 82 944 B
    of LDS, both above 64 KB -- the opt-in -- and within the 160 KB of a CDNA4 workgroup), cues_fr and forget."""
    assert {c[3] % 4 == 0 for c in S.COSTVOL_CASES} == {True, False}
    paths = [_warp_path(c) for c in S.WARP_CASES]
    assert {p[0] for p in paths} == {"staged", "staged opt-in", "unstaged by size", "unstaged by alignment"}
    assert {p[1] for p in paths if p[0].startswith("staged")} == {64, 128, 256}
    assert {c[3] for c in S.FUSION_CASES} == {3, 5} and {c[3] for c in S.CUES_LR_CASES} == {3, 5}
    lds = {P: (4 if P >= 5 else 8) * (3 * P * P + 6) * 64 * 4 for P in (3, 5)}
    assert lds == {3: 67584, 5: 82944} and all(64 * 1024 < v <= 160 * 1024 for v in lds.values())
    assert any(c[0] == 2 for c in S.WARP_CASES) and any(c[0] == 2 for c in S.COSTVOL_CASES) and any(c[0] == 2 for c in S.FUSION_CASES)


# ------------------------------------------------------------------------------------------------ cost volume
def _costvol(tl, tr, D):
    """ops.tile_costvol_argmin into slices at channel 1 of 3 (cost) and 2 of 20 (hypothesis) -> (cost [B,Ht,Wt], the
    three written hypothesis channels [B,3,Ht,Wt], NaN before), after checking that nothing else was written."""
    from codd_amd import ops
    B, _, Ht, Wt = tl.shape
    cbuf, cs = _host(B, 3, Ht, Wt, 1, 1)
    hbuf, hs = _host(B, 20, Ht, Wt, 2, 3)
    ops.tile_costvol_argmin(tl, tr, D, cs, hs)
    assert _untouched(cbuf, 1, 1) and _untouched(hbuf, 2, 3)
    return cbuf[:, 1].clone(), hbuf[:, 2:5].clone()


@pytest.mark.parametrize("case", S.COSTVOL_CASES, **ids)
def test_tile_costvol_argmin_against_fp64(case):
    """Min cost under c 2^-24 M against the reference cost AT THE KERNEL'S PICK; the pick = the reference's first
    arg-min except at near ties (at most 0.1 % of the tiles; never a later member of an exact tie: the zero-padded
    candidates); dx = dy = 0 written; outputs into slices of wider buffers."""
    _threads()
    B, Ht, Wt, D = case
    tl, tr = S.costvol_case(case)
    tld, trd = tl.to(DEV), tr.to(DEV)
    cost, hyp = _costvol(tld, trd, D)
    assert torch.isfinite(cost).all() and torch.isfinite(hyp).all() and (hyp[:, 1:] == 0).all()
    c2, h2 = _costvol(tld, trd, D)
    assert _bits(cost, c2) and _bits(hyp, h2)
    if B > 1:
        for b in range(B):
            c1, h1 = _costvol(_items(tld, b), _items(trd, b), D)
            assert _bits(c1, cost[b:b + 1]) and _bits(h1, hyp[b:b + 1]), (case, b)
    ref = S.costvol(tl, tr, D)
    chk = S.argmin_check(ref, cost.cpu(), hyp[:, 0].cpu(), S.C["costvol"])
    print(f"{S.case_id(case)} cost volume ({'vector' if D % 4 == 0 else 'scalar'} kernel): cost err / (2^-24 M) {chk['cost']:.3g}, "
          f"near-tie picks {chk['near']:.2e} of the tiles, picks without excuse {chk['wrong']} {chk['where'] or ''}")
    assert chk["wrong"] == 0 and chk["near"] <= S.NEAR_TIE_CAP, (case, chk)
    _note("tile_costvol_argmin", case, {"costvol": chk["cost"]})


# ------------------------------------------------------------------------------------------------ warp costs
def _shifted(t):
    """A contiguous copy of ``t`` on the device that starts 4 bytes into a larger (aligned) allocation."""
    base = torch.empty(t.numel() + 4, device=DEV)
    out = base[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _warp(fl, fr, h0, h1=None):
    """codd_tile_warp_cost with the outputs pre-filled with NaN -> (out0, out1 or None)."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    B, Cc, H, W = fl.shape
    out0 = _nan(B, 64, H // 4, W // 4)
    out1 = _nan(B, 64, H // 4, W // 4) if h1 is not None else None
    _abi.check(lib.codd_tile_warp_cost(fl.data_ptr(), fr.data_ptr(), B, Cc, H // 4, W // 4, ops._view(h0), ops._view(h1),
                                       2 if h1 is not None else 1, out0.data_ptr(),
                                       None if out1 is None else out1.data_ptr(), _stream()), "tile_warp_cost")
    return out0, out1


@functools.lru_cache(maxsize=2)
def _warp_refs(key):
    _threads()
    c = S.warp_case(key)
    return c, [S.tile_warp(c["fl"], c["fr"], c[h])[:2] for h in ("h0", "h1")]


@pytest.mark.parametrize("case", S.WARP_CASES, **ids)
def test_tile_warp_cost_against_fp64(case):
    """The 16 sum_c |fl| channels and the 48 warp costs of one and of two hypothesis sets, the hypotheses passed as
    slices at channels 48 and 32 of a 64-channel buffer; two sets == two single-set launches; the wrapper == the raw
    launch; batch items; repeat.  The case with a 4-byte-shifted fr takes the unstaged kernel: it meets the bound like
    its staged twin (the aligned launch of the same inputs), and their largest difference is printed."""
    from codd_amd import ops
    B, Cc, Ht, Wt, shift = case
    c, refs = _warp_refs(case[:4])
    fl = c["fl"].to(DEV)
    fr = _shifted(c["fr"]) if shift else c["fr"].to(DEV)
    assert fl.data_ptr() % 16 == 0 and (fr.data_ptr() % 16 == 0) == (not shift)
    h0, h1 = _embed(c["h0"], 64, 48), _embed(c["h1"], 64, 32)
    o0, o1 = _warp(fl, fr, h0, h1)
    assert torch.isfinite(o0).all() and torch.isfinite(o1).all()
    name = S.case_id(case) + " [%s, %d threads]" % _warp_path(case)
    for s, (o, ref) in enumerate(zip((o0, o1), refs)):
        _note(f"tile_warp_cost set {s}", case, S.warp_ratios(ref, o.cpu(), f"{name} set {s}"))
    a0, _ = _warp(fl, fr, h0)
    a1, _ = _warp(fl, fr, h1)
    assert _bits(a0, o0) and _bits(a1, o1), "two hypothesis sets differ from two single-set launches"
    w0, w1 = ops.tile_warp_cost(fl, fr, h0, h1)
    assert _bits(w0, o0) and _bits(w1, o1)
    p0, _ = _warp(fl, fr, c["h0"].to(DEV))  # (a plain 16-channel tensor instead of the slice)
    assert _bits(p0, o0)
    if B > 1:
        for b in range(B):
            i0, i1 = _warp(_items(fl, b), _items(fr, b) if not shift else _shifted(c["fr"][b:b + 1]),
                           _embed(c["h0"][b:b + 1], 64, 48), _embed(c["h1"][b:b + 1], 64, 32))
            assert _bits(i0, o0[b:b + 1]) and _bits(i1, o1[b:b + 1]), (case, b)
    if shift:
        s0, s1 = _warp(fl, c["fr"].to(DEV), h0, h1)
        for s, (o, ref) in enumerate(zip((s0, s1), refs)):
            S.within(S.warp_ratios(ref, o.cpu(), f"{name} staged twin set {s}"), 1.0, (case, "staged twin"))
        print(f"{name}: largest |staged - unstaged| {max((s0 - o0).abs().max().item(), (s1 - o1).abs().max().item()):.3g}")


# ------------------------------------------------------------------------------------------------ planes, selection
@pytest.mark.parametrize("case", S.HYP_CASES, **ids)
def test_hyp_upsample_and_select_against_fp64(case):
    """ops.hyp_upsample (scale 1 and 2) from / into slices at channel 32 of 64 (TileUpdate.forward) and at channels 5 of
    24 / 3 of 20; ops.hyp_select with its operands at channels 0 and 32 of one 64-channel buffer (as the product) and at
    48 / 16, into a plain tensor and into a slice; ties pick "previous"; channels 1 .. 15 of the planes are exact copies."""
    from codd_amd import ops
    B, h, w = case
    c = S.hyp_case(case)
    top = 0.0
    for scale in (1.0, 2.0):
        ref, Mg = S.hyp_upsample(c["prev"], scale)
        outs = []
        for (ictot, icoff, octot, ocoff) in ((16, 0, 64, 32), (24, 5, 20, 3), (64, 32, 16, 0)):
            src = _embed(c["prev"], ictot, icoff)
            buf, dst = _host(B, octot, 2 * h, 2 * w, ocoff, 16)
            ops.hyp_upsample(src, scale, dst)
            assert _untouched(buf, ocoff, 16)
            got = buf[:, ocoff:ocoff + 16]
            assert torch.isfinite(got).all()
            outs.append(got.clone())
            top = max(top, S.worst(f"{S.case_id(case)} hyp_upsample x{scale}", S.ratio(got.cpu(), ref, Mg, 1.0))[0])
        assert _bits(outs[0], outs[1]) and _bits(outs[0], outs[2])
        if B > 1:
            for b in range(B):
                buf, dst = _host(1, 16, 2 * h, 2 * w, 0, 16)
                ops.hyp_upsample(_embed(c["prev"][b:b + 1], 64, 32), scale, dst)
                assert _bits(buf, outs[0][b:b + 1])
    _note("hyp_upsample", case, {"hyp_upsample": top})
    ref, Mg, sel = S.hyp_select(c["upd"], c["cur"], c["prv"])
    upd = c["upd"].to(DEV)
    outs = []
    for (ccoff, pcoff, octot, ocoff) in ((0, 32, 16, 0), (48, 16, 20, 3)):
        from codd_amd.ops import Slice
        aug = torch.full((B, 64, h, w), SENTINEL, device=DEV)
        aug[:, ccoff:ccoff + 16], aug[:, pcoff:pcoff + 16] = c["cur"].to(DEV), c["prv"].to(DEV)
        buf, dst = _host(B, octot, h, w, ocoff, 16)
        ops.hyp_select(upd, Slice(aug, ccoff, 16), Slice(aug, pcoff, 16), dst)
        assert _untouched(buf, ocoff, 16)
        got = buf[:, ocoff:ocoff + 16]
        assert torch.isfinite(got).all()
        outs.append(got.clone())
    assert _bits(outs[0], outs[1])
    got = outs[0].cpu()
    # the selection compares inputs: exact.  Where "current" and "previous" give different values the pick is visible
    a, b = (c["cur"] + c["upd"][:, 18:34]), (c["prv"] + c["upd"][:, 2:18])
    a[:, 0], b[:, 0] = a[:, 0].clamp(min=0), b[:, 0].clamp(min=0)
    differ = a != b
    assert torch.equal(got[differ], torch.where(sel, a, b)[differ])
    _note("hyp_select", case, {"hyp_select": S.worst(f"{S.case_id(case)} hyp_select", S.ratio(got, ref, Mg, 1.0))[0]})
    if B > 1:
        for b_ in range(B):
            one = torch.full((1, 16, h, w), float("nan"), device=DEV)
            ops.hyp_select(_items(upd, b_), c["cur"][b_:b_ + 1].to(DEV), c["prv"][b_:b_ + 1].to(DEV), one)
            assert _bits(one, outs[0][b_:b_ + 1])


# ------------------------------------------------------------------------------------------------ fusion
def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


def _cues_lr(d, P, ds):
    """codd_fusion_cues_lr with corr_feat pre-filled with NaN and (pc, pw) written into channels 30, 31 of a 32-channel
    buffer (Fusion._memory_query's ``tail``) -> (corr_feat, dsub [B,2,h,w])."""
    from codd_amd import _abi
    lib = _abi.load()
    B, _, H, W = d["pc"].shape
    h, w = H // ds, W // ds
    corr = _nan(B, 3 * P * P + 4, h, w)
    buf, dst = _host(B, 32, h, w, 30, 2)
    _abi.check(lib.codd_fusion_cues_lr(d["pc"].data_ptr(), d["pw"].data_ptr(), d["fc"].data_ptr(), d["fw"].data_ptr(),
                                       d["fl"].data_ptr(), d["fr"].data_ptr(), B, H, W, P, ds, d["fc"].shape[1],
                                       d["fl"].shape[1], corr.data_ptr(), buf.data_ptr(), 32, 30, _stream()), "fusion_cues_lr")
    assert _untouched(buf, 30, 2)
    return corr, buf[:, 30:32].clone()


def _cues_fr(d, P):
    from codd_amd import _abi
    B, _, H, W = d["pc"].shape
    out = _nan(B, 3 * P * P + 5, H, W)
    _abi.check(_abi.load().codd_fusion_cues_fr(d["pc"].data_ptr(), d["pw"].data_ptr(), d["flow"].data_ptr(),
                                               d["conf"].data_ptr(), B, H, W, P, out.data_ptr(), _stream()), "fusion_cues_fr")
    return out


def _forget(d, P, weff):
    from codd_amd import _abi
    B, _, H, W = d["pc"].shape
    wr = _nan(B, 1, H, W)
    _abi.check(_abi.load().codd_fusion_forget(d["pc"].data_ptr(), d["pw"].data_ptr(), d["flow"].data_ptr(),
                                              d["conf"].data_ptr(), B, H, W, P, weff.data_ptr(), wr.data_ptr(), _stream()),
               "fusion_forget")
    return wr


def _blend(pc, pw, wf_lr, wr, ds):
    from codd_amd import _abi
    B, _, H, W = pc.shape
    fused, wf, wro = _nan(B, 1, H, W), _nan(B, 1, H, W), _nan(B, 1, H, W)
    _abi.check(_abi.load().codd_fusion_blend(pc.data_ptr(), pw.data_ptr(), wf_lr.data_ptr(), wr.data_ptr(), B, H, W, ds,
                                             fused.data_ptr(), wf.data_ptr(), wro.data_ptr(), _stream()), "fusion_blend")
    return fused, wf, wro


def _product_weff(sd, P):
    """The merged head as the product forms it: Fusion.forget_matrix() of a module carrying ``sd``'s forget_head."""
    from codd_amd import configs
    from codd_amd.registry import MODELS
    cfg = dict(configs.codd(iters=2)["fusion"])
    cfg["corr_cfg"] = dict(cfg.get("corr_cfg", {}), patch_size=P)
    fus = MODELS.build(cfg).eval()
    for i in range(3):
        fus.forget_head[i].weight.data = sd[f"fusion.forget_head.{i}.weight"].clone()
        fus.forget_head[i].bias.data = sd[f"fusion.forget_head.{i}.bias"].clone()
    weff = fus.forget_matrix()
    assert (weff.double() - S.merge_forget(sd)).abs().max() <= 2 * S.U * S.merge_forget(sd).abs().max()
    return weff.to(DEV).contiguous()


@functools.lru_cache(maxsize=1)
def _fusion_inputs(case):
    _threads()
    return S.fusion_case(case)


@pytest.mark.parametrize("case", S.CUES_LR_CASES, **ids)
def test_fusion_cues_lr_against_fp64(case):
    """The 3 P^2 - 2 correlations and the 6 stereo costs per element; the sub-sampled disparities exact; corr_feat
    pre-filled with NaN; the wrapper == the raw launch; batch items; repeat."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    B, H, W, P, ds, CF, CS = case
    c = _fusion_inputs(case)
    d = _dev(c)
    corr, dsub = _cues_lr(d, P, ds)
    assert torch.isfinite(corr).all() and torch.isfinite(dsub).all()
    ref = S.cues_lr(c, P, ds)
    assert torch.equal(dsub.cpu().double(), ref[2])
    _note("fusion_cues_lr", case, S.cues_lr_ratios(ref, corr.cpu(), P, S.case_id(case)))
    c2, d2 = _cues_lr(d, P, ds)
    assert _bits(corr, c2) and _bits(dsub, d2)
    tail = torch.full((B, 32, H // ds, W // ds), SENTINEL, device=DEV)
    assert _bits(ops.fusion_cues_lr(d["pc"], d["pw"], d["fc"], d["fw"], d["fl"], d["fr"], Slice(tail, 30, 2), patch=P, ds=ds), corr)
    assert _bits(tail[:, 30:], dsub)
    if B > 1:
        for b in range(B):
            c1, d1 = _cues_lr({k: _items(v, b) for k, v in d.items()}, P, ds)
            assert _bits(c1, corr[b:b + 1]) and _bits(d1, dsub[b:b + 1]), (case, b)


@pytest.mark.parametrize("case", S.FUSION_CASES, **ids)
def test_fusion_cues_fr_forget_and_blend_against_fp64(case):
    """ops.fusion_cues_fr (the first stage of the FUSE_FORGET = False chain) against its own reference; ops.fusion_forget
    against the INDEPENDENT fp64 reference -- the fp64 cue tensor through the three forget_head layers one by one, the
    product's own merged matrix (Fusion.forget_matrix) fed to the kernel -- with logits from the middle of the sigmoid
    to saturation; ops.fusion_blend with the fused disparity under its bound and both masked weights exact.  Outputs
    pre-filled with NaN; wrappers == raw launches; batch items; repeat."""
    from codd_amd import ops
    B, H, W, P, ds, CF, CS = case
    name = S.case_id(case)
    c = _fusion_inputs(case)
    d = _dev(c)
    cues, Mc = S.cues_fr(c, P)
    got = _cues_fr(d, P)
    assert torch.isfinite(got).all()
    _note("fusion_cues_fr", case, {"cues_fr": S.worst(f"{name} cues_fr", S.ratio(got.cpu(), cues, Mc, 1.0))[0]})
    assert torch.equal(got[:, 3 * P * P + 1].cpu(), (c["pw"][:, 0] > 0).float())  # the pw > 0 channel
    assert _bits(got, _cues_fr(d, P)) and _bits(got, ops.fusion_cues_fr(d["pc"], d["pw"], d["flow"], d["conf"], patch=P))
    sd = S.forget_weights(case, cues)
    f = S.forget(cues, sd)
    del cues, Mc
    weff = _product_weff(sd, P)
    wr = _forget(d, P, weff)
    assert torch.isfinite(wr).all() and (wr >= 0).all() and (wr <= 1).all()
    _note("fusion_forget", case, S.forget_ratio(f, wr.cpu(), name))
    assert _bits(wr, _forget(d, P, weff)) and _bits(wr, ops.fusion_forget(d["pc"], d["pw"], d["flow"], d["conf"], weff, patch=P))
    wf_lr, wr_in = S.blend_case(case)
    wfd, wrd = wf_lr.to(DEV), wr_in.to(DEV)
    fused, wf, wro = _blend(d["pc"], d["pw"], wfd, wrd, ds)
    b = S.blend(c["pc"], c["pw"], wf_lr, wr_in, ds)
    assert torch.isfinite(fused).all()
    assert torch.equal(wf.cpu().double(), b["wf"]) and torch.equal(wro.cpu().double(), b["wr"])  # masks and weights: exact
    _note("fusion_blend", case, {"blend": S.worst(f"{name} blend", S.ratio(fused.cpu(), b["fused"], b["M"], 1.0))[0]})
    again = _blend(d["pc"], d["pw"], wfd, wrd, ds)
    wrap = ops.fusion_blend(d["pc"], d["pw"], wfd, wrd, ds)
    assert all(_bits(x, y) and _bits(x, z) for x, y, z in zip((fused, wf, wro), again, wrap))
    if B > 1:
        for i in range(B):
            di = {k: _items(v, i) for k, v in d.items()}
            assert _bits(_cues_fr(di, P), got[i:i + 1]) and _bits(_forget(di, P, weff), wr[i:i + 1]), (case, i)
            one = _blend(di["pc"], di["pw"], _items(wfd, i), _items(wrd, i), ds)
            assert all(_bits(x, y[i:i + 1]) for x, y in zip(one, (fused, wf, wro))), (case, i)


# ------------------------------------------------------------------------------------------------ non-finite inputs
def _same_nonfinite(got, ref, what):
    g, r = ~torch.isfinite(got), ~torch.isfinite(ref)
    print(f"{what}: reference non-finite at {int(r.sum())} elements, kernel at {int((g & r).sum())} of them and {int((g & ~r).sum())} others")
    assert r.any() and torch.equal(g, r), what
    return ~r


def test_nonfinite_hypothesis_gives_nonfinite_costs_exactly_where_the_reference_has_them():
    """A NaN and a +inf planted in the disparity of two tiles' hypotheses (both sets): the 48 warp costs of exactly those
    tiles are non-finite, as in the fp64 reference; sum_c |fl| and every other tile stay within the bound."""
    case = S.WARP_CASES[5]
    B, Cc, Ht, Wt, _ = case
    c = dict(S.warp_case(case[:4]))
    for k in ("h0", "h1"):
        c[k] = c[k].clone()
        c[k][B - 1, 0, 2, 3] = float("nan")
        c[k][0, 0, Ht - 1, Wt - 2] = float("inf")
    o0, o1 = _warp(c["fl"].to(DEV), c["fr"].to(DEV), _embed(c["h0"], 64, 48), _embed(c["h1"], 64, 32))
    for s, (o, h) in enumerate(zip((o0, o1), (c["h0"], c["h1"]))):
        ref = S.tile_warp(c["fl"], c["fr"], h)
        keep = _same_nonfinite(o.cpu(), ref[0], f"tile_warp_cost set {s}")
        assert int((~keep).sum()) == 2 * 48
        S.within(S.warp_ratios(ref, o.cpu(), f"non-finite d, set {s}", keep), 1.0, "tile_warp_cost with non-finite d")


def test_nonfinite_pred_warp_gives_nonfinite_fusion_outputs_exactly_where_the_reference_has_them():
    """A NaN and a +inf planted in pred_warp at two pixels that the quarter-resolution cues read: cues_lr (fusion.hip's
    explicit NaN path: the three cost_warp channels of those pixels; the sub-sampled pw a copy), cues_fr and the blend
    are non-finite exactly where the fp64 reference is and within their bounds elsewhere.  The forget branch with the NaN
    alone: under +inf the layered fp64 reference forms inf - inf = NaN where the merged kernel may form one signed
    infinity, whose sigmoid is a finite 0 or 1 -- there the non-finite set is a property of the association order, not of
    the operation; for it only the elements the +inf cannot reach are held to the bound."""
    case = S.FUSION_CASES[3]
    B, H, W, P, ds, CF, CS = case
    c = {k: v.clone() for k, v in S.fusion_case(case).items()}
    (yn, xn), (yi, xi) = (ds * 9 + 1, ds * 20 + 1), (ds * 30 + 1, ds * 41 + 1)
    c["pw"][B - 1, 0, yn, xn] = float("nan")
    d_nan = _dev(c)
    cues_nan, Mc_nan = S.cues_fr(c, P)
    sd = S.forget_weights(case, S.cues_fr(S.fusion_case(case), P)[0])
    weff = _product_weff(sd, P)
    f = S.forget(cues_nan, sd)
    wr = _forget(d_nan, P, weff).cpu()
    keep = _same_nonfinite(wr, f["wr"], "fusion_forget, NaN in pred_warp")
    S.within(S.forget_ratio(f, wr, "forget with a NaN", keep), 1.0, "forget with a NaN")
    c["pw"][0, 0, yi, xi] = float("inf")
    d = _dev(c)
    corr, dsub = _cues_lr(d, P, ds)
    ref = S.cues_lr(c, P, ds)
    keep = _same_nonfinite(corr.cpu(), ref[0], "fusion_cues_lr")
    assert int((~keep).sum()) == 6 and torch.equal(torch.nan_to_num(dsub.cpu().double(), 1e30, 2e30), torch.nan_to_num(ref[2], 1e30, 2e30))
    S.within(S.cues_lr_ratios(ref, corr.cpu(), P, "cues_lr with non-finite pw", keep), 1.0, "cues_lr with non-finite pw")
    cues, Mc = S.cues_fr(c, P)
    got = _cues_fr(d, P).cpu()
    keep = _same_nonfinite(got, cues, "fusion_cues_fr")
    S.within({"cues_fr": S.worst("cues_fr with non-finite pw", S.ratio(got, cues, Mc, 1.0), keep)[0]}, 1.0, "cues_fr")
    f = S.forget(cues, sd)
    wr = _forget(d, P, weff).cpu()
    reach = torch.nn.functional.max_pool2d((~torch.isfinite(cues)).any(1, keepdim=True).double(), 3, 1, 1) > 0
    far = ~reach  # (every output whose 3 x 3 neighbourhood holds no cue that the two plants touch)
    assert torch.isfinite(wr[far]).all() and torch.isfinite(f["wr"][far]).all() and torch.isnan(wr[torch.isnan(S.forget(cues_nan, sd)["wr"])]).all()
    S.within(S.forget_ratio(f, wr, "forget with NaN and +inf", far), 1.0, "forget with NaN and +inf")
    wf_lr, wr_in = S.blend_case(case)
    fused, wf, wro = _blend(d["pc"], d["pw"], wf_lr.to(DEV), wr_in.to(DEV), ds)
    b = S.blend(c["pc"], c["pw"], wf_lr, wr_in, ds)
    keep = _same_nonfinite(fused.cpu(), b["fused"], "fusion_blend")
    assert int((~keep).sum()) == 2 and torch.equal(wf.cpu().double(), b["wf"]) and torch.equal(wro.cpu().double(), b["wr"])
    S.within({"blend": S.worst("blend with non-finite pw", S.ratio(fused.cpu(), b["fused"], b["M"], 1.0), keep)[0]}, 1.0, "blend")


def test_zz_print_worst_error_over_bound_per_kernel_and_case():
    """The figures of DESIGN finding 68: worst err / bound per kernel figure and case, collected by the tests above."""
    for (kernel, case), v in sorted(SUMMARY.items()):
        print(f"fp64 summary: {kernel:44s} {case:24s} worst err / bound {v:.3g}")
    assert SUMMARY and all(v <= 1.0 for v in SUMMARY.values())
