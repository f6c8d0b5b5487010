"""The fp64 references of tests/stereo_fusion_fp64.py that tests/test_gpu_stereo_fusion_fp64.py holds the HIP kernels of
csrc/stereo.hip and csrc/fusion.hip against: pinned here to the CPU oracle fed fp64 and to the golden arrays of the
imported reference; the planted inputs are what they claim; the fp32 oracle measured against the references on the GPU
cases' own inputs (the measurement every constant ``c`` of stereo_fusion_fp64.C is 4 x of); the reference's own
near-tie shares of the arg-min; and the power of the bounds -- every wrong variant listed in test_power_of_the_bounds
must exceed the GPU bound by 2 x, the legitimate fp32-merged forget head must stay under it.  CPU only; run with -s for
the figures."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import stereo_fusion_fp64 as S
from oracle import fusion as ofu
from oracle import stereo as ost

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _upd(acc, res):
    for k, v in res.items():
        k = k.split(":")[0]
        acc[k] = max(acc.get(k, 0.0), v)


# ------------------------------------------------------------------------------ the oracle's forms (fp32, or fed fp64)
def o_warp(c, h, dt=torch.float32):
    fl, fr, p = c["fl"].to(dt), c["fr"].to(dt), h[:, :3].to(dt)
    return torch.cat([ost.unshuffle4(fl.abs().sum(1, keepdim=True)), ost.tile_warping(p, fl, fr)], 1)


def o_select(c, dt=torch.float32):
    upd, cur, prv = c["upd"].to(dt), c["cur"].to(dt), c["prv"].to(dt)
    sel = upd[:, :2].argmax(1, keepdim=True).to(dt)  # (oracle.stereo.tile_update: ties -> 0 = previous)
    return sel * ost._relu_d(cur + upd[:, 18:34]) + (1 - sel) * ost._relu_d(prv + upd[:, 2:18])


def o_cues(c, P, ds, dt=torch.float32):
    k = lambda n: c[n].to(dt)
    return ofu.input_cues(k("pc"), k("pw"), k("fc"), k("fw"), k("flow"), k("conf"), k("fl"), k("fr"), P=P, ds=ds)


def o_blend(pc, pw, wf_lr, wr, ds, dt=torch.float32):
    """The tail of oracle.fusion.memory_query / fuse."""
    pc, pw, wr = pc.to(dt), pw.to(dt), wr.to(dt)
    valid = (pw > 0.0).to(dt)
    wf = wf_lr.to(dt).repeat_interleave(ds, 2).repeat_interleave(ds, 3) * valid
    wr = wr * valid
    return pc * (1 - wf * wr) + pw * wf * wr, wf, wr


def _sd(sd, dt):
    return {k: v.to(dt) for k, v in sd.items()}


# ------------------------------------------------------------------------------ the references themselves
def test_references_equal_the_oracle_fed_fp64():
    """Every reference of stereo_fusion_fp64 (restated there to carry M and the wrong variants) equals the oracle's
    function fed fp64 to 1e-12 relative, on a small case of the GPU list each."""
    _threads()
    close = lambda a, b, tol=1e-12: (a - b).abs().max() <= tol * max(1.0, b.abs().max().item())
    for case in (S.COSTVOL_CASES[2], S.COSTVOL_CASES[6], S.COSTVOL_CASES[9]):
        tl, tr = S.costvol_case(case)
        ref = S.costvol(tl, tr, case[3])
        assert torch.equal(ref["cv"], ost.tile_cost_volume(tl.double(), tr.double(), case[3]))
        cost, d = ost.tile_cost_volume_min(tl.double(), tr.double(), case[3])
        assert torch.equal(ref["cost"], cost[:, 0]) and torch.equal(ref["arg"], d[:, 0].long())
        assert (ref["Mv"] >= ref["cv"]).all()
    for case in (S.WARP_CASES[5], S.WARP_CASES[2]):
        c = S.warp_case(case)
        keep = torch.ones(1, 1, case[2], case[3], dtype=torch.bool)
        keep[:, :, case[2] // 2, case[3] // 2] = False  # (the 1e6 plant: the oracle's x - d is not the kernel's 4 tx + ix - delta to 1e-12)
        for h in (c["h0"], c["h1"]):
            out, Mg, _ = S.tile_warp(c["fl"], c["fr"], h)
            want = o_warp(c, h, F64)
            assert close(out * keep, want * keep, 1e-11) and (Mg >= out - 1e-9).all()
            assert (out - want).abs().max() < 1e-6  # (at 1e6: to the fp64 rounding of the position)
    for case in S.HYP_CASES:
        c = S.hyp_case(case)
        for scale in (1.0, 2.0):
            assert torch.equal(S.hyp_upsample(c["prev"], scale)[0], ost.upsample_hyp(c["prev"].double(), scale, 2))
        assert torch.equal(S.hyp_select(c["upd"], c["cur"], c["prv"])[0], o_select(c, F64))
    for case in (S.FUSION_CASES[3], S.FUSION_CASES[4], S.FUSION_CASES[6], S.FUSION_CASES[7], S.CUES_LR_CASES[-1]):
        B, H, W, P, ds, CF, CS = case
        c = S.fusion_case(case)
        lr, fr = o_cues(c, P, ds, F64)
        got, Mg, dsub, xs = S.cues_lr(c, P, ds)
        py, px = H // ds - 1, W // ds - 1  # (the 1e6 plant, as above)
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[:, 3 * P * P - 2:, py, px] = False
        assert close(got * keep, lr * keep, 1e-11), case
        assert (Mg + 1e-9 >= got.abs()).all()
        so = ds // 2 - 1
        assert torch.equal(dsub, torch.cat([c["pc"], c["pw"]], 1)[..., so::ds, so::ds].double())
        gfr, Mfr = S.cues_fr(c, P)
        assert torch.equal(gfr, fr), case
        sd = S.forget_weights(case, gfr)
        f = S.forget(gfr, sd)
        assert close(f["wr"], ofu.forget_head(_sd(sd, F64), "fusion", fr), 1e-13)
        # the merged form (what the kernel evaluates) is the same function
        vm = S.forget_merged(gfr, S.merge_forget(sd))
        assert ((vm - f["v"]).abs() <= 1e-12 * f["Mv"]).all(), case
        wf_lr, wr = S.blend_case(case)
        b = S.blend(c["pc"], c["pw"], wf_lr, wr, ds)
        want = o_blend(c["pc"], c["pw"], wf_lr, wr, ds, F64)
        assert torch.equal(b["fused"], want[0]) and torch.equal(b["wf"], want[1]) and torch.equal(b["wr"], want[2])


def test_references_against_the_golden_arrays_of_the_imported_reference():
    """Where tests/golden/reference_outputs.npz has the quantity from the imported reference: disp_warp (the bilinear row
    sampler of warp_rows, to fp32 rounding); fusion_reset_weights / fusion_p5_reset_weights (cues_fr + forget, P = 3 and
    5, on the golden inputs directly: nothing but the kernels' own arithmetic lies in between) and fusion_pred_disp /
    fusion_p5_pred_disp (blend, from the golden weights).  Left out, because they cannot be made tight:
    stereo_*_init_d{i} (the arg-min sits behind the backbone and tile convolutions, whose fp32 rounding differs between the
    reference's and the oracle's convolutions and flips near ties) and fusion_weights (behind the whole weight-head
    chain); the cost volume and the quarter-resolution cues are pinned to the oracle above, and the oracle to these arrays
    by tests/test_oracle_golden.py."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import cases
    G = np.load(os.path.join(HERE, "golden", "reference_outputs.npz"))
    gold = lambda k: torch.from_numpy(G[k]).to(F64)
    img, disp = cases.warp_inputs()
    B, Cc, h, w = img.shape
    K = 1024.0  # |K - v| with K above every |v|: the sampled value itself from the cost form
    x = torch.arange(w, dtype=F64)[None, None, :].expand(B, h, w)
    xs = x - disp[:, 0].double()
    # (the imported sampler normalises the position to [-1, 1] and back: X = 2 (|x| + |disp| + w) for its roundings)
    rows = [S.warp_rows(torch.full((B, 1, h, w), K), img[:, c:c + 1], xs, 2 * (x + disp[:, 0].double().abs() + w)) for c in range(Cc)]
    got, Mg = torch.stack([K - r[0][:, 1] for r in rows], 1), torch.stack([r[1][:, 1] - K for r in rows], 1)
    top = S.worst("golden disp_warp", S.ratio(gold("disp_warp").view_as(got), got, Mg, 1.0))[0]
    assert top <= 8.0, top
    for P, tag, sd in ((3, "fusion_", cases.state_dict()), (5, "fusion_p5_", cases.fusion_p5_state_dict())):
        o, st = cases.fusion_case()
        _, _, conf, pw, flow = st["memory"]
        c = dict(pc=o["pred_disp"], pw=pw, flow=flow, conf=conf)
        cues, _ = S.cues_fr(c, P)
        f = S.forget(cues, sd)
        valid = (pw > 0).double()
        r = S.ratio(gold(tag + "reset_weights").view_as(valid), f["wr"] * valid, f["M"], 1.0)
        top = S.worst(f"golden {tag}reset_weights", r)[0]
        assert top <= 8.0, top
        wf = gold(tag + "fusion_weights").view_as(valid)
        wr = gold(tag + "reset_weights").view_as(valid)  # (both golden weights are masked already: masking is idempotent)
        b = S.blend(c["pc"], pw, F.max_pool2d(wf, 4), wr, 4)
        assert torch.equal(b["wf"], wf) and torch.equal(b["wr"], wr)
        r = S.ratio(gold(tag + "pred_disp").view_as(valid), b["fused"], b["M"], 1.0)
        assert S.worst(f"golden {tag}pred_disp", r)[0] <= 8.0


def test_planted_inputs_are_what_they_claim():
    """The sample positions, holes, ties and logits that the cases promise, checked on the references alone."""
    _threads()
    for case in S.WARP_CASES:
        B, Cc, Ht, Wt = case[:4]
        W = 4 * Wt
        c = S.warp_case(case)
        assert (c["fl"] < 0).any() and c["h0"][:, 1:3].abs().max() <= 0.5
        xs, X = S.plane_positions(c["h0"])
        pl = S.warp_plants(Ht, Wt)
        row = lambda n: xs[:, 4 * pl[n][0]:4 * pl[n][0] + 4, 4 * pl[n][1]:4 * pl[n][1] + 4]
        assert torch.equal(row("integer_and_zero")[0], torch.arange(4.0, dtype=F64).expand(4, 4))
        assert (row("w_minus_1")[..., 3] == W - 1).all() and (row("w_minus_1_last_row")[..., 3] == W - 1).all()
        assert (row("inside_-1_0")[..., 0] == -0.5).all()
        assert (row("beyond_-4") < -5).all() and (row("beyond_w+4") > W + 5).all()
        assert (row("1e6") < -9e5).all()
        s = row("slanted")
        assert (s != torch.floor(s)).any() and (s[:, 0] != s[:, 3]).all()
        assert pl["beyond_w+4"][:2] == (Ht - 1, Wt - 1)  # the last lane of the last workgroup
        # most samples land inside the row
        assert ((xs >= 0) & (xs <= W - 1)).double().mean() > 0.5
    for case in S.COSTVOL_CASES:
        B, Ht, Wt, D = case
        tl, tr = S.costvol_case(case)
        ref = S.costvol(tl, tr, D)
        x = torch.arange(Wt)[None, None, :]
        padded = ref["arg"] > 4 * x
        assert ref["tied"][padded].all()
        if D > 1:
            assert ref["tied"][:, 0, 0].all() and (ref["arg"][:, 0, 0] == 1).all() and (ref["cost"][:, 0, 0] == 0).all()
            assert (ref["arg"][:, Ht - 1, min(1, Wt - 1)] == 4 * min(1, Wt - 1) + 1).all()
        assert (ref["arg"][:, Ht - 1, Wt - 1] == 0).all() and (ref["cost"][:, Ht - 1, Wt - 1] == 0).all()
        if D > 4 * Wt:
            assert (4 * x + 1 < D).all()  # every tile has padded candidates
    for case in S.HYP_CASES:
        c = S.hyp_case(case)
        v, Mg, sel = S.hyp_select(c["upd"], c["cur"], c["prv"])
        tie = c["upd"][:, 1:2] == c["upd"][:, 0:1]
        assert tie[:, :, 0].all() and tie[:, :, -1, -1].all() and not sel[tie].any()
        assert tie.float().mean() >= 0.1 or case[1] * case[2] < 8
        if case[1] > 1:
            assert sel.any() and (v[:, 0] == 0).any()
    for case in S.CUES_LR_CASES:
        B, H, W, P, ds, CF, CS = case
        h, w = H // ds, W // ds
        c = S.fusion_case(case)
        pc, pw = c["pc"], c["pw"]
        assert (pc >= 0).all() and (pw == 0).float().mean() > 0.01 and 0 < (pw < 0).sum() <= 9 * B
        assert (pw[:, 0, 0, 0] <= 0).all() and (pw[:, 0, -1, -1] == 0).all()  # (ds = 2: the corner plant IS the first pixel)
        hole = pw[:, 0, H // 4:H // 4 + H // 8 + 1, W // 3:W // 3 + W // 6 + 1]
        assert (hole <= 0).all()  # (an isolated negative value may sit inside the rectangle)
        far = ((pw - pc).abs() > 20) & (pw > 0)
        assert H * W < 1000 or (far.float().mean() > 0.01 and (pw - pc).abs()[pw > 0].median() < 1.0)
        _, _, dsub, xs = S.cues_lr(dict(c, fl=c["fl"][:, :1], fr=c["fr"][:, :1], fc=c["fc"][:, :1], fw=c["fw"][:, :1]), P, ds)
        pl = S.fusion_plants(H, W, ds)
        at = lambda n, s: xs[:, s, pl[n][0], pl[n][1]]
        assert (at("corner", 0) == 0).all() and (at("corner", 1) == w + 6).all() and (dsub[:, 0, 0, 0] == 0).all()
        assert (at("w_minus_1", 0) == w - 1).all() and (at("w_minus_1", 1) == w - 3).all()
        assert (at("last_row", 0) == -0.5).all() and (at("last_row", 1) == -6).all()
        assert (at("last_pixel", 0) < -9e5).all() and (at("last_pixel", 1) == w - 1 - 1.25).all()
        assert (at("interior", 0) == w // 2 - 1).all()
    for case in S.FUSION_CASES:
        c = S.fusion_case(case)
        cues, _ = S.cues_fr(c, case[3])
        f = S.forget(cues, S.forget_weights(case, cues))
        mid, sat = (f["v"].abs() < 2).double().mean().item(), (f["v"].abs() > 8).double().mean().item()
        print(f"{S.case_id(case)}: forget logits |v| < 2 on {mid:.1%}, |v| > 8 on {sat:.1%}")
        assert mid >= 0.10 and (sat > 0.005 or case[1] * case[2] < 1000), (case, mid, sat)


# ------------------------------------------------------------------------------ the measurement behind every c
def _oracle_figures(verbose=True):
    """{key of C: worst |oracle32 - ref64| / (2^-24 M)} over every GPU case, and the arg-min figures per cost-volume case."""
    _threads()
    acc, ties = {}, {}
    for case in S.COSTVOL_CASES:
        B, Ht, Wt, D = case
        tl, tr = S.costvol_case(case)
        ref = S.costvol(tl, tr, D)
        cost, d = ost.tile_cost_volume_min(tl, tr, D)
        chk = S.argmin_check(ref, cost[:, 0], d[:, 0], S.C["costvol"])
        ties[case] = (S.near_tie_share(ref, S.C["costvol"]), chk["near"], chk["wrong"], chk["where"])
        _upd(acc, {"costvol": chk["cost"]})
    for case in S.WARP_CASES:
        if case[4]:
            continue  # (the same inputs as its aligned twin)
        c = S.warp_case(case)
        for h in (c["h0"], c["h1"]):
            _upd(acc, S.warp_ratios(S.tile_warp(c["fl"], c["fr"], h), o_warp(c, h), S.case_id(case)))
    for case in S.HYP_CASES:
        c = S.hyp_case(case)
        top = 0.0
        for scale in (1.0, 2.0):
            v, Mg = S.hyp_upsample(c["prev"], scale)
            top = max(top, S.worst(f"{S.case_id(case)} hyp_upsample x{scale}", S.ratio(ost.upsample_hyp(c["prev"], scale, 2), v, Mg, 1.0))[0])
        v, Mg, _ = S.hyp_select(c["upd"], c["cur"], c["prv"])
        _upd(acc, {"hyp_upsample": top,
                   "hyp_select": S.worst(f"{S.case_id(case)} hyp_select", S.ratio(o_select(c), v, Mg, 1.0))[0]})
    for case in S.CUES_LR_CASES:
        B, H, W, P, ds, CF, CS = case
        name = S.case_id(case)
        c = S.fusion_case(case)
        lr32, fr32 = o_cues(c, P, ds)
        _upd(acc, S.cues_lr_ratios(S.cues_lr(c, P, ds), lr32, P, name))
        if case not in S.FUSION_CASES:
            continue
        cues, Mc = S.cues_fr(c, P)
        _upd(acc, {"cues_fr": S.worst(f"{name} cues_fr", S.ratio(fr32, cues, Mc, 1.0))[0]})
        sd = S.forget_weights(case, cues)
        f = S.forget(cues, sd)
        wr32 = ofu.forget_head(sd, "fusion", fr32)
        _upd(acc, S.forget_ratio(f, wr32, name))
        wf_lr, wr = S.blend_case(case)
        b = S.blend(c["pc"], c["pw"], wf_lr, wr, ds)
        fused, wf, wro = o_blend(c["pc"], c["pw"], wf_lr, wr, ds)
        assert torch.equal(wf.double(), b["wf"]) and torch.equal(wro.double(), b["wr"])
        _upd(acc, {"blend": S.worst(f"{name} blend", S.ratio(fused, b["fused"], b["M"], 1.0))[0]})
    return acc, ties


def test_fp32_oracle_within_a_quarter_of_every_bound():
    """Worst |oracle32 - ref64| / (2^-24 M) of the project's fp32 CPU oracle per kernel figure over the GPU cases' inputs:
    the figures of stereo_fusion_fp64.MEASURED (printed), each at most c / 4; the oracle's arg-min obeys the arg-min rule;
    and the reference's own near-tie share of every cost-volume case is below half the cap for the final c."""
    acc, ties = _oracle_figures()
    print("measured:", {k: float(f"{v:.3g}") for k, v in acc.items()})
    print("c / 4   :", {k: S.C[k] / 4 for k in acc})
    for case, (share, near, wrong, where) in ties.items():
        print(f"arg-min {S.case_id(case)}: reference near-tie share {share:.2e}, fp32 oracle differs at near ties on {near:.2e}, "
              f"without excuse at {wrong} tiles {where or ''}")
        assert share < S.NEAR_TIE_CAP / 2 and near <= S.NEAR_TIE_CAP and wrong == 0, (case, share, near, wrong, where)
    S.within(acc, 0.25, "fp32 oracle")
    assert set(acc) == set(S.C) == set(S.MEASURED)
    # MEASURED is what the module says it is (to two digits, rounded up), and C is 4 x it
    for k, v in acc.items():
        assert abs(v - S.MEASURED[k]) <= 0.03 * v, (k, v, S.MEASURED[k])
        assert 4 * S.MEASURED[k] <= S.C[k] <= 4 * S.MEASURED[k] * 1.07, k


# ------------------------------------------------------------------------------ power of the bounds
def _excess(wrong, ref, Mg, c, keep=None):
    """(worst err / bound, its location, share of the elements at >= 2 x the bound) of a wrong variant against the GPU bound."""
    r = S.ratio(wrong, ref, Mg, c)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    if keep is not None:
        r = torch.where(keep.expand_as(r), r, torch.zeros_like(r))
    v, at = r.reshape(-1).max(0)
    return v.item(), tuple(int(i) for i in torch.unravel_index(at, r.shape)), (r >= 2).double().mean().item()


def test_power_of_the_bounds():
    """Each wrong variant of a kernel, evaluated in fp64 on a product case, exceeds the GPU bound (c 2^-24 M, or the
    arg-min rule) by at least 2 x on at least one element; the forget head with its weights merged in fp32 instead of
    fp64 -- a legitimate evaluation -- stays under the bound."""
    _threads()
    rows = []
    wcase = S.WARP_CASES[1]
    c = S.warp_case(wcase)
    out, Mg, _ = S.tile_warp(c["fl"], c["fr"], c["h0"])
    for v in ("swap_k", "offset", "clamp"):
        rows.append((f"tile_warp {v}", *_excess(S.tile_warp(c["fl"], c["fr"], c["h0"], v)[0], out, Mg, S.C["warp_cost"])))
    ccase = S.COSTVOL_CASES[2]
    tl, tr = S.costvol_case(ccase)
    ref = S.costvol(tl, tr, ccase[3])
    bad = S.costvol(tl, tr, ccase[3], "clamp")
    rows.append(("costvol border clamp (cost)", *_excess(bad["cost"], ref["cost"], ref["Mv"].gather(1, ref["arg"][:, None])[:, 0], S.C["costvol"])))
    for v in ("clamp", "last"):
        bad = S.costvol(tl, tr, ccase[3], v)
        chk = S.argmin_check(ref, ref["cv"].gather(1, bad["arg"][:, None])[:, 0], bad["arg"].double(), S.C["costvol"])
        rows.append((f"costvol {v} (arg-min: tiles that differ without a near tie)", float(chk["wrong"]) * 2, chk["where"], chk["wrong"] / bad["arg"].numel()))
    hc = S.hyp_case(S.HYP_CASES[1])
    v0, M0, _ = S.hyp_select(hc["upd"], hc["cur"], hc["prv"])
    rows.append(("hyp_select ties pick current", *_excess(S.hyp_select(hc["upd"], hc["cur"], hc["prv"], "ties_current")[0], v0, M0, S.C["hyp_select"])))
    for fcase in (S.FUSION_CASES[3], S.FUSION_CASES[4]):
        B, H, W, P, ds, CF, CS = fcase
        tag = f"P = {P}"
        fc = S.fusion_case(fcase)
        lr, Ml, _, _ = S.cues_lr(fc, P, ds)
        n = 3 * P * P - 2
        for v, key, sl in (("offset", "cues_cost", slice(n, None)), ("dilation", "cues_corr", slice(0, n)),
                           ("drop", "cues_corr", slice(0, n)), ("norm", "cues_corr", slice(0, n))):
            w = S.cues_lr(fc, P, ds, v)[0]
            rows.append((f"cues_lr {v} {tag}", *_excess(w[:, sl], lr[:, sl], Ml[:, sl], S.C[key])))
        cues, Mc = S.cues_fr(fc, P)
        rows.append((f"cues_fr replicate padding {tag}", *_excess(S.cues_fr(fc, P, "replicate")[0], cues, Mc, S.C["cues_fr"])))
        sd = S.forget_weights(fcase, cues)
        f = S.forget(cues, sd)
        sig = torch.sigmoid
        rows.append((f"forget beta_k outside the image {tag}",
                     *_excess(sig(S.forget_merged(cues, S.merge_forget(sd), beta_outside=True)), f["wr"], f["M"], S.C["forget"])))
        for name, weff in (("merged in fp64, rounded to fp32 (the product's)", S.merge_forget(sd).float()),
                           ("merged in fp32", S.merge_forget(sd, torch.float32))):
            top, at, _ = _excess(sig(S.forget_merged(cues, weff)), f["wr"], f["M"], S.C["forget"])
            print(f"power: forget {name} {tag}: {top:.3g} x the bound at {at} (legitimate: must stay under 1)")
            assert top <= 1.0, (name, fcase, top, at)
        wf_lr, wr = S.blend_case(fcase)
        b = S.blend(fc["pc"], fc["pw"], wf_lr, wr, ds)
        for v in ("no_mask", "wf_offset"):
            rows.append((f"blend {v} {tag}", *_excess(S.blend(fc["pc"], fc["pw"], wf_lr, wr, ds, v)["fused"], b["fused"], b["M"], S.C["blend"])))
    weak = []
    for name, top, at, share in rows:
        print(f"power: {name}: {top:.3g} x the bound at {at}, >= 2 x on {share:.2%}")
        if not top >= 2:
            weak.append((name, top, at))
    assert not weak, weak
