"""The HIP dense SE3 Gauss-Newton step (codd_se3_gn_step / codd_se3_gn_step_heads: prep, pair builders 3 and 5, solve)
against the fp64 windowed reference of tests/gn_fp64.py, at the product's shapes (72 x 120 at r = 32: the benchmarked
960 x 576 / 8), B = 2, odd widths, partial tiles, every work split (q4 = 16 .. 4096), with stale scratch, and through
the fused heads.  Bound per pixel, in the twist domain: |log(T_gpu o T_ref^-1)|_inf <= TOL_REL |dx_ref|_inf + TOL_ABS
(its power: tests/test_gauss_newton_fp64_reference.py)."""
import functools
import os

import pytest
import torch

import gn_fp64 as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUILDERS, Q4S = (3, 5), (16, 192, 4096)
HEADS_CASES = [(1, 72, 120, 32), (2, 37, 61, 32)]


@functools.lru_cache(maxsize=None)
def _case(case, common=False):
    """make_case inputs + their fp64 reference step (computed once per case)."""
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))
    c = G.make_case(*case, common=common)
    c["ref"] = G.reference(c)
    return c


def _options(builder, q4):
    from codd_amd import _abi
    _abi.set_option("gn_builder", builder)
    _abi.set_option("gn_q4", q4)  # (before the scratch is sized: codd_se3_gn_scratch depends on it)


def _defaults():
    _options(5, 192)


def _step(c, builder=5, q4=192, item=None):
    """ops.se3_gn_step on (one batch item of) a case under (builder, q4) -> the updated field on the host."""
    from codd_amd import ops
    sl = slice(None) if item is None else slice(item, item + 1)
    T = c["T"][sl].contiguous().to(DEV)
    args = [c[k][sl].contiguous().to(DEV) for k in ("ae", "xyz", "delta", "weight", "d1")]
    try:
        _options(builder, q4)
        ops.se3_gn_step(T, *args, list(c["K8"]), radius=c["radius"])
        torch.cuda.synchronize()
    finally:
        _defaults()
    return T.cpu()


def _check(c, ref, Tg, what, tol_rel):
    """All finite, every pixel with a real reference step moved, and the per-pixel twist bound.  Returns the measured
    worst max(err - TOL_ABS, 0) / |dx_ref|_inf (what TOL_REL is set from)."""
    assert torch.isfinite(Tg).all(), what
    err = G.twist_error(Tg, ref["T_new"])
    dxn = ref["dx"].abs().amax(-1)
    moved = (Tg != c["T"]).any(-1)
    assert moved[dxn > 1e-5].all(), (what, int((~moved[dxn > 1e-5]).sum()))
    rel = ((err - G.TOL_ABS).clamp(min=0) / dxn.clamp(min=1e-30)).max().item()
    lim = tol_rel * dxn + G.TOL_ABS
    print(f"{what}: worst twist error {err.max().item():.3g}, measured rel {rel:.3g}, "
          f"worst err / bound {(err / lim).max().item():.3g}, |dx| median {dxn.median().item():.3g}")
    assert (err <= lim).all(), (what, (err / lim).max().item(), rel)
    return rel


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "B%d_%dx%d_r%d" % c)
def test_gn_step_against_fp64_reference(case):
    """Both builders x q4 in {16, 192, 4096} (at r = 32: up to 324 groups per tile down to one) against the fp64 step;
    builders 3 and 5 bit-identical at every grouping."""
    c = _case(case)
    for q4 in Q4S:
        outs = {b: _step(c, b, q4) for b in BUILDERS}
        assert torch.equal(outs[3], outs[5]), (case, q4)
        _check(c, c["ref"], outs[5], f"{case} q4={q4}", G.TOL_REL)


def test_gn_step_with_large_common_embedding_component():
    """Embeddings with one common component at the top of the measured range (|a|^2 ~ 1.9, gn_fp64.A2_MAX) and the
    usual differences: the kernel's expanded affinity |a_i|^2 + |a_j|^2 - 2 a_i.a_j against the reference's difference."""
    c = _case((2, 37, 61, 32), common=True)
    a2 = ((c["ae"] / 8.0) ** 2).sum(1)
    assert a2.min() > 1.0 and a2.median() > 1.5
    for q4 in (16, 192):
        _check(c, c["ref"], _step(c, 5, q4), f"large |a|^2 q4={q4}", G.TOL_REL)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "B%d_%dx%d_r%d" % c)
def test_gn_step_does_not_read_stale_scratch(case):
    """codd_se3_gn_step with its scratch filled with NaN (and a little larger than asked for) and with zeros: the same
    bits, all finite -- no partial, record or geo2 slot is read before a kernel of the step wrote it (ops.se3_gn_step
    takes its scratch from torch.empty).  The floats past codd_se3_gn_scratch are still NaN afterwards: no kernel of the
    step writes past the size the library asks for."""
    from codd_amd import _abi
    lib = _abi.load()
    c = _case(case)
    B, h, w, r = case
    args = [c[k].contiguous().to(DEV) for k in ("ae", "xyz", "delta", "weight", "d1")]
    ae, xyz, delta, weight, d1 = args
    for builder in BUILDERS:
        for q4 in Q4S:
            outs = []
            try:
                _options(builder, q4)
                n = lib.codd_se3_gn_scratch(B, h, w, r)
                for fill, extra in ((float("nan"), 4096), (0.0, 0)):
                    T = c["T"].contiguous().to(DEV)
                    scratch = torch.full((n + extra,), fill, device=DEV)
                    _abi.check(lib.codd_se3_gn_step(T.data_ptr(), ae.data_ptr(), ae.shape[1], xyz.data_ptr(),
                                                    delta.data_ptr(), weight.data_ptr(), d1.data_ptr(), B, h, w,
                                                    *c["K8"], r, 1e-4, 10.0, scratch.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "se3_gn_step")
                    torch.cuda.synchronize()
                    outs.append(T.cpu())
                    if extra:
                        assert torch.isnan(scratch[n:]).all(), (case, builder, q4, "a write past codd_se3_gn_scratch")
            finally:
                _defaults()
            assert torch.isfinite(outs[0]).all(), (case, builder, q4)
            assert torch.equal(outs[0], outs[1]), (case, builder, q4)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "B%d_%dx%d_r%d" % c)
def test_gn_step_batch_items_and_repeat_launches_are_bitwise_equal(case):
    """Two launches on the same inputs give the same bits; each item of a B = 2 launch equals a B = 1 launch on that
    item alone (the arithmetic does not depend on blockIdx.z)."""
    c = _case(case)
    for q4 in (16, 192):
        full = _step(c, 5, q4)
        assert torch.equal(full, _step(c, 5, q4)), (case, q4)
        if case[0] == 2:
            for item in range(2):
                assert torch.equal(full[item:item + 1], _step(c, 5, q4, item=item)), (case, q4, item)


@functools.lru_cache(maxsize=None)
def _heads_case(case):
    """make_case geometry with hidden channels / head weights instead of ae, delta, weight: hidden = relu of a segment
    centre + noise (768 channels), head weights ~ N(0, 1/16^2) (ae rows x 2.5 so that |ae / 8|^2 ~ 1); the fp64 heads
    and the fp64 step on their outputs."""
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))
    c = dict(G.make_case(*case))
    B, h, w, r = case
    g = torch.Generator().manual_seed(7 * h + w)
    cen = torch.randn(B, 5, 768, generator=g) * 0.6
    hid = cen[torch.arange(B)[:, None, None], c["segment"]] + 0.15 * torch.randn(B, h, w, 768, generator=g)
    c["hidden"] = torch.relu(hid).permute(0, 3, 1, 2).contiguous()
    Wm = torch.randn(38, 256, generator=g) / 16
    Wm[:32] *= 2.5
    Wm[32:35] *= 0.1
    bm = torch.randn(38, generator=g) * 0.1
    c["Wm"], c["bm"] = Wm, bm
    ae, delta, weight, pre, mag = G.heads(c["hidden"], Wm, bm)
    c["weight_ref"], c["weight_mag"] = weight, mag
    target = c["xyz"].double().permute(0, 3, 1, 2) + delta
    c["ref"] = G.gn_step(c["T"], ae / 8.0, target, weight, c["d1"], c["K8"], r)
    return c


@pytest.mark.parametrize("mode,wbound", [("split", 3.5 * 2.0 ** -18), ("split16", 2.0 ** -20)])
@pytest.mark.parametrize("case", HEADS_CASES, ids=lambda c: "B%d_%dx%d_r%d" % c)
def test_gn_step_with_fused_heads_against_fp64_heads_and_step(case, mode, wbound):
    """codd_se3_gn_step_heads on the product path (1x1 heads inside the record packing, hidden channels as split
    records) against fp64 heads + the fp64 step.  weight_out: the split bound of the convolution tests before the
    sigmoid (slope <= 1/4); the step: TOL_REL_HEADS."""
    from codd_amd import ops
    from codd_amd.motion import pack_head_matrix
    c = _heads_case(case)
    prev = ops.set_conv_precision(mode)
    try:
        hs = ops.split_input(c["hidden"].to(DEV), border=0)
        assert hs is not None and hs.terms == ops._TERMS[mode]
        T = c["T"].contiguous().to(DEV)
        w_out = ops.se3_gn_step_heads(T, hs, pack_head_matrix(c["Wm"].to(DEV), f16=mode == "split16"),
                                      c["bm"].to(DEV), c["xyz"].to(DEV), c["d1"].to(DEV), list(c["K8"]),
                                      radius=case[3])
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision(prev)
    werr = (w_out.cpu().double() - c["weight_ref"]).abs()
    wlim = 0.25 * (wbound + 2e-7) * (c["weight_mag"] + 1e-6) + 2.0 ** -22
    print(f"heads {mode} {case}: weight err / bound {(werr / wlim).max().item():.3g}")
    assert (werr <= wlim).all()
    _check(c, c["ref"], T.cpu(), f"heads {mode} {case}", G.TOL_REL_HEADS)
