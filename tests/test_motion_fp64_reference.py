"""The fp64 references of tests/motion_fp64.py that tests/test_gpu_motion_fp64.py holds the HIP kernels against: pinned
here to the CPU oracle fed fp64 and to the golden arrays of the imported reference; the fp32 oracle measured against
them on the GPU cases' own inputs (the measurement every constant ``c`` of motion_fp64.C is 4 x of); the SE3 table of
DESIGN finding 67 as a test; and the power of the bounds -- every wrong variant of a kernel listed in
test_power_of_the_bounds must exceed the GPU bound by 2 x.  CPU only; run with -s for the figures."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import motion_fp64 as M
from oracle import motion as om
from oracle import se3

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _upd(acc, res):
    for k, v in res.items():
        k = k.split(":")[0]
        acc[k] = max(acc.get(k, 0.0), v)


def _flat(pyr):
    return [c.reshape(c.shape[0], c.shape[1] * c.shape[2], -1) for c in pyr]


# ------------------------------------------------------------------------------ the references themselves
def test_references_equal_the_oracle_fed_fp64_and_the_golden_arrays():
    """lookup / bilinear / cvx / project / the pyramid (restated in motion_fp64 to carry M, G and the wrong variants) ==
    oracle.motion's functions fed fp64, and the arrays of tests/golden/reference_outputs.npz that pin the oracle to the
    imported reference (corr_lvl*, cvx_upsample, project, depth_sampler) to fp32 rounding of the stored values."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import cases
    G = np.load(os.path.join(HERE, "golden", "reference_outputs.npz"))
    gold = lambda k: torch.from_numpy(G[k]).to(F64)
    f1, f2 = cases.fmaps()
    pyr64 = _flat(om.corr_pyramid(f1.double(), f2.double()))
    for lvl in range(4):
        for b, r0, r1, ref, Mg in M.pyramid_blocks(f1, f2, lvl, rows=1 << 20):  # (one block: 384 rows)
            assert (ref - pyr64[lvl][b, r0:r1]).abs().max() < 1e-12
            assert ((ref[::5, ::3] - gold(f"corr_lvl{lvl}")[b]).abs() <= 16 * M.U * Mg[::5, ::3]).all()
    h, w = f1.shape[-2:]
    coords = M.lookup_coords(1, h, w)
    out, Mg, Gd = M.lookup(pyr64, coords, h, w)
    ref = om.corr_lookup([p.view(1, h, w, h >> i, w >> i) for i, p in enumerate(pyr64)],
                         coords.double().permute(0, 3, 1, 2).contiguous())
    assert (out - ref).abs().max() < 1e-13 and (Mg >= out.abs() - 1e-13).all()
    data, mask = cases.cvx_inputs()
    assert torch.equal(M.cvx(data, mask), om.cvx_upsample(data.double(), mask.double()))
    assert (M.cvx(data, mask)[:, ::3, ::5] - gold("cvx_upsample")).abs().max() < 1e-5
    depth, K, cd = cases.proj_inputs()
    X = om.inv_project(depth.double(), K.double())
    uvz, Z = M._project(X, [float(v) for v in K[0]])
    assert torch.equal(uvz, om.project(X, K.double()))
    assert ((uvz - gold("project")).abs() <= 4 * M.U * (uvz.abs() + 8.0)).all()  # (fx X / Z and cx = 8 cancel at the first pixels)
    v, Ms, Gx, Gy = M.bilinear(depth.double(), cd[..., 0].double(), cd[..., 1].double())
    assert (v - om.sample_bilinear(depth.double()[:, None], cd.double())).abs().max() < 1e-13
    assert (v - gold("depth_sampler")).abs().max() < 8 * M.U * 60
    # se3.log / exp run in fp64 when fed fp64
    xi = torch.randn(1000, 6, dtype=F64, generator=torch.Generator().manual_seed(1)) * 0.3
    assert (se3.log(se3.exp(xi)) - xi).abs().max() < 1e-14


def test_planted_inputs_are_what_they_claim():
    """All five rotation regimes, q.w < 0, the 1.0005e-3 plants; |Z| < MIN_DEPTH on under 1 % of the pixels of every case
    with the planted depths among them and the near patch behind the camera; a saturated soft-max returns exp(log(T)) of
    the selected pixel (the centre) or identity (a neighbour outside the image)."""
    for case in M.CASES:
        c = M.geometry_case(*case)
        ref = M.geometry(c["T"], c["d1"], c["d2"], c["K"])
        assert all((c["regime"] == r).any() for r in range(5)), case
        assert (c["T"][..., 6] < 0).any()
        th = se3.log(c["T"].double())[..., 3:].norm(dim=-1)
        assert ((th - 1.0005e-3).abs() < 1e-8).any()
        share = ref["excluded"].float().mean(dim=(1, 2))
        print(f"{M.case_id(case)}: |Z| < MIN_DEPTH on {ref['excluded'].sum().item()} pixels ({share.max().item():.3%})")
        assert 0 < share.max() < 0.01 and ref["excluded"][c["d1"] < M.MIN_DEPTH].any(), case
        py, px = M.near_patch(*case[1:])
        assert (ref["Z"][:, py:py + 2, px:px + 2] < -M.MIN_DEPTH).all(), case
    for case in M.FULLRES_CASES:
        c = M.geometry_case(*case, scale=8)
        ex = M.induced_flow(c["T"], c["d1"], c["K"])[2]
        assert 0 < ex.float().mean(dim=(1, 2)).max() < 0.01
    B, h, w = 2, 37, 61
    u = M.upsample_case(B, h, w)
    out, Mg, th = M.upsample_se3(u["T"], u["mask"])
    rt = se3.exp(se3.log(u["T"].double()))
    ident = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=F64)
    for (b, y, x, k) in u["hot"]:
        yy, xx = y + k // 3 - 1, x + k % 3 - 1
        want = rt[b, yy, xx] if 0 <= yy < h and 0 <= xx < w else ident
        assert (out[b, 8 * y:8 * y + 8, 8 * x:8 * x + 8] - want).abs().max() < 1e-15, (b, y, x, k)


# ------------------------------------------------------------------------------ the fp32 oracle against them: sets c
def _oracle_geometry(c):
    B, h, w = c["d1"].shape
    Kt = torch.tensor([list(c["K"])] * B)
    xyz = om.project(se3.act(c["T"], om.inv_project(c["d1"], Kt)), Kt)
    zinv = om.sample_bilinear((1.0 / c["d2"])[:, None], xyz[..., :2])
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    mi = om.motion_info(xyz[..., :2] - torch.stack([xx, yy], -1)[None], se3.log(c["T"]), zinv.unsqueeze(-1) - xyz[..., 2:])
    return xyz, mi


def test_fp32_oracle_within_a_quarter_of_every_bound():
    """Worst |oracle32 - ref64| / (2^-24 M) of the project's fp32 CPU oracle per kernel over the GPU cases' inputs: the
    figures of motion_fp64.MEASURED (printed), each at most c / 4."""
    _threads()
    acc = {}
    for case in M.CASES:
        B, h, w = case
        name = M.case_id(case)
        f1, f2 = M.features(*case)
        pyr32 = _flat(om.corr_pyramid(f1, f2))
        _upd(acc, M.pyramid_ratios(f1, f2, pyr32, name))
        coords = M.lookup_coords(*case)
        got = om.corr_lookup([p.view(B, h, w, h >> i, w >> i) for i, p in enumerate(pyr32)],
                             coords.permute(0, 3, 1, 2).contiguous())
        _upd(acc, M.lookup_ratios(M.lookup(pyr32, coords, h, w), got, name))
        del pyr32
        c = M.geometry_case(*case)
        ref = M.geometry(c["T"], c["d1"], c["d2"], c["K"])
        _upd(acc, M.geometry_ratios(ref, *_oracle_geometry(c), c["regime"], name))
        u = M.upsample_case(*case)
        for D in (6, 3, 2):
            v, Mg = M.cvx_data(u[f"data{D}"], u["mask"])
            _upd(acc, {"cvx": M.worst(f"{name} cvx mode 0 dim {D}", M.ratio(om.cvx_upsample(u[f"data{D}"], u["mask"]), v, Mg, 1.0))[0]})
        wl = u["weight"].permute(0, 2, 3, 1)
        v, Mg = M.cvx_data(wl, u["mask"])
        _upd(acc, {"cvx": M.worst(f"{name} cvx mode 2", M.ratio(om.cvx_upsample(wl, u["mask"]), v, Mg, 1.0))[0]})
        r8 = u["regime"].repeat_interleave(8, 1).repeat_interleave(8, 2)
        _upd(acc, M.se3_up_ratios(M.upsample_se3(u["T"], u["mask"]), om.upsample_se3(u["T"], u["mask"]), r8, name))
        x = f2[:, :16]
        v, Mg = M.avgpool2(x)
        _upd(acc, {"avgpool2": M.worst(f"{name} avgpool2", M.ratio(F.avg_pool2d(x, 2), v, Mg, 1.0))[0]})
    for case in M.FULLRES_CASES:
        name = M.case_id(case) + " x8"
        c = M.geometry_case(*case, scale=8)
        B = case[0]
        flow, Mg, ex = M.induced_flow(c["T"], c["d1"], c["K"])
        got = om.induced_flow2d(c["T"], c["d1"], torch.tensor([list(c["K"])] * B))
        _upd(acc, {"induced_flow": M.worst(f"{name} induced flow", M.ratio(got, flow, Mg, 1.0), ~ex[..., None], c["regime"])[0]})
        disp = M.disparity_map(B, 8 * case[1], 8 * case[2])
        v, Mg = M.disp_to_depth(disp)
        got = om.disp_to_depth(disp, torch.tensor([[1.0]]))  # (scale * K[0, 0] = 210 exactly)
        _upd(acc, {"disp_to_depth": M.worst(f"{name} disp_to_depth", M.ratio(got, v, Mg, 1.0))[0]})
    for case in M.INORM_CASES:
        x, res = M.instnorm_case(*case)
        v, Mg = M.instnorm(x, res, relu=True)
        got = F.relu(F.instance_norm(x, eps=1e-5) + res)
        _upd(acc, {"instnorm": M.worst(f"{M.case_id(case)} instnorm", M.ratio(got, v, Mg, 1.0))[0]})
    print("measured:", {k: float(f"{v:.3g}") for k, v in acc.items()})
    print("c / 4   :", {k: M.C[k] / 4 for k in acc})
    M.within(acc, 0.25, "fp32 oracle")
    # MEASURED is what the module says it is (to two digits, rounded up), and C is 4 x it
    for k, v in acc.items():
        assert abs(v - M.MEASURED[k]) <= 0.03 * v, (k, v, M.MEASURED[k])
        assert 4 * M.MEASURED[k] <= M.C[k] <= 4 * M.MEASURED[k] * 1.07, k


def _exp_errors(ang, n=40000, seed=0):
    """Worst |exp32 - exp64| of the translation in units of 2^-24 |tau| without / with the 1/th factor."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=F64)
    xi = torch.cat([torch.randn(n, 3, generator=g, dtype=F64), d / d.norm(dim=-1, keepdim=True) * ang], -1).float()
    e = (se3.exp(xi)[..., :3].double() - se3.exp(xi.double())[..., :3]).abs().amax(-1)
    tau, th = xi[..., :3].double().norm(dim=-1), xi[..., 3:].double().norm(dim=-1)
    return (e / (M.U * tau)).max().item(), (e / (M.U * tau * M.exp_factor(th))).max().item()


def test_se3_exp_table():
    """fp32 oracle.se3.exp against fp64, 40 000 random twists per rotation angle: the translation error stays below
    c 2^-24 |tau| (1 + [th^2 >= 1e-6] / th) at every angle, and WITHOUT the 1/th term it does not in [1e-3, 1e-2]: the
    cancellation of (1 - cos th) / th^2 in left_jac_apply, shared by the kernel (se3.h) and the reference's lietorch."""
    c = M.C["se3_exp_t"]
    top = 0.0
    for ang in (1e-4, 9.99e-4, 1.0005e-3, 3e-3, 1e-2, 0.1, 1.0, 3.0):
        plain, scaled = _exp_errors(ang)
        print(f"se3.exp fp32 at {ang:g} rad: err / (2^-24 |tau|) = {plain:.3g}, with the 1/th factor {scaled:.3g}")
        top = max(top, scaled)
        assert scaled <= c / 4, (ang, scaled)
        if 1.0005e-3 <= ang <= 3e-3:
            assert plain > 2 * c, (ang, plain)
        if ang < 1e-3:
            assert plain == scaled
    assert abs(top - M.MEASURED["se3_exp_t"]) <= 0.03 * top and 4 * top <= c <= 4.3 * top


# ------------------------------------------------------------------------------ power of the bounds
@functools.lru_cache(maxsize=None)
def _lookup_setup(case):
    B, h, w = case
    f1, f2 = M.features(*case)
    pyr = _flat(om.corr_pyramid(f1, f2))
    coords = M.lookup_coords(*case)
    return pyr, coords, M.lookup(pyr, coords, h, w)


def _excess(wrong, ref, Mg, c, keep=None):
    """(worst err / bound, share of the elements at >= 2 x the bound) of a wrong variant against the GPU bound."""
    r = M.ratio(wrong, ref, Mg, c)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    if keep is not None:
        r = r[keep.expand_as(r)]
    return r.max().item(), (r >= 2).double().mean().item()


def test_power_of_the_bounds():
    """Each wrong variant of a kernel, applied to the fp64 reference on the GPU cases' own inputs, exceeds the GPU bound
    (c 2^-24 M) by at least 2 x on at least one element -- the first five on at least 1 % of the elements."""
    _threads()
    case = (2, 37, 61)
    B, h, w = case
    rows = []  # (name, worst ratio, share, needs 1 %)
    pyr, coords, (out, Mg, Gd) = _lookup_setup(case)
    for i, v in enumerate(("channel_order", "level_coord", "clamp_edge", "shift")):
        rows.append(("lookup " + v, *_excess(M.lookup(pyr, coords, h, w, variant=v)[0], out, Mg, M.C["lookup"]), True))
    u = M.upsample_case(*case)
    ref, Mu = M.cvx_data(u["data6"], u["mask"])
    rows.append(("cvx softmax64", *_excess(M.cvx(u["data6"], u["mask"], "softmax64"), ref, Mu, M.C["cvx"]), True))
    rows.append(("cvx order", *_excess(M.cvx(u["data6"], u["mask"], "order"), ref, Mu, M.C["cvx"]), False))
    rows.append(("cvx replicate", *_excess(M.cvx(u["data6"], u["mask"], "replicate"), ref, Mu, M.C["cvx"]), False))
    sref = M.upsample_se3(u["T"], u["mask"])
    rows.append(("upsample_se3 order", *_excess(M.upsample_se3(u["T"], u["mask"], "order")[0][..., :3], sref[0][..., :3],
                                                sref[1][..., :3], M.C["cvx_se3_t"]), False))
    f1, f2 = M.features(*case)
    top = 0.0
    for lvl in (1, 2, 3):
        good = list(M.pyramid_blocks(f1, f2, lvl, rows=4096))
        bad = list(M.pyramid_blocks(f1, f2, lvl, rows=4096, variant="ceil"))
        for (_, _, _, r0, M0), (_, _, _, r1, _) in zip(good, bad):
            top = max(top, _excess(r1, r0, M0, M.C["pyramid_fp32"])[0],
                      M.ratio(r1, r0, M0, 0.0, extra=M.SPLIT_BOUND["split"][0] * M0 + M.SPLIT_BOUND["split"][1]).max().item())
    rows.append(("pyramid ceil sizes (fp32 and split bound)", top, 0.0, False))
    c = M.geometry_case(*case)
    g0 = M.geometry(c["T"], c["d1"], c["d2"], c["K"])
    keep = ~g0["excluded"]
    g1 = M.geometry(c["T"], c["d1"], c["d2"], c["K"], "no_peps")
    rows.append(("project without +1e-5 (xyz.uv)", *_excess(g1["xyz"][..., :2], g0["xyz"][..., :2], g0["M_xyz"][..., :2],
                                                           M.C["xyz_uv"], keep[..., None]), False))
    g1 = M.geometry(c["T"], c["d1"], c["d2"], c["K"], "nearest")
    rows.append(("1/d2 sampled nearest", *_excess(g1["minfo"][:, 8], g0["minfo"][:, 8], g0["M_minfo"][:, 8],
                                                 M.C["minfo_dz"], keep), False))
    g1 = M.geometry(c["T"], c["d1"], c["d2"], c["K"], "twist_scale")
    rows.append(("twist not scaled by 10", *_excess(g1["minfo"][:, 2:8], g0["minfo"][:, 2:8], g0["M_minfo"][:, 2:8],
                                                   M.C["minfo_twist"], keep[:, None]), False))
    x, res = M.instnorm_case(2, 64, 37, 61)
    n0, Mn = M.instnorm(x, res)
    rows.append(("instnorm unbiased variance", *_excess(M.instnorm(x, res, unbiased=True)[0], n0, Mn, M.C["instnorm"]), False))
    rows.append(("instnorm eps = 0", *_excess(M.instnorm(x, res, eps=0.0)[0], n0, Mn, M.C["instnorm"]), False))
    disp = M.disparity_map(2, 8 * 37, 8 * 61)
    d0, Md = M.disp_to_depth(disp)
    rows.append(("disp_to_depth without +1e-5", *_excess(M.disp_to_depth(disp, eps=0.0)[0], d0, Md, M.C["disp_to_depth"]), False))
    weak = []
    for name, top, share, wide in rows:
        print(f"power: {name}: {top:.3g} x the bound at the worst element, >= 2 x on {share:.2%}")
        if not top >= 2 or (wide and not share >= 0.01):
            weak.append((name, top, share))
    assert not weak, weak
