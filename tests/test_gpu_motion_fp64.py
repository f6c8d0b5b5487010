"""The HIP kernels in and around the RAFT3D update loop -- all-pairs pyramid (split, split16, exact fp32), 2x2 pooling,
pyramid lookup, per-iteration geometry (alone, fused with the lookup, writing conv-input records), convex up-sampling
(modes 0 / 1 / 2 and the fused SE3 + weight form), induced flow, disparity -> depth, sub-sampling, instance norm (plain
and record-writing) -- against the fp64 references of tests/motion_fp64.py at the product's shapes (72 x 120: the
benchmarked 960 x 576 / 8), B = 2, odd sizes and a map whose level 3 is 2 x 2.  Bound per output element:
|gpu - ref64| <= c 2^-24 M (motion_fp64.C; its origin and power: tests/test_motion_fp64_reference.py).  Also: every
output element is written (outputs pre-filled with NaN, record buffers compared whole), fused forms equal their parts
bit for bit, a batch item does not depend on its neighbour, two launches give the same bits, and a NaN leaves the
+-50 clamp of the motion-info channels as a NaN."""
import functools
import os

import pytest
import torch

import motion_fp64 as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
ids = dict(ids=M.case_id)
SUMMARY = {}  # (kernel, case) -> worst err / bound


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _note(kernel, case, res, frac=1.0):
    """Record worst err / bound per figure of ``res`` ({key of C: err / (2^-24 M)}) and assert the bound."""
    for k, v in res.items():
        SUMMARY[(f"{kernel} {k}", M.case_id(case))] = v / M.C[k.split(":")[0]]
    M.within(res, frac, (kernel, case))


class _precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from codd_amd import ops
        self.prev = ops.set_conv_precision(self.mode)

    def __exit__(self, *exc):
        from codd_amd import ops
        ops.set_conv_precision(self.prev)


def _items(x, b):
    return x[b:b + 1].clone()  # (a fresh, aligned allocation)


# ------------------------------------------------------------------------------------------------ pyramid, pooling
@functools.lru_cache(maxsize=2)
def _features(case):
    return M.features(*case)


@pytest.mark.parametrize("mode", ["split", "split16", "fp32"])
@pytest.mark.parametrize("case", M.CASES, **ids)
def test_allpairs_pyramid_against_fp64(case, mode):
    """ops.allpairs_corr: the split-bf16 / split-fp16 GEMM paths under the project's split bounds, the exact-fp32 path
    under c 2^-24 M; items of a B = 2 launch equal B = 1 launches; two launches equal."""
    from codd_amd import ops
    _threads()
    f1, f2 = _features(case)
    f1d, f2d = f1.to(DEV), f2.to(DEV)
    with _precision("split" if mode == "fp32" else mode):
        run = lambda a, b: [l.cpu() for l in ops.allpairs_corr(a, b, split=mode != "fp32")]
        pyr = run(f1d, f2d)
        again = run(f1d, f2d)
        single = [run(_items(f1d, b), _items(f2d, b)) for b in range(case[0])] if case[0] > 1 else []
    for i in range(4):
        assert pyr[i].shape == (case[0], case[1] * case[2], (case[1] >> i) * (case[2] >> i))
        assert torch.equal(pyr[i], again[i]), (case, mode, i)
        for b, s in enumerate(single):
            assert torch.equal(pyr[i][b:b + 1], s[i]), (case, mode, i, b)
    res = M.pyramid_ratios(f1, f2, pyr, M.case_id(case), mode)
    if mode == "fp32":
        _note("allpairs fp32", case, res)
    else:
        for k, v in res.items():
            SUMMARY[(f"allpairs {k}", M.case_id(case))] = v
        assert all(v <= 1.0 for v in res.values()), (case, mode, res)


@pytest.mark.parametrize("case", M.CASES, **ids)
def test_avgpool2_against_fp64(case):
    """codd_avgpool2 on the 128-channel feature map and on its pooled maps (odd sizes drop a row / column), output
    pre-filled with NaN."""
    from codd_amd import _abi
    lib = _abi.load()
    B, h, w = case
    x = _features(case)[1]
    for lvl in range(3):
        if min(h >> lvl, w >> lvl) < 2:
            break
        hh, ww = h >> lvl, w >> lvl
        xd = x.to(DEV).contiguous()
        out = _nan(B, 128, hh >> 1, ww >> 1)
        _abi.check(lib.codd_avgpool2(xd.data_ptr(), B * 128, hh, ww, out.data_ptr(), _stream()), "avgpool2")
        ref, Mg = M.avgpool2(x)
        got = out.cpu()
        assert torch.isfinite(got).all()
        _note(f"avgpool2 level {lvl}", case, {"avgpool2": M.worst(f"{M.case_id(case)} avgpool2 {hh}x{ww}", M.ratio(got, ref, Mg, 1.0))[0]})
        x = got


# ------------------------------------------------------------------------------------------------ lookup
@functools.lru_cache(maxsize=1)
def _pyramid(case):
    """The GPU's own pyramid (default precision) on the device and copied back: the lookup's input on both sides."""
    from codd_amd import ops
    f1, f2 = _features(case)
    pyr = ops.allpairs_corr(f1.to(DEV), f2.to(DEV))
    return pyr, [p.cpu() for p in pyr]


@pytest.mark.parametrize("case", M.CASES, **ids)
def test_corr_lookup_against_fp64(case):
    """ops.corr_lookup at planted and random coordinates from the GPU's own pyramid against the fp64 lookup of the same
    volumes; output pre-filled with NaN; coordinate stride 2 and 3; batch items; repeat launch."""
    from codd_amd import ops
    _threads()
    B, h, w = case
    pyr, pyr_cpu = _pyramid(case)
    coords = M.lookup_coords(*case)
    cd = coords.to(DEV)
    got = ops.corr_lookup(pyr, cd, h, w, out=_nan(B, 196, h, w))
    assert torch.isfinite(got).all()
    assert torch.equal(got, ops.corr_lookup(pyr, cd, h, w, out=_nan(B, 196, h, w)))
    c3 = torch.cat([cd, _nan(B, h, w, 1)], -1).contiguous()
    assert torch.equal(got, ops.corr_lookup(pyr, c3, h, w))
    if B > 1:
        for b in range(B):
            one = ops.corr_lookup([_items(p, b) for p in pyr], _items(cd, b), h, w)
            assert torch.equal(got[b:b + 1], one), (case, b)
    _note("corr_lookup", case, M.lookup_ratios(M.lookup(pyr_cpu, coords, h, w), got.cpu(), M.case_id(case)))


# ------------------------------------------------------------------------------------------------ geometry
@functools.lru_cache(maxsize=None)
def _geo(case):
    _threads()
    c = M.geometry_case(*case)
    c["ref"] = M.geometry(c["T"], c["d1"], c["d2"], c["K"])
    return c


def _geometry(T, d1, d2, K):
    """codd_raft_geometry with both outputs pre-filled with NaN -> (xyz, minfo) on the device."""
    from codd_amd import _abi
    lib = _abi.load()
    B, h, w = d1.shape
    xyz, minfo = _nan(B, h, w, 3), _nan(B, 9, h, w)
    _abi.check(lib.codd_raft_geometry(T.data_ptr(), d1.data_ptr(), d2.data_ptr(), B, h, w, *K, xyz.data_ptr(),
                                      minfo.data_ptr(), _stream()), "raft_geometry")
    return xyz, minfo


@pytest.mark.parametrize("case", M.CASES, **ids)
def test_raft_geometry_against_fp64(case):
    """ops.raft_geometry: xyz and the 9 motion-info channels per element against fp64 over five rotation regimes and
    depths 0.7 .. 60; the pixels with |Z| < MIN_DEPTH (under 1 %, decided by the reference alone) are not compared --
    every other pixel is bit-identical to a launch in which those pixels' depth is 10."""
    from codd_amd import ops
    c = _geo(case)
    ref, K = c["ref"], list(c["K"])
    B, h, w = case
    ex = ref["excluded"]
    assert ex.float().mean(dim=(1, 2)).max() < 0.01
    T, d1, d2 = c["T"].to(DEV), c["d1"].to(DEV), c["d2"].to(DEV)
    xyz, minfo = _geometry(T, d1, d2, K)
    xc, mc = xyz.cpu(), minfo.cpu()
    keep = ~ex
    assert torch.isfinite(xc[keep]).all() and torch.isfinite(mc.permute(0, 2, 3, 1)[keep]).all()
    _note("raft_geometry", case, M.geometry_ratios(ref, xc, mc, c["regime"], M.case_id(case)))
    d1b = torch.where(ex, torch.full_like(c["d1"], 10.0), c["d1"]).to(DEV)
    xb, mb = _geometry(T, d1b, d2, K)
    assert torch.equal(xb.cpu()[keep], xc[keep]) and torch.equal(mb.cpu().permute(0, 2, 3, 1)[keep], mc.permute(0, 2, 3, 1)[keep])
    x2, m2 = ops.raft_geometry(T, d1, d2, K)
    assert torch.equal(x2.cpu(), xc) and torch.equal(m2.cpu(), mc)  # (NaN-free: no excluded pixel overflows here)
    if B > 1:
        for b in range(B):
            x1, m1 = _geometry(_items(T, b), _items(d1, b), _items(d2, b), K)
            assert torch.equal(x1, xyz[b:b + 1]) and torch.equal(m1, minfo[b:b + 1]), (case, b)


@pytest.mark.parametrize("case", M.CASES, **ids)
def test_fused_geometry_lookup_against_its_parts_and_fp64(case):
    """ops.raft_geometry_lookup: xyz / minfo bit-equal to raft_geometry; the correlation features against the fp64
    lookup AT THE PUBLISHED xyz under the lookup bound + 8 2^-24 G max(|x|, |y|, 1) (the fused kernel re-projects per
    lane and may differ from the published coordinate by a few ulp; G = the sample's sum of absolute adjacent-tap
    differences); the record-writing form (split / split16 / fp16) == split_input of the fp32 results over the WHOLE
    buffer (borders and channel padding included), written into zeroed buffers."""
    from codd_amd import ops
    c = _geo(case)
    B, h, w = case
    K = list(c["K"])
    pyr, pyr_cpu = _pyramid(case)
    T, d1, d2 = c["T"].to(DEV), c["d1"].to(DEV), c["d2"].to(DEV)
    xyz, minfo = ops.raft_geometry(T, d1, d2, K)
    xyz2, minfo2, corr = ops.raft_geometry_lookup(T, d1, d2, K, pyr)
    assert torch.equal(xyz, xyz2) and torch.equal(minfo, minfo2)
    assert torch.isfinite(xyz).all() and torch.isfinite(corr).all()
    ref = M.lookup(pyr_cpu, xyz.cpu()[..., :2].contiguous(), h, w)
    _note("raft_geometry_lookup corr", case, M.lookup_ratios(ref, corr.cpu(), M.case_id(case) + " fused", extra_c=8.0))
    from codd_amd import _abi  # (the same launch with all three outputs pre-filled with NaN)
    x3, m3, c3 = _nan(B, h, w, 3), _nan(B, 9, h, w), _nan(B, 196, h, w)
    _abi.check(_abi.load().codd_raft_geometry_lookup(T.data_ptr(), d1.data_ptr(), d2.data_ptr(), *[p.data_ptr() for p in pyr],
                                                     B, h, w, *K, x3.data_ptr(), m3.data_ptr(), c3.data_ptr(), _stream()),
               "raft_geometry_lookup")
    assert torch.equal(corr, c3) and torch.equal(minfo2, m3) and torch.equal(xyz2, x3)
    if B > 1:
        for b in range(B):
            _, m1, c1 = ops.raft_geometry_lookup(_items(T, b), _items(d1, b), _items(d2, b), K, [_items(p, b) for p in pyr])
            assert torch.equal(c1, corr[b:b + 1]) and torch.equal(m1, minfo[b:b + 1]), (case, b)
    for mode in ("split", "split16", "fp16"):
        with _precision(mode):
            cxs = ops.split_buffer(("fp64", "corr_in"), B, 196, h, w, 1, DEV)
            mxs = ops.split_buffer(("fp64", "minfo_in"), B, 9, h, w, 3, DEV)
            cxs.buf.zero_(), mxs.buf.zero_()
            xr, mr, cr = ops.raft_geometry_lookup(T, d1, d2, K, pyr, minfo_xs=mxs, corr_xs=cxs)
            assert mr is None and cr is None and torch.equal(xr, xyz)
            assert torch.equal(ops.split_input(corr, border=1).buf, cxs.buf), (case, mode)
            assert torch.equal(ops.split_input(minfo, border=3).buf, mxs.buf), (case, mode)


def _nonfinite_case(B, h, w):
    """A geometry case with integer cx, cy and planted: a NaN pose at one pixel; an identity pose at the principal point
    with depth 5 (its sample position is exactly (cx, cy): the three other taps get weight 0) and 1/d2 = inf at its
    right neighbour tap; 1/d2 = inf at the first tap of another pixel's sample, which has positive weight.  Around both
    planted taps the exact-identity poses are replaced by a 0.1 rad motion, so that no other sample lands within
    rounding of an integer position (where fp32 and fp64 could disagree about a weight being exactly 0).
    -> (case dict without the plants, the same with them, the planted d2 locations, the NaN pixel, the +inf pixel)."""
    from oracle import se3
    c = M.geometry_case(B, h, w, tag=7)
    cx, cy = w // 2, h // 2
    c["K"] = (131.25, 131.25, float(cx), float(cy))
    ref = M.geometry(c["T"], c["d1"], c["d2"], c["K"])
    # a moving pixel whose sample has all four taps inside the image and a first-tap weight of at least 0.1
    u, v = ref["xyz"][0, ..., 0], ref["xyz"][0, ..., 1]
    fu, fv = torch.floor(u), torch.floor(v)
    okp = (fu >= 3) & (fu < w - 4) & (fv >= 3) & (fv < h - 4) & ((1 - (u - fu)) * (1 - (v - fv)) > 0.1) & ~ref["excluded"][0]
    okp &= (c["regime"][0] == 3) & ((fu - cx).abs() > 8)
    okp[:, :w // 2] = False  # (away from the near patch)
    qy, qx = [int(i) for i in torch.nonzero(okp)[0]]
    ty, tx = int(fv[qy, qx]), int(fu[qy, qx])
    moving = se3.exp(torch.tensor([0.1, -0.05, 0.02, 0.05, 0.03, -0.04], dtype=F64)).float()
    for (y, x) in ((cy, cx), (ty, tx)):
        win = c["T"][:, y - 3:y + 4, x - 3:x + 4]
        win[c["regime"][:, y - 3:y + 4, x - 3:x + 4] == 0] = moving
    c["T"][:, cy, cx] = torch.tensor([0, 0, 0, 0, 0, 0, 1.0])
    c["d1"][:, cy, cx] = 5.0
    p = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c.items()}
    ny, nx = 3, w - 5  # the NaN pose
    p["T"][B - 1, ny, nx] = float("nan")
    plants = sorted({(0, cy, cx + 1), (B - 1, cy, cx + 1), (0, ty, tx)})
    for (b, y, x) in plants:
        p["d2"][b, y, x] = 0.0
    return c, p, plants, (B - 1, ny, nx), (0, qy, qx)


@pytest.mark.parametrize("case", [M.CASES[3], M.CASES[0]], **ids)
def test_nonfinite_motion_info_is_not_clamped_to_a_finite_value(case):
    """A NaN motion-info value must leave the +-50 clamp as NaN (torch.clamp in the reference and the oracle keeps it;
    FrameRunner(check_finite=True) relies on it), in the fp32 and in the record-writing form: where the fp64 reference
    is NaN -- a NaN pose; a 1/d2 tap that is inf (depth 0) met with weight exactly 0 -- the kernel's output is NaN; an
    inf tap met with positive weight gives +inf, clamped to 50 on both sides; every pixel the plants cannot reach is
    bit-identical to a launch without them."""
    from codd_amd import ops
    _threads()
    B, h, w = case
    c, p, plants, nanpix, infpix = _nonfinite_case(B, h, w)
    K = list(c["K"])
    ref = M.geometry(p["T"], p["d1"], p["d2"], K)
    raw = ref["raw"]
    cy, cx = h // 2, w // 2
    assert torch.isnan(raw[nanpix[0], :, nanpix[1], nanpix[2]]).all() and torch.isnan(raw[:, 8, cy, cx]).all()
    assert (ref["xyz"][:, cy, cx, 0] == cx).all() and (ref["xyz"][:, cy, cx, 1] == cy).all()
    assert raw[infpix[0], 8, infpix[1], infpix[2]] == float("inf")
    x0, m0 = _geometry(c["T"].to(DEV), c["d1"].to(DEV), c["d2"].to(DEV), K)
    T, d1, d2 = p["T"].to(DEV), p["d1"].to(DEV), p["d2"].to(DEV)
    x1, m1 = _geometry(T, d1, d2, K)
    x0, m0, x1, m1 = x0.cpu(), m0.cpu(), x1.cpu(), m1.cpu()
    # pixels the plants may reach: the NaN pose itself, and every sample whose 4 x 4 tap neighbourhood holds a planted d2
    clean = M.geometry(c["T"], c["d1"], c["d2"], K)
    fu, fv = torch.floor(clean["xyz"][..., 0]), torch.floor(clean["xyz"][..., 1])
    reach = torch.zeros(B, h, w, dtype=torch.bool)
    for (b, y, x) in plants:
        reach[b] |= (fu[b] - 1 <= x) & (x <= fu[b] + 2) & (fv[b] - 1 <= y) & (y <= fv[b] + 2)
    reach[nanpix] = True
    assert reach.float().mean() < 0.02
    far = ~reach
    assert torch.equal(x1[far], x0[far]) and torch.equal(m1.permute(0, 2, 3, 1)[far], m0.permute(0, 2, 3, 1)[far])
    want_nan = torch.isnan(ref["minfo"])
    got_nan = torch.isnan(m1)
    print(f"{M.case_id(case)}: reference NaN at {int(want_nan.sum())} motion-info elements, kernel NaN at "
          f"{int((got_nan & want_nan).sum())} of them; kernel value at the weight-0 inf tap: {m1[0, 8, cy, cx].item()}, "
          f"at the NaN pose: {m1[nanpix[0], :, nanpix[1], nanpix[2]].tolist()}")
    assert torch.equal(got_nan, want_nan), (int(want_nan.sum()), int(got_nan.sum()))
    pinf = torch.isinf(raw) & (raw > 0)
    assert (m1[pinf] == 50.0).all() and torch.isnan(x1[nanpix]).all()
    # the fused and the record-writing forms carry the same bits (records: the NaN's bf16 / fp16 image)
    pyr, _ = _pyramid(case)
    x2, m2, corr = ops.raft_geometry_lookup(T, d1, d2, K, pyr)
    assert torch.equal(m2.cpu().view(torch.int32), m1.view(torch.int32)) and torch.equal(x2.cpu().view(torch.int32), x1.view(torch.int32))
    for mode in ("split", "split16", "fp16"):
        with _precision(mode):
            cxs = ops.split_buffer(("fp64", "corr_in"), B, 196, h, w, 1, DEV)
            mxs = ops.split_buffer(("fp64", "minfo_in"), B, 9, h, w, 3, DEV)
            cxs.buf.zero_(), mxs.buf.zero_()
            ops.raft_geometry_lookup(T, d1, d2, K, pyr, minfo_xs=mxs, corr_xs=cxs)
            assert torch.equal(ops.split_input(m2, border=3).buf, mxs.buf), (case, mode)
            assert torch.equal(ops.split_input(corr, border=1).buf, cxs.buf), (case, mode)


# ------------------------------------------------------------------------------------------------ up-sampling
@functools.lru_cache(maxsize=2)
def _up(case):
    _threads()
    return M.upsample_case(*case)


def _cvx(data, mask, mode):
    """codd_cvx_upsample with the output pre-filled with NaN."""
    from codd_amd import _abi
    lib = _abi.load()
    if mode == 2:
        B, D, h, w = data.shape
        out = _nan(B, D, 8 * h, 8 * w)
    else:
        B, h, w, D = data.shape
        out = _nan(B, 8 * h, 8 * w, D)
    _abi.check(lib.codd_cvx_upsample(data.data_ptr(), mask.data_ptr(), B, h, w, D, mode, out.data_ptr(), _stream()),
               "cvx_upsample")
    return out


@pytest.mark.parametrize("case", M.CASES, **ids)
def test_cvx_upsample_against_fp64(case):
    """ops.cvx_upsample modes 0 (6, 3, 2 channels), 1 (SE3: log -> blend -> exp over five rotation regimes) and 2, and
    ops.cvx_upsample_se3_weight (bit-equal to modes 1 and 2), with saturated soft-maxes at image corners and borders."""
    from codd_amd import ops
    u = _up(case)
    B, h, w = case
    name = M.case_id(case)
    mask = u["mask"].to(DEV)
    outs = {}
    for D in (6, 3, 2):
        got = _cvx(u[f"data{D}"].to(DEV), mask, 0)
        outs[D] = got
        assert torch.isfinite(got).all()
        assert torch.equal(got, ops.cvx_upsample(u[f"data{D}"].to(DEV), mask, 0))
        ref, Mg = M.cvx_data(u[f"data{D}"], u["mask"])
        _note(f"cvx_upsample mode 0 dim {D}", case, {"cvx": M.worst(f"{name} cvx mode 0 dim {D}", M.ratio(got.cpu(), ref, Mg, 1.0))[0]})
    wd = u["weight"].to(DEV)
    got2 = _cvx(wd, mask, 2)
    assert torch.isfinite(got2).all()
    ref, Mg = M.cvx_data(u["weight"].permute(0, 2, 3, 1), u["mask"])
    _note("cvx_upsample mode 2", case, {"cvx": M.worst(f"{name} cvx mode 2", M.ratio(got2.cpu().permute(0, 2, 3, 1), ref, Mg, 1.0))[0]})
    Td = u["T"].to(DEV)
    got1 = _cvx(Td, mask, 1)
    assert torch.isfinite(got1).all()
    r8 = u["regime"].repeat_interleave(8, 1).repeat_interleave(8, 2)
    _note("cvx_upsample mode 1", case, M.se3_up_ratios(M.upsample_se3(u["T"], u["mask"]), got1.cpu(), r8, name))
    from codd_amd import _abi
    lib = _abi.load()
    To, wo = _nan(B, 8 * h, 8 * w, 7), _nan(B, 3, 8 * h, 8 * w)
    _abi.check(lib.codd_cvx_upsample_se3_weight(Td.data_ptr(), wd.data_ptr(), mask.data_ptr(), B, h, w, To.data_ptr(),
                                                wo.data_ptr(), _stream()), "cvx_upsample_se3_weight")
    assert torch.equal(To, got1) and torch.equal(wo, got2)
    T2, w2 = ops.cvx_upsample_se3_weight(Td, wd, mask)
    assert torch.equal(T2, got1) and torch.equal(w2, got2)
    if B > 1:
        for b in range(B):
            mb = _items(mask, b)
            assert torch.equal(_cvx(_items(Td, b), mb, 1), got1[b:b + 1]) and torch.equal(_cvx(_items(wd, b), mb, 2), got2[b:b + 1])
            assert torch.equal(_cvx(_items(u["data6"].to(DEV), b), mb, 0), outs[6][b:b + 1])
            T1, w1 = ops.cvx_upsample_se3_weight(_items(Td, b), _items(wd, b), mb)
            assert torch.equal(T1, got1[b:b + 1]) and torch.equal(w1, got2[b:b + 1])


# ------------------------------------------------------------------------------------------------ full resolution
@pytest.mark.parametrize("case", M.FULLRES_CASES, **ids)
def test_full_resolution_kernels_against_fp64(case):
    """ops.induced_flow, ops.disp_to_depth and ops.subsample at 8 x the case (960 x 576; 488 x 296 at B = 2)."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    _threads()
    B, H, W = case[0], 8 * case[1], 8 * case[2]
    name = M.case_id(case) + " x8"
    c = M.geometry_case(*case, scale=8)
    K = list(c["K"])
    T, d1 = c["T"].to(DEV), c["d1"].to(DEV)
    out = _nan(B, H, W, 3)
    _abi.check(lib.codd_induced_flow(T.data_ptr(), d1.data_ptr(), B, H, W, *K, out.data_ptr(), _stream()), "induced_flow")
    flow, Mg, ex = M.induced_flow(c["T"], c["d1"], K)
    assert ex.float().mean(dim=(1, 2)).max() < 0.01
    got = out.cpu()
    assert torch.isfinite(got[~ex]).all()
    _note("induced_flow", case, {"induced_flow": M.worst(f"{name} induced flow", M.ratio(got, flow, Mg, 1.0), ~ex[..., None], c["regime"])[0]})
    assert torch.equal(ops.induced_flow(T, d1, K).cpu()[~ex], got[~ex])
    d1b = torch.where(ex, torch.full_like(c["d1"], 10.0), c["d1"]).to(DEV)
    assert torch.equal(ops.induced_flow(T, d1b, K).cpu()[~ex], got[~ex])
    if B > 1:
        for b in range(B):
            assert torch.equal(ops.induced_flow(_items(T, b), _items(d1, b), K).cpu()[~ex[b:b + 1]], got[b:b + 1][~ex[b:b + 1]])
    disp = M.disparity_map(B, H, W)
    dd = disp.to(DEV)
    out = _nan(B, 1, H, W)
    _abi.check(lib.codd_disp_to_depth(dd.data_ptr(), dd.numel(), M.BF, out.data_ptr(), _stream()), "disp_to_depth")
    ref, Mg = M.disp_to_depth(disp)
    assert torch.isfinite(out).all() and torch.equal(out, ops.disp_to_depth(dd, M.BF))
    _note("disp_to_depth", case, {"disp_to_depth": M.worst(f"{name} disp_to_depth", M.ratio(out.cpu(), ref, Mg, 1.0))[0]})
    assert (out.cpu()[disp <= 0] == torch.where(disp[disp <= 0] < -1e-5, 0.0, M.BF)).all()
    for (oy, ox, step) in ((3, 3, 8), (1, 1, 4), (0, 0, 1), (H - 1, W - 1, 8)):
        hh, ww = -(-(H - oy) // step), -(-(W - ox) // step)
        out = _nan(B, hh, ww)
        _abi.check(lib.codd_subsample(d1.data_ptr(), B, H, W, oy, ox, step, out.data_ptr(), _stream()), "subsample")
        assert torch.equal(out, d1[:, oy::step, ox::step]) and torch.equal(out, ops.subsample(d1, oy, ox, step))


# ------------------------------------------------------------------------------------------------ instance norm
@pytest.mark.parametrize("case", M.INORM_CASES, **ids)
def test_instnorm_against_fp64(case):
    """ops.instnorm, plain (ReLU on / off, residual or none; the scalar path where h*w is not a multiple of 4) and
    writing conv-input records (ReLU before and after the residual on / off; with and without the fp32 tensor), on
    planes with |mean| = 300 std, a constant plane and one of 1e-3 scale; 1 x 64 x 288 x 480 splits the statistics over
    32 partial sums.  Records: the WHOLE buffer equals split_input of the fp32 result."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    _threads()
    B, Cc, h, w = case
    name = M.case_id(case)
    x, res = M.instnorm_case(*case)
    xd, rd = x.to(DEV), res.to(DEV)
    top = 0.0
    for relu, with_res in ((True, True), (False, True), (True, False), (False, False)):
        y = _nan(B, Cc, h, w)
        stats = torch.full((128 * B * Cc,), float("nan"), device=DEV)
        _abi.check(lib.codd_instnorm(xd.data_ptr(), B, Cc, h * w, stats.data_ptr(), rd.data_ptr() if with_res else None,
                                     int(relu), y.data_ptr(), _stream()), "instnorm")
        assert torch.isfinite(y).all()
        assert torch.equal(y, ops.instnorm(xd, relu=relu, res=rd if with_res else None))
        ref, Mg = M.instnorm(x, res if with_res else None, relu=relu)
        top = max(top, M.worst(f"{name} instnorm relu={relu} res={with_res}", M.ratio(y.cpu(), ref, Mg, 1.0))[0])
        if B > 1 and relu and with_res:
            for b in range(B):
                assert torch.equal(ops.instnorm(_items(xd, b), relu=True, res=_items(rd, b)), y[b:b + 1])
    _note("instnorm", case, {"instnorm": top})
    # a NaN in a plane makes the whole plane NaN, through both ReLUs (torch.relu keeps a NaN; fmaxf(NaN, 0) is 0) and in
    # both apply kernels; the other planes keep their bits
    xn = xd.clone()
    xn[B - 1, 5, h // 2, w // 3] = float("nan")
    want = torch.zeros(B, Cc, 1, 1, dtype=torch.bool, device=DEV)
    want[B - 1, 5] = True
    clean = ops.instnorm(xd, relu=True, res=rd)
    yn = ops.instnorm(xn, relu=True, res=rd)
    assert torch.equal(torch.isnan(yn), want.expand_as(yn)) and torch.equal(yn[~want.expand_as(yn)], clean[~want.expand_as(yn)])
    with _precision("split"):
        xs = ops.split_buffer(("fp64", "inorm"), B, Cc, h, w, 1, DEV)
        for relu2 in (False, True):
            yn = ops.instnorm(xn, relu=True, res=rd, res_relu=relu2, xs_out=xs, want_fp32=True)
            assert torch.equal(torch.isnan(yn), want.expand_as(yn)), relu2
    top = 0.0
    with _precision("split"):
        for relu, with_res, relu2 in ((True, False, False), (True, True, True), (False, True, False), (True, True, False)):
            xs = ops.split_buffer(("fp64", "inorm"), B, Cc, h, w, 1, DEV)
            xs.buf.zero_()
            y = ops.instnorm(xd, relu=relu, res=rd if with_res else None, res_relu=relu2, xs_out=xs, want_fp32=True)
            assert torch.isfinite(y).all()
            ref, Mg = M.instnorm(x, res if with_res else None, relu=relu, res_relu=relu2)
            top = max(top, M.worst(f"{name} instnorm_xs relu={relu} res={with_res} res_relu={relu2}", M.ratio(y.cpu(), ref, Mg, 1.0))[0])
            want = ops.split_input(y, border=1)
            assert (want.c8, want.hp, want.wp) == (xs.c8, xs.hp, xs.wp) and torch.equal(want.buf, xs.buf), (case, relu, with_res, relu2)
            xs.buf.zero_()
            assert ops.instnorm(xd, relu=relu, res=rd if with_res else None, res_relu=relu2, xs_out=xs, want_fp32=False) is None
            assert torch.equal(want.buf, xs.buf), (case, relu, with_res, relu2, "records only")
    _note("instnorm_xs", case, {"instnorm": top})


# ------------------------------------------------------------------------------------------------ splat: batch, repeat
@pytest.mark.parametrize("ds,radius", [(1, 2.0), (4, 4.0)])
def test_splat_batch_items_and_repeat_launches_are_bitwise_equal(ds, radius):
    """ops.splat at (2, 37, 61) x 8: each item of the B = 2 launch equals a B = 1 launch on that item, two launches
    equal (the splat's arithmetic itself: test_splat, test_splat_pileup_... of test_gpu_motion_ops.py)."""
    from codd_amd import ops
    case = (2, 37, 61)
    c = M.geometry_case(*case, scale=8, tag=8)
    B, HT, WT = c["d1"].shape
    o = ds // 2 - 1 if ds > 1 else 0
    H, W = HT // ds, WT // ds
    K = [v / ds for v in c["K"]]
    g = torch.Generator().manual_seed(ds)
    feat = torch.randn(B, 6, H, W, generator=g).to(DEV)
    T, d = c["T"].to(DEV), c["d1"].to(DEV)
    run = lambda T_, d_, f_: ops.splat(T_, d_, f_[:, :3].contiguous(), f_[:, 3:].contiguous(), ds == 1, H, W, o, o, ds, K, radius,
                                       bf=M.BF if ds == 1 else 0.0)
    out, z = run(T, d, feat)
    out2, z2 = run(T, d, feat)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(out, out2) and same(z, z2)
    for b in range(B):
        o1, z1 = run(_items(T, b), _items(d, b), _items(feat, b))
        assert same(o1, out[b:b + 1]) and same(z1, z[b:b + 1]), b


def test_zz_print_worst_error_over_bound_per_kernel_and_case():
    """The figures of DESIGN finding 67: worst err / bound per kernel and case, collected by the tests above."""
    for (kernel, case), v in sorted(SUMMARY.items()):
        print(f"fp64 summary: {kernel:44s} {case:16s} worst err / bound {v:.3g}")
    assert all(v <= 1.0 for v in SUMMARY.values())
