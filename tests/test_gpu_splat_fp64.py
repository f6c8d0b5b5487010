"""The forward splat's HIP kernels (codd_splat: splat_count, splat_reserve, splat_fill, splat_gather; ops.splat) against
the fp64 reference of tests/splat_fp64.py on every case of its table -- one partial block; B = 2 with a second reserve
workgroup and a partial 4-tuple; portrait shapes (R = 0.607 and 1.21 px); the 1/4-resolution path from a map whose sides
are no multiples of 4; R = 2.6; CA = 0 or CB = 0, with and without flow and disparity -- and on the planted cases
(pile-up, on the circle, disparity threshold, nine candidates), which have no excluded pixel.
Bound per output element: |gpu - ref64| <= c 2^-24 M + CF 2^-24 Mb off the reference's fragile pixels (splat_fp64.C; its
origin and power: tests/test_splat_fp64_reference.py).  Also: every output element is written (outputs pre-filled with
NaN), covered pixels equal the reference's, candidate-free pixels are exactly 0, ops.splat gives the same bits, and the
scratch holds what include/codd_hip.h documents: count == fill, cursor == sum of the counts, disjoint lists that tile
[0, cursor), the reference's candidate count, list entries that are valid points covering their pixel."""
import functools
import os

import numpy as np
import pytest
import torch

import splat_fp64 as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
EINVAL = -1  # CODD_EINVAL
ALL = list(S.CASES) + list(S.PLANTED)
SUMMARY = {}  # (figure, case) -> worst err / bound


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _ref(name):
    _threads()
    return S.reference(S.make_case(name))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _cover_bound(R):
    s = 2 * int(np.ceil(np.float32(R))) + 1
    return s * s


def _launch(c):
    """codd_splat on case ``c`` with the test's own scratch (pre-filled with -7) and NaN-pre-filled out / zout ->
    (out, zout, scratch) on the CPU, after the stream has drained."""
    from codd_amd import _abi
    lib = _abi.load()
    B, H, W = c["B"], c["H"], c["W"]
    HT, WT = c["T"].shape[1:3]
    A, Bf = _dev(c["featA"]), _dev(c["featB"])
    CA, CB = (0 if A is None else A.shape[1]), (0 if Bf is None else Bf.shape[1])
    Cn = CA + (3 if c["with_flow"] else 0) + CB
    T, d = _dev(c["T"]), _dev(c["depth"])
    out = torch.full((B, Cn, H, W), float("nan"), device=DEV)
    zout = torch.full((B, 1, H, W), float("nan"), device=DEV)
    ns = lib.codd_splat_scratch(B, H, W, float(c["radius"]))
    n = B * H * W
    nhead = (3 * n + 4 + 3) & ~3
    assert ns == nhead + ((n * _cover_bound(S.radius_px(c["radius"], H, W)) + 3) & ~3) + 4 * n  # (the documented size)
    scratch = torch.full((ns,), -7, device=DEV, dtype=torch.int32)
    assert scratch.data_ptr() % 16 == 0
    _abi.check(lib.codd_splat(T.data_ptr(), d.data_ptr(), HT, WT, c["oy"], c["ox"], c["ds"], _ptr(A), CA, _ptr(Bf), CB,
                              int(c["with_flow"]), B, H, W, *c["K"], float(c["radius"]), float(c["bf"]), out.data_ptr(),
                              zout.data_ptr(), scratch.data_ptr(), _stream()), "splat")
    torch.cuda.synchronize()
    return out.cpu(), zout.cpu(), scratch.cpu()


def _ops_splat(c):
    from codd_amd import ops
    out, z = ops.splat(_dev(c["T"]), _dev(c["depth"]), _dev(c["featA"]), _dev(c["featB"]), c["with_flow"], c["H"], c["W"],
                       c["oy"], c["ox"], c["ds"], list(c["K"]), c["radius"], bf=c["bf"])
    return out.cpu(), z.cpu()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _note(name, res):
    for k, v in res.items():
        SUMMARY[(k, name)] = v / S.C[k]
    S.within(res, 1.0, name)


def _scratch_checks(name, c, r, scratch):
    """The documented scratch contract (include/codd_hip.h, codd_splat_scratch) after a launch."""
    B, H, W = c["B"], c["H"], c["W"]
    n, HW = B * H * W, H * W
    R = S.radius_px(c["radius"], H, W)
    nhead = (3 * n + 4 + 3) & ~3
    nlist = (n * _cover_bound(R) + 3) & ~3
    cnt, off, cur = scratch[:n].long(), scratch[n:2 * n].long(), scratch[2 * n:3 * n].long()
    cursor = int(scratch[3 * n])
    lst = scratch[nhead:nhead + nlist].long()
    uvz = scratch[nhead + nlist:nhead + nlist + 4 * n].view(torch.float32).view(B, HW, 4)
    # count == fill, cursor, padding
    assert torch.equal(cnt, cur), (name, int((cnt != cur).sum()))
    assert (cnt >= 0).all() and cursor == int(cnt.sum()) and cursor <= nlist, (name, cursor, int(cnt.sum()))
    assert (scratch[3 * n + 1:3 * n + 4] == 0).all()
    # the [off, off + cnt) ranges of the pixels with candidates are disjoint and tile [0, cursor)
    has = torch.nonzero(cnt > 0)[:, 0]
    o, k = off[has], cnt[has]
    order = torch.argsort(o)
    o, k = o[order], k[order]
    if len(o):
        assert o[0] == 0 and torch.equal(o[1:], (o + k)[:-1]) and int(o[-1] + k[-1]) == cursor, name
    else:
        assert cursor == 0
    # the reference's candidate count off the pixels with an open coverage decision
    keep = ~r["frag_cnt"].reshape(-1)
    assert torch.equal(cnt[keep], r["cnt"].reshape(-1)[keep]), (name, int((cnt[keep] != r["cnt"].reshape(-1)[keep]).sum()))
    # the stored projection: the reference's validity, and (u, v, z) within the zone constant CF of their magnitudes
    worst = 0.0
    for b in range(B):
        p = r["pts"][b]
        sure = ~p["unc"]
        valid = uvz[b, :, 3] == 1.0
        assert ((uvz[b, :, 3] == 1.0) | (uvz[b, :, 3] == 0.0)).all()
        assert torch.equal(valid[sure], p["valid"][sure]), (name, b)
        ok = valid & p["valid"] & sure
        for j, (key, mk) in enumerate((("u", "Mu"), ("v", "Mv"), ("z", "Mz"))):
            err = (uvz[b, :, j].to(F64) - p[key]).abs()[ok]
            lim = (S.U * p[mk])[ok]
            if c["exact"]:
                assert (err == 0).all(), (name, key)
            elif len(err):
                worst = max(worst, float((err / lim).max()))
    print(f"{name}: stored (u, v, z): worst err / (2^-24 M) = {worst:.3g} (the zone constant CF = {S.CF})")
    assert worst <= S.CF
    SUMMARY[("stored uvz / CF", name)] = worst / S.CF
    # list contents: a valid point of the same item whose stored (u, v) covers the pixel -- d^2 from the stored fp32
    # coordinates in fp64, against R^2 as the kernel holds it (fl(R R)), with 4 ulp for the fp32 evaluation of d^2
    R2 = float(np.float32(R) * np.float32(R))
    pix = torch.repeat_interleave(has, cnt[has])
    pos = torch.repeat_interleave(off[has], cnt[has]) + (torch.arange(len(pix)) - torch.repeat_interleave(torch.cumsum(cnt[has], 0) - cnt[has], cnt[has]))
    ent = lst[pos]
    assert ((ent >= 0) & (ent < HW)).all(), name
    b_of = pix // HW
    q = uvz[b_of, ent].to(F64)
    assert (q[:, 3] == 1.0).all(), name
    px, py = (pix % HW) % W, (pix % HW) // W
    d2 = (q[:, 0] - (px.to(F64) + 0.5)) ** 2 + (q[:, 1] - (py.to(F64) + 0.5)) ** 2
    assert (d2 < R2 * (1 + 4 * S.U)).all(), (name, float((d2 / R2).max()))
    # ... and no point twice in a list
    key = pix * HW + ent
    assert len(torch.unique(key)) == len(key), name


@pytest.mark.parametrize("name", ALL)
def test_splat_against_fp64(name):
    """codd_splat on one case: outputs, coverage, zeros, ops.splat's bits, the scratch contract."""
    c, r = S.make_case(name), _ref(name)
    out, zout, scratch = _launch(c)
    assert not torch.isnan(out).any() and not torch.isnan(zout).any(), "an output element was not written"
    _note(name, S.compare(name, r, out, zout, c))
    keep = ~r["frag_z"]
    assert torch.equal((zout[:, 0] > 0)[keep], r["zpos"][keep]), name
    empty = (r["cnt"] == 0) & ~r["frag_cnt"]
    assert (out.permute(0, 2, 3, 1)[empty] == 0).all() and (zout[:, 0][empty] == 0).all(), name
    if c["exact"] and c["bf"] == 0:
        assert torch.equal(zout[:, 0].to(F64), r["zout"]), name
    o2, z2 = _ops_splat(c)
    assert _bits(o2, out) and _bits(z2, zout), name
    _scratch_checks(name, c, r, scratch)


def test_threshold_and_circle_plants_decide_as_the_reference():
    """The decisions the plants are built for, spelled out: bf / (z + 1e-5f) == W is kept and the next fp32 above is
    zeroed; a point at d^2 == R^2 is no candidate, one at the next fp32 coordinate inside is."""
    c, r = S.make_case("threshold"), _ref("threshold")
    _, zout, _ = _launch(c)
    assert (zout[0, 0, 23:25, 31:33] == float(S.PW)).all() and (zout[0, 0, 23:25, 47:49] == 0).all()
    for name in ("circle_R1", "circle_R2"):
        c, r = S.make_case(name), _ref(name)
        _, zout, scratch = _launch(c)
        n = c["H"] * c["W"]
        assert torch.equal(scratch[:n].long(), r["cnt"].reshape(-1)) and torch.equal(zout[0, 0].to(F64), r["zout"][0])


def _nonfinite_case():
    """Case 2 with planted: a NaN quaternion, an inf translation, a NaN depth, an inf depth (four points, item 0 and 1),
    and a NaN in feature channel 1 of featA at a point that is a kept candidate of some pixel."""
    c = dict(S.make_case("2_B2_37x61_flow"))
    c["T"], c["depth"], c["featA"] = c["T"].clone(), c["depth"].clone(), c["featA"].clone()
    H, W = c["H"], c["W"]
    c["T"][0, 5, 7, 4] = float("nan")
    c["T"][1, 20, 30, 0] = float("inf")
    c["depth"][0, 12, 40] = float("nan")
    c["depth"][1, 30, 11] = float("inf")
    c["featA"][0, 1, 18, 25] = float("nan")
    c["featA"][1, 1, 9, 50] = float("inf")
    c["name"] = "2_B2_37x61_flow nonfinite"
    return c


def test_nonfinite_inputs():
    """A point whose pose or depth is NaN / inf is dropped (stored as invalid, in no list) and nothing else changes: the
    reference of the planted inputs holds under the same bound; a NaN / inf feature reaches exactly the pixels whose
    kept candidates include its point (NaN where the reference is NaN, nowhere else)."""
    _threads()
    c = _nonfinite_case()
    r = S.reference(c)
    assert torch.isnan(r["out"][0, 1]).any() and not torch.isfinite(r["out"][1, 1]).all()
    out, zout, scratch = _launch(c)
    B, H, W = c["B"], c["H"], c["W"]
    n = B * H * W
    bad = [(0, 5 * W + 7), (1, 20 * W + 30), (0, 12 * W + 40), (1, 30 * W + 11)]
    for b, i in bad:
        assert not r["pts"][b]["valid"][i]
    keep = ~r["frag_out"][:, None].expand_as(out)
    assert torch.equal(torch.isnan(out)[keep], torch.isnan(r["out"])[keep])
    assert not torch.isnan(zout).any()
    fin = torch.isfinite(r["out"]) & torch.isfinite(r["M"])
    rr = dict(r)
    # (non-finite reference elements are compared above and here as bits of inf; the bound applies to the finite ones)
    inf = torch.isinf(r["out"]) & keep
    assert torch.equal(out.to(F64)[inf], r["out"][inf])
    rr["out"] = torch.where(fin, r["out"], torch.zeros_like(r["out"]))
    rr["M"] = torch.where(fin, r["M"], torch.ones_like(r["M"]))
    rr["Mb"] = torch.where(fin, r["Mb"], torch.zeros_like(r["Mb"]))
    got = torch.where(fin, out, torch.zeros_like(out))
    _note(c["name"], S.compare(c["name"], rr, got, zout, c))
    _scratch_checks(c["name"], c, r, scratch)
    nhead = (3 * n + 4 + 3) & ~3
    nlist = (n * _cover_bound(S.radius_px(c["radius"], H, W)) + 3) & ~3
    uvz = scratch[nhead + nlist:nhead + nlist + 4 * n].view(torch.float32).view(B, H * W, 4)
    for b, i in bad:
        assert uvz[b, i, 3] == 0.0, (b, i)


def test_invalid_arguments_are_refused():
    """CODD_EINVAL, nothing launched: the sub-sampling edge oy + ds (H - 1) >= HT (and the same in x; one row / column
    less is accepted by the check), a scratch that is not 16-byte aligned, radius <= 0 or NaN, a non-positive size or
    step, a negative offset, a missing feature pointer; codd_splat_scratch returns -1 for a size or radius it cannot
    serve."""
    from codd_amd import _abi
    lib = _abi.load()
    c = S.make_case("4_B2_150x246_ds4")
    T, d = _dev(c["T"]), _dev(c["depth"])
    B, HT, WT = 2, 150, 246
    A = torch.zeros(B, 32, 40, 64, device=DEV)  # (every buffer large enough for the largest size tried)
    out, zout = torch.zeros(B, 32, 40, 64, device=DEV), torch.zeros(B, 1, 40, 64, device=DEV)
    scratch = torch.zeros(lib.codd_splat_scratch(B, 40, 64, 4.0) + 4, device=DEV, dtype=torch.int32)

    def call(H=37, W=61, oy=1, ox=1, ds=4, radius=4.0, sp=None, fa=A.data_ptr(), CA=32, B_=B, Tp=T.data_ptr()):
        return lib.codd_splat(Tp, d.data_ptr(), HT, WT, oy, ox, ds, fa, CA, None, 0, 0, B_, H, W, *c["K"], radius, 0.0,
                              out.data_ptr(), zout.data_ptr(), scratch.data_ptr() if sp is None else sp, _stream())

    assert 1 + 4 * (38 - 1) < HT <= 1 + 4 * (39 - 1) and 1 + 4 * (62 - 1) < WT <= 1 + 4 * (63 - 1)
    assert call(H=39) == EINVAL and call(W=63) == EINVAL and call(oy=6) == EINVAL and call(ox=6) == EINVAL
    assert call(sp=scratch.data_ptr() + 4) == EINVAL and call(sp=scratch.data_ptr() + 8) == EINVAL
    assert call(radius=0.0) == EINVAL and call(radius=-2.0) == EINVAL and call(radius=float("nan")) == EINVAL
    assert call(H=0) == EINVAL and call(W=0) == EINVAL and call(B_=0) == EINVAL and call(ds=0) == EINVAL
    assert call(oy=-1) == EINVAL and call(ox=-1) == EINVAL
    assert call(fa=None) == EINVAL and call(CA=-1) == EINVAL and call(Tp=None) == EINVAL and call(sp=0) == EINVAL
    assert lib.codd_splat_scratch(B, 37, 61, 0.0) == -1 and lib.codd_splat_scratch(B, 37, 61, float("nan")) == -1
    assert lib.codd_splat_scratch(0, 37, 61, 4.0) == -1 and lib.codd_splat_scratch(B, 0, 61, 4.0) == -1
    torch.cuda.synchronize()
    assert (out == 0).all() and (scratch == 0).all()  # (nothing ran)
    assert call() == 0 and call(H=38, W=62) == 0 and call(oy=5, ox=5) == 0  # (the last row / column / offset inside the map)
    torch.cuda.synchronize()


def test_zz_print_worst_error_over_bound_per_case():
    """The figures of DESIGN finding 74: worst err / bound per output class and case, collected by the tests above."""
    for (k, name), v in sorted(SUMMARY.items()):
        print(f"splat fp64 summary: {k:16s} {name:28s} worst err / bound {v:.3g}")
    assert all(v <= 1.0 for v in SUMMARY.values())
