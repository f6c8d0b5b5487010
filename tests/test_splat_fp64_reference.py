"""The fp64 reference of tests/splat_fp64.py that tests/test_gpu_splat_fp64.py holds the forward splat's HIP kernels
against: the planted cases are what they claim (the fp32 projection is exact on them, the plants sit where the
docstrings say); the fp32 CPU oracle (oracle.motion.splat) measured against the reference on every case -- the
measurement every constant ``c`` of splat_fp64.C is 4 x of; the share of fragile pixels under its cap; and the power of
the bounds: every wrong variant of test_power_of_the_bounds, evaluated in fp64, exceeds the GPU bound by 1000 x.
CPU only; run with -s for the figures."""
import functools
import math
import os

import pytest
import torch

import splat_fp64 as S
from oracle import motion as om

F64 = torch.float64
ALL = list(S.CASES) + list(S.PLANTED)


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


@functools.lru_cache(maxsize=None)
def _ref(name):
    _threads()
    return S.reference(S.make_case(name))


def oracle32(c):
    """The project's fp32 CPU oracle on a case: om.splat of [featA | induced flow | featB] at the sampled positions,
    the disparity conversion in fp32 -> (out [B,C,H,W], zout [B,1,H,W])."""
    Ts, d = S.sampled(c)
    Kt = torch.tensor([list(c["K"])] * c["B"])
    fs = [c["featA"]] if c["featA"] is not None else []
    if c["with_flow"]:
        fs.append(om.induced_flow2d(Ts, d, Kt).permute(0, 3, 1, 2))
    if c["featB"] is not None:
        fs.append(c["featB"])
    out, z = om.splat(Ts, d, torch.cat(fs, 1).contiguous(), Kt, c["radius"])
    if c["bf"] > 0:
        dsp = torch.tensor(c["bf"]) / (z + 1e-5)
        z = torch.where(dsp > c["W"], torch.zeros_like(dsp), dsp)
    return out, z


# ------------------------------------------------------------------------------ the inputs are what they claim
def test_cases_exercise_the_paths_they_are_listed_for():
    """R of every case (portrait: not an integer, below 1 at radius 2); the reserve pass's second workgroup and partial
    4-tuple; gather grids that are no multiple of 8 blocks; every side of the frame has points driven out of it; points
    behind the camera and at depth 0 exist; some pixel has nine or more candidates wherever R >= 1."""
    for name in S.CASES:
        c, r = S.make_case(name), _ref(name)
        B, H, W = c["B"], c["H"], c["W"]
        u = torch.stack([p["u"] for p in r["pts"]])
        v = torch.stack([p["v"] for p in r["pts"]])
        ok = torch.stack([p["valid"] for p in r["pts"]])
        z = torch.stack([p["z"] for p in r["pts"]])
        assert (ok & (u < 0)).any() and (ok & (u > W)).any() and (ok & (v < 0)).any() and (ok & (v > H)).any(), name
        assert (z < 0).any() and (~ok).any() and (S.sampled(c)[1] == 0).any(), name
        print(f"{name}: R = {r['R']:.6g} px, {B * H * W} pixels, {-(-H * W // 256)} gather blocks per item, "
              f"candidates per pixel up to {int(r['cnt'].max())}, covered {r['covered'].float().mean().item():.3f}")
    assert abs(_ref("3_61x37_r2")["R"] - 2.0 * 37 / 122) < 1e-6 and abs(_ref("3_61x37_r4_flow")["R"] - 4.0 * 37 / 122) < 1e-6
    assert abs(_ref("5_64x96_r5.2")["R"] - 2.6) < 1e-6 and _ref("4_B2_150x246_ds4")["R"] == 2.0
    c = S.make_case("2_B2_37x61_flow")
    n = c["B"] * c["H"] * c["W"]
    assert n == 4514 and n > 4096 and n % 4 != 0 and -(-c["H"] * c["W"] // 256) == 9
    c = S.make_case("4_B2_150x246_ds4")
    assert (c["H"], c["W"]) == (37, 61) and c["T"].shape[1] % 4 and c["T"].shape[2] % 4 and c["featA"].shape[1] == 32
    assert -(-64 * 96 // 256) == 24
    for name in ("2_B2_37x61_flow", "4_B2_150x246_ds4", "5_64x96_r5.2"):
        assert _ref(name)["cnt"].max() > S.KEEP, name


def test_planted_cases_project_exactly_in_fp32_and_hold_their_plants():
    """On the planted cases the fp32 evaluation of (u, v, z, valid) equals the fp64 one bit for bit (what makes their
    magnitudes 0 and their fragile masks empty), and: the pile-up has > 1000 candidates on a pixel with exact z ties among
    the nearest; the circle cases have candidates at d^2 = R^2 exactly (not counted) and within 1e-5 inside it
    (counted), in all four directions; the threshold case's two pixels' disparities are exactly W (kept) and the next
    fp32 above W (zeroed); the ninth-nearest candidate of the ninth case's pixel has the largest alpha."""
    for name in S.PLANTED:
        c = S.make_case(name)
        Ts, d = S.sampled(c)
        p32 = S.project_points(Ts[0], d[0], c["K"], True)
        p64 = S.project_points(Ts[0].to(F64), d[0].to(F64), c["K"], True)
        assert torch.equal(p32["valid"], p64["valid"]), name
        for k in ("u", "v", "z"):
            assert p32[k].dtype == torch.float32 and torch.equal(p32[k].to(F64)[p64["valid"]], p64[k][p64["valid"]]), (name, k)
        r = _ref(name)
        assert not (r["frag_out"] | r["frag_flow"] | r["frag_z"] | r["frag_cnt"]).any() and r["Mb"].abs().max() == 0, name
    r = _ref("pileup")
    assert r["cnt"].max() > 1000 and (r["covered"].sum() <= 30)
    p = r["pts"][0]
    assert (p["z"] == 4.0).sum() > 700
    yy, xx = torch.meshgrid(torch.arange(S.PH, dtype=F64) + 0.5, torch.arange(S.PW, dtype=F64) + 0.5, indexing="ij")
    for name, R in (("circle_R1", 1.0), ("circle_R2", 2.0)):
        r = _ref(name)
        p = r["pts"][0]
        moved = torch.nonzero(p["z"] == 2.0)[:, 0]
        assert len(moved) == 8
        on, inside = set(), set()
        for n in moved:
            d2 = (p["u"][n] - xx) ** 2 + (p["v"][n] - yy) ** 2
            if (d2 == R * R).sum() >= 1 and not ((d2 < R * R) & (d2 > R * R - 1e-4)).any():
                on.add(int(n))
            if ((d2 < R * R) & (d2 > R * R - 1e-4)).any():
                inside.add(int(n))
                at = torch.nonzero((d2 < R * R) & (d2 > R * R - 1e-4))[0]
                assert r["zout"][0, at[0], at[1]] == 2.0  # (the pixel just inside sees the point)
        assert len(on) == 4 and len(inside) == 4, (name, on, inside)
    c, r = S.make_case("threshold"), _ref("threshold")
    z = r["zout"][0]
    assert (z[23:25, 31:33] == float(S.PW)).all() and (z[23:25, 47:49] == 0).all() and r["cnt"][0, 23:25, 47:49].min() > 0
    assert c["bf"] / (float(c["depth"][0, 24, 48]) + S.EPS32) > S.PW and abs(c["bf"] / (float(c["depth"][0, 24, 48]) + S.EPS32) - S.PW) < 1e-5
    r = _ref("ninth")
    assert r["cnt"][0, 20, 30] >= 9
    # (out at that pixel does not hold the ninth point's feature: the variant that keeps the largest alphas differs)


# ------------------------------------------------------------------------------ the fp32 oracle: sets c; the cap
@functools.lru_cache(maxsize=None)
def _oracle_res(name):
    c, r = S.make_case(name), _ref(name)
    out, z = oracle32(c)
    return out, z, S.compare(name + " oracle32", r, out, z, c)


def test_fp32_oracle_within_a_quarter_of_every_bound():
    """Worst |oracle32 - ref64| / (2^-24 M) of the fp32 CPU oracle per output class over every case, off the fragile
    pixels: the figures of splat_fp64.MEASURED (printed), each at most c / 4 with c = 4 x MEASURED rounded up to two
    digits.  Off the fragile pixels the oracle also agrees on which pixels are covered and on every candidate-free pixel
    being 0; on the planted cases (no fragile pixel) zout is bit-exact wherever its magnitude is 0."""
    acc = {}
    for name in ALL:
        c, r = S.make_case(name), _ref(name)
        out, z, res = _oracle_res(name)
        for k, v in res.items():
            acc[k] = max(acc.get(k, 0.0), v)
        keep = ~r["frag_z"]
        assert torch.equal((z[:, 0] > 0)[keep], r["zpos"][keep]), name
        empty = (r["cnt"] == 0) & ~r["frag_cnt"]
        assert (out.permute(0, 2, 3, 1)[empty] == 0).all() and (z[:, 0][empty] == 0).all(), name
        if c["exact"] and c["bf"] == 0:
            assert torch.equal(z[:, 0].to(F64), r["zout"]), name
    for k, v in sorted(acc.items()):
        print(f"splat fp32 oracle, {k}: worst err / (2^-24 M) = {v:.3g}; MEASURED {S.MEASURED[k]}, c = {S.C[k]}")
    for k, v in acc.items():
        assert v <= S.MEASURED[k] <= 1.01 * v + 0.005, (k, v)  # (MEASURED is this figure, rounded up to three digits)
        c4 = 4.0 * S.MEASURED[k]
        digits = 10.0 ** (math.floor(math.log10(c4)) - 1)
        assert c4 <= S.C[k] <= c4 + digits, (k, c4)
    S.within(acc, 0.25, "fp32 oracle")


def test_fragile_share_is_under_one_percent_of_the_covered_pixels():
    """The pixels the reference calls open -- per mask and item -- are at most 1 % of the covered pixels of every random
    case and none of any planted one."""
    for name in ALL:
        sh = S.shares(_ref(name))
        print(f"{name}: fragile share of the covered pixels: " + ", ".join(f"{k[5:]} {v:.3%}" for k, v in sh.items()))
        cap = 0.0 if name in S.PLANTED else 0.01
        assert all(v <= cap for v in sh.values()), (name, sh)


# ------------------------------------------------------------------------------ power
POWER = [("alpha_linear", "2_B2_37x61_flow"), ("trans_first", "2_B2_37x61_flow"), ("largest_alpha", "5_64x96_r5.2"),
         ("largest_alpha", "ninth"), ("tie_high", "pileup"), ("le_circle", "circle_R1"), ("le_circle", "circle_R2"),
         ("centre0", "1_9x13"), ("R_half", "3_61x37_r2"), ("span_short2", "5_64x96_r5.2"),
         ("span_short1", "3_61x37_r4_flow"), ("flow_z_sign", "2_B2_37x61_flow")]


@pytest.mark.parametrize("variant,name", POWER, ids=[f"{v}-{n}" for v, n in POWER])
def test_power_of_the_bounds(variant, name):
    """A wrong splat, evaluated in fp64, exceeds the GPU bound c 2^-24 M (+ CF 2^-24 Mb) off the fragile pixels by at
    least 1000 x in some output class (inf: a value where the reference has none), or -- ``<=`` at the circle with
    R = 1, where the extra candidates have alpha = 0 -- changes zout and the candidate count."""
    c, r = S.make_case(name), _ref(name)
    w = S.reference(c, variant)
    res = S.compare(f"{name} {variant}", r, w["out"], w["zout"][:, None], c, quiet=True)
    f = {k: v / S.C[k] for k, v in res.items()}
    ncnt = int(((w["cnt"] != r["cnt"]) & ~r["frag_cnt"]).sum())
    print(f"power: {variant:14s} on {name:18s}: err / bound " + ", ".join(f"{k} {v:.3g}" for k, v in f.items())
          + f"; candidate count differs at {ncnt} pixels")
    assert max(f.values()) >= 1000.0, (variant, name, f)
    if variant in ("le_circle", "centre0", "R_half", "span_short1", "span_short2"):
        assert ncnt > 0


def test_the_kernel_window_has_a_pixel_to_spare_at_R_2_6():
    """The window ox, oy in [-span + 1, span] around floor(u - 0.5), span = (int)(R + 1.5), holds every centre within R
    with one pixel to spare on each side when frac(R) >= 0.5 or R is an integer (R = 2.6: span = 4, the disc needs
    [-2, 3]): one short changes nothing there, two short does (above); at R = 1.213 (portrait, radius 4) the window is
    tight and one short is wrong (above)."""
    c, r = S.make_case("5_64x96_r5.2"), _ref("5_64x96_r5.2")
    w = S.reference(c, "span_short1")
    assert torch.equal(w["out"], r["out"]) and torch.equal(w["cnt"], r["cnt"]) and torch.equal(w["zout"], r["zout"])
