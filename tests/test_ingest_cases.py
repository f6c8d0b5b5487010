"""No GPU needed: tests/golden/ingest_bits.json names exactly the launches of tests/ingest_cases.py, and those launches
reach what the ingest kernel branches on."""
import re

import numpy as np

import ingest_cases as IC
import live_fmt_ref as fr
import parent_bits as P

FIXTURE = P.load(IC.NAME)


def test_fixture_keys_are_the_case_list():
    P.assert_keys(FIXTURE, P.all_keys(IC))
    assert re.fullmatch(r"[0-9a-f]{40}", FIXTURE["library_commit"])
    assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in FIXTURE["sha256"].values())


def test_shapes_take_both_store_paths_and_every_entry_and_format():
    h, w = IC.IMAGE
    assert [HW[1] % 4 for HW in IC.OUTPUTS] == [0, 3]  # 16-byte stores; the scalar stores
    assert all(H >= h and W >= w and H - h < h and W - w < w for H, W in IC.OUTPUTS)
    assert w % 4 and w % 2 == 0 and h % 2 == 0  # a group of four that straddles the image's edge; valid for YUV and NV12
    assert {f for f, _ in IC.FRAME_FORMATS} == set(fr.FORMATS)
    assert {y for f, y in IC.FRAME_FORMATS if f == "nv12"} == set(fr.YUV)
    assert {f for f, _ in IC.CALIB_FORMATS} == {"rgb8"} | set(fr.FORMATS) and ("rgb8", True) in IC.CALIB_FORMATS
    assert [s[1] % 4 for s in IC.MAP_SHAPES] == [2, 1] and set(IC.MODELS) == {"brown", "fisheye"}
    kinds = {k.split("/")[3] for k in P.all_keys(IC) if k.startswith("frames/")}
    assert kinds == set(IC.FRAME_KINDS) >= set(IC.PAIR_KINDS)


def test_the_mapped_cases_are_exact_in_fp32():
    """Every map entry is a multiple of 1/64 (or non-finite), so the weights have 6 fractional bits, a product with a tap
    <= 255 has 14 significant bits and the blend's last sum 20: no operation rounds, whatever is fused."""
    h, w = IC.IMAGE
    for kind in ("identity", "q64"):
        for pair in IC.host_maps(kind):
            for m in pair:
                f = m[np.isfinite(m)].astype(np.float64)
                assert np.array_equal(f * 64.0, np.round(f * 64.0))
    (mx, my), (rx, _) = IC.host_maps("q64")
    assert np.isnan(mx).sum() == 1 and np.isposinf(my).sum() == 1 and np.isneginf(mx).sum() == 1
    fx, fy = mx[np.isfinite(mx)], my[np.isfinite(my)]
    assert (fx < -1).any() and (fx > w).any() and (fy < -1).any() and (fy > h).any()  # entries whose four taps are outside
    assert ((fx > -1) & (fx < 0)).any() or ((fx > w - 1) & (fx < w)).any()  # and entries with taps on both sides of an edge
    assert not np.array_equal(mx, rx, equal_nan=True)
    assert IC.host_maps("left")[1] is None and IC.host_maps("right")[0] is None
    assert IC.padded("nv12")[0] == w + 3 and IC.padded("rgb8")[0] == 3 * w + 3
