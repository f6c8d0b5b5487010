"""LiveSession stereo confidence without a GPU: the properties of the restatement in tests/live_conf_ref.py (occlusion
band of a fronto-parallel box, the out-of-view border, zero residual on identical images), its residual bound against a
straight fp32 evaluation of the header's expression, the 1 % condition of the MISMATCH rule, the validation of
LiveSession(confidence=...), and every call codd_export_confidence rejects before a launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_conf_ref as lc  # noqa: E402

case_id = lambda s: "%dx%d" % s[0]  # noqa: E731
_CACHE = {}


def _case(shape):
    if shape not in _CACHE:
        c = lc.case(shape)
        _CACHE[shape] = (c, lc.reference(c))
    return _CACHE[shape]


# ---- the reference's own properties -----------------------------------------------------------------------------
def test_box_occludes_exactly_its_band():
    """Background d_b = 2, box d_f = 8 over columns [30, 40) of rows [4, 9): the box lands on right columns 22 .. 32
    (floor(u) and floor(u) + 1 of u = 22 .. 31), a background pixel x looks at column x - 2, so exactly x = 24 .. 29
    (30 .. 34 belong to the box) are occluded; nothing inside the box is; no other row has an occlusion."""
    h, w = 12, 64
    disp = np.full((h, w), 2.0, np.float32)
    disp[4:9, 30:40] = 8.0
    flags, *_ = lc.flags_reference(disp, (h, w), occ_px=1.0)
    want = np.zeros((h, w), np.uint8)
    want[:, :2] = lc.OUT_OF_VIEW  # the left border band x < d
    want[4:9, 24:30] = lc.OCCLUDED
    assert np.array_equal(flags, want)
    # the tolerance: a box less than occ_px in front occludes nothing, one just beyond it does
    for d_f, occluded in ((3.0, False), (3.25, True)):
        disp[4:9, 30:40] = d_f
        flags, *_ = lc.flags_reference(disp, (h, w), occ_px=1.0)
        assert bool((flags[4:9] & lc.OCCLUDED).any()) == occluded
        assert not (flags[4:9, 30:40] & lc.OCCLUDED).any()


def test_left_border_band_is_out_of_view():
    h, w = 4, 40
    disp = np.tile(np.array([5.25, 7.0, 0.5, 12.75], np.float32)[:, None], (1, w))
    flags, U, _, _ = lc.flags_reference(disp, (h, w))
    x = np.arange(w, dtype=np.float32)[None]
    assert np.array_equal(flags == lc.OUT_OF_VIEW, x < disp)
    assert flags[1, 7] == 0 and U[1, 7] == 0  # u == 0 exactly is in view
    assert not (flags & ~np.uint8(lc.OUT_OF_VIEW)).any()  # a constant disparity occludes nothing


def test_identical_images_at_zero_disparity_have_zero_residual():
    c = lc.case(lc.CASES[0])
    c = dict(c, disp=np.full_like(c["disp"], 1e-9), right=c["left"])  # u == x: the match is the pixel itself
    ref = lc.reference(c)
    h, w = c["crop"]
    assert ref["flags124"][:, 1:].max() == 0 and (ref["flags124"][:, 0] == lc.OUT_OF_VIEW).all()  # (0 - 1e-9 < 0)
    assert (ref["residual"][:, 1:] == 0).all() and not ref["mismatch"].any()
    assert (lc.residual_fp32(c, ref["U"], ref["F"])[:, 1:] == 0).all()


# ---- the cases and the bound -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lc.CASES, ids=case_id)
def test_fp32_evaluation_stays_inside_the_bound(shape):
    c, ref = _case(shape)
    got = lc.residual_fp32(c, ref["U"], ref["F"])
    flags = ref["flags124"] | np.where(got > np.float32(lc.TAU), lc.MISMATCH, 0).astype(np.uint8)
    ratio = lc.check_outputs(flags, got, ref, name=case_id(shape))
    assert ratio <= 1.0


@pytest.mark.parametrize("shape", lc.CASES, ids=case_id)
def test_cases_exercise_what_they_claim(shape):
    c, ref = _case(shape)
    (h, w), disp = c["crop"], c["disp"]
    # at most 1 % of the pixels may have their MISMATCH bit left open by the bound
    assert int((~ref["decided"]).sum()) <= 0.01 * h * w
    # quarter-integer disparities (the last awkward value aside), so u + 0.5 lands exactly on integers somewhere
    fin = np.isfinite(disp) & (disp != np.float32(1e-9))
    assert (disp[fin] * 4 == np.round(disp[fin] * 4)).all()
    for (y, x), v in dict(zip(lc.awkward_positions(h, w), lc.AWKWARD + lc.AWKWARD)).items():  # (folded: the last one stays)
        assert np.array_equal(disp[y, x], np.float32(v), equal_nan=True)
    if w >= 2:
        assert ref["U"][h - 1, 1] == 0 and not ref["flags124"][h - 1, 1] & (lc.OUT_OF_VIEW | lc.INVALID)
    if w < 32:
        return  # (15 and 3 pixels: no room for 8 of each of 1, 128 and 2 | 4, which exclude each other, nor for a box)
    u = ref["U"]
    assert (np.isfinite(u) & (u + np.float32(0.5) == np.floor(u + np.float32(0.5)))).sum() >= 8
    flags = ref["flags124"] | np.where(ref["mismatch"], lc.MISMATCH, 0).astype(np.uint8)
    for bit in (lc.OUT_OF_VIEW, lc.OCCLUDED, lc.MISMATCH, lc.INVALID):
        assert int(((flags & bit) != 0).sum()) >= 8, f"fewer than 8 pixels with flag {bit}"
    assert int((flags == (lc.OCCLUDED | lc.MISMATCH)).sum()) >= 1
    # true occlusion bands of known position: background pixels just left of each box are occluded, none inside it
    assert len(c["boxes"]) == 2
    for y0, y1, x0, x1, d in c["boxes"]:
        assert 0 <= y0 < y1 <= h and 3 <= x0 < x1 <= w  # both boxes exist
        assert (ref["flags124"][y0:y1, x0 - 3:x0] & lc.OCCLUDED).sum() >= 2 * (y1 - y0)
        inside = ref["flags124"][y0:y1, x0:x1]
        assert not (inside[disp[y0:y1, x0:x1] == np.float32(d)] & lc.OCCLUDED).any()  # (the awkward values aside)
        # neighbouring box pixels offer the same d to the column between them
        assert disp[y0, x0 + 1] == disp[y0, x0 + 2]
    # the mismatches are the boxes: the background matches
    bg = np.ones((h, w), bool)
    for y0, y1, x0, x1, d in c["boxes"]:
        bg[y0:y1, x0:x1] = False
    visible_bg = bg & (ref["flags124"] == 0)
    assert ref["mismatch"][visible_bg].mean() < 0.02 and ref["mismatch"][~bg].mean() > 0.3


def test_store_pass_model_writes_every_flag_byte_once():
    """A model of confidence.hip's flag store (lane t of pass k holds row element i = 256 k + t = pixel i - s, s the byte
    phase of the row's first flag; a quad 4j .. 4j+3 that lies inside the row leaves as one word from lane 4j, every other
    pixel as a byte): for every row length around the pass and quad boundaries and every phase, each byte of the row is
    written exactly once, every word is 4-byte aligned, inside the row, and gathered from lanes of one wave."""
    T = 256
    for w in list(range(1, 40)) + [61, 255, 256, 257, 259, 260, 511, 512, 513, 517, 1023, 1027]:
        for s in range(4):
            n, written = w + s, np.zeros(w, int)
            for i in range(-(-n // T) * T):  # (uniform trip count: whole passes)
                x, x0 = i - s, (i & ~3) - s
                if x0 >= 0 and x0 + 3 < w:
                    if i & 3 == 0:
                        assert (s + x0) % 4 == 0 and (i % T) % 64 + 3 < 64
                        written[x0:x0 + 4] += 1
                elif 0 <= x < w:
                    written[x] += 1
            assert (written == 1).all(), (w, s)


# ---- LiveSession(confidence=...) validation: no device call --------------------------------------------------------
def test_confidence_option_validation():
    from codd_amd import live
    assert live._check_conf(False) is None and live._check_conf(None) is None
    assert live._check_conf(True) == dict(occ_px=1.0, tau=24.0)
    assert live._check_conf(dict(tau=10)) == dict(occ_px=1.0, tau=10.0)
    assert live._check_conf(dict(occ_px=0)) == dict(occ_px=0.0, tau=24.0)

    class NoDevice:  # an estimator stand-in that fails on any use
        def __getattr__(self, name):
            raise AssertionError(f"the estimator was touched ({name}) before the option was validated")

    for bad in (dict(occ=1.0), dict(occ_px=-0.5), dict(occ_px=float("nan")), dict(tau=float("nan")), dict(tau="x"), "yes",
                1.0, [1.0, 24.0]):
        with pytest.raises(ValueError, match="confidence"):
            live.LiveSession(NoDevice(), (100, 200), confidence=bad)
    assert live.Confidence._fields == ("flags", "residual")


def test_cli_flags_need_each_other():
    from codd_amd import inference
    a = inference.parse_args(["--img-dir", "l", "--r-img-dir", "r", "--live", "--confidence", "--occ-px", "2", "--tau", "30"])
    assert a.confidence and a.occ_px == 2.0 and a.tau == 30.0
    for argv in (["--confidence"], ["--live", "--tau", "3"], ["--live", "--occ-px", "3"]):
        with pytest.raises(SystemExit):
            inference.parse_args(["--img-dir", "l", "--r-img-dir", "r"] + argv)


# ---- calls rejected before any launch (the library loads without a GPU) ---------------------------------------------
P = 0x1000  # a dummy non-NULL pointer: nothing below reaches a launch
EINVAL, EUNSUPPORTED = -1, -2


def _call(disp=P, left=P, right=P, H=64, W=64, h=37, w=61, stdv=True, occ_px=1.0, tau=24.0, flags=P, residual=P):
    from codd_amd import _abi
    s = (C.c_float * 3)(*lc.STD) if stdv else None
    return _abi.load().codd_export_confidence(disp, left, right, H, W, h, w, s, occ_px, tau, flags, residual, None)


@pytest.mark.parametrize("kw", [
    dict(disp=None), dict(flags=None),
    dict(left=None), dict(right=None), dict(stdv=False),  # one image without the other; images without stdv
    dict(left=None, right=None, stdv=False),  # (residual given) residual without images
    dict(left=None, right=None),  # the same with a stray stdv
    dict(h=0), dict(w=0), dict(h=-1), dict(H=0, h=0), dict(W=0), dict(h=65), dict(w=65),
    dict(occ_px=-1e-3), dict(occ_px=float("nan")), dict(occ_px=float("-inf")), dict(tau=float("nan")),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_calls_are_rejected(kw):
    assert _call(**kw) == EINVAL


def test_rows_beyond_the_lds_limit_are_unsupported():
    from codd_amd import ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_hip.h")).read()
    assert "#define CODD_CONF_MAX_W 8192" in header
    assert _call(H=4, W=8256, h=4, w=8193) == EUNSUPPORTED
    assert _call(H=4, W=8256, h=4, w=8193, left=None, right=None, stdv=False, residual=None) == EUNSUPPORTED
    assert _call(H=4, W=8256, h=5, w=8193) == EINVAL  # an invalid call stays invalid
    assert (ops.CONF_OUT_OF_VIEW, ops.CONF_OCCLUDED, ops.CONF_MISMATCH, ops.CONF_INVALID) == (1, 2, 4, 128)
