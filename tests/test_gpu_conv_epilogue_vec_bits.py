"""The vector epilogue of the exact-fp32 convolution kernels (conv_kernel.h conv_epilogue on swapped MFMA operands: a lane
holds four consecutive pixels of one channel) reproduces, bit for bit, what the library of the PARENT commit produced on
the launches of tests/conv_epilogue_vec_cases.py: tests/golden/conv_epilogue_vec_bits.json holds sha256 of the output bytes
per launch (tools/parent_bits.py wrote it on the GPU with that library).

* bits against the parent fixture: five layers x seven output sizes x seven launch configurations, and one
  codd_conv2d_multi launch mixing a Wout % 4 == 0 job with a Wout % 4 != 0 one;
* alignment fallback: output buffer, res1 and post 4 bytes off a 16-byte boundary -> the bits of the aligned launch (which
  is pinned by the fixture), the floats around every allocation untouched;
* in place: res1 IS the output Slice -> the bits of the out-of-place launch;
* in every launch the sentinel channels around the output Slice come back untouched and, the output being pre-filled with
  NaN, an element that was not written shows in the digest (conv_epilogue_cases.launch asserts the sentinels).
A key missing from the fixture, or one the fixture has and the tree does not, fails."""
import pytest

import conv_epilogue_vec_cases as VC
import parent_bits as P
import test_gpu_conv_fp64 as T

pytestmark = pytest.mark.gpu
FIXTURE = P.load(VC.NAME)
GOLD = FIXTURE["sha256"]
CASES = VC.cases()


def test_fixture_is_from_another_commit_and_names_every_launch():
    """parent_bits.assert_from_another_commit states the rule.  The fixture's keys are exactly the launches of this tree."""
    P.assert_from_another_commit(FIXTURE, VC.SOURCES)
    P.assert_keys(FIXTURE, P.all_keys(VC))


def test_cases_reach_every_decision():
    """No GPU needed: the case list holds every size, configuration and layer the vector epilogue branches on."""
    got = {(name, (H, W), (npb, nw, layout)) for (_, name, H, W, npb, nw, layout) in CASES}
    for name in VC.LAYERS:
        for hw in VC.SIZES:
            for cfg in VC.CONFIGS:
                quad_runs = VC.geometry(name, hw[0], hw[1], cfg[2]) is not None
                assert ((name, hw, cfg) in got) == quad_runs
    # 4 sizes with Wout % 4 == 0: 5 layers x 7 configurations; 3 without: 4 layers x 7 + the transposed store on layout 0
    assert (sum(1 for c in CASES if c[3] % 4 == 0), sum(1 for c in CASES if c[3] % 4)) == (4 * 5 * 7, 3 * (4 * 7 + 3))
    assert not any(VC.geometry(n, H, W, 0) is None for n in VC.LAYERS for (H, W) in VC.SIZES)


@pytest.mark.parametrize("name", list(VC.LAYERS))
@pytest.mark.parametrize("hw", VC.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_cases_keep_the_parents_bits(name, hw):
    mine = [c for c in CASES if c[1] == name and (c[2], c[3]) == hw]
    assert len(mine) >= 3
    bad = P.changed({key: VC.digest(VC.launch(*rest)) for (key, *rest) in mine}, GOLD, [c[0] for c in mine])
    assert not bad, ("%d of %d launches changed bits" % (len(bad), len(mine)), bad)


def test_multi_launch_with_a_flag_per_job_keeps_its_bits():
    got = VC.multi_digests()
    assert list(got) == VC.multi_keys()
    assert not P.changed(got, GOLD, list(got))


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("hw", [(9, 20), (6, 36)], ids=lambda hw: "%dx%d" % hw)
def test_misaligned_operands_take_the_fallback_with_the_same_bits(hw, layout):
    """Output buffer, res1 and post one float into their allocations: ConvK.evec is off, the 4-byte path runs on a
    Wout % 4 == 0 map.  Bit-equal to the aligned launch, which the fixture pins."""
    name, (H, W) = "all_operands_relu_ch0", hw
    for (npb, nw) in ((1, 4), (2, 4), (4, 4)):
        aligned = VC.launch(name, H, W, npb, nw, layout)
        off = VC.launch(name, H, W, npb, nw, layout, misalign=True)
        assert T._bits(off, aligned), (H, W, npb, nw, layout)
        assert VC.digest(aligned) == GOLD[VC.key_of(name, H, W, npb, nw, layout)]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("name", ["cout18", "all_operands_relu_ch0", "no_bias"])
def test_res1_may_be_the_output_itself(name, layout):
    """res1 = out, element for element, on the 16-byte and on the 4-byte path, two blocks per lane along x and two rows
    per wave: every lane reads its quad before it writes it."""
    for (H, W) in ((9, 20), (9, 22)):
        for (npb, nw) in ((2, 4), (4, 4)):
            out_of_place = VC.launch(name, H, W, npb, nw, layout)
            in_place = VC.launch(name, H, W, npb, nw, layout, in_place=True)
            assert T._bits(in_place, out_of_place), (name, H, W, npb, nw, layout)
            assert VC.digest(in_place) == GOLD[VC.key_of(name, H, W, npb, nw, layout)]
