"""The exact-fp32 convolution kernels (conv_kernel.h, conv_quad_kernel.h) reproduce, bit for bit, the outputs that the
library of an EARLIER commit produced: tests/golden/conv_epilogue_bits.json holds sha256 of the output bytes per launch
(tools/parent_bits.py wrote it on the GPU with that library; the launches: tests/conv_epilogue_cases.py).  The
batched epilogue (conv_epilogue) only moves loads ahead of stores, so not one rounding may change:

* every exact-fp32 entry of the shipped-configuration sweep (launched as tests/test_gpu_conv_fp64.py::_launch does);
* one codd_conv2d_multi launch of four jobs;
* hand-made layers at a 9 x 21 and a 10 x 24 output on the classic and the quad kernel: cout = 18, two inputs, the
  transposed-convolution store, res1 + res2 + post with relu_ch0;
* in place: res1 IS the output Slice (the aliasing contract of include/codd_hip.h) -- the bits of the out-of-place launch.
A key missing from the fixture, or one the fixture has and the tree does not, fails."""
import pytest

import conv_epilogue_cases as E
import parent_bits as P
import test_gpu_conv_fp64 as T

pytestmark = pytest.mark.gpu
FIXTURE = P.load(E.NAME)
GOLD = FIXTURE["sha256"]
SWEEP = E.sweep_entries()


def test_fixture_is_from_another_commit_and_names_every_launch():
    """parent_bits.assert_from_another_commit states the rule.  The fixture's keys are exactly the launches of this tree."""
    P.assert_from_another_commit(FIXTURE, E.SOURCES)
    P.assert_keys(FIXTURE, P.all_keys(E))


@pytest.mark.parametrize("L", list(SWEEP), ids=E.V.layer_id)
def test_shipped_fp32_configurations_keep_their_bits(L):
    bad = P.changed(E.sweep_digests(SWEEP[L]), GOLD, [key for (key, *_) in SWEEP[L]])
    assert not bad, ("%d of %d launches changed bits" % (len(bad), len(SWEEP[L])), bad[:4])


def test_multi_launch_keeps_its_bits(monkeypatch):
    got = E.multi_digests(monkeypatch)
    assert list(got) == E.multi_keys()
    assert not P.changed(got, GOLD, list(got))


@pytest.mark.parametrize("name", list(E.HAND))
def test_hand_made_cases_keep_their_bits(name):
    keys = [k for k in E.hand_keys() if k.split("/")[1] == name]
    assert len(keys) >= 3
    for key in keys:
        _, _, hw, lay = key.split("/")
        H, W = (int(v) for v in hw.split("x"))
        assert E.digest(E.hand_launch(name, H, W, int(lay[1:]))) == GOLD[key], key


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("name", ["cout18", "all_operands_relu_ch0"])
def test_res1_may_be_the_output_itself(name, layout):
    """res1 = out, element for element: every lane reads its element before it writes it.  Bit-equal to the launch with
    res1 in a tensor of its own, which equals the recorded bits."""
    for (H, W) in E.HAND_SIZES:
        out_of_place = E.hand_launch(name, H, W, layout)
        in_place = E.hand_launch(name, H, W, layout, in_place=True)
        assert T._bits(in_place, out_of_place), (name, H, W, layout)
        assert E.digest(in_place) == GOLD["hand/%s/%dx%d/l%d" % (name, H, W, layout)]
