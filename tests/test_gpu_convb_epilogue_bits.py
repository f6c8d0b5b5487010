"""The epilogues of the split-bf16 convolution kernel (conv_bf16_kernel.h) reproduce, bit for bit, what the library of the
PARENT commit wrote on the launches of tests/convb_epilogue_cases.py: tests/golden/convb_epilogue_bits.json holds sha256 of
the written bytes per launch (tools/parent_bits.py made it on the GPU with that library).

* every wave grid X(PGW, CGW, A, B, KS) of CONVB_ALL x terms 1 | 3 | 16 | 48 x three maps: record output without a gate
  (cout 64 | 18, bias | none, relu | none, three borders, a channel offset), the three gate epilogues (gate 2 with G = 16
  and 32, gate 3 out of place and with out = post), and the fp32 epilogue (all operands with relu_ch0, res1 = the output
  Slice, the transposed store);
* gate 3 in place gives the bits of gate 3 out of place;
* a bias 4 bytes off a 16-byte boundary is refused with CODD_EINVAL;
* the case list reaches every branch (no GPU needed), and the fixture is not from the library under test.
A key missing from the fixture, or one the fixture has and the tree does not, fails."""
import pytest

import convb_epilogue_cases as BC
import parent_bits as P

FIXTURE = P.load(BC.NAME)
GOLD = FIXTURE["sha256"]
CASES = BC.cases()
gpu = pytest.mark.gpu


@gpu
def test_fixture_is_from_another_commit_and_names_every_launch():
    """parent_bits.assert_from_another_commit states the rule.  The fixture's keys are exactly the launches of this tree."""
    P.assert_from_another_commit(FIXTURE, BC.SOURCES)
    P.assert_keys(FIXTURE, P.all_keys(BC))


def test_cases_reach_every_branch():
    """No GPU needed.  The case list names exactly the instantiations of CONVB_ALL in the header, each in the four operand
    formats on the three maps; the maps hold partial tiles in both axes, a unit valid for a few lanes only and empty
    units; the record cases take the 16-byte and the per-element bias path, the gates all three tile kinds of gate 2."""
    header = BC.header_convb_all()
    assert header == list(BC.CONVB_ALL) and len(set(header)) == 16
    got = {(X, (H, W), t, n) for (_, X, H, W, t, n) in CASES}
    for X in BC.CONVB_ALL:
        xb, th, ck, mb, layout, pgw, cgw, _, ks = BC.cfg_of(X, 3)
        assert (layout, xb * th, mb, ks) == (2, X[0] * X[2], X[1] * X[3], X[4]) and -(-xb * th // pgw) == X[2]
        for hw in BC.SIZES:
            for t in BC.TERMS:
                for n in list(BC.REC) + list(BC.GATES) + list(BC.F32):
                    assert ((X, hw, t, n) in got) == (not (n == "f32_deconv" and X[4] == 2))
        # tile kinds: a partial tile in y on some map, and in x on every map (W < 32 or a second unit cut short)
        assert any(H % th for (H, W) in BC.SIZES) and all(W % 32 for (H, W) in BC.SIZES)
    assert {W % 4 == 0 for (H, W) in BC.SIZES} == {True, False}           # both paths of the fp32 epilogue
    assert {(W - 16) for (H, W) in BC.SIZES} == {5, 8, 14}                # lanes of the second unit that hold a pixel
    couts = {v[0] for v in BC.REC.values()}
    assert couts == {64, 18} and {v[1] for v in BC.REC.values()} == {True, False}
    assert {v[2] for v in BC.REC.values()} == {"relu", "none"} and {v[3] for v in BC.REC.values()} == {0, 1, 4}
    assert 3 * 16 % 64 and {"g1", "g2_G16", "g2_G32", "g3", "g3_inplace"} == set(BC.GATES)


@gpu
@pytest.mark.parametrize("terms", BC.TERMS)
@pytest.mark.parametrize("X", BC.CONVB_ALL, ids=BC.xname)
def test_cases_keep_the_parents_bits(X, terms):
    mine = [c for c in CASES if c[1] == X and c[4] == terms]
    assert len(mine) == 3 * len(BC.case_names(X))
    bad = P.changed(BC.case_digests(mine), GOLD, [c[0] for c in mine])
    assert not bad, ("%d of %d launches changed bits" % (len(bad), len(mine)), bad)


@gpu
@pytest.mark.parametrize("X", BC.CONVB_ALL, ids=BC.xname)
def test_gate3_in_place_gives_the_bits_of_out_of_place(X):
    """out = post: the new hidden state and its records are those of the launch into a tensor of its own."""
    import torch
    from codd_amd import ops
    H, W, G = 9, 21, 32
    for terms in (3, 1):
        d, cfg = BC.inputs(H, W), BC.cfg_of(X, terms)
        prev = ops.set_conv_precision(BC.MODE_OF_TERMS[terms])
        try:
            res = []
            for in_place in (False, True):
                pc = ops.PackedConv(d["w", G].to(BC.DEV), d["b", G].to(BC.DEV))
                xs = ops.split_input(d["x"].to(BC.DEV), border=1)
                rec = BC._record_tensor(G, H, W, 1, 0, terms)
                zq, h = BC._c4(d["zq", 2 * G]), BC._c4(d["h", G])
                out = h if in_place else BC._c4(torch.full((BC.B, G, H, W), float("nan")))
                key = ("gate", 3, H, W, BC.B, 1, 1, 0, terms)
                P.forced(pc, key, cfg, lambda: ops.conv_gate(pc, xs, 3, pad=1, out=out, res1=zq, post=h, xs_out=rec))
                res.append(BC.digest(out.buf, rec.buf))
            assert res[0] == res[1], (X, terms)
        finally:
            ops.set_conv_precision(prev)


@gpu
def test_bias_off_alignment_is_refused():
    from codd_amd import _abi
    for X in ((4, 2, 3, 2, 1), (8, 1, 4, 4, 1)):
        with pytest.raises(_abi.CoddHipError, match=r"code -1\b"):
            BC.launch(X, 9, 21, 3, "rec_c64_bias_relu_b1", bias_off4=True)
