"""No GPU needed: tests/golden/load_chain_bits.json names exactly the launches of tests/load_chain_cases.py, and those
launches reach what the batched loads of motion.hip branch on."""
import os
import re

import load_chain_cases as LC
import parent_bits as P

FIXTURE = P.load(LC.NAME)


def _source_define(name):
    src = open(os.path.join(P.ROOT, "codd_amd", "csrc", "motion.hip")).read()
    return int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))


def test_fixture_keys_are_the_case_list():
    P.assert_keys(FIXTURE, P.all_keys(LC))
    assert re.fullmatch(r"[0-9a-f]{40}", FIXTURE["library_commit"])
    assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in FIXTURE["sha256"].values())


def test_instnorm_shapes_reach_every_trip_count_and_path():
    D = LC.STATS_DEPTH
    assert D == _source_define("IN_STATS_DEPTH")
    facts = {s: LC.inorm_parts(s[0], s[1], s[2] * s[3]) for s in LC.INORM_SHAPES}
    trips = {t for (_, t, _, _) in facts.values()}
    assert {1, D - 1, D, D + 1, 2 * D + 1} <= trips, trips
    assert {p for (p, _, _, _) in facts.values()} >= {1, 32}
    assert any(last < per for (parts, _, last, per) in facts.values() if parts > 1)  # a shorter last part
    assert facts[(1, 8, 288, 480)][:2] == (32, 17)
    hw = [s[2] * s[3] for s in LC.INORM_SHAPES]
    assert 1 in hw and (2, 64, 37, 61) in LC.INORM_SHAPES and (37 * 61) % 4
    assert any(s[1] == 8 for s in LC.INORM_SHAPES) and any(s[:2] == (2, 128) for s in LC.INORM_SHAPES)
    assert {s[4] for s in LC.INORM_PLANTED} == {"nan", "const"}
    assert len(LC.INORM_PLAIN) == 4 and len(LC.INORM_XS) == 12


def test_gn_cases_reach_every_group_count():
    Bt = LC.SOLVE_BATCH
    assert Bt == _source_define("GN_SOLVE_BATCH") and 27 <= 2 * Bt
    G = {c: LC.gn_groups(c) for c in LC.GN_CASES}
    assert set(G[(16, 24, 4, 0)][0]) == {1}
    assert len(set(G[(37, 61, 8, 0)][0])) > 1 and 37 % 8 and 61 % 8
    g, gmax = G[(72, 80, 32, 0)]
    assert gmax == 27 and max(g) == 27 and min(g) < 27
    g, gmax = G[(24, 40, 8, 16)]
    assert gmax == 36 and max(g) == 36 > 2 * Bt and any(Bt < v <= 2 * Bt for v in g)


def test_splat_geometries_hold_empty_sparse_and_crowded_pixels():
    for n, v in LC.splat_candidate_classes().items():  # (the case builder's own assertions run here too)
        print(n, "pixels with 0: %d, 1-7: %d, 8: %d, > 8 candidates: %d" % v)
    cnt = {n: LC.splat_candidate_counts(n) for n in LC.SPLAT_GEOMETRIES}
    assert (cnt["ds4r8"] > 2 * 8).mean() > 0.5
    band = (cnt["ds4r4shift"] == 0).all(axis=1)  # whole columns without a candidate, in every item
    assert band.any(axis=1).all() and band.sum() > cnt["ds4r4"].shape[0] * 2
    assert [v[1:3] for v in LC.SPLAT_VARIANTS if v[0] and not v[3]] == [(0, 0), (1, 0), (3, 2), (9, 0)]
    assert {v[0] for v in LC.SPLAT_VARIANTS} == {0, 1} and {v[3] for v in LC.SPLAT_VARIANTS} == {0, 1}
