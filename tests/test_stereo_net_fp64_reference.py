"""The fp64 stage restatement of the stereo network (tests/stereo_net_fp64.py) on the CPU: (1) its fp32 twin, the same
stages over the oracle's own functions, chained, IS oracle.stereo.stereo_matching bit for bit; (2) the fp64 stages,
chained, agree with the oracle at the level of one fp32 evaluation (ORACLE_LEVEL), with every arg-min and select equal;
(3) the measurement that sets every constant: D re-measured, 4 D <= BOUND <= 8 D; (4) the reference-alone near-tie and
near-select counts stay within the cap; (5) power: each of eleven planted wiring errors, written as a variant of the
restatement and teacher-forced like the product, exceeds a bound or produces un-excused arg-min / select differences.
Run with -s for the figures."""
import functools

import pytest
import torch

import stereo_fusion_fp64 as SF
import stereo_net_fp64 as N
from oracle import stereo as ost

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _measured():
    return N.measure()


@pytest.mark.parametrize("name", list(N.CASES))
def test_stage32_chained_is_the_fp32_oracle_bit_for_bit(name):
    w = N.oracle_world(name)
    B = w["left"].shape[0]
    with torch.no_grad():
        ref = ost.stereo_matching(N.estimator()[1], w["left"], w["right"], max_disp=N.MAX_DISP, return_intermediates=True)
    T = w["T32"]
    assert torch.equal(T["pred_disp"], ref["pred_disp"])
    for i in range(5):
        assert torch.equal(T[f"fea{i}"][:B], ref["fea_l"][i]) and torch.equal(T[f"fea{i}"][B:], ref["fea_r"][i]), i
        assert torch.equal(T[f"init{i}.hyp"], ref["init"][i]), i
    assert torch.equal(T["fea2"][:B], ref["left_feat"]) and torch.equal(T["fea2"][B:], ref["right_feat"])


def _level_of(q, g):
    if q.startswith(("enc", "fea")):
        return "unet"
    if q.startswith("init"):
        return "init"
    if q == "pred_disp":
        return q
    if q.endswith((".aug", ".upd")):
        return None  # (inner quantities of the update: held by the teacher-forced bounds)
    kind = "upd" if q.startswith("upd") else "post"
    return kind + ("_d" if g == "d" else "_sf")


@pytest.mark.parametrize("name", list(N.CASES))
def test_restatement_chained_agrees_with_the_fp32_oracle(name):
    """Free running from the same images: fp64 stages against the oracle's trajectory."""
    w = N.oracle_world(name)
    with torch.no_grad():
        R = N.evaluate(N.K64, N.weights(F64), w["left"], w["right"])
    T = w["T32"]
    worst = {}
    for lvl in range(5):
        assert torch.equal(R[f"init{lvl}.hyp"][:, :3].float(), T[f"init{lvl}.hyp"][:, :3]), (name, lvl, "arg-min")
        if lvl:
            u = T[f"upd{lvl}.upd"]
            assert torch.equal(R[f"_upd{lvl}.sel"], u[:, 1:2] > u[:, 0:1]), (name, lvl, "select")
    for q in N.quantities():
        ref, x = R[q], T[N.traced_name(q)].to(F64)
        for g, sl in N.groups(q, ref.shape[1]):
            key = _level_of(q, g)
            if key is not None:
                worst[key] = max(worst.get(key, 0.0), (x[:, sl] - ref[:, sl]).abs().max().item())
    print(f"{name}: fp64 chain - fp32 oracle: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert set(worst) == set(N.ORACLE_LEVEL)
    assert all(v <= N.ORACLE_LEVEL[k] for k, v in worst.items()), (name, worst)


def test_constants_are_four_to_eight_times_the_measured_deviation():
    D, infos = _measured()
    assert set(D) == set(N.BOUND) == set(N.MEASURED), set(D) ^ set(N.BOUND)
    for k, v in D.items():
        print(f"D[{k}] = {v:.3g}   shipped: measured {N.MEASURED[k]:.3g}, bound {N.BOUND[k]:.3g}")
    bad = {k: (v, N.BOUND[k]) for k, v in D.items() if not 4 * v <= N.BOUND[k] <= 8 * v}
    assert not bad, bad
    for name, info in infos.items():  # the oracle takes every arg-min and every select as the fp64 stages do
        assert all(c["wrong"] == 0 for c in info["argmin"].values()), (name, info["argmin"])
        assert all(s[1] == 0 for s in info["select"].values()), (name, info["select"])


@pytest.mark.parametrize("name", list(N.CASES))
def test_reference_alone_near_ties_and_near_selects_within_the_cap(name):
    w = N.oracle_world(name)
    R = w["R64"]
    near, ties, tiles = 0, 0, 0
    for lvl in range(5):
        ref = R[f"_init{lvl}.full"]
        n = ref["arg"].numel()
        near += round(SF.near_tie_share(ref, SF.C["costvol"]) * n)
        ties += int(ref["tied"].sum())
        tiles += n
    assert tiles == N.tiles(name)
    sel = [N.near_select_count(R, i, N.BOUND[f"upd{i}.upd:conf"]) for i in range(1, 5)]
    excused_a = sum(round(c["near"] * R[f"init{l}.cost"].numel()) for l, c in N.deviations(w["T32"], R)[1]["argmin"].items())
    print(f"{name}: arg-min near ties {near} of {tiles} (cap {N.excuse_cap(tiles)}), exact ties {ties}; near selects per "
          f"level {sel} of {N.tiles(name, 1)} (cap {N.excuse_cap(N.tiles(name, 1))}); the oracle used {excused_a} excuses")
    assert ties > 0  # (the zero-padded region: the first-index rule is exercised)
    assert near <= N.excuse_cap(tiles) and excused_a <= N.excuse_cap(tiles)
    assert sum(sel) <= N.excuse_cap(N.tiles(name, 1))


@pytest.mark.parametrize("variant", N.VARIANTS)
def test_planted_wiring_error_exceeds_a_bound(variant):
    """The variant's stages, evaluated from the oracle trajectory's inputs as the product's are from its own trace, held
    against the fp64 stages under BOUND and the two rules: caught on at least one case."""
    caught = {}
    for name in N.CASES:
        w = N.oracle_world(name)
        with torch.no_grad():
            got = N.evaluate(N.K64, N.weights(F64), w["left"], w["right"], w["T32"], variant)
        got = {k: v for k, v in got.items() if not k.startswith("_")}
        dev, info = N.deviations(got, w["R64"])
        r = N.ratios(dev)
        over = {k: v for k, v in r.items() if v > 1.0}
        if over:
            k = max(over, key=over.get)
            caught[name] = (k, over[k], len(over))
            break
    print(f"{variant}: caught on {caught}")
    assert caught, variant
