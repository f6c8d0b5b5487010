"""The fp64 module restatement of RAFT3D's context network (tests/context_net_fp64.py) on the CPU: (1) its fp32 twin, the
same modules over the oracle's own functions, chained, IS oracle.hrnet.hrnet / cnet bit for bit; (2) the running bound
holds for independent fp32 evaluations -- the oracle, on the host's threads and on one, and K32S, a sequential fp32
evaluation with a fixed order of operations -- on every case, module and output element, and K32S's worst err / bound
per module equals the committed MEASURED table (a measurement, asserted only as <= 1 and to re-measure within 3 %;
the oracle's own figures follow the host's convolution library and thread count and are printed beside it); (3) power: every planted wiring error moves at least one element
of every module it touches by more than 10 x the bound, on every case; (4) the gap this closes: the global figure of
test_gpu_motion_ops.py::test_fnet_cnet_update_block, max |got - ref| / max |ref| < 2e-4 over the network's 512 output
channels, for each variant chained from the image; (5) hrnet.packed_cbn's fold restated in fp32 against unfolded fp64
on planted BatchNorm channels, inside the derived FOLD.

(4), measured on T and on B (128 x 192, the old test's shape): ``bn_eps0`` gives 9.8e-5 / 1.0e-4, a factor 2 under the
old figure (the network carries the 5e-6 it puts on every s up to 1e-4 of the output), and ``split_at_256`` gives 0
(context_split lies behind the tensor the old test reads); every other variant is far above 2e-4 (the smallest:
fuse_align_true 0.10, head_align_false 0.14, down_on_block1 0.15).  So at these weights the old figure does see each
planted error of the fuse sums -- none of them slips under it, and none was constructed to --; what it cannot see is
a relative error of 1e-4 and below (1e-5 was the size that flipped pixels in the splat) and anything behind the head.
bn_eps0 stays below the network-level bound as well (context_net_fp64's docstring) and is caught on the planted
channels of the fold case; the accumulated bound of the free-running network is of no use at all (the oracle sits at
1e-48 .. 1e-52 of it): what holds the network is the teacher-forced bound of every module.
Run with -s for the figures."""
import functools

import pytest
import torch

import context_net_fp64 as N
from oracle import hrnet as ohr

F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _measured():
    return N.measure()


@pytest.mark.parametrize("name", list(N.CASES))
def test_modules_chained_over_k32_are_the_fp32_oracle_bit_for_bit(name):
    w = N.oracle_world(name)
    sd = N.estimator()[1]
    with torch.no_grad():
        ys, out = ohr.hrnet(sd, N.H, w["image"]), ohr.cnet(sd, N.P, w["image"])
    B, Hh, W = N.CASES[name]
    assert [tuple(y.shape) for y in ys] == [(B, c, Hh >> (2 + i), W >> (2 + i)) for i, c in enumerate((18, 36, 72, 144))]
    assert all(torch.equal(a, b) for a, b in zip(ys, w["T32"]["stage4.1"]))
    assert torch.equal(out, w["T32"]["head"][0]) and out.shape == (B, 512, Hh >> 3, W >> 3)
    for m in N.STAGE_MODULES:  # the fuse layers alone, from the trajectory's branch outputs, are the module's outputs
        assert all(torch.equal(a, b) for a, b in zip(w["T32"][m], w["T32"][m + ".fuse"])), m


def test_bound_holds_for_the_fp32_oracle_and_matches_the_measured_table():
    """The re-measured table is that of K32S, whose order of operations is fixed.  Its figures still depend on the CPU:
    single modules were seen to move by up to 19 % on another CPU model (layer1.1 0.000548 for 0.000459, split 0.146
    for 0.175; every figure <= 1), the oracle's own by up to 2 x (T head 0.024 for 0.055).  Not established why --
    candidates are the vectorised fp32 sin / cos that build the synthetic frames and tanh."""
    tab, per = _measured()
    for m in N.MODULES:
        cases = "  ".join(f"{n} {' / '.join('%.3g' % per[(n, ev, m)] for ev in ('seq', 'oracle', 'oracle/1'))}" for n in N.CASES)
        print(f"err / bound  {m:14s} worst {tab[m]:.3g}  (committed {N.MEASURED[m]:.3g})   K32S / oracle / oracle on 1 thread: {cases}")
    assert set(tab) == set(N.MEASURED) == set(N.MODULES)
    assert len(per) == 3 * len(N.CASES) * len(N.MODULES)
    assert all(v <= 1.0 for v in per.values()), {k: v for k, v in per.items() if not v <= 1.0}
    bad = {m: (v, N.MEASURED[m]) for m, v in tab.items() if not 0.97 * N.MEASURED[m] <= v <= 1.03 * N.MEASURED[m]}
    assert not bad, bad


@pytest.mark.parametrize("name", list(N.CASES))
def test_report_restatement_chained_against_the_oracle_and_the_accumulated_bound(name):
    """Free running from the image: the bound carried through the whole network.  A REPORT: the oracle sits at 1e-48 ..
    1e-52 of it, so the <= 1 below cannot fail; the live figure is the global one against the fp64 chain."""
    w = N.oracle_world(name)
    with torch.no_grad():
        R = N.evaluate(N.K64, N.weights(F64), w["image"])
    worst = {m: N.worst(w["T32"][m], R[m]) for m in ("stage4.1", "head", "split")}
    print(f"{name}: free-running oracle err / accumulated bound: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    glob = (w["T32"]["head"][0].double() - R["head"][0].v).abs().max().item() / R["head"][0].v.abs().max().item()
    print(f"{name}: max |oracle - fp64| / max |fp64| over the head's output = {glob:.3g}")
    assert glob < 2e-5  # (one fp32 evaluation of the network against fp64: 1e-6 measured; the old test allows 2e-4)


@pytest.mark.parametrize("variant", list(N.VARIANTS))
def test_planted_wiring_error_exceeds_ten_times_the_bound(variant):
    if variant == "bn_eps0":  # (the path on which eps matters: var << eps, context_net_fp64's docstring)
        for bias in (False, True):
            case = N.fold_case(bias)
            r = N.ratio(N.fold_ref(case, variant).v, N.fold_ref(case))
            per = [r[:, c].max().item() for c in range(8)]
            print(f"bn_eps0 on the planted channels (bias={bias}): err / bound per channel " + " ".join(f"{v:.3g}" for v in per))
            assert per[0] > 10.0 and max(per[1:]) <= 1.0, per  # var = 1e-12 is the channel that sees it
        return
    for name in N.CASES:
        fac = {m: N.power(name, variant, m) for m in N.VARIANTS[variant]}
        print(f"{variant} on {name}: exceeds the bound by  " + "  ".join(f"{m} {v:.3g}x" for m, v in fac.items()))
        assert fac and all(v > 10.0 for v in fac.values()), (variant, name, fac)


def test_the_old_global_figure_on_the_planted_variants():
    """max |variant - restatement| / max |restatement| over the head's 512 channels, both chained in fp64 from the image
    (the figure test_fnet_cnet_update_block holds below 2e-4); module docstring (4)."""
    figs = {}
    for name in ("T", "B"):
        image = N.inputs(name)
        with torch.no_grad():
            ref = N.evaluate(N.K64, N.weights(F64), image)
            for variant in N.VARIANTS:
                R = N.evaluate(N.K64, N.weights(F64), image, variant=variant)
                figs[(variant, name)] = max(
                    (R[m][i].v - ref[m][i].v).abs().max().item() / ref[m][i].v.abs().max().item()
                    for m, i in (("head", 0),))
                behind = max((a.v - b.v).abs().max().item() for a, b in zip(R["split"], ref["split"]))
                print(f"old figure  {variant:22s} {name}: {figs[(variant, name)]:.3g}   (behind the head: {behind:.3g})")
    under = sorted({v for (v, n), f in figs.items() if f < 2e-4})
    assert under == ["bn_eps0", "split_at_256"], under
    assert all(5e-5 < figs[("bn_eps0", n)] < 2e-4 and figs[("split_at_256", n)] == 0.0 for n in ("T", "B"))
    assert min(f for (v, n), f in figs.items() if v not in under) > 0.05


@pytest.mark.parametrize("bias", [False, True])
def test_fold_arithmetic_in_fp32_stays_inside_the_derived_constant(bias):
    worst = 0.0
    for stats in (0, 1):
        case = N.fold_case(bias, stats)
        fig, ref, M = N.fold_figure(case)
        per = [fig[:, c].max().item() for c in range(8)]
        print(f"fold (bias={bias}, stats={stats}): |folded - unfolded| / (2^-24 M) per channel " +
              " ".join(f"{v:.3g}" for v in per) + f"   (FOLD = {N.FOLD})")
        worst = max(worst, max(per))
        sd = case["sd"]
        s = (sd["b.weight"].double() / torch.sqrt(sd["b.running_var"].double() + 1e-5))
        assert 300 < abs(s[0] / sd["b.weight"][0].double()) < 320 and s[1] < 0 and s[2] == 0  # the planted channels
        assert (ref[:, 2] == sd["b.bias"][2].double()).all()  # gamma = 0: the output is beta
        big = (sd["b.running_mean"].double() * s)[3].abs()
        inner = ref[:, 3, 1:-1, 1:-1].abs().mean()  # (the zero-padded border rows reach 4/9 or 6/9 of the mean only)
        assert 300 < big / inner < 3000, big / inner  # the bias cancels against the convolution
    assert worst <= N.FOLD, worst
