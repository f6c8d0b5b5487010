"""The fp64 restatement of one RAFT3D update (tests/raft_loop_fp64.py) that tests/test_gpu_raft_loop_fp64.py holds the
product's loop against: pinned here to the fp32 CPU oracle (oracle.motion.raft3d(trace=)); its dense Gauss-Newton form
pinned to gn_fp64.gn_step; the deviations D that every bound constant is 4.3 x of re-measured (4 D <= constant <= 8 D);
the share of fragile pixels capped; and the power of the bounds -- each of nine planted wiring errors must exceed its
bound by 10 x on some traced quantity at some iteration >= 2.  CPU only; run with -s for the figures."""
import torch

import gn_fp64 as G
import raft_loop_fp64 as L
from oracle import motion as om

F64 = torch.float64


def test_dense_gn_equals_windowed():
    """gn_dense (all pairs, window mask) == gn_fp64.gn_step (row walk over the window) where the window is smaller
    than the map (radius 6 at 21x45: the mask cuts on every side) and at B = 2 where it holds the whole map."""
    for case in ((1, 21, 45, 6), (2, 9, 14, 32)):
        c = G.make_case(*case)
        ref = G.reference(c)
        got = L.gn_dense(c["T"], c["ae"] / 8.0, c["target"], c["weight"], c["d1"], c["K8"], radius=c["radius"], chunk=100)
        assert (got["dx"] - ref["dx"]).abs().max().item() <= 1e-12 * max(1.0, ref["dx"].abs().max().item())
        assert (got["T_new"] - ref["T_new"]).abs().max().item() <= 1e-12
        # (make_case's three pixels whose motion puts the near patch at Y.z = -0.05: 0.1 from the skip, seen by ``near``)
        assert (got["near"] < 0.15).sum().item() >= 3 and not L.fragile(got).all()
        rows = [0, c["T"].shape[1] // 2, c["T"].shape[1] - 1]  # (the row-restricted form the GPU test uses at 72x120)
        part = L.gn_dense(c["T"], c["ae"] / 8.0, c["target"], c["weight"], c["d1"], c["K8"], radius=c["radius"], chunk=7, rows=rows)
        assert all((part[k] - got[k][:, rows]).abs().max().item() <= 1e-12 for k in ("dx", "T_new", "near"))


def test_restatement_agrees_with_the_fp32_oracle_at_iteration_one():
    """loop64 and oracle.motion.raft3d(trace=) on the same weights and inputs: at iteration 1 (both start from the
    identity field and the same fp32 features) they agree to ORACLE_LEVEL = 4 x one fp32 evaluation's distance from
    the fp64 one: net 1.7e-4, weight 6e-6, T inside gn_fp64.TOL_ABS in the twist domain.  Later iterations: printed."""
    for name in L.SMALL_CASES:
        wd = L.oracle_world(name)
        x, B = wd["inp"], L.CASES[name][0]
        tr = []
        with torch.no_grad():
            om.raft3d(wd["sd"], "motion.raft3d", x["img_curr"], x["depth_prev"], x["depth_curr"],
                      torch.tensor([list(x["K"])] * B, dtype=torch.float32), dict(wd["state0"]), iters=x["iters"], trace=tr)
        for k, (o, t) in enumerate(zip(wd["traj"], tr)):
            d = L.deviation(dict(T=t["T"], net=t["net"], weight=t["weight"]), o)
            terr = G.twist_error(t["T"], o["T"]).max().item()
            print(f"case {name} iteration {k + 1}: oracle32 - loop64: net {d['net']:.3g}  weight {d['weight']:.3g}  "
                  f"T twist error {terr:.3g} (rel beyond TOL_ABS {d['T']:.3g})")
            if k == 0:
                assert d["net"] <= L.ORACLE_LEVEL["net"] and d["weight"] <= L.ORACLE_LEVEL["weight"], d
                assert d["T"] <= L.ORACLE_LEVEL["T_rel"] and terr <= G.TOL_ABS, (d, terr)


def _measure():
    """{mode: {q: D_q}} over D_CASES and iterations, along loop64's own trajectory."""
    D = {m: dict(net=0.0, weight=0.0, mask=0.0, T=0.0) for m in L.MODES}
    for name in L.D_CASES:
        wd = L.oracle_world(name)
        n = len(wd["traj"])
        with torch.no_grad():
            for k, o in enumerate(wd["traj"]):
                last = k == n - 1
                wT = o["T"] is not None
                s = L.deviation(L.step_full(wd["sd32"], wd["pre"], o["T_in"], o["net_in"], last, "f32", with_T=wT), o)
                for mode in L.MODES:
                    e = {q: 0.0 for q in s} if mode == "fp32" else \
                        L.deviation(L.step_full(wd["sd64"], wd["pre"], o["T_in"], o["net_in"], last, mode, with_T=wT), o)
                    for q in s:
                        D[mode][q] = max(D[mode][q], e[q] + s[q])
                    print(f"case {name} iteration {k + 1} {mode}: emulated {e}  fp32 {s}")
    return D


def test_constants_are_four_to_eight_times_the_measured_deviation():
    """D_q(mode) = worst |step_emulated(mode) - step64| + |step32 - step64| re-measured; 4 D <= BOUND <= 8 D, so a
    bound can neither be missed nor quietly loosened (fp32: the emulation IS step64, its term is 0)."""
    D = _measure()
    for mode in L.MODES:
        print(f"{mode}: D = {D[mode]}  BOUND = {L.BOUND[mode]}")
    for mode in L.MODES:
        for q, d in D[mode].items():
            assert 4.0 * d <= L.BOUND[mode][q] <= 8.0 * d, (mode, q, d, L.BOUND[mode][q])


def test_fragile_share_is_at_most_one_percent():
    """Pixels are left out of the T check only by the reference's own criterion, and at most 1 % per iteration."""
    for name in L.D_CASES:
        for k, o in enumerate(L.oracle_world(name)["traj"]):
            if o["fragile"] is None:  # (P's last iteration: no Gauss-Newton step in the reference, T not checked)
                continue
            share = o["fragile"].float().mean().item()
            print(f"case {name} iteration {k + 1}: fragile share {share:.3g}, |dx|_inf median "
                  f"{o['dx'].abs().amax(-1).median().item():.3g}")
            assert share <= L.FRAGILE_CAP, (name, k, share)


def test_power_every_planted_wiring_error_exceeds_its_bound_tenfold():
    """Each variant of raft_loop_fp64.VARIANTS, teacher-forced like the GPU test (the wrong step from loop64's own
    (T_k, net_k), with loop64's previous iteration as the stale state), against step64: on some traced quantity at some
    iteration >= 2 it is >= 10 x the bound of EVERY mode (the widest, split, decides)."""
    best = {v: 0.0 for v in L.VARIANTS}
    for name in L.SMALL_CASES:
        wd = L.oracle_world(name)
        n = len(wd["traj"])
        with torch.no_grad():
            for v in L.VARIANTS:
                for k in range(1, n):
                    last = k == n - 1
                    if v == "mask_prev" and not last:
                        continue
                    o = wd["traj"][k]
                    x = L.step_full(wd["sd64"], wd["pre"], o["T_in"], o["net_in"], last, "f64", v, wd["traj"][k - 1])
                    r = min((max(L.ratios(x, o, mode).values()) for mode in L.MODES))
                    rs = L.ratios(x, o, "split")
                    print(f"case {name} iteration {k + 1} variant {v}: err / bound (split) "
                          + "  ".join(f"{q} {val:.3g}" for q, val in rs.items()))
                    best[v] = max(best[v], r)
    print("power:", {v: round(b, 1) for v, b in best.items()})
    assert all(b >= 10.0 for b in best.values()), best
