"""CPU side of tests/pointwise_fp64.py: the project's fp32 oracle / restatement of every operation against the fp64
references on the GPU cases' inputs (the measurement that sets pointwise_fp64.C), the power of the bounds (wrong variants
must exceed them), the threshold clearance of the metric inputs (which lets the GPU test compare counts exactly, with no
excluded element), the tie measurement of the nearest warp against grid_sample's arithmetic, and the batch semantics of
the metric references.  No GPU needed."""
import functools
import os

import torch

import pointwise_fp64 as P
from oracle import ablation as oab

F64 = torch.float64


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _acc(acc, res):
    for k, v in res.items():
        acc[k] = max(acc.get(k, 0.0), v)


@functools.lru_cache(None)
def _case(case, kind="float"):
    return P.metrics_case(case, kind)


@functools.lru_cache(None)
def _oracle_figures():
    """{key of C: worst |oracle32 - ref64| / (2^-24 M)} over every case of the module, + the exact figures under
    "count" / "select" (0 or inf)."""
    _threads()
    acc = {}
    for (B, h, w) in P.GATE_CASES:
        d = P.gate_inputs(B, h, w)
        for summed in (False, True):
            zr32, rh32, h32 = P.gate_oracle32(d, summed)
            ref = P.gate_zr(d, summed)
            _acc(acc, {"gate_z": P.fig("z|r", zr32, *ref["gate_z"]), "gate_rh": P.fig("rh", rh32, *ref["gate_rh"])})
            _acc(acc, {"gate_q": P.fig("q", h32, *P.gate_q(d, zr32, summed))})
    for case in P.RESIZE_CASES:
        x, out0, extra = P.resize_inputs(case)
        for form in P.RESIZE_FORMS:
            ref = P.resize(x, case[4:6], case[6], form, out0, extra)
            _acc(acc, {"resize": P.fig("resize", P.resize_oracle32(x, case[4:6], case[6], form, out0, extra), *ref)})
    for n in P.ADD_RELU_N:
        g = P._gen(91, n)
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        for relu in (False, True):
            v = a + b
            _acc(acc, {"add_relu": P.fig("add_relu", torch.relu(v) if relu else v, *P.add_relu(a, b, relu))})
    for (B, h, w) in P.SPLIT_CASES:
        x = P.split_input(B, h, w)
        (net, Mn), (inp, Mi) = P.context_split(x)
        _acc(acc, {"ctx_tanh": P.fig("tanh", torch.tanh(x[:, :128]), net, Mn),
                   "select": P.fig("relu", torch.relu(x[:, 128:]), inp, Mi)})
    for case in P.SELECT_CASES:
        for K, (R, Q) in ((0.5, (1.0, 1.0)), (0.25, (3.0, 1.0))):
            cur, warp, gt = P.select_inputs(case, K)
            ref, Mg, _ = P.fusion_select("kalman", cur, warp, K=K)
            _acc(acc, {"kalman": P.fig("kalman", oab.kalman_fuse(cur, warp, R, Q), ref, Mg)})
            ref, Mg, _ = P.fusion_select("gt", cur, warp, gt)
            got = oab.gt_fuse(cur, warp, torch.nan_to_num(gt, nan=0.0))  # (torch.where(NaN > 0) is the same decision)
            _acc(acc, {"gt_avg": P.fig("gt", got, ref, Mg)})
    for case in P.GT_MOTION_CASES:
        a = P.gt_motion_inputs(case, "float")
        for i, (got, ref) in enumerate(zip(oab.gt_motion(a[0], a[1], a[2], a[3], a[4], a[5]), P.gt_motion(*a))):
            _acc(acc, {"select": P.fig(f"gt_motion[{i}]", got.reshape(ref.shape), ref.to(F64), torch.zeros_like(ref, dtype=F64))})
    for case in P.METRIC_CASES:
        d = _case(case)
        for um, ug in P.TEPE_VARIANTS:
            for uo in ((False, True) if (um, ug) == (False, False) else (True,)):
                rd, rt, rs = P.metrics_oracle32(d, um, ug, uo)
                _acc(acc, P.meter_figures("tepe", rt, *P.tepe_metrics(d, um, ug)))
                _acc(acc, P.meter_figures("sceneflow", rs, *P.sceneflow_metrics(d, uo)))
        _acc(acc, P.meter_figures("disp", rd, *P.disp_metrics(d)))
        _acc(acc, P.element_figures(d))
    return acc


def test_fp32_oracle_within_a_quarter_of_every_bound():
    """Worst |oracle32 - ref64| / (2^-24 M) per figure over every case of pointwise_fp64: the figures of MEASURED
    (printed), each at most c / 4; the exact figures (selections, counts, the gt_motion outputs) agree exactly.  The warps
    and the metrics are pinned on the non-tie flow kind only (the restatement samples through grid_sample)."""
    acc = dict(_oracle_figures())
    exact = {k: acc.pop(k) for k in ("count", "select")}
    print("measured:", {k: float(f"{v:.3g}") for k, v in acc.items()})
    print("c / 4   :", {k: P.C[k] / 4 for k in acc})
    assert exact == {"count": 0.0, "select": 0.0}, exact
    P.within(acc, 0.25, "fp32 oracle")
    assert set(acc) == set(P.C) == set(P.MEASURED)
    for k, v in acc.items():
        assert abs(v - P.MEASURED[k]) <= 0.03 * v, (k, v, P.MEASURED[k])
        assert 4 * P.MEASURED[k] <= P.C[k] <= 4 * P.MEASURED[k] * 1.07, k


def _over(name, v):
    print(f"{name}: worst err / bound {v:.3g}")
    assert v > 1.0, (name, v)


def test_power_of_the_bounds():
    """Each wrong variant, evaluated in fp64, exceeds its bound (c 2^-24 M; any difference where M = 0)."""
    _threads()
    d = P.gate_inputs(*P.GATE_CASES[1])
    ref = P.gate_zr(d)
    bad = P.gate_zr(d, variant="swap_zr")
    _over("gates: z and r halves swapped", P.fig("", bad["gate_z"][0], *ref["gate_z"]) / P.C["gate_z"])
    _over("gates: r h from the z half", P.fig("", bad["gate_rh"][0], *ref["gate_rh"]) / P.C["gate_rh"])
    zr = ref["gate_z"][0]
    q, Mq = P.gate_q(d, zr)
    _over("gates: inp read at the wrong 128-channel block", P.fig("", P.gate_q(d, zr, variant="q_block")[0], q, Mq) / P.C["gate_q"])
    _over("gates: z and 1 - z exchanged", P.fig("", P.gate_q(d, zr, variant="blend_swap")[0], q, Mq) / P.C["gate_q"])
    for case in (P.RESIZE_CASES[0], P.RESIZE_CASES[5], P.RESIZE_CASES[6], P.RESIZE_CASES[7]):
        x, out0, extra = P.resize_inputs(case)
        ref = P.resize(x, case[4:6], case[6])
        _over(f"resize {P.case_id(case)}: align_corners exchanged",
              P.fig("", P.resize(x, case[4:6], case[6], variant="ac_swap")[0], *ref) / P.C["resize"])
        if not case[6]:
            _over(f"resize {P.case_id(case)}: half-pixel offset dropped",
                  P.fig("", P.resize(x, case[4:6], case[6], variant="no_half")[0], *ref) / P.C["resize"])
    for case in P.METRIC_CASES[:2]:
        d = _case(case)
        for kind, fn in (("disp", P.disp_metrics), ("tepe", P.tepe_metrics), ("sceneflow", P.sceneflow_metrics)):
            ref = fn(d)
            _over(f"{kind} {P.case_id(case)}: >= at a threshold", P.meter_figures(kind, fn(d, variant="ge")[0], *ref)["count"])
        for kind, fn, key in (("disp", P.disp_metrics, "disp_epe"), ("tepe", P.tepe_metrics, "tepe")):
            ref = fn(d)
            _over(f"{kind} {P.case_id(case)}: mean over the crop",
                  P.meter_figures(kind, fn(d, variant="crop_mean")[0], *ref)[key] / P.C[key])
        ref = P.tepe_metrics(d)
        res = P.meter_figures("tepe", P.tepe_metrics(d, variant="mask_unwarped")[0], *ref)
        _over(f"tepe {P.case_id(case)}: warped mask at the un-warped position", max(res["tepe"] / P.C["tepe"], res["count"]))
    for case in P.GT_MOTION_CASES:
        a = P.gt_motion_inputs(case, "float")
        ref, bad = P.gt_motion(*a)[1], P.gt_motion(*a, variant="quarter_scale")[1]
        _over(f"gt_motion {P.case_id(case)}: quarter-resolution flow scaled by 1/4",
              P.fig("", bad, ref.to(F64), torch.zeros_like(ref, dtype=F64)))


def test_metric_inputs_clear_every_threshold():
    """Away from the planted pixels every thresholded quantity of the fp64 reference is farther from its threshold than
    2 x 64 x 2^-24 M (any c up to 64; every C of a metric figure is far below) for all flow kinds, the plants are there,
    and the fp32 restatement agrees with the reference on every count -- so the GPU test compares counts exactly."""
    _threads()
    assert max(P.C[k] for k in ("disp_epe", "tepe", "tepe_rel", "sf_epe3", "sf_epe2")) <= P.CLEAR_C
    for case in P.METRIC_CASES:
        for kind in P.FLOW_KINDS:
            d = _case(case, kind)
            bad1, bad0 = P.threshold_violations(d)
            print(f"{P.case_id(case)} {kind}: {d['cleared']} pixels invalidated by clear_thresholds, {int(bad1.sum() + bad0.sum())} left")
            assert not bad1.any() and not bad0.any()
        d = _case(case)
        B, H, W, h, w = case
        if h * w >= 16:  # (the plants of a smaller crop overwrite each other)
            t = P.tepe_elems(d)
            m, err, _ = P.disp_elems(d)
            pl = P._crop(d["plant"], h, w)
            assert (err[pl & m] == P.THR).sum() == 2 and (t["te"][pl & t["mask"]] == 3.0).sum() >= 1
            assert (t["rel"][pl & t["mask"]] == 1.0).sum() == 1 and (t["mag"][pl] == P.BF).sum() == 1
        for um, ug in P.TEPE_VARIANTS:
            rd, rt, rs = P.metrics_oracle32(d, um, ug, True)
            assert P.meter_figures("tepe", rt, *P.tepe_metrics(d, um, ug))["count"] == 0.0, (case, um, ug)
        assert P.meter_figures("disp", rd, *P.disp_metrics(d))["count"] == 0.0
        assert P.meter_figures("sceneflow", rs, *P.sceneflow_metrics(d))["count"] == 0.0


def _tie_shares(flow):
    """(share of pixels whose source pixel or in-bounds decision differs between metrics.flow_warp_nearest and the
    exact rule, the same outside exact half-integer coordinates)."""
    B, _, h, w = flow.shape
    sy, sx, inside = P.warp_source(flow, h, w)
    idx, valid = P.grid_sample_source(flow)
    differ = (inside != valid) | (inside & valid & (idx != sy * w + sx))
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    cx, cy = xx[None] + flow[:, 0], yy[None] + flow[:, 1]
    half = ((cx - cx.floor()) == 0.5) | ((cy - cy.floor()) == 0.5)
    return differ.double().mean().item(), (differ & ~half).double().mean().item()


def test_nearest_warp_ties_against_grid_sample():
    """The kernels' rule rint(float32(x) + fx) against the reference's grid_sample arithmetic (normalise, un-normalise,
    nearbyint): they part only at exact half-integer coordinates (or within an ulp of one).  Measured and printed: the
    share of differing pixels per flow kind and size, and what it does to the four TEPE columns of a metrics case.
    Asserted: under 1 % for 1/64-px flows; at most 1e-5 outside exact half-integers.  Nothing is excluded from any GPU
    comparison on account of this: the GPU tests hold the kernels to the exact rule on all three kinds."""
    _threads()
    for (h, w) in ((60, 90), (37, 61), (375, 1242)):
        g = P._gen(95, h, w)
        for kind in P.FLOW_KINDS:
            share, off_half = _tie_shares(P.flows(kind, 1, h, w, h, w, g))
            print(f"{h}x{w} {kind}: {share:.3%} of the pixels differ, {off_half:.2e} outside exact half-integer coordinates")
            assert off_half <= 1e-5, (h, w, kind, off_half)
            if kind == "q64":
                assert share < 0.01
            if kind == "half":
                assert share > 0.01  # (the measurement does reach the ties)
    for kind in ("q64", "half"):
        d = _case(P.METRIC_CASES[0], kind)
        ref, got = P.tepe_metrics(d)[0], P.metrics_oracle32(d)[1]
        print(f"tepe columns, {kind} flows: exact rule {[float(f'{v:.6g}') for v in ref[0, :4]]}, "
              f"grid_sample {[float(f'{v:.6g}') for v in got[0, :4]]}")


def test_a_batch_is_B_frames_in_index_order():
    """The references treat a batch of B as B frames: item b of a B = 2 call equals the B = 1 call on that item, and an
    item whose mask is empty adds nothing -- neither a mean nor a count."""
    _threads()
    case = P.METRIC_CASES[3]
    d = P.metrics_case(case, empty_item=0)
    for fn in (P.disp_metrics, P.tepe_metrics, P.sceneflow_metrics):
        rows, Ms = fn(d)
        for b in range(case[0]):
            r1, M1 = fn(P.metrics_item(d, b))
            assert torch.equal(rows[b], r1[0]) and torch.equal(Ms[b], M1[0]), (fn.__name__, b)
    assert P.disp_metrics(d)[0][0].abs().sum() == 0 and P.disp_metrics(d)[0][1, 2] == 1
    t = P.tepe_metrics(d)[0]
    assert t[0, :5].abs().sum() == 0 and t[0, 6] == 1 and t[1, 4] == 1  # (|flow| is a mean over the crop: every item counts)
    assert P.sceneflow_metrics(d)[0][0].abs().sum() == 0
