"""The RAFT3D update loop of the product (RAFT3D.forward + BasicUpdateBlock.run / _heads, traced through
``forward(..., trace=[])``) against the fp64 restatement of one update (tests/raft_loop_fp64.py), TEACHER-FORCED: the
fp64 step from the product's own (T_k, net_k) against the product's entry k + 1, so no error accumulates and the bounds
are as sharp as the kernel tests' (raft_loop_fp64.BOUND: c x the reference's own deviation, set and re-measured on the
CPU by tests/test_raft_loop_fp64_reference.py, never from GPU output).  Cases A (24x40, 4 iterations), B (16x32, B = 2,
3 iterations) and P (72x120, the benchmarked map, 2 iterations) under split, fp32 and split16; on A under split also
the wirings FUSE_GATES = False and MERGE_ENC_HEADS = False.  net, weight and the last mask are checked at every
iteration of every case; T at every iteration of A and B.  P checks T against fp64 at its last iteration on the map rows
P_ROWS only (first, two middle, last: the whole 72x120 fp64 Gauss-Newton step takes 22 s on the host, four rows of it
3 s) and covers the rest of its T through the schedule tests below.

The loop's INPUTS are not taken on trust: after every run the first trace entry is held to values formed from the test's
own inputs -- d1, d2 bit-equal to depth[:, 3::8, 3::8], K8 == float32(K) / float32(8), fmap_prev bit-equal to the stored
feature map, inp bit-equal to relu and net within pointwise_fp64's tanh bound of the stored context output -- so a
wrong sub-sampling, K for K / 8 or swapped context parts in front of the trace point fails here.

Final outputs: outputs["Ts"] / ["weight"] / ["flow2d_est_induced"] against motion_fp64.upsample_se3 / cvx /
induced_flow of the traced last T, weight and mask, under those kernels' own bounds (motion_fp64.C).

Schedule and state invariance (bit comparisons of the whole trace and the outputs; A in all three modes, P under
split): serial against forked launches; with RAFT3D.prefetch against without; the same frame twice; the same frame
after another shape and another precision mode ran on the module, against a fresh module; with the interior of every
persistent buffer of the update block set to NaN before the run.  After every run the borders and the channel padding
of every split buffer the update block owns are still zero.  Autotune off throughout.  Run with -s for the figures."""
import functools
import os

import numpy as np
import pytest
import torch

import motion_fp64 as M
import pointwise_fp64 as PW
import raft_loop_fp64 as L
from oracle import se3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SUMMARY = {}
CASE_MODES = [(c, m) for c in ("A", "B", "P") for m in L.MODES]
SCHEDULE = [("A", m) for m in L.MODES] + [("P", "split")]
P_ROWS = [0, 35, 36, 71]
ids = dict(ids=lambda cm: f"{cm[0]}_{cm[1]}")


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 16)))


def _fresh():
    import codd_amd  # noqa: F401
    from codd_amd import configs, synth
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd(iters=4)).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    return est.to(DEV)


@functools.lru_cache(maxsize=None)
def _est():
    return _fresh()


@functools.lru_cache(maxsize=None)
def _sd64():
    return L.sd_of(L.estimator()[1], F64)  # (the same deterministic filler as _fresh)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return L.inputs(name)


class _mode:
    """Conv precision ``mode`` with autotune off; optionally the A/B switches of codd_amd.motion and Fork.serial."""

    def __init__(self, mode, serial=False, **switches):
        self.mode, self.serial, self.switches = mode, serial, switches

    def __enter__(self):
        from codd_amd import motion, ops
        self.prev_auto = ops._AUTOTUNE
        ops.enable_autotune(False)
        self.prev = ops.set_conv_precision(self.mode)
        self.prev_serial, ops.Fork.serial = ops.Fork.serial, self.serial
        self.prev_sw = {k: getattr(motion, k) for k in self.switches}
        for k, v in self.switches.items():
            setattr(motion, k, v)

    def __exit__(self, *exc):
        from codd_amd import motion, ops
        for k, v in self.prev_sw.items():
            setattr(motion, k, v)
        ops.Fork.serial = self.prev_serial
        ops.set_conv_precision(self.prev)
        ops.enable_autotune(self.prev_auto)
        return False


def _owned(ub):
    from codd_amd import ops
    sp = [st for k, st in ops._SPLIT_BUFFERS.items() if isinstance(k[0], tuple) and k[0][0] == id(ub)]
    c4 = [t for k, t in ops._C4_BUFFERS.items() if isinstance(k[0], tuple) and k[0][0] == id(ub)]
    return sp, c4


def _records(st):
    """The int16 view [B][plane][octet][hp][wp][8] of a SplitTensor (include/codd_hip.h, codd_split_bf16)."""
    planes = 2 if st.terms in (3, 48) else 1
    assert st.buf.numel() == st.B * planes * st.c8 * st.hp * st.wp * 16
    return st.buf.view(torch.int16).view(st.B, planes, st.c8, st.hp, st.wp, 8)


def _interior(st, v):
    """(full octets, the partial octet or None) of the image interior of the record view ``v``."""
    ys, xs = slice(st.bt, st.bt + st.H), slice(st.bl, st.bl + st.W)
    full = v[:, :, :st.C // 8, ys, xs, :]
    part = v[:, :, st.C // 8, ys, xs, :st.C % 8] if st.C % 8 else None
    return full, part


def _assert_borders_zero(ub, what):
    sp, _ = _owned(ub)
    assert sp or what[1] == "fp32", what  # (the exact-fp32 mode has no record tensors)
    for st in sp:
        v = _records(st).clone()
        for part in _interior(st, v):
            if part is not None:
                part.zero_()
        assert not v.any().item(), (what, "border or channel padding of a split buffer written", st.C, st.H, st.W, st.bt)


def _poison(ub):
    """NaN into the interior of every persistent buffer of the update block (records: the 16-bit NaN of the format)."""
    sp, c4 = _owned(ub)
    for st in sp:
        nan16 = 0x7E00 if st.terms in (16, 48) else 0x7FC0
        for part in _interior(st, _records(st)):
            if part is not None:
                part.fill_(nan16)
    for t in c4:
        t.buf.fill_(float("nan"))
    return len(sp), len(c4)


def _run(est, name, mode, prefetch=False, serial=False, item=None, first=None, poison=False, **switches):
    """The product on case ``name``: raft3d on the previous image with an empty state (fills raft_feat / raft_netinp),
    then on the current image with the two depth maps and trace=[] -> dict(trace, out, first) on the host.  ``item``:
    that batch item alone (B = 1); ``first``: the (raft_feat, raft_netinp) of an earlier run instead of the first call."""
    x = _inputs(name)
    sl = slice(None) if item is None else slice(item, item + 1)
    g = lambda k: x[k][sl].contiguous().to(DEV)
    r3 = est.motion.raft3d
    ub = r3.update_block
    with _mode(mode, serial, **switches), torch.no_grad():
        if first is None:
            st = {}
            r3(g("img_prev"), None, None, None, st, {})
            first = (st["raft_feat"], st["raft_netinp"])
        state = dict(raft_feat=first[0], raft_netinp=first[1], memory=[])
        if poison:
            torch.cuda.synchronize()
            n = _poison(ub)
            assert n[0] > 0 or mode == "fp32", n
        from codd_amd import ops
        img = g("img_curr")
        side = None
        if prefetch:
            r3.prefetch(img, state)
            pend = r3._pending
            assert pend is not None and "pyr" in pend and "pre" in pend and "fmap" in pend, "the side-stream path was not taken"
            side = dict(fmap=pend["fmap"], net=pend["pre"]["net"], inp=pend["pre"]["inp"])
        # forward builds the pyramid and splits the context itself exactly when no side-stream result is accepted
        calls = dict(allpairs_corr=0, context_split=0)
        orig = {k: getattr(ops, k) for k in calls}

        def counted(k):
            def f(*a, **kw):
                calls[k] += 1
                return orig[k](*a, **kw)
            return f
        out, tr = {}, []
        try:
            for k in calls:
                setattr(ops, k, counted(k))
            r3(img, g("depth_prev"), g("depth_curr"), list(x["K"]), state, out, iters=x["iters"], trace=tr)
        finally:
            for k in calls:
                setattr(ops, k, orig[k])
        torch.cuda.synchronize()
        want = 0 if prefetch else 1
        assert calls == dict(allpairs_corr=want, context_split=want), (prefetch, calls)
        if prefetch:
            assert "pre" not in r3._pending and "pyr" not in r3._pending, "pre / pyr were not consumed"
            torch.cuda.synchronize()
            assert torch.equal(tr[0]["fmap_curr"], side["fmap"]) and torch.equal(tr[0]["net"], side["net"]) and \
                torch.equal(tr[0]["inp"], side["inp"]), "forward did not use the side streams' tensors"
        _assert_borders_zero(ub, (name, mode))
    assert len(tr) == x["iters"] + 1 and "mask" in tr[-1] and all("mask" not in e for e in tr[1:-1])
    host = lambda d: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}
    run = dict(trace=[host(e) for e in tr], out=host(out), first=first)
    _check_loop_inputs(run["trace"][0], x, sl, first, (name, mode))
    return run


def _check_loop_inputs(e0, x, sl, first, what):
    """The first trace entry against values formed from the test's own inputs (module docstring)."""
    assert torch.equal(e0["d1"], x["depth_prev"][sl][:, 3::8, 3::8]), (what, "d1")
    assert torch.equal(e0["d2"], x["depth_curr"][sl][:, 3::8, 3::8]), (what, "d2")
    assert not torch.equal(e0["d1"], e0["d2"])
    assert list(e0["K8"]) == [float(np.float32(v) / np.float32(8.0)) for v in x["K"]], (what, e0["K8"])
    assert torch.equal(e0["fmap_prev"], first[0].cpu()), (what, "fmap_prev")
    ni = first[1].cpu()
    assert ni.shape[1] == 512 and e0["net"].shape[1] == 128 and e0["inp"].shape[1] == 384
    (rn, Mn), (ri, _) = PW.context_split(ni)
    assert torch.equal(e0["inp"], ri.float()), (what, "inp != relu(net_inp[:, 128:])")
    fig = PW.fig("tanh", e0["net"], rn, Mn)
    assert fig <= PW.C["ctx_tanh"], (what, "net != tanh(net_inp[:, :128])", fig)


def _same_bits(a, b):
    """Every traced tensor and every output of two runs is bit-equal -> list of the names that are not."""
    bad = []
    for i, (ea, eb) in enumerate(zip(a["trace"], b["trace"])):
        for k in ea:
            if torch.is_tensor(ea[k]) and not torch.equal(ea[k].view(torch.int32), eb[k].view(torch.int32)):
                bad.append(f"trace[{i}].{k}")
    for k in ("Ts", "weight", "flow2d_est_induced"):
        if not torch.equal(a["out"][k].view(torch.int32), b["out"][k].view(torch.int32)):
            bad.append(f"out.{k}")
    return bad


def _finite(run):
    return all(torch.isfinite(v).all().item() for e in run["trace"] for v in e.values() if torch.is_tensor(v)) and \
        all(torch.isfinite(run["out"][k]).all().item() for k in ("Ts", "weight", "flow2d_est_induced"))


def _teacher_forced(run, mode, with_T, last_rows=None):
    """-> (per-iteration {quantity: err / bound}, the fp64 step_full dicts) of a run's trace.  ``last_rows``: T also at
    the last iteration, on those map rows."""
    _threads()
    tr = run["trace"]
    e0 = tr[0]
    pre = L.make_pre(e0["fmap_prev"], e0["fmap_curr"], e0["net"], e0["inp"], e0["d1"], e0["d2"], e0["K8"])
    B, h, w = e0["d1"].shape
    T, net = se3.identity(B, h, w), e0["net"]
    res, refs = [], []
    n = len(tr) - 1
    with torch.no_grad():
        for k in range(1, n + 1):
            rows = last_rows if k == n and not with_T else None
            wT = with_T or rows is not None
            ref = L.step_full(_sd64(), pre, T, net, k == n, "f64", with_T=wT, T_rows=rows)
            got = dict(T=tr[k]["T"] if wT else None, net=tr[k]["net"], weight=tr[k]["weight"], mask=tr[k].get("mask"))
            res.append(L.ratios(got, ref, mode))
            refs.append(ref)
            if wT:
                assert ref["fragile"].float().mean().item() <= L.FRAGILE_CAP
            T, net = tr[k]["T"], tr[k]["net"]
    return res, refs


def _check(res, what):
    worst = {}
    for k, r in enumerate(res):
        print(f"{what} iteration {k + 1}: err / bound " + "  ".join(f"{q} {v:.3g}" for q, v in r.items()))
        for q, v in r.items():
            worst[q] = max(worst.get(q, 0.0), v)
    for q, v in worst.items():
        SUMMARY[(q,) + what] = v
    assert all(v <= 1.0 for v in worst.values()), (what, worst)


@functools.lru_cache(maxsize=None)
def _default_run(name, mode):
    return _run(_est(), name, mode)


# ------------------------------------------------------------------------------------------------ teacher-forced
@pytest.mark.parametrize("cm", CASE_MODES, **ids)
def test_update_loop_teacher_forced_against_fp64(cm):
    """Every iteration of the shipped wiring of the mode (split / split16: records, gates as convolution epilogues,
    heads inside se3_gn_step_heads; fp32: plain tensors, gru_gate_* kernels, se3_gn_step)."""
    name, mode = cm
    run = _default_run(name, mode)
    assert _finite(run)
    res, _ = _teacher_forced(run, mode, with_T=name != "P", last_rows=P_ROWS)
    _check(res, (mode, name))
    assert all("net" in r and "weight" in r for r in res) and "mask" in res[-1] and "T" in res[-1]
    assert all("T" in r for r in res) or name == "P"


@pytest.mark.parametrize("switch", ["FUSE_GATES", "MERGE_ENC_HEADS"])
def test_update_loop_ab_wirings_teacher_forced_against_fp64(switch):
    """Case A under split with one A/B switch off: the separate gate kernels / the two encoder chains unmerged."""
    run = _run(_est(), "A", "split", **{switch: False})
    assert _finite(run)
    _check(_teacher_forced(run, "split", True)[0], ("split", f"A {switch}=False"))


# ------------------------------------------------------------------------------------------------ final outputs
@pytest.mark.parametrize("cm", [("A", m) for m in L.MODES] + [("B", "split")], **ids)
def test_final_outputs_against_fp64_of_the_traced_last_state(cm):
    name, mode = cm
    _threads()
    run = _default_run(name, mode)
    x, last = _inputs(name), run["trace"][-1]
    out = run["out"]
    res = M.se3_up_ratios(M.upsample_se3(last["T"], last["mask"]), out["Ts"], None, f"{name} {mode}")
    ref, Mg = M.cvx_data(last["weight"].permute(0, 2, 3, 1), last["mask"])
    res["cvx"] = M.worst(f"{name} {mode} weight", M.ratio(out["weight"].permute(0, 2, 3, 1), ref, Mg, 1.0))[0]
    flow, Mg, ex = M.induced_flow(out["Ts"], x["depth_prev"], list(x["K"]))
    assert ex.float().mean().item() < 0.01
    res["induced_flow"] = M.worst(f"{name} {mode} induced flow", M.ratio(out["flow2d_est_induced"], flow, Mg, 1.0), ~ex[..., None])[0]
    for k, v in res.items():
        SUMMARY[(f"final {k}", mode, name)] = v / M.C[k]
    M.within(res, 1.0, cm)


# ------------------------------------------------------------------------------------------------ schedule, state
@pytest.mark.parametrize("cm", SCHEDULE, **ids)
def test_schedule_and_state_do_not_change_a_bit(cm):
    name, mode = cm
    other = "B" if name == "A" else "A"
    other_mode = "split16" if mode != "split16" else "split"
    est = _est()
    base = _default_run(name, mode)
    first = base["first"]
    checks = {}
    checks["(i) serial launches"] = _run(est, name, mode, serial=True, first=first)
    checks["(ii) prefetch on side streams"] = _run(est, name, mode, prefetch=True, first=first)
    checks["(iii) the same frame again"] = _run(est, name, mode, first=first)
    _run(est, other, mode)
    _run(est, other, other_mode)
    _run(est, name, other_mode)
    checks["(iv) after another shape and another precision mode"] = _run(est, name, mode, first=first)
    checks["(v) persistent buffers poisoned with NaN"] = _run(est, name, mode, first=first, poison=True)
    fresh = _run(_fresh(), name, mode)
    checks["(iv) a fresh module"] = fresh
    for what, run in checks.items():
        bad = _same_bits(base, run)
        print(f"{name} {mode} {what}: {'bit-equal' if not bad else 'DIFFERS in ' + ', '.join(bad)}")
        SUMMARY[("bits " + what, mode, name)] = 0.0 if not bad else float("inf")
        assert _finite(run), (cm, what)
        assert not bad, (cm, what, bad)


# ------------------------------------------------------------------------------------------------ batch
def test_batch_items_meet_the_bounds_of_their_single_runs():
    """Each item of B = 2 run alone (B = 1) is held to the same teacher-forced bounds as inside the batch; whether the
    bits are equal is reported, not asserted (the launch heuristics depend on B)."""
    both = _default_run("B", "split")
    for b in range(2):
        one = _run(_est(), "B", "split", item=b)
        assert _finite(one)
        _check(_teacher_forced(one, "split", True)[0], ("split", f"B item {b} alone"))
        diff = [k for i, (ea, eb) in enumerate(zip(one["trace"], both["trace"])) for k in ea
                if torch.is_tensor(ea[k]) and not torch.equal(ea[k], eb[k][b:b + 1])]
        print(f"B item {b}: alone against inside the batch: {'bit-equal' if not diff else 'not bit-equal: ' + ', '.join(sorted(set(diff)))}")


# ------------------------------------------------------------------------------------------------ free run
def test_free_run_divergence_is_reported():
    """The product's trajectory against loop64 free running from the same inputs, per iteration: printed (DESIGN), not
    asserted -- the recurrence amplifies."""
    _threads()
    run = _default_run("A", "split")
    e0 = run["trace"][0]
    pre = L.make_pre(e0["fmap_prev"], e0["fmap_curr"], e0["net"], e0["inp"], e0["d1"], e0["d2"], e0["K8"])
    with torch.no_grad():
        traj = L.loop64(_sd64(), pre, len(run["trace"]) - 1)
    for k, (o, t) in enumerate(zip(traj, run["trace"][1:])):
        d = L.deviation(dict(T=t["T"], net=t["net"], weight=t["weight"], mask=t.get("mask")), o)
        print(f"free run A split iteration {k + 1}: product - loop64: " + "  ".join(f"{q} {v:.3g}" for q, v in d.items()))
    assert _finite(run)


def test_zz_print_worst_error_over_bound_per_quantity_mode_and_case():
    """The figures of the DESIGN finding: worst err / bound per quantity, mode and case, collected by the tests above."""
    for key, v in sorted(SUMMARY.items()):
        print(f"loop fp64 summary: {key[0]:58s} {key[1]:8s} {key[2]:24s} worst err / bound {v:.3g}")
    assert all(v <= 1.0 for v in SUMMARY.values())
