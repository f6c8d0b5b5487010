"""The stereo network of the product (codd_amd/stereo.py, traced through ``HITNetMF.stereo_matching(trace=[])``) against
the fp64 restatement of every stage (tests/stereo_net_fp64.py), TEACHER-FORCED: each stage in fp64 from the product's
own traced inputs of that stage against the product's traced results of it, so no error accumulates and the bounds are
as sharp as the kernel tests' (stereo_net_fp64.BOUND: 5 x the fp32 oracle's own deviation per quantity and channel
group, set and re-measured on the CPU by tests/test_stereo_net_fp64_reference.py, never from GPU output).  Cases S
(64x128), B (128x256, two pairs), A (192x320), W (64x384: wider than max_disp) and A-roll (A with ops.ROLL_MIN_PIXELS
low enough that the 16-channel layers take conv_roll) under the default ``split`` mode.  A bound is a maximum norm over
the batch, so B is held item by item; a batch made of the same pair twice must give bit-equal items.

The two discontinuities follow stereo_net_fp64's rules (arg-min: stereo_fusion_fp64.argmin_check on the cost volume of
the product's own tile features; select: may differ where the reference's |conf0 - conf1| <= 2 x the confidence bound,
then held against the other candidate), excused tiles per case and rule <= excuse_cap.

Inputs and outputs are not taken on trust: fea0 is held against the fp64 U-Net encoder of the test's own images
(BOUND["fea0_img"]); left_feat / right_feat are bit-equal to fea2[:B] / fea2[B:], pred_disp to the traced final stage;
every slice of every ``aug`` buffer is bit-equal to its producer's own trace entry (init hypothesis, ``up``, both
``decrease`` outputs); each update's result is the traced ``lastconv`` output applied to the traced hypotheses (the
hyp_select kernel's own bound).

Precision policy: on A, trace and output under fp32, split16 and fp16mix are bit-equal to split (ops.stage("stereo")
routes HITNet to the exact-fp32 kernels).  Schedule and state invariance (bit comparisons of the whole trace and the
output on S and A): pipelined against STEREO_PIPE = False, against Fork.serial, PIPE_INIT_SIDE 0 / 1 / 2,
FORK_INIT_LEVELS with FORK_INIT_FINE = 0, the same frame twice, after another shape ran on the module against a fresh
module, after NaN-filled blocks of the frame's footprint were allocated and freed (aug, cost and the select output come
from torch.empty: a channel read before it is written shows as a NaN or a changed bit), and trace=None against
trace=[].  Autotune off throughout.  Run with -s for the figures."""
import functools

import pytest
import torch

import stereo_fusion_fp64 as SF
import stereo_net_fp64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SUMMARY = {}
EXCUSED = {}
RUN_CASES = ("S", "B", "A", "A-roll", "W")
SWITCHES = ("STEREO_PIPE", "PIPE_INIT_SIDE", "FORK_INIT_LEVELS", "FORK_INIT_FINE")


def _fresh():
    import codd_amd  # noqa: F401
    from codd_amd import synth
    from codd_amd.registry import build_estimator
    est = build_estimator(dict(type="ConsistentOnlineDynamicDepth", stereo=N.STEREO_CFG)).eval()
    synth.load_synthetic_weights(est, gain=1.4)  # (the same deterministic filler as stereo_net_fp64.estimator)
    return est.to(DEV)


@functools.lru_cache(maxsize=None)
def _est():
    return _fresh()


class _env:
    """Conv precision ``mode`` with autotune off; optionally Fork.serial, ops.ROLL_MIN_PIXELS and the A/B switches of
    codd_amd.stereo.  Everything is restored on exit."""

    def __init__(self, mode="split", serial=False, roll_min=None, **switches):
        assert set(switches) <= set(SWITCHES), switches
        self.mode, self.serial, self.roll_min, self.switches = mode, serial, roll_min, switches

    def __enter__(self):
        from codd_amd import ops, stereo
        self.prev_auto = ops._AUTOTUNE
        ops.enable_autotune(False)
        self.prev = ops.set_conv_precision(self.mode)
        self.prev_serial, ops.Fork.serial = ops.Fork.serial, self.serial
        self.prev_roll = ops.ROLL_MIN_PIXELS
        if self.roll_min is not None:
            ops.ROLL_MIN_PIXELS = self.roll_min
        self.prev_sw = {k: getattr(stereo, k) for k in self.switches}
        for k, v in self.switches.items():
            setattr(stereo, k, v)

    def __exit__(self, *exc):
        from codd_amd import ops, stereo
        for k, v in self.prev_sw.items():
            setattr(stereo, k, v)
        ops.ROLL_MIN_PIXELS = self.prev_roll
        ops.Fork.serial = self.prev_serial
        ops.set_conv_precision(self.prev)
        ops.enable_autotune(self.prev_auto)
        return False


def _images(name):
    return N.inputs(name.split("-")[0])


def _run(est, name, mode="split", serial=False, images=None, trace=True, **switches):
    """The product on case ``name`` -> dict(T = the flat trace on the host (stereo_net_fp64.flatten), out = the returned
    dict on the host, rolls = the number of rolling-window launches)."""
    from codd_amd import ops
    left, right = _images(name) if images is None else images
    roll = N.ROLL_PIXELS_A if name.endswith("-roll") else None
    calls = [0]
    orig = ops.conv_roll

    def counted(*a, **kw):
        calls[0] += 1
        return orig(*a, **kw)
    tr = [] if trace else None
    with _env(mode, serial, roll, **switches), torch.no_grad():
        ops.conv_roll = counted
        try:
            out = est.stereo.stereo_matching(left.to(DEV), right.to(DEV), trace=tr)
        finally:
            ops.conv_roll = orig
        torch.cuda.synchronize()
    assert (calls[0] > 0) == (roll is not None), (name, calls, "rolling-window launches")
    return dict(T=N.flatten(tr) if trace else {}, out={k: v.detach().cpu() for k, v in out.items()}, rolls=calls[0])


@functools.lru_cache(maxsize=None)
def _default_run(name):
    return _run(_est(), name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Every stage in fp64 from the default run's own trace (computed once per case and process)."""
    N._threads()
    left, right = _images(name)
    with torch.no_grad():
        return N.evaluate(N.K64, N.weights(F64), left, right, _default_run(name)["T"])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    """Every traced tensor and every output of two runs is bit-equal -> list of the names that are not."""
    bad = [k for k in a["T"] if k not in b["T"] or not torch.equal(_bits(a["T"][k]), _bits(b["T"][k]))]
    bad += [k for k in b["T"] if k not in a["T"]]
    return bad + ["out." + k for k in ("pred_disp", "left_feat", "right_feat")
                  if not torch.equal(_bits(a["out"][k]), _bits(b["out"][k]))]


def _finite(run):
    return all(torch.isfinite(v).all().item() for v in run["T"].values()) and \
        all(torch.isfinite(run["out"][k]).all().item() for k in ("pred_disp", "left_feat", "right_feat"))


def _expected_names():
    return set(N.traced_name(q) for q in N.quantities()) | {f"upd{i}.cvc" for i in range(5)} | \
        {f"upd{i}.cvp" for i in range(1, 5)}


def _item(D, b, B):
    """Item ``b`` of a flat dict of a batch of B (the U-Net's tensors hold left | right: items b and B + b)."""
    out = {}
    for k, v in D.items():
        if isinstance(v, dict):  # (stereo_fusion_fp64.costvol's dict)
            out[k] = {kk: vv[b:b + 1] for kk, vv in v.items()}
        elif k.startswith(("enc", "fea")):
            out[k] = torch.cat([v[b:b + 1], v[B + b:B + b + 1]], 0)
        else:
            out[k] = v[b:b + 1]
    return out


# ------------------------------------------------------------------------------------------------ teacher-forced
@pytest.mark.parametrize("name", RUN_CASES)
def test_every_stage_teacher_forced_against_fp64(name):
    run = _default_run(name)
    assert set(run["T"]) == _expected_names(), set(run["T"]) ^ _expected_names()
    assert _finite(run)
    B, H, W = N.CASES[name.split("-")[0]]
    assert run["out"]["pred_disp"].shape == (B, 1, H, W) and run["T"]["fea0"].shape[0] == 2 * B
    R = _reference(name)
    dev, info = N.deviations(run["T"], R)
    r = N.ratios(dev)
    for k, v in r.items():
        print(f"{name} {k}: err {dev[k]:.3g}  err / bound {v:.3g}")
        SUMMARY[(k, name)] = v
    case = name.split("-")[0]
    ex_arg = sum(round(c["near"] * R[f"init{l}.cost"].numel()) for l, c in info["argmin"].items())
    ex_sel = sum(s[0] for s in info["select"].values())
    wrong = {f"arg-min {l}": (c["wrong"], c["where"]) for l, c in info["argmin"].items() if c["wrong"]}
    wrong.update({f"select {i}": s[1] for i, s in info["select"].items() if s[1]})
    EXCUSED[name] = (ex_arg, ex_sel)
    print(f"{name}: excused arg-min tiles {ex_arg} of {N.tiles(case)} (cap {N.excuse_cap(N.tiles(case))}), excused selects "
          f"{ex_sel} of {N.tiles(case, 1)} (cap {N.excuse_cap(N.tiles(case, 1))}); cost at the pick / (2^-24 M): "
          + " ".join(f"{c['cost']:.3g}" for c in info["argmin"].values()) + f" (C {SF.C['costvol']})")
    assert not wrong, (name, wrong)
    assert all(c["cost"] <= SF.C["costvol"] for c in info["argmin"].values()), (name, info["argmin"])
    assert ex_arg <= N.excuse_cap(N.tiles(case)) and ex_sel <= N.excuse_cap(N.tiles(case, 1)), (name, ex_arg, ex_sel)
    over = {k: v for k, v in r.items() if not v <= 1.0}
    assert not over, (name, over)
    for b in range(B if B > 1 else 0):  # each item on its own: its figures, its arg-mins, its selects
        dev_b, info_b = N.deviations(_item(run["T"], b, B), _item(R, b, B))
        r_b = N.ratios(dev_b)
        k = max(r_b, key=r_b.get)
        print(f"{name} item {b}: worst err / bound {r_b[k]:.3g} ({k})")
        SUMMARY[(f"item {b}: worst of all quantities", name)] = r_b[k]
        assert r_b[k] <= 1.0 and not any(c["wrong"] for c in info_b["argmin"].values()) and \
            not any(s[1] for s in info_b["select"].values()), (name, b, k, r_b[k])


# ------------------------------------------------------------------------------------------------ inputs, outputs, slices
@pytest.mark.parametrize("name", RUN_CASES)
def test_outputs_and_buffer_slices_are_what_their_producers_traced(name):
    run = _default_run(name)
    T, out = run["T"], run["out"]
    B = N.CASES[name.split("-")[0]][0]
    left, _ = _images(name)
    eq = lambda a, b: a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    assert eq(out["left_feat"], T["fea2"][:B]) and eq(out["right_feat"], T["fea2"][B:])
    assert eq(out["pred_disp"], T["pred_disp"]) and eq(out["left_img"], left)
    for i in range(5):
        aug = T[f"upd{i}.aug"]
        assert aug.shape[1] == (32 if i == 0 else 64)
        assert eq(aug[:, 0:16], T[f"init{i}.hyp"]), (name, i, "aug[0:16] is not the init hypothesis")
        assert eq(aug[:, 16:32], T[f"upd{i}.cvc"]), (name, i, "aug[16:32] is not decrease(current costs)")
        if i:
            assert eq(aug[:, 32:48], T[f"upd{i}.up"]), (name, i, "aug[32:48] is not the up-sampled previous hypothesis")
            assert eq(aug[:, 48:64], T[f"upd{i}.cvp"]), (name, i, "aug[48:64] is not decrease(previous costs)")
            assert not eq(T[f"upd{i}.cvc"], T[f"upd{i}.cvp"])
        # the result is the traced lastconv output applied to the traced hypotheses: the kernel's own bound
        if i:
            v, M, _ = SF.hyp_select(T[f"upd{i}.upd"], T[f"init{i}.hyp"], T[f"upd{i}.up"])
        else:
            a, b = T["init0.hyp"].to(F64), T["upd0.upd"].to(F64)
            v, M = a + b, a.abs() + b.abs()
            v = torch.cat([torch.relu(v[:, :1]), v[:, 1:]], 1)
        fig = SF.worst(f"{name} update {i} result", SF.ratio(T[f"upd{i}.hyp"], v, M, 1.0), quiet=True)[0]
        SUMMARY[(f"upd{i}.hyp from traced upd / C[hyp_select]", name)] = fig / SF.C["hyp_select"]
        assert fig <= SF.C["hyp_select"], (name, i, fig)
    for k in ("up_r1", "up_r05"):  # channels 1..15 of an up-sampling are copies
        src = T[k[3:]]
        assert eq(T[k][:, 1:], src[:, 1:].repeat_interleave(2, 2).repeat_interleave(2, 3)), (name, k)


def test_a_batch_of_the_same_pair_twice_gives_bit_equal_items():
    left, right = _images("A")
    run = _run(_est(), "A", images=(torch.cat([left, left]).contiguous(), torch.cat([right, right]).contiguous()))
    assert _finite(run)
    bad = []
    for k, v in run["T"].items():
        pairs = [(0, 1), (2, 3)] if k.startswith(("enc", "fea")) else [(0, 1)]
        bad += [k for a, b in pairs if not torch.equal(_bits(v[a]), _bits(v[b]))]
    assert not bad, bad
    assert torch.equal(_bits(run["out"]["pred_disp"][0]), _bits(run["out"]["pred_disp"][1]))
    assert not torch.equal(run["T"]["fea2"][0], run["T"]["fea2"][2])  # (left is not right)


# ------------------------------------------------------------------------------------------------ precision policy
@pytest.mark.parametrize("mode", ["fp32", "split16", "fp16mix"])
def test_precision_modes_leave_the_stereo_network_on_the_exact_fp32_kernels(mode):
    from codd_amd import ops
    before = (ops.CONV_PRECISION, ops.BF16_STAGE_POLICY)
    run = _run(_est(), "A", mode=mode)
    assert (ops.CONV_PRECISION, ops.BF16_STAGE_POLICY) == before  # (restored)
    bad = _same_bits(_default_run("A"), run)
    SUMMARY[(f"bits {mode} against split", "A")] = 0.0 if not bad else float("inf")
    assert _finite(run) and not bad, (mode, bad)


# ------------------------------------------------------------------------------------------------ schedule, state
def _poison_allocator(nbytes):
    """NaN-filled blocks of at least ``nbytes`` in all -- one large block and a spread of small ones, so that both pools of
    the caching allocator hold them -- allocated, filled and freed."""
    nan = float("nan")
    blocks = [torch.full((max(nbytes, 1 << 22) // 4,), nan, device=DEV)]
    for sz in (1 << 9, 1 << 12, 1 << 15, 1 << 18, 1 << 20):
        blocks += [torch.full((sz // 4,), nan, device=DEV) for _ in range(24)]
    torch.cuda.synchronize()
    del blocks


@pytest.mark.parametrize("name", ["S", "A"])
def test_schedule_and_state_do_not_change_a_bit(name):
    from codd_amd import ops, stereo
    before = {k: getattr(stereo, k) for k in SWITCHES}, ops.Fork.serial, ops.ROLL_MIN_PIXELS
    est = _est()
    base = _default_run(name)
    checks = {}
    checks["(i) STEREO_PIPE = False"] = _run(est, name, STEREO_PIPE=False)
    checks["(ii) Fork.serial"] = _run(est, name, serial=True)
    for v in (0, 1, 2):
        checks[f"(iii) PIPE_INIT_SIDE = {v}"] = _run(est, name, PIPE_INIT_SIDE=v)
    checks["(iv) FORK_INIT_LEVELS, FORK_INIT_FINE = 0"] = _run(est, name, STEREO_PIPE=False, FORK_INIT_LEVELS=True, FORK_INIT_FINE=0)
    checks["(v) the same frame again"] = _run(est, name)
    _run(est, "B" if name == "A" else "W")
    checks["(vi) after another shape"] = _run(est, name)
    checks["(vi) a fresh module"] = _run(_fresh(), name)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    _run(est, name)
    footprint = torch.cuda.max_memory_allocated() - m0
    assert footprint > 0
    _poison_allocator(2 * footprint)
    checks["(vii) after NaN-filled blocks were freed"] = _run(est, name)
    _poison_allocator(2 * footprint)
    checks["(viii) trace=None"] = dict(_run(est, name, trace=False), T=base["T"])
    assert (({k: getattr(stereo, k) for k in SWITCHES}, ops.Fork.serial, ops.ROLL_MIN_PIXELS)) == before
    for what, run in checks.items():
        bad = _same_bits(base, run)
        print(f"{name} {what}: {'bit-equal' if not bad else 'DIFFERS in ' + ', '.join(bad)}")
        SUMMARY[("bits " + what, name)] = 0.0 if not bad else float("inf")
        assert _finite(run), (name, what)
        assert not bad, (name, what, bad)


def test_zz_print_worst_error_over_bound_per_stage_quantity_and_case():
    """The figures of the pull request: worst err / bound per quantity and case, and the excused tiles per case."""
    for key, v in sorted(SUMMARY.items()):
        print(f"stereo net fp64 summary: {key[0]:52s} {key[1]:8s} worst err / bound {v:.3g}")
    fam = lambda q: "U-Net" if q.startswith(("enc", "fea")) else "init" if q.startswith("init") else \
        "update" if q.startswith("upd") and "/" not in q else "post" if q.split(":")[0] in ("r1", "up_r1", "r05", "up_r05", "pred_disp") else None
    for f in ("U-Net", "init", "update", "post"):
        row = {c: max([v for (q, n), v in SUMMARY.items() if n == c and fam(q) == f] or [float("nan")]) for c in RUN_CASES}
        print(f"stereo net fp64 summary: worst err / bound of the {f} stages: " + "  ".join(f"{c} {v:.3g}" for c, v in row.items()))
    for name, (a, s) in EXCUSED.items():
        print(f"stereo net fp64 summary: excused tiles on {name}: arg-min {a}, select {s}")
    assert all(v <= 1.0 for v in SUMMARY.values())
