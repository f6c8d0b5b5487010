"""RAFT3D's context network on the device (codd_amd/hrnet.py: the stem, Bottleneck.run, the transitions, HRModule.run,
ResizeConcatConv.forward, ops.context_split) against the fp64 restatement of every module (tests/context_net_fp64.py),
TEACHER-FORCED: module m runs on the fp32 oracle's own activation at that point -- computed once per case on the host,
never device output -- inside ops.stage("context") under the default ``split`` mode, so that HRModule.run takes its
conv2d_multi path, and every output ELEMENT is held to the running bound carried beside the fp64 value (conv_fp64's
c, pointwise_fp64's resize and tanh constants, the derived FOLD; none of it from device output).  An HRModule is held
by its parts (context_net_fp64.MODULES), because a worst-case bound seven to nine convolutions deep cannot fail:
"stageN.m.stepK", the outputs of the four branch steps captured where HRModule.run receives them from
ops.conv2d_multi, each against its fp64 reference from the device's own outputs of the step before (step 0: from the
teacher-forced input; which tensor feeds which step is the restatement's wiring); "stageN.m", the module's output
against the fuse layers in fp64 from the device's own branch outputs (the whole-module figure is printed as a
report); "stageN.m.fuse", HRModule.run's fuse code alone on the oracle's branch outputs (an HRModule without blocks
that shares the real one's fuse_layers).  Cases T (64 x 64), E (64 x 128), B (two images, 128 x 192),
A (192 x 320); B is held item by item.

Beside the bound: the multi-job launches are the ones intended (four-job groups on E's four-branch modules, a
three-job group plus single launches on T, B and A); HRNet.forward is the composition of the module methods and
RAFT3D.context the head applied to it (bits); the free-running context() against the chained restatement (the old
global figure; its accumulated bound is reported only, it cannot fail); the
BatchNorm fold on the device with planted channels and the version key of its cache; the precision policy (fp32,
split16, bf16mix, fp16mix bit-equal to split on A); state and schedule (twice, after another shape against a fresh
module, after NaN-filled blocks were allocated and freed, prefetch, Fork.serial: bits, on T and A); batch items; and
the footprint of a NaN planted in the image, as the restatement defines it.  Autotune off throughout.  Run with -s
for the figures."""
import collections
import copy
import functools

import pytest
import torch

import context_net_fp64 as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SUMMARY = {}
MODES = ("fp32", "split16", "bf16mix", "fp16mix")


def _fresh():
    """RAFT3D with the host estimator's weights, on the device (a module no launch has touched)."""
    return copy.deepcopy(N.estimator()[0].motion.raft3d).eval().to(DEV)


@functools.lru_cache(maxsize=None)
def _r3():
    return _fresh()


class _env:
    """Conv precision ``mode`` with autotune off, optionally Fork.serial; restored on exit."""

    def __init__(self, mode="split", serial=False):
        self.mode, self.serial = mode, serial

    def __enter__(self):
        from codd_amd import ops
        N._threads()
        self.prev_auto = ops._AUTOTUNE
        ops.enable_autotune(False)
        self.prev = ops.set_conv_precision(self.mode)
        self.prev_serial, ops.Fork.serial = ops.Fork.serial, self.serial
        self.grad = torch.no_grad()
        self.grad.__enter__()

    def __exit__(self, *exc):
        from codd_amd import ops
        self.grad.__exit__(*exc)
        ops.Fork.serial = self.prev_serial
        ops.set_conv_precision(self.prev)
        ops.enable_autotune(self.prev_auto)
        return False


def _hrmodule(r3, name):
    st, m = name.split(".")[:2]
    return getattr(r3.cnet[0], st)[int(m)]


def _module(r3, name, xs):
    """Module ``name`` of the product on the device tensors ``xs`` -> its output list (inside ops.stage("context"))."""
    from codd_amd import ops
    from codd_amd.hrnet import HRModule, cbn
    hr, head = r3.cnet[0], r3.cnet[1]
    with ops.stage("context"):
        if name == "stem":
            return [cbn(hr.conv2, hr.bn2, cbn(hr.conv1, hr.bn1, xs[0], "relu"), "relu")]
        if name.startswith("layer1"):
            return [hr.layer1[int(name[-1])].run(xs[0])]
        if name == "transition1":
            t0, t1 = hr.transition1[0], hr.transition1[1][0]
            return [cbn(t0[0], t0[1], xs[0], "relu"), cbn(t1[0], t1[1], xs[0], "relu")]
        if name.startswith("transition"):
            n = int(name[-1])
            t = getattr(hr, name)[n][0]
            return [cbn(t[0], t[1], xs[-1], "relu")]
        if name.endswith(".fuse"):
            real = _hrmodule(r3, name)
            fm = HRModule([x.shape[1] for x in xs], 0)
            fm.fuse_layers = real.fuse_layers
            return list(fm.run(xs))
        if name.startswith("stage"):
            return list(_hrmodule(r3, name).run(xs))
        if name == "head":
            return [head(xs)]
        assert name == "split", name
        return list(ops.context_split(xs[0]))


def _teacher_forced(name, module, r3=None):
    w = N.oracle_world(name)
    xs = [t.to(DEV).contiguous() for t in N.module_inputs(module, w["T32"], w["image"])]
    outs = _module(_r3() if r3 is None else r3, module, xs)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def _context(r3, image, mode="split", serial=False):
    with _env(mode, serial):
        out = r3.context(image.to(DEV))
        torch.cuda.synchronize()
        return out.cpu()


@functools.lru_cache(maxsize=None)
def _default(name):
    return _context(_r3(), N.inputs(name))


@functools.lru_cache(maxsize=None)
def _chained(name):
    """The restatement chained in fp64 from the image, the bound accumulated through the whole network."""
    N._threads()
    with torch.no_grad():
        return N.evaluate(N.K64, N.weights(F64), N.inputs(name))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ every module
@functools.lru_cache(maxsize=None)
def _stage_run(name, stage):
    """HRModule ``stage`` of the product, teacher-forced on case ``name``, with the outputs of its four branch steps
    captured where HRModule.run receives them from ops.conv2d_multi -> dict(outs, steps), tensors on the host."""
    from codd_amd import ops
    steps, real = [], ops.conv2d_multi

    def spy(jobs):
        outs = real(jobs)
        steps.append(list(outs))
        return outs
    ops.conv2d_multi = spy
    try:
        with _env():
            outs = _teacher_forced(name, stage)
    finally:
        ops.conv2d_multi = real
    assert len(steps) == 4 and all(len(s) == len(outs) for s in steps), [len(s) for s in steps]
    return dict(outs=outs, steps=[[t.cpu() for t in s] for s in steps])


def _from_device(name, stage, module):
    """The fp64 reference of part ``module`` of HRModule ``stage`` from the outputs the device produced for the part
    before it (step 0: from the module's teacher-forced input): one convolution deep (the fuse layers: up to three)."""
    w = N.oracle_world(name)
    T = dict(w["T32"])
    T.update({f"_{stage}.step{st}": v for st, v in enumerate(_stage_run(name, stage)["steps"])})
    N._threads()
    with torch.no_grad():
        xs = [N.K64.lift(t) for t in N.module_inputs(module, T, w["image"])]
        return N.run_module(N.K64, N.weights(F64), module, xs)


def _per_item(got, ref, B):
    assert [tuple(g.shape) for g in got] == [tuple(q.shape) for q in ref]
    return [max(N.ratio(g[b:b + 1], N.Q(q.v[b:b + 1], q.bound()[b:b + 1])).max().item() for g, q in zip(got, ref))
            for b in range(B)]


@pytest.mark.parametrize("module", N.MODULES)
@pytest.mark.parametrize("name", list(N.CASES))
def test_module_teacher_forced_within_the_running_bound(name, module):
    w = N.oracle_world(name)
    B = N.CASES[name][0]
    if module in N.STEP_MODULES:  # one branch step of HRModule.run, from the device's own outputs of the step before
        stage, st = module[:-6], int(module[-1])
        got = _stage_run(name, stage)["steps"][st]
        per_item = _per_item(got, _from_device(name, stage, module), B)
        if st == 3:  # the branch outputs against the four steps chained in fp64 from the module's teacher-forced input
            chained = _per_item(got, w["R64"][f"_{stage}.step3"], B)
            print(f"{name} {stage}: branch outputs, four convolutions deep: " + " ".join(f"{v:.3g}" for v in chained))
            assert all(v <= 1.0 for v in chained), (name, module, chained)
    elif module in N.STAGE_MODULES:
        run = _stage_run(name, module)
        whole = _per_item(run["outs"], w["R64"][module], B)
        print(f"{name} {module}: whole module from its inputs (report: a worst-case bound seven to nine convolutions "
              f"deep cannot fail): " + " ".join(f"{v:.3g}" for v in whole))
        assert all(v <= 1.0 for v in whole), (name, module, whole)
        # what holds the output: the fuse layers in fp64 from the branch outputs the device itself handed to them
        per_item = _per_item(run["outs"], _from_device(name, module, module + ".fuse"), B)
    else:
        with _env():
            got = _teacher_forced(name, module)
        per_item = _per_item(got, w["R64"][module], B)
    SUMMARY[(name, module)] = per_item
    print(f"{name} {module}: worst err / bound per item " + " ".join(f"{v:.3g}" for v in per_item))
    assert all(v <= 1.0 for v in per_item), (name, module, per_item)


# ------------------------------------------------------------------------------------------------ launch paths
def _launches(name, module):
    """(job counts of the multi-job launches, number of single convolution launches) of one teacher-forced module."""
    from codd_amd import ops
    multi, single = [], [0]
    real_m, real_s = ops._launch_conv_multi, ops._launch_conv

    def spy_m(lib, params, n, stream):
        rc = real_m(lib, params, n, stream)
        if rc == 0:
            multi.append(n)
        return rc

    def spy_s(lib, p, stream):
        single[0] += 1
        return real_s(lib, p, stream)
    ops._launch_conv_multi, ops._launch_conv = spy_m, spy_s
    try:
        with _env():
            _teacher_forced(name, module)
    finally:
        ops._launch_conv_multi, ops._launch_conv = real_m, real_s
    return collections.Counter(multi), single[0]


@pytest.mark.parametrize("name", list(N.CASES))
def test_branch_steps_leave_as_the_intended_multi_job_launches(name):
    """The four branch steps of an HRModule (conv1 / conv2 of two blocks) = the module's launches less those of its fuse
    layers alone: one group of nb jobs per step where every branch width is a multiple of 4, else the aligned branches
    in one group and the others through single launches."""
    widths = [N.CASES[name][2] >> (2 + i) for i in range(4)]
    for module in N.STAGE_MODULES:
        nb = {"stage2": 2, "stage3": 3, "stage4": 4}[module.split(".")[0]]
        whole_m, whole_s = _launches(name, module)
        fuse_m, fuse_s = _launches(name, module + ".fuse")
        steps = whole_m - fuse_m
        assert not fuse_m - whole_m, (name, module, whole_m, fuse_m)
        aligned = sum(1 for wd in widths[:nb] if wd % 4 == 0)
        print(f"{name} {module}: branch steps {dict(steps)} + {whole_s - fuse_s} single; fuse layers {dict(fuse_m)} + {fuse_s} single")
        assert steps == collections.Counter({aligned: 4}), (name, module, steps, aligned)
        assert whole_s - fuse_s == 4 * (nb - aligned), (name, module, whole_s, fuse_s)
    assert aligned == (4 if name == "E" else 3)  # (stage4.1: E takes four-job groups, T / B / A three jobs + singles)


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", list(N.CASES))
def test_forward_is_the_composition_and_free_running_context_report(name):
    """The live checks are the bit comparisons and the global figure.  The ratio to the bound accumulated through the
    whole network is a REPORT: the fp32 oracle sits at 1e-48 .. 1e-52 of that bound, the assertion on it cannot fail."""
    r3, image = _r3(), N.inputs(name)
    with _env():
        R = {}
        for module in N.MODULES:
            if module in N.STEP_MODULES or module in N.FUSE_MODULES or module == "split":
                continue
            xs = [image.to(DEV)] if not N.INPUTS[module] else [t for src in N.INPUTS[module] for t in R[src]]
            R[module] = _module(r3, module, xs)
        from codd_amd import ops
        with ops.stage("context"):
            ys = r3.cnet[0](image.to(DEV))
        ctx = r3.context(image.to(DEV))
        torch.cuda.synchronize()
        assert len(ys) == 4 and all(_same(a, b) for a, b in zip(ys, R["stage4.1"]))
        assert _same(ctx, R["head"][0]) and _same(ctx.cpu(), _default(name))
        split = [t.cpu() for t in ops.context_split(ctx)]
    C = _chained(name)
    worst = {"head": N.worst([ctx.cpu()], C["head"]), "split": N.worst(split, C["split"])}
    glob = (ctx.cpu().double() - C["head"][0].v).abs().max().item() / C["head"][0].v.abs().max().item()
    SUMMARY[(name, "context() free running")] = [worst["head"], worst["split"]]
    print(f"{name}: free-running context() err / accumulated bound (report only): head {worst['head']:.3g}  split {worst['split']:.3g};"
          f"  max |got - fp64| / max |fp64| = {glob:.3g}")
    assert all(v <= 1.0 for v in worst.values()), worst  # (report only, see the docstring)
    assert glob < 2e-4  # (the old global figure, against fp64)


# ------------------------------------------------------------------------------------------------ the BatchNorm fold
@pytest.mark.parametrize("bias", [False, True])
def test_packed_cbn_on_planted_batchnorm_channels_and_its_version_key(bias):
    from codd_amd import hrnet
    conv = torch.nn.Conv2d(16, 8, 3, 1, 1, bias=bias)
    bn = torch.nn.BatchNorm2d(8)
    case = N.fold_case(bias, 0)
    conv.load_state_dict({k[2:]: v for k, v in case["sd"].items() if k.startswith("c.")})
    bn.load_state_dict({k[2:]: v for k, v in case["sd"].items() if k.startswith("b.")}, strict=False)
    conv, bn = conv.to(DEV).eval(), bn.to(DEV).eval()
    x = case["x"].to(DEV)
    outs = []
    with _env("fp32"):
        for stats in (0, 1):
            case = N.fold_case(bias, stats)
            if stats:
                bn.load_state_dict({k[2:]: v for k, v in case["sd"].items() if k.startswith("b.")}, strict=False)
            got = hrnet.cbn(conv, bn, x).cpu()
            r = N.ratio(got, N.fold_ref(case))
            per = [r[:, c].max().item() for c in range(8)]
            print(f"cbn (bias={bias}, stats={stats}): err / bound per channel " + " ".join(f"{v:.3g}" for v in per))
            SUMMARY[("cbn", f"bias={bias} stats={stats}")] = [max(per)]
            assert max(per) <= 1.0, per
            outs.append(got)
    assert not torch.equal(outs[0], outs[1])  # the fold followed the new statistics


# ------------------------------------------------------------------------------------------------ policy, state, batch
def test_precision_policy_keeps_the_context_network_on_exact_fp32():
    base = _default("A")
    for mode in MODES:
        assert _same(_context(_r3(), N.inputs("A"), mode), base), mode


@pytest.mark.parametrize("name", ["T", "A"])
def test_state_and_schedule_leave_the_bits_alone(name):
    r3, image, base = _r3(), N.inputs(name), _default(name)
    assert _same(_context(r3, image), base), "the same image twice"
    _context(r3, N.inputs("E"))
    fresh = _context(_fresh(), image)
    assert _same(_context(r3, image), fresh) and _same(fresh, base), "after another shape / a fresh module"
    w = N.oracle_world(name)
    blocks = [torch.full(t.shape, float("nan"), device=DEV) for v in w["T32"].values() for t in v for _ in range(2)]
    torch.cuda.synchronize()
    del blocks
    got = _context(r3, image)
    assert torch.isfinite(got).all() and _same(got, base), "after NaN-filled blocks of the network's footprint"
    with _env():
        r3.prefetch(image.to(DEV))
        torch.cuda.synchronize()
        pend = r3._pending["netinp"].cpu()
        r3._pending = None
    assert _same(pend, base), "prefetch"
    assert _same(_context(r3, image, serial=True), base), "Fork.serial"


def test_batch_items():
    image = N.inputs("B")
    got = _default("B")
    twice = _context(_r3(), torch.cat([image[:1], image[:1]], 0))
    assert _same(twice[0], twice[1])
    singles = [_context(_r3(), image[b:b + 1])[0] for b in range(2)]
    print("B: items bit-equal to the single runs: " + " ".join(str(_same(got[b], singles[b])) for b in range(2)) +
          f"; the item run twice in one batch bit-equal to its single run: {_same(twice[0], singles[0])}")
    C = _chained("B")["head"][0]
    for b in range(2):  # each item against its own reference: the global figure (the accumulated bound is a report only,
        # it cannot fail; the teacher-forced tests hold the modules item by item)
        assert N.ratio(got[b:b + 1], N.Q(C.v[b:b + 1], C.bound()[b:b + 1])).max().item() <= 1.0
        glob = (got[b].double() - C.v[b]).abs().max().item() / C.v[b].abs().max().item()
        assert glob < 2e-4, (b, glob)


def test_a_nan_in_the_image_reaches_the_footprint_the_restatement_defines():
    """One NaN pixel of A's image: non-finite exactly where the restatement, chained from the same image, is.  At
    context()'s output that is every element (the 1/32 branch and the up paths spread it over the whole map), so the
    modules up to stage2.0, issued by hand as forward issues them, are held too: their footprints are partial."""
    image = N.inputs("A").clone()
    image[0, 1, 37, 250] = float("nan")
    N._threads()
    with torch.no_grad():
        ref = N.evaluate(N.K64, N.weights(F64), image, modules=[m for m in N.MODULES if m not in N.STEP_MODULES + N.FUSE_MODULES])
    got = {"head": [_context(_r3(), image)]}
    with _env():
        R = {}
        for module in ("stem", "layer1.0", "layer1.1", "transition1", "stage2.0"):
            xs = [image.to(DEV)] if not N.INPUTS[module] else [t for src in N.INPUTS[module] for t in R[src]]
            R[module] = _module(_r3(), module, xs)
            got[module] = [t.cpu() for t in R[module]]
    partial = 0
    for module, outs in got.items():
        for i, (g, q) in enumerate(zip(outs, ref[module])):
            bad_ref, bad_got = ~torch.isfinite(q.v), ~torch.isfinite(g)
            print(f"NaN footprint {module}[{i}]: reference {int(bad_ref.sum())} of {bad_ref.numel()} elements, device "
                  f"{int(bad_got.sum())}; missing {int((bad_ref & ~bad_got).sum())}, extra {int((bad_got & ~bad_ref).sum())}")
            assert bad_ref.any() and torch.equal(bad_ref, bad_got), (module, i)
            partial += int(not bad_ref.all())
    assert partial >= 5  # (stem .. transition1 and at least one output of stage2.0)


def test_zz_summary():
    for (name, what), v in SUMMARY.items():
        print(f"err / bound  {name:4s} {what:24s} " + " ".join(f"{x:.3g}" for x in v))
    assert all(x <= 1.0 for v in SUMMARY.values() for x in v)
