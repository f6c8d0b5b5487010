"""Cost of LiveSession's rectification health check (codd_epipolar_check), 540x960 in 576x960.

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, on a planted scene of tests/live_epi_ref.py at that size: the default parameters, then one parameter
   changed at a time -- step 1 / 4 / 8 (the measure launch scales with 1 / step^2), range_px 4, iters 1 (the difference to
   iters 4 is three weighted passes) and map=None.
2. LiveSession.step frames/s with epipolar=True against epipolar=False: one process, both sessions on one estimator,
   alternated in rounds, median over the rounds.
3. With --bench: ``bench.py --gpus 1 --steps 200 --warmup 5`` of this tree and, with --parent-tree DIR, of a built checkout
   of the parent commit there, each in a child process of its own, the two alternated --bench-runs times.

    python tools/live_epi_bench.py [--calls 200 --rounds 5 --per-round 25] [--bench [--parent-tree DIR]] [--out profiles/live_epi.md]

Kernel times: ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o epi -- python tools/live_epi_bench.py
--defaults-only --no-session --calls 100`` (a run of its own: tracing slows the host).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import live_conf_bench as lcb  # noqa: E402  (time_calls, frames, bench_part)

H, W = lcb.H, lcb.W
HP, WP = lcb.HP, lcb.WP
DEV = lcb.DEV
VARIANTS = [("defaults (step 2, range_px 2, iters 4)", {}), ("step 1", dict(step=1)), ("step 4", dict(step=4)),
            ("step 8", dict(step=8)), ("range_px 4", dict(range_px=4)), ("iters 1", dict(iters=1))]


def kernel_part(n, defaults_only=False):
    import live_epi_ref as le
    from codd_amd import ops
    spec = dict(crop=(H, W), padded=(HP, WP), K=(1050.0, 1050.0, 479.5, 269.5), par={}, plant=(3e-4, 2e-4, 8e-4, 5e-4))
    c = le.case(spec)
    disp, left, right = (torch.from_numpy(c[k]).to(DEV) for k in ("disp", "left", "right"))
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    dy = torch.empty(H, W, device=DEV)
    scratch = torch.empty(ops.epipolar_scratch(H, W), dtype=torch.uint8, device=DEV)
    rows = []
    for name, over in (VARIANTS[:1] if defaults_only else VARIANTS + [("defaults, dy_map=None", None)]):
        par = dict(c["par"], **(over or {}))
        out = None if over is None else dy
        eager, graph = lcb.time_calls(lambda: ops.epipolar_check(disp, left, right, c["K"], (H, W), rec, out, scratch=scratch, **par), n)
        r = rec.cpu().numpy()
        rows.append(dict(variant=name, launches=2 + par["iters"], eager_us=eager, graph_us=graph, measurable=int(r[5]),
                         ok=bool(r[4]), coef=r[:4].tolist()))
    return rows, c["plant"]


def session_part(rounds, per_round, warmup=6):
    import time
    from codd_amd import configs, ops, synth
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd()).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    est = est.to(DEV)
    ops.enable_autotune(True)  # as bench.py and the CLI run
    src = lcb.frames(16)
    sess = {"epipolar=False": LiveSession(est, (H, W), output="depth"),
            "epipolar=True": LiveSession(est, (H, W), output="depth", epipolar=True)}
    fps = {k: [] for k in sess}
    i = 0
    with torch.no_grad():
        for s in sess.values():
            for _ in range(warmup):
                s.step(*src[i % 16])
                i += 1
        for _ in range(rounds):
            for k, s in sess.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_round):
                    s.step(*src[i % 16])
                    i += 1
                torch.cuda.synchronize()
                fps[k].append(per_round / (time.perf_counter() - t0))
    for s in sess.values():
        s.close()
    return [dict(variant=k, rounds=rounds, per_round=per_round, fps_median=float(np.median(v)), fps_min=min(v), fps_max=max(v))
            for k, v in fps.items()]


def bench_part(trees, runs, steps, timeout=600):
    """bench.py's headline (frames/s) per tree, one child process per run, the trees alternated."""
    import subprocess
    fps = {k: [] for k in trees}
    for _ in range(runs):
        for k, root in trees.items():
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "5"], cwd=root,
                                 stdout=subprocess.PIPE, text=True, check=True, timeout=timeout).stdout
            fps[k].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["value"])
            print(f"bench.py, {k}: {fps[k][-1]:.2f} frames/s", file=sys.stderr, flush=True)
    return [dict(tree=k, fps=v) for k, v in fps.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--no-session", action="store_true", help="the kernel part only")
    ap.add_argument("--defaults-only", action="store_true", help="the default parameters only (for a kernel trace)")
    ap.add_argument("--bench", action="store_true", help="also run bench.py's headline, in child processes")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its bench.py headline too")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    trees = {"this commit": ROOT, **({"parent commit": os.path.abspath(args.parent_tree)} if args.parent_tree else {})}
    # (first: this process has not touched the device yet)
    brows = bench_part(trees, args.bench_runs, args.bench_steps) if args.bench else []
    from codd_amd import ops
    ops.enable_autotune(False)
    krows, plant = kernel_part(args.calls, args.defaults_only)
    srows = [] if args.no_session else session_part(args.rounds, args.per_round)
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], calls=args.calls, kernel=krows, plant=plant, session=srows, bench=brows)))
    lines = [f"codd_epipolar_check at {W}x{H} in {WP}x{HP}, HIP events over {args.calls} calls after 20 warm-ups; planted "
             f"coefficients {list(plant)}", "",
             "| variant | launches | us / call, issued eagerly | us / call, graph replay | measurable pixels | ok | fitted coefficients |",
             "|---|---|---|---|---|---|---|"]
    lines += [f"| {r['variant']} | {r['launches']} | {r['eager_us']:.2f} | {r['graph_us']:.2f} | {r['measurable']} | {r['ok']} | "
              f"{', '.join(f'{v:.2e}' for v in r['coef'])} |" for r in krows]
    by = {r["variant"]: r["graph_us"] for r in krows}
    if not args.defaults_only:
        lines += ["", f"three weighted passes (iters 4 - iters 1): {by[VARIANTS[0][0]] - by['iters 1']:.2f} us; "
                  f"the measure launch from step 2 to step 1: +{by['step 1'] - by[VARIANTS[0][0]]:.2f} us"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max |", "|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} |"
                  for r in srows]
        a, b = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the epipolar output per synchronous frame: {1e3 / b - 1e3 / a:.3f} ms of {1e3 / a:.3f} ms"]
    if brows:
        lines += ["", f"`bench.py --gpus 1 --steps {args.bench_steps} --warmup 5`, a process per run, the trees alternated (the "
                  "flagship workload does not run this code)", "", "| tree | frames/s per run | median | min | max |", "|---|---|---|---|---|"]
        lines += [f"| {r['tree']} | {', '.join(f'{v:.2f}' for v in r['fps'])} | {float(np.median(r['fps'])):.2f} | {min(r['fps']):.2f} | "
                  f"{max(r['fps']):.2f} |" for r in brows]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
