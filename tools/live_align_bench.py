"""Cost of LiveSession's aligned-depth output (codd_align_depth), 540x960 in 576x960 onto a 720x1280 colour camera.

1. One call (the fill and the splat) replayed from a captured graph and issued eagerly, HIP events over N calls after 20
   warm-ups (live_conf_bench.time_calls), for footprints 1 and 2, with and without uv_out.  The bytes the two launches must
   move (one disparity plane in, the target plane written by the fill, 8 bytes of uv per source pixel; the atomics on top
   are counted separately as k^2 dwords per source pixel) over the graph-replayed time.
2. The PIPELINED session rate (push / pop, two frames in flight) with and without align_to: a child process per run, both
   sessions on one estimator, alternated in rounds, median over the rounds; with --parent-tree DIR the same session without
   align_to on a built checkout of the parent commit, its child processes alternated with this tree's.
3. With --bench: ``bench.py --gpus 1 --steps 20 --warmup 5`` of this tree and of --parent-tree, alternated.

    python tools/live_align_bench.py [--calls 200 --rounds 4 --per-round 30] [--parent-tree DIR] [--bench] [--out profiles/live_align.md]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H, W, HP, WP = 540, 960, 576, 960
HT, WT = 720, 1280
INTRINSICS, CALIB = (1050.0, 1050.0, 479.5, 269.5), 210.0
DEV = "cuda:0"


def colour_target():
    """A 720x1280 Brown camera 6 cm to the right of the left one, slightly rotated: it magnifies the 540x960 grid by 4/3."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import live_align_ref as la
    from codd_amd import calibration
    t = la.make_target("brown", (HT, WT), 1400.0, T3=(0.06, -0.01, 0.005))
    return calibration.AlignTarget(la.as_camera(t), t["R"], t["T"])


def kernel_part(n):
    import torch
    sys.path.insert(0, HERE)
    from live_conf_bench import copy_rate, time_calls
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import live_align_ref as la
    from codd_amd import ops
    disp = torch.from_numpy(la.scene(((H, W), (HP, WP)), "bench", lo=4.0, hi=120.0)).to(DEV)
    view = ops.align_view(colour_target())
    depth = torch.empty(HT, WT, device=DEV)
    uv = torch.empty(H, W, 2, device=DEV)
    rows = []
    for k in (1, 2):
        for with_uv in (True, False):
            fn = lambda: ops.align_depth(disp, (H, W), INTRINSICS, CALIB, view, (HT, WT), k, depth, uv if with_uv else None)  # noqa: E731
            eager, graph = time_calls(fn, n)
            torch.cuda.synchronize()
            nbytes = H * W * 4 + HT * WT * 4 + (H * W * 8 if with_uv else 0)
            rows.append(dict(k=k, uv=with_uv, eager_us=eager, graph_us=graph, bytes=nbytes, atomic_bytes=H * W * 4 * k * k,
                             reached=float(torch.isfinite(depth).float().mean())))
    return rows, copy_rate(n)


def frames(n):
    import torch
    from codd_amd import synth
    img, r_img, _ = synth.stereo_sequence(H, W, n)

    def u8(t):
        return np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())

    return [(u8(img[0, i]), u8(r_img[0, i])) for i in range(n)]


def session_child(tree, with_align, rounds, per_round, warmup=8):
    """Runs in a process of its own with ``tree`` first on sys.path: pipelined frames/s per round and variant."""
    sys.path.insert(0, tree)
    import torch
    from codd_amd import configs, ops, synth
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd()).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    est = est.to(DEV)
    ops.enable_autotune(True)  # as bench.py and the CLI run
    src = frames(16)
    kw = dict(intrinsics=INTRINSICS, calib=CALIB, output="depth")
    sess = {"without align_to": LiveSession(est, (H, W), **kw)}
    if with_align:
        s = LiveSession(est, (H, W), align_to=colour_target(), **kw)
        sess["align_to, k = %d" % s.align["footprint"]] = s
    fps = {k: [] for k in sess}

    def run(s, n):
        for i in range(n):
            s.push(*src[i % 16])
            if s.pending() == 2:
                s.pop()
        while s.pending():
            s.pop()

    with torch.no_grad():
        for s in sess.values():
            run(s, warmup)
        for _ in range(rounds):
            for k, s in sess.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(s, per_round)
                torch.cuda.synchronize()
                fps[k].append(per_round / (time.perf_counter() - t0))
    for s in sess.values():
        s.close()
    print(json.dumps(fps))


def child(tree, args, with_align):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--rounds", str(args.rounds), "--per-round", str(args.per_round)]
    out = subprocess.run(cmd + (["--with-align"] if with_align else []), stdout=subprocess.PIPE, text=True, check=True,
                         timeout=args.child_timeout, cwd=tree).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--per-round", type=int, default=30)
    ap.add_argument("--session-runs", type=int, default=2, help="child processes per tree")
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--no-session", action="store_true", help="the kernel part only")
    ap.add_argument("--bench", action="store_true", help="also run bench.py's headline, in child processes")
    ap.add_argument("--bench-runs", type=int, default=1)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--with-align", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return session_child(args.child, args.with_align, args.rounds, args.per_round)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    trees = {"this commit": ROOT, **({"parent commit": parent} if parent else {})}
    # child processes first: this process has not touched the device yet
    brows = []
    if args.bench:
        from live_conf_bench import bench_part
        brows = bench_part(trees, args.bench_runs)
    fps = {}
    if not args.no_session:
        for _ in range(args.session_runs):
            for name, tree in trees.items():
                for k, v in child(tree, args, tree == ROOT).items():
                    fps.setdefault((name, k), []).extend(v)
                    print(f"session, {name}, {k}: {np.median(v):.2f} frames/s", file=sys.stderr, flush=True)
    from codd_amd import ops
    ops.enable_autotune(False)
    krows, crate = kernel_part(args.calls)
    print(json.dumps(dict(kernel=krows, copy_rate=crate, session={"%s, %s" % k: v for k, v in fps.items()}, bench=brows)))
    lines = [f"codd_align_depth, {W}x{H} in {WP}x{HP} onto a {WT}x{HT} Brown camera, HIP events over {args.calls} calls after 20 warm-ups",
             "", "| footprint | uv_out | us / call, issued eagerly | us / call, graph replay | plain bytes | atomic dwords x 4 | plain bytes / graph time | target pixels reached |",
             "|---|---|---|---|---|---|---|---|"]
    lines += [f"| {r['k']} | {'yes' if r['uv'] else 'no'} | {r['eager_us']:.2f} | {r['graph_us']:.2f} | {r['bytes']} | {r['atomic_bytes']} | "
              f"{r['bytes'] / (r['graph_us'] * 1e-6) / 1e12:.2f} TB/s | {100 * r['reached']:.1f} % |" for r in krows]
    lines += ["", f"a 256 MiB device copy reaches {crate / 1e12:.2f} TB/s in the same run"]
    if fps:
        lines += ["", f"LiveSession push / pop with two frames in flight, {args.session_runs} processes per tree x {args.rounds} rounds x "
                  f"{args.per_round} frames, the sessions alternated in rounds and the trees by process", "",
                  "| tree | session | frames/s median | min | max |", "|---|---|---|---|---|"]
        lines += [f"| {name} | {k} | {np.median(v):.2f} | {min(v):.2f} | {max(v):.2f} |" for (name, k), v in fps.items()]
        mine = {k: float(np.median(v)) for (name, k), v in fps.items() if name == "this commit"}
        if len(mine) == 2:
            a, b = mine["without align_to"], [v for k, v in mine.items() if k != "without align_to"][0]
            lines += ["", f"cost of the aligned output per pipelined frame: {1e3 / b - 1e3 / a:.3f} ms"]
    if brows:
        lines += ["", "`bench.py --gpus 1 --steps 20 --warmup 5`, a process per run, the trees alternated (the flagship workload does "
                  "not run this code)", "", "| tree | frames/s per run | median |", "|---|---|---|"]
        lines += [f"| {r['tree']} | {', '.join(f'{v:.2f}' for v in r['fps'])} | {float(np.median(r['fps'])):.2f} |" for r in brows]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
