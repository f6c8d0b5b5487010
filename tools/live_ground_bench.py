"""Cost of LiveSession's ground plane (codd_ground_plane), 540x960 in 576x960, defaults with a 128x128 grid.

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, on a scene of tests/live_ground_ref.py at that size (a pitched and rolled camera 1.2 above a floor with
   three boxes, sky, a NaN band and 0.05 px of noise): the defaults with the grid and the heights, then one thing changed
   at a time -- no grid, no heights, step 1, iters 4 (the difference to iters 8 is four weighted passes), a seed.
2. The host route this replaces, timed in the same process: the download of the padded disparity into pinned memory, then
   tests/live_ground_ref.py's numpy fit (float64), classification and grid, medians over --host-runs.
3. LiveSession.step frames/s with ground= against without: sessions on one estimator, alternated in rounds, median over
   the rounds.  With --parent-tree DIR (a built checkout of the parent commit) the parent's LiveSession without ground= is
   measured too: every tree in a child process of its own, the trees alternated --tree-runs times.

    python tools/live_ground_bench.py [--calls 200 --rounds 5 --per-round 25] [--parent-tree DIR] [--out profiles/live_ground.md]

Kernel times: ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ground -- python tools/live_ground_bench.py
--defaults-only --no-session --calls 100`` (a run of its own: tracing slows the host).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, HP, WP = 540, 960, 576, 960
DEV = "cuda:0"
GRID, CELL = (128, 128), 0.1
GROUND = dict(map=True, grid=GRID, cell=CELL)
SPEC = dict(crop=(H, W), padded=(HP, WP), K=(1050.0, 1050.0, 479.5, 269.5), calib=210.0, cam_h=1.2, pitch=0.15, roll=0.03,
            name="bench", scene="bench", par={}, seed=None, grid=(GRID, CELL))
BOXES = [(60, 300, 150, 400), (380, 620, 190, 470), (700, 900, 170, 360)]
VARIANTS = [("defaults (step 2, iters 8), heights, 128x128 grid", {}, {}), ("no grid", {}, dict(grid=False)),
            ("no heights", {}, dict(height=False)), ("step 1", dict(step=1), {}), ("iters 4", dict(iters=4), {}),
            ("seeded (height 1.0, pitch off by 0.08 rad)", {}, dict(seed=True))]


def time_calls(fn, n, warmup=20):
    """(eager us / call, graph-replayed us / call) by HIP events; the graph holds ONE call and is replayed n times."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    eager = 1e3 * e0.elapsed_time(e1) / n
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        e0.record()
        for _ in range(n):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        reps.append(1e3 * e0.elapsed_time(e1) / n)
    return eager, float(np.median(reps))


def scene():
    import live_ground_ref as lg
    lg.SCENES["bench"] = dict(boxes=BOXES)
    return lg, lg.case(SPEC)


def kernel_part(n, defaults_only=False):
    from codd_amd import ops
    lg, c = scene()
    disp = torch.from_numpy(c["disp"]).to(DEV)
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    lab, hgt = torch.empty(H, W, dtype=torch.uint8, device=DEV), torch.empty(H, W, device=DEV)
    cnt, gh = torch.empty((2,) + GRID, dtype=torch.int32, device=DEV), torch.empty(GRID, device=DEV)
    scratch = torch.empty(ops.ground_scratch(H, W, GRID), dtype=torch.uint8, device=DEV)
    seed = lg.plane_coef(1.0, c["K"], c["calib"], lg.up_vector(SPEC["pitch"] + 0.08))
    yy, xx = np.mgrid[0:H, 0:W]
    rows = []
    for name, over, sw in (VARIANTS[:1] if defaults_only else VARIANTS):
        par = dict(ops.GROUND_PARAMS, cell=CELL, **over)
        grid = (cnt, gh) if sw.get("grid", True) else (None, None)
        fn = lambda: ops.ground_plane(disp, c["K"], c["calib"], (H, W), rec, lab, hgt if sw.get("height", True) else None,  # noqa: E731
                                      *grid, scratch=scratch, seed=seed if sw.get("seed") else None, **par)
        eager, graph = time_calls(fn, n)
        r = rec.cpu().numpy()
        err = np.abs(lg.plane_disp(r[:3], c["K"], xx, yy) - lg.plane_disp(c["plant"], c["K"], xx, yy))[c["floor"]].max()
        rows.append(dict(variant=name, launches=par["iters"] + 1, eager_us=eager, graph_us=graph, ok=bool(r[3]), fit=int(r[4]),
                         inliers=int(r[5]), camera_height=float(r[11]), plane_err_px=float(err),
                         grid_pixels=int(cnt.sum().item()) if grid[0] is not None else 0))
    return rows


def host_part(runs):
    """The route a user had to write: download, numpy fit, classification and grid -> median milliseconds of each."""
    lg, c = scene()
    disp = torch.from_numpy(c["disp"]).to(DEV)
    pinned = torch.empty(HP, WP, pin_memory=True)
    t = dict(download=[], fit=[], classify_and_grid=[])
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(disp, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = dict(c, disp=pinned.numpy())
        f = lg.fit(host, np.float64)
        m = lg.metric(host, f)
        t2 = time.perf_counter()
        lg.pixels(host, f, m, np.float64)
        t3 = time.perf_counter()
        for k, v in zip(t, (t1 - t0, t2 - t1, t3 - t2)):
            t[k].append(1e3 * v)
    return {k: float(np.median(v)) for k, v in t.items()}, bool(m["ok"])


def session_part(rounds, per_round, variants, warmup=6):
    """LiveSession.step frames/s of each ``variants`` entry (name -> LiveSession keywords), alternated in rounds."""
    from codd_amd import configs, ops, synth
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd()).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    est = est.to(DEV)
    ops.enable_autotune(True)  # as bench.py and the CLI run
    img, r_img, _ = synth.stereo_sequence(H, W, 16)
    u8 = lambda t: np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())  # noqa: E731
    src = [(u8(img[0, i]), u8(r_img[0, i])) for i in range(16)]
    sess = {k: LiveSession(est, (H, W), output="depth", **kw) for k, kw in variants.items()}
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


def tree_part(trees, runs, rounds, per_round, timeout=600):
    """LiveSession.step frames/s without ground= per tree, one child process per run (this file with --tree), alternated."""
    fps = {k: [] for k in trees}
    for _ in range(runs):
        for k, root in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", root, "--rounds", str(rounds),
                                  "--per-round", str(per_round)], stdout=subprocess.PIPE, text=True, check=True,
                                 timeout=timeout).stdout
            fps[k].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["fps_median"])
            print(f"LiveSession without ground=, {k}: {fps[k][-1]:.2f} frames/s", file=sys.stderr, flush=True)
    return [dict(tree=k, fps=v) for k, v in fps.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--no-session", action="store_true", help="the kernel and host parts only")
    ap.add_argument("--defaults-only", action="store_true", help="the default parameters only (for a kernel trace)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its LiveSession too")
    ap.add_argument("--tree-runs", type=int, default=2)
    ap.add_argument("--tree", default=None, help="(child) LiveSession without ground= of the package in this tree; one JSON line")
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if args.tree:
        print(json.dumps(session_part(args.rounds, args.per_round, {"no ground": {}})[0]))
        return
    # (first: this process has not touched the device yet)
    trows = []
    if args.parent_tree and not args.no_session:
        trows = tree_part({"this commit": ROOT, "parent commit": os.path.abspath(args.parent_tree)}, args.tree_runs, args.rounds,
                          args.per_round)
    from codd_amd import ops
    ops.enable_autotune(False)
    krows = kernel_part(args.calls, args.defaults_only)
    host, host_ok = ({}, False) if args.defaults_only else host_part(args.host_runs)
    srows = [] if args.no_session else session_part(args.rounds, args.per_round, {"ground=False": {}, "ground=dict(map=True, "
                                                    "grid=(128, 128))": dict(ground=GROUND)})
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], calls=args.calls, kernel=krows, host=host, session=srows, trees=trows)))
    lines = [f"codd_ground_plane at {W}x{H} in {WP}x{HP}, HIP events over {args.calls} calls after 20 warm-ups; a camera 1.2 above a "
             f"floor, pitched by 0.15 rad and rolled by 0.03 rad, three boxes, sky, a NaN band, 0.05 px of noise; grid "
             f"{GRID[0]}x{GRID[1]} cells of {CELL}", "",
             "| variant | launches | us / call, issued eagerly | us / call, graph replay | ok | fit pixels | inliers | camera height | "
             "worst plane error on the floor, px | pixels in the grid |", "|---|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {r['variant']} | {r['launches']} | {r['eager_us']:.2f} | {r['graph_us']:.2f} | {r['ok']} | {r['fit']} | {r['inliers']} | "
              f"{r['camera_height']:.4f} | {r['plane_err_px']:.4f} | {r['grid_pixels']} |" for r in krows]
    if host:
        total = sum(host.values())
        lines += ["", f"the host route it replaces, same scene, medians over {args.host_runs} runs (numpy, float64; floor found: "
                  f"{host_ok}): download of the padded disparity {host['download']:.3f} ms, fit (8 re-weighted steps over the "
                  f"fit pixels) {host['fit']:.3f} ms, classification and grid {host['classify_and_grid']:.3f} ms: {total:.3f} ms "
                  f"per frame against {krows[0]['graph_us'] / 1e3:.3f} ms"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max |", "|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} |"
                  for r in srows]
        a, b = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the ground output per synchronous frame: {1e3 / b - 1e3 / a:.3f} ms of {1e3 / a:.3f} ms"]
    if trows:
        lines += ["", "LiveSession.step without ground=, a process per run, the trees alternated (the same launches in both)", "",
                  "| tree | frames/s per run | median | min | max |", "|---|---|---|---|---|"]
        lines += [f"| {r['tree']} | {', '.join(f'{v:.2f}' for v in r['fps'])} | {float(np.median(r['fps'])):.2f} | {min(r['fps']):.2f} | "
                  f"{max(r['fps']):.2f} |" for r in trows]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
