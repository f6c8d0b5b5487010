"""Cost of LiveSession's stereo-confidence output (codd_export_confidence), 540x960 in 576x960.

1. One call replayed from a captured graph (device time, launch gap included) and issued eagerly, HIP events over N calls
   after 20 warm-ups; against the route a user writes today: the same computation as torch ops on the device
   (scatter-amax per row for the z-buffer, gathers for its read-back and the two right-image taps, element-wise ops for
   the rest), timed the same two ways.  The bytes the kernel must move (one disparity plane, six image planes, 5 bytes out
   per pixel) over the graph-replayed time are reported as a fraction of the HBM rate.
2. LiveSession.step frames/s with confidence=True against confidence=False: one process, both sessions on one estimator,
   alternated in rounds, median over the rounds.
3. With --bench: ``bench.py --gpus 1 --steps 20 --warmup 5`` of this tree and, with --parent-tree DIR, of a built checkout
   of the parent commit there, each in a child process of its own, the two alternated --bench-runs times.

    python tools/live_conf_bench.py [--calls 200 --rounds 5 --per-round 25] [--bench [--parent-tree DIR]] [--out profiles/live_conf.md]
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 540, 960
HP, WP = 576, 960
DEV = "cuda:0"
HBM_SPEC = 8.0e12  # bytes/s, the MI355X data sheet; the rate a plain copy reaches is measured in the same run (copy_rate)


def time_calls(fn, n, warmup=20, graph=True):
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
    if not graph:
        return eager, None
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


def copy_rate(n, nbytes=1 << 28):
    """bytes/s (read + written) of a device-to-device copy of ``nbytes``, far beyond the caches: the yardstick for 'HBM rate'."""
    src = torch.empty(nbytes // 4, device=DEV).normal_()
    dst = torch.empty_like(src)
    _, us = time_calls(lambda: dst.copy_(src), max(n // 4, 10))
    return 2 * nbytes / (us * 1e-6)


def torch_route(disp, left, right, h, w, std, occ_px, tau):
    """The same flags and residual with torch ops on the device -> (flags uint8 [h,w], residual fp32 [h,w])."""
    d = disp[:h, :w]
    x = torch.arange(w, device=d.device, dtype=torch.float32)[None]
    valid = torch.isfinite(d) & (d > 0)
    u = x - d
    inview = valid & ~(u < 0)
    fu = torch.floor(torch.where(inview, u, torch.zeros_like(u)))
    f = fu.long()
    offer = torch.where(inview, d, torch.zeros_like(d))
    z = torch.zeros(h, w, device=d.device)
    z.scatter_reduce_(1, f, offer, "amax")
    f1 = f + 1
    z.scatter_reduce_(1, f1.clamp(max=w - 1), torch.where(f1 < w, offer, torch.zeros_like(d)), "amax")
    r = torch.floor(torch.where(inview, u + 0.5, torch.zeros_like(u))).long()
    occluded = inview & (z.gather(1, r) > d + occ_px)
    a = torch.where(inview, u, torch.zeros_like(u)) - fu
    x1 = f1.clamp(max=w - 1)
    L, R = left[:, :h, :w], right[:, :h, :w]
    Rv = R.gather(2, f[None].expand(3, h, w)) * (1 - a) + R.gather(2, x1[None].expand(3, h, w)) * a
    res = ((L - Rv).abs() * std[:, None, None]).sum(0) * (1.0 / 3.0)
    res = torch.where(inview, res, torch.full_like(res, float("nan")))
    flags = (~valid).to(torch.uint8) * 128 + (valid & (u < 0)).to(torch.uint8) + occluded.to(torch.uint8) * 2 \
        + (res > tau).to(torch.uint8) * 4
    return flags, res


def kernel_part(n):
    import live_conf_ref as lc
    from codd_amd import ops
    c = lc.case(((H, W), (HP, WP)))
    disp, left, right = (torch.from_numpy(c[k]).to(DEV) for k in ("disp", "left", "right"))
    flags = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    res = torch.empty(H, W, device=DEV)
    std = torch.tensor(ops.IMAGENET_STD, device=DEV)
    rows = []
    eager, graph = time_calls(lambda: ops.export_confidence(disp, flags, res, left, right, occ_px=lc.OCC_PX, tau=lc.TAU), n)
    rows.append(dict(route="codd_export_confidence", launches=1, eager_us=eager, graph_us=graph))
    eager, graph = time_calls(lambda: ops.export_confidence(disp, flags, None, None, None, occ_px=lc.OCC_PX), n)
    rows.append(dict(route="codd_export_confidence, no images (flags 1, 2, 128 only)", launches=1, eager_us=eager, graph_us=graph))
    ops.export_confidence(disp, flags, res, left, right, occ_px=lc.OCC_PX, tau=lc.TAU)
    route = lambda: torch_route(disp, left, right, H, W, std, lc.OCC_PX, lc.TAU)  # noqa: E731
    try:
        eager, graph = time_calls(route, n)
    except RuntimeError as e:  # (an op of the route that cannot be captured: the eager figure alone)
        print("torch route: graph capture failed:", e, file=sys.stderr)
        eager, graph = time_calls(route, n, graph=False)
    rows.append(dict(route="torch ops on the device (scatter-amax, gathers, element-wise)", launches=None, eager_us=eager, graph_us=graph))
    tflags, tres = torch_route(disp, left, right, H, W, std, lc.OCC_PX, lc.TAU)
    torch.cuda.synchronize()
    agree = dict(flag_bytes_differing=int((tflags != flags).sum()),
                 residual_max_abs_diff=float(torch.nan_to_num(tres - res).abs().max()),
                 pixels_per_flag=[int(((flags & b) != 0).sum()) for b in (1, 2, 4, 128)])
    nbytes = H * W * (4 + 6 * 4 + 5)
    traffic = dict(bytes=nbytes, rate=nbytes / (rows[0]["graph_us"] * 1e-6), copy_rate=copy_rate(n))
    return rows, agree, traffic


def frames(n):
    from codd_amd import synth
    img, r_img, _ = synth.stereo_sequence(H, W, n)

    def u8(t):
        return np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())

    return [(u8(img[0, i]), u8(r_img[0, i])) for i in range(n)]


def session_part(rounds, per_round, warmup=6):
    from codd_amd import configs, ops, synth
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd()).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    est = est.to(DEV)
    ops.enable_autotune(True)  # as bench.py and the CLI run
    src = frames(16)
    sess = {"confidence=False": LiveSession(est, (H, W), output="depth"),
            "confidence=True": LiveSession(est, (H, W), output="depth", confidence=True)}
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


def bench_part(trees, runs, timeout=300):
    """bench.py's headline (frames/s) per tree, one child process per run, the trees alternated."""
    fps = {k: [] for k in trees}
    for _ in range(runs):
        for k, root in trees.items():
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=root,
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
    ap.add_argument("--bench", action="store_true", help="also run bench.py's headline, in child processes")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its bench.py headline too")
    ap.add_argument("--bench-runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    trees = {"this commit": ROOT, **({"parent commit": os.path.abspath(args.parent_tree)} if args.parent_tree else {})}
    brows = bench_part(trees, args.bench_runs) if args.bench else []  # (first: this process has not touched the device yet)
    from codd_amd import ops
    ops.enable_autotune(False)
    krows, agree, traffic = kernel_part(args.calls)
    srows = [] if args.no_session else session_part(args.rounds, args.per_round)
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], calls=args.calls, kernel=krows, agreement=agree, traffic=traffic,
                          session=srows, bench=brows)))
    us = lambda v: "-" if v is None else f"{v:.2f}"  # noqa: E731
    lines = [f"codd_export_confidence at {W}x{H} in {WP}x{HP}, HIP events over {args.calls} calls after 20 warm-ups", "",
             "| route | launches | us / call, issued eagerly | us / call, graph replay |", "|---|---|---|---|"]
    lines += [f"| {r['route']} | {r['launches'] or 'dozens'} | {us(r['eager_us'])} | {us(r['graph_us'])} |" for r in krows]
    lines += ["", f"torch route / kernel (graph replay): {(krows[2]['graph_us'] or krows[2]['eager_us']) / krows[0]['graph_us']:.1f} x; "
              f"(eager): {krows[2]['eager_us'] / krows[0]['eager_us']:.1f} x", "",
              f"bytes the kernel must move (one disparity plane, six image planes, 5 bytes out per pixel): {traffic['bytes']}; over "
              f"the graph-replayed time: {traffic['rate'] / 1e12:.2f} TB/s = {100 * traffic['rate'] / traffic['copy_rate']:.0f} % of the "
              f"{traffic['copy_rate'] / 1e12:.2f} TB/s a 256 MiB device copy reaches in the same run ({100 * traffic['rate'] / HBM_SPEC:.0f} % of the "
              f"{HBM_SPEC / 1e12:.1f} TB/s data-sheet rate)", "",
              f"kernel against the torch route on this scene: {agree['flag_bytes_differing']} flag bytes differ, residuals differ "
              f"by at most {agree['residual_max_abs_diff']:.2e} grey levels; pixels per flag (1, 2, 4, 128): {agree['pixels_per_flag']}"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max |", "|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} |"
                  for r in srows]
        a, b = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the confidence output per synchronous frame: {1e3 / b - 1e3 / a:.3f} ms"]
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
