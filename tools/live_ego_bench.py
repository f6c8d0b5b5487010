"""Cost of LiveSession's ego-motion output (codd_ego_motion), 540x960 in 576x960.

1. The iters + 1 launches of one call, replayed from a captured graph (device time, launch gaps included) and issued
   eagerly, HIP events over N calls after 20 warm-ups; against the route a user writes today: the same algorithm as torch
   ops on the device (tests/live_ego_ref.py evaluate32: fp32 per-pixel terms, fp64 sums, the 6x6 solve on the host in
   every iteration), wall clock around synchronised calls because its host syncs cannot be captured.
2. LiveSession.step frames/s with egomotion=True against egomotion=False: one process, both sessions on one estimator,
   alternated in rounds, median over the rounds.

    python tools/live_ego_bench.py [--calls 200 --rounds 5 --per-round 25] [--out profiles/live_ego.md]
"""
import argparse
import json
import os
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


def kernel_part(n, torch_calls=10):
    import live_ego_ref as le
    from codd_amd import ops
    s = le.scene(((H, W), (HP, WP)), True, seed=0)
    T, depth, K = s["T"].to(DEV), s["depth"].to(DEV), s["K"]
    rec = torch.zeros(16, device=DEV)
    mov = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    res = torch.empty(H, W, device=DEV)
    scratch = torch.empty(ops.ego_motion_scratch(H, W), dtype=torch.uint8, device=DEV)
    rows = []
    for iters in (1, 5):  # (the record of the last call, iters=5, is compared with the torch route below)
        eager, graph = time_calls(lambda: ops.ego_motion(T, depth[0], K, (H, W), rec, mov, res, scale=le.SCALE, iters=iters,
                                                         scratch=scratch), n)
        rows.append(dict(route=f"codd_ego_motion iters={iters}", launches=iters + 1, eager_us=eager, graph_us=graph))
    record = rec.cpu()
    # the torch route: the same definition as device tensor ops
    with torch.device(DEV):
        for _ in range(2):
            trec, tmov, tres = le.evaluate32(T, depth, K, (H, W), scale=le.SCALE)
        torch.cuda.synchronize()
        ts = []
        for _ in range(torch_calls):
            t0 = time.perf_counter()
            le.evaluate32(T, depth, K, (H, W), scale=le.SCALE)
            torch.cuda.synchronize()
            ts.append(1e6 * (time.perf_counter() - t0))
    rows.append(dict(route="torch ops on the device (evaluate32), iters=5", launches=None, eager_us=float(np.median(ts)), graph_us=None))
    agree = dict(pose_max_abs_diff=float((record[:7] - trec.cpu()[:7]).abs().max()),
                 mask_pixels_differing=int((mov.cpu() != tmov.cpu()).sum()), record=record[:12].tolist())
    return rows, agree


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
    sess = {"egomotion=False": LiveSession(est, (H, W), output="depth"),
            "egomotion=True": LiveSession(est, (H, W), output="depth", egomotion=True)}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--no-session", action="store_true", help="the kernel part only")
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    from codd_amd import ops
    ops.enable_autotune(False)
    krows, agree = kernel_part(args.calls)
    srows = [] if args.no_session else session_part(args.rounds, args.per_round)
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], calls=args.calls, kernel=krows, agreement=agree, session=srows)))
    us = lambda v: "-" if v is None else f"{v:.2f}"  # noqa: E731
    lines = [f"codd_ego_motion at {W}x{H} in {WP}x{HP}, HIP events over {args.calls} calls after 20 warm-ups (the torch route: "
             "median wall clock of 10 synchronised calls)", "",
             "| route | launches | us / call, issued eagerly | us / call, graph replay |", "|---|---|---|---|"]
    lines += [f"| {r['route']} | {r['launches'] or 'dozens + host syncs'} | {us(r['eager_us'])} | {us(r['graph_us'])} |" for r in krows]
    lines += ["", f"torch route / kernel (graph replay, iters=5): {krows[-1]['eager_us'] / krows[1]['graph_us']:.0f} x; "
              f"torch route / kernel (eager): {krows[-1]['eager_us'] / krows[1]['eager_us']:.0f} x", "",
              f"kernel against the torch route on this scene: pose differs by at most {agree['pose_max_abs_diff']:.2e}, "
              f"{agree['mask_pixels_differing']} mask pixels differ"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max |", "|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} |"
                  for r in srows]
        a, b = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the ego-motion output per synchronous frame: {1e3 / b - 1e3 / a:.3f} ms"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
