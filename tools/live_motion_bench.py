"""Cost of LiveSession's motion output (codd_export_motion), 540x960 in 576x960.

1. The launch itself against the three-launch route that yields the same numbers on the parent commit
   (ops.disp_to_depth + ops.induced_flow + a torch crop), HIP events around N launches after warm-up, two ways:
   issued eagerly (host issue cost included: what a frame outside the graph pays) and replayed from a captured graph
   (device time only, launch gaps included).
2. LiveSession.step frames/s with motion="sceneflow" against motion=None: one process, both sessions on one estimator,
   alternated in rounds, median over the rounds.

    python tools/live_motion_bench.py [--launches 200 --rounds 5 --per-round 25] [--out profiles/live_motion.md]
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


def time_launches(fn, n, warmup=20):
    """(eager us / call, graph-replayed us / call) by HIP events."""
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
            for _ in range(n):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        reps.append(1e3 * e0.elapsed_time(e1) / n)
    return eager, float(np.median(reps))


def kernel_part(n):
    import live_motion_ref as lm
    from codd_amd import ops
    dev = "cuda:0"
    c = lm.case(HP, WP)
    T, K, bf = c["T"].to(dev), c["K"], c["bf"]
    disp = (torch.rand(1, 1, HP, WP, generator=torch.Generator().manual_seed(1)) * 300.0 + 0.5).to(dev)
    depth_prev = c["depth"][0].to(dev).contiguous()
    rows = []
    for mode in lm.MODES:
        out = torch.empty(H, W, lm.CHANNELS[mode], device=dev)
        eager, graph = time_launches(lambda: ops.export_motion(T, disp, depth_prev, out, mode, K, bf, scale=0.37), n)
        rows.append(dict(route=f"codd_export_motion {mode}", launches=1, eager_us=eager, graph_us=graph))
    dprev3 = c["depth"].to(dev).contiguous()  # [1,HP,WP]

    def parent():
        ops.disp_to_depth(disp, bf)  # the depth the NEXT frame's field refers to
        return ops.induced_flow(T, dprev3, list(K))[0, :H, :W].contiguous()

    eager, graph = time_launches(parent, n)
    rows.append(dict(route="disp_to_depth + induced_flow + crop (flow_dd's numbers / bf)", launches=3, eager_us=eager,
                     graph_us=graph))
    return rows


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
    est = est.to("cuda:0")
    ops.enable_autotune(True)  # as bench.py and the CLI run
    src = frames(16)
    sess = {"motion=None": LiveSession(est, (H, W), output="depth"),
            "motion=sceneflow": LiveSession(est, (H, W), output="depth", motion="sceneflow")}
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
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    from codd_amd import ops
    ops.enable_autotune(False)
    krows = kernel_part(args.launches)
    srows = session_part(args.rounds, args.per_round)
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], launches=args.launches, kernel=krows, session=srows)))
    lines = [f"codd_export_motion at {W}x{H} in {WP}x{HP}, HIP events over {args.launches} launches after 20 warm-ups", "",
             "| route | launches | us / call, issued eagerly | us / call, graph replay |", "|---|---|---|---|"]
    lines += [f"| {r['route']} | {r['launches']} | {r['eager_us']:.2f} | {r['graph_us']:.2f} |" for r in krows]
    lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
              "| session | rounds x frames | frames/s median | min | max |", "|---|---|---|---|---|"]
    lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} |"
              for r in srows]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
