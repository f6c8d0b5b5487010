"""Host-to-host latency and throughput of the live session against the routes that existed before it.

One process, one run, 540x960 full CODD, graph replay, after warm-up; the variants are ALTERNATED in rounds so that
clock and thermal drift hit all of them alike:

  a       device-resident replay: FrameRunner.step on frames already preprocessed on the device (what bench.py times)
  b, b2   the route a user had to write: from_numpy().to(dev) x2 -> ops.preprocess x2 -> FrameRunner.step -> crop ->
          .cpu(); b2 is the same thing again -- the difference between the two is the spread of this measurement
  c       LiveSession.step (synchronous), c_rect with rectification maps
  d       LiveSession.push / pop pipelined, d_rect with rectification maps

    python tools/live_latency.py [--rounds 8 --per-round 25] [--out profiles/live_session.md]
    rocprofv3 --kernel-trace --stats -- python tools/live_latency.py --trace c,c_rect    # ingest / export kernel times
    rocprofv3 --kernel-trace --memory-copy-trace -- python tools/live_latency.py --trace d    # do the copies overlap?
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 540, 960


def frames(n):
    from codd_amd import synth
    img, r_img, _ = synth.stereo_sequence(H, W, n)

    def u8(t):
        return np.ascontiguousarray((t * 58.0 + 118.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())

    return [(u8(img[0, i]), u8(r_img[0, i])) for i in range(n)]


def radial_maps():
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    r2 = ((xx - cx) ** 2 + (yy - cy) ** 2) / (cx * cx + cy * cy)
    m = (xx + 4.0 * r2 * (xx - cx) / cx).astype(np.float32), (yy + 4.0 * r2 * (yy - cy) / cy).astype(np.float32)
    return (m, m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    ap.add_argument("--trace", default=None, metavar="VARIANTS", help="run only 40 untimed frames of these live variants "
                    "(comma-separated from c, c_rect, d, d_rect) -- for a profiler trace")
    args = ap.parse_args()
    from codd_amd import configs, ops, synth
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    from codd_amd.runtime import FrameRunner
    dev = torch.device("cuda:0")
    est = build_estimator(configs.codd()).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    est = est.to(dev)
    ops.enable_autotune(True)  # as bench.py and the CLI run
    src = frames(16)
    HP, WP = -(-H // 64) * 64, -(-W // 64) * 64
    metas = synth.default_metas(HP, WP, img_shape=(H, W, 3))[0]
    resident = [(ops.preprocess(torch.from_numpy(a).to(dev), bgr=False), ops.preprocess(torch.from_numpy(b).to(dev), bgr=False))
                for a, b in src]
    state = dict(i=0)

    def nxt():
        state["i"] += 1
        return state["i"] % len(src)

    run_a, run_b, run_b2 = (FrameRunner(est, metas, use_graph=True) for _ in range(3))
    sess = {k: LiveSession(est, (H, W), output="disp", rectify=radial_maps() if k.endswith("rect") else None)
            for k in (args.trace.split(",") if args.trace else ["c", "c_rect", "d", "d_rect"])}

    def do_a(n, lat):
        for _ in range(n):
            run_a.step(*resident[nxt()])
        torch.cuda.synchronize()

    def parent(runner):
        def go(n, lat):
            for _ in range(n):
                a, b = src[nxt()]
                t0 = time.perf_counter()
                dl = ops.preprocess(torch.from_numpy(a).to(dev), bgr=False)
                dr = ops.preprocess(torch.from_numpy(b).to(dev), bgr=False)
                runner.step(dl, dr)[0, 0, :H, :W].cpu()
                lat.append(time.perf_counter() - t0)
        return go

    def sync(s):
        def go(n, lat):
            for _ in range(n):
                a, b = src[nxt()]
                t0 = time.perf_counter()
                s.step(a, b)
                lat.append(time.perf_counter() - t0)
        return go

    def piped(s):
        def go(n, lat):
            for _ in range(n):
                if s.pending() == 2:
                    s.pop()
                s.push(*src[nxt()])
            while s.pending():
                s.pop()
        return go

    variants = {k: (sync if k.startswith("c") else piped)(s) for k, s in sess.items()}
    if not args.trace:
        variants = {"a": do_a, "b": parent(run_b), "b2": parent(run_b2), **variants}
    with torch.no_grad():
        for fn in variants.values():
            fn(args.warmup, [])
        torch.cuda.synchronize()
        if args.trace:
            for fn in variants.values():
                fn(40, [])
            torch.cuda.synchronize()
            return
        wall = {k: 0.0 for k in variants}
        lats = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(args.per_round, lats[k])
                torch.cuda.synchronize()
                wall[k] += time.perf_counter() - t0
    n = args.rounds * args.per_round
    rows = []
    for k in variants:
        lat = np.array(lats[k]) * 1e3
        rows.append(dict(variant=k, frames=n, fps=n / wall[k], ms_per_frame=1e3 * wall[k] / n,
                         lat_mean_ms=float(lat.mean()) if lat.size else None,
                         lat_worst_ms=float(lat.max()) if lat.size else None))
    by = {r["variant"]: r for r in rows}
    spread = abs(by["b"]["ms_per_frame"] - by["b2"]["ms_per_frame"])
    res = dict(shape=[H, W], rounds=args.rounds, per_round=args.per_round, rows=rows, spread_b_ms=spread,
               d_ge_b=by["d"]["fps"] >= max(by["b"]["fps"], by["b2"]["fps"]),
               c_le_b_by_more_than_spread=by["c"]["lat_mean_ms"] < min(by["b"]["lat_mean_ms"], by["b2"]["lat_mean_ms"]) - spread)
    print(json.dumps(res))
    f2 = lambda v: "-" if v is None else f"{v:.2f}"  # noqa: E731
    lines = ["| variant | frames | frames/s | ms/frame | host-to-host mean ms | worst ms |", "|---|---|---|---|---|---|"]
    lines += [f"| {r['variant']} | {r['frames']} | {r['fps']:.1f} | {f2(r['ms_per_frame'])} | {f2(r['lat_mean_ms'])} | "
              f"{f2(r['lat_worst_ms'])} |" for r in rows]
    lines.append(f"\nspread of (b), |b - b2|: {spread:.3f} ms/frame")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for s in sess.values():
        s.close()


if __name__ == "__main__":
    main()
