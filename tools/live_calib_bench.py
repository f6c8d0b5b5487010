"""Cost of the ingest launch with the rectifying map evaluated in registers (codd_ingest_calibrated) against streaming it
from map arrays (codd_ingest_pair / codd_ingest_frames), 540x960 in 576x960, rgb8 and nv12.

Routes, each one launch:
  maps-identity    the parent's path with identity maps resident (16 B of map per output pixel);
  maps-brown       the parent's path with the maps codd_rectify_maps writes for the brown rig (the taps wander as the
                   fused routes' do);
  fused-brown, fused-fisheye                 codd_ingest_calibrated, source 540x960;
  fused-brown-1280x800, fused-fisheye-...    codd_ingest_calibrated, source 800x1280.
Each route is captured into a graph of ONE call; a round replays every route's graph N times between two HIP events, the
routes alternated inside the round; reported are the median and the min .. max over the rounds, in us per call (device
time, launch gap of a graph replay included).  One process, one device.

    python tools/live_calib_bench.py [--calls 200 --rounds 9] [--out profiles/live_calib.md] [--raw profiles/live_calib_raw.jsonl]
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

H, W = 540, 960
HP, WP = 576, 960
BIG = (800, 1280)
DEV = "cuda:0"


def rig(model, size):
    import live_calib_ref as cr
    from codd_amd.calibration import CameraModel, StereoCalibration
    (Kl, dl), (Kr, dr), R, T = cr.make_rig(model, size)
    return StereoCalibration(CameraModel(size, Kl, model, dl), CameraModel(size, Kr, model, dr), R, T)


def source(fmt, size, rng):
    hs, ws = size
    n = hs * ws * 3 if fmt == "rgb8" else hs * ws * 3 // 2
    a = torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)).to(DEV)
    return a.view(hs, ws, 3) if fmt == "rgb8" else a


def routes(fmt):
    from codd_amd import ops
    rng = np.random.default_rng(5)
    out = tuple(torch.empty(1, 3, HP, WP, device=DEV) for _ in range(2))
    small = tuple(source(fmt, (H, W), rng) for _ in range(2))
    big = tuple(source(fmt, BIG, rng) for _ in range(2))
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=DEV), torch.arange(W, dtype=torch.float32, device=DEV),
                            indexing="ij")
    ident = ((xx.contiguous(), yy.contiguous()), (xx.clone(), yy.clone()))
    rects = {(m, s): ops.calib_structs(rig(m, s).rectify((H, W))) for m in ("brown", "fisheye") for s in ((H, W), BIG)}
    brown_maps = ops.rectify_maps(rects[("brown", (H, W))], (H, W), DEV)

    def via_maps(maps):
        if fmt == "rgb8":
            return lambda: ops.ingest_pair(small[0], small[1], out[0], out[1], bgr=False, maps=maps)
        return lambda: ops.ingest_frames(small[0], small[1], out[0], out[1], fmt, (H, W), maps=maps)

    def fused(model, size):
        src = small if size == (H, W) else big
        return lambda: ops.ingest_calibrated(src[0], src[1], out[0], out[1], rects[(model, size)], fmt, size, (H, W))

    r = {"maps-identity": via_maps(ident), "maps-brown": via_maps(brown_maps)}
    for model in ("brown", "fisheye"):
        r[f"fused-{model}"] = fused(model, (H, W))
    for model in ("brown", "fisheye"):
        r[f"fused-{model}-{BIG[1]}x{BIG[0]}"] = fused(model, BIG)
    return r


def capture(fn, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--raw", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "live_calib_bench needs a GPU: there is nothing to time without one"
    raw, rows = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fmt in ("rgb8", "nv12"):
        graphs = {name: capture(fn) for name, fn in routes(fmt).items()}
        times = {name: [] for name in graphs}
        for rnd in range(args.rounds):
            for name, g in graphs.items():
                e0.record()
                for _ in range(args.calls):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                us = 1e3 * e0.elapsed_time(e1) / args.calls
                times[name].append(us)
                raw.append(dict(fmt=fmt, route=name, round=rnd, calls=args.calls, us_per_call=us))
                print(json.dumps(raw[-1]), flush=True)
        for name, t in times.items():
            rows.append((fmt, name, float(np.median(t)), min(t), max(t)))
    lines = [f"Ingest launch, {H}x{W} in {HP}x{WP}, graph replays, {args.calls} calls x {args.rounds} rounds, us per call on "
             f"{torch.cuda.get_device_name(0)}:", "", "| format | route | median | min | max |", "|---|---|---|---|---|"]
    lines += [f"| {f} | {n} | {m:.2f} | {lo:.2f} | {hi:.2f} |" for f, n, m, lo, hi in rows]
    text = "\n".join(lines) + "\n"
    print(text)
    for path, body in ((args.out, text), (args.raw, "".join(json.dumps(r) + "\n" for r in raw))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(body)


if __name__ == "__main__":
    main()
