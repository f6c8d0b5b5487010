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

Raw camera formats (LiveSession(pixel_format=)): `--pixel-format all` adds one pipelined variant d:<format> per format, fed
raw frames of the same images, and an upload-bytes column; the ingest kernel alone, every format map-free and rectified
next to rgb8's ingest_kernel<0, ArrayMaps> (three times, for the spread), is timed per dispatch from a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/live_latency.py --pixel-format all --ingest-kernels 40
    python tools/live_latency.py --pixel-format all --ingest-kernels 40 --parse-trace DIR/t_kernel_trace.csv    # the table
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


def raw_of(rgb, fmt):
    """A raw ``fmt`` frame that looks like the RGB image (tight, shaped rows x pitch): the mosaic a sensor records, G as
    luma, (B, R) halved around 128 as chroma sub-sampled by dropping.  Any bytes are a valid frame; timing does not
    depend on them, the network's run time on an image-like input is what a user sees."""
    if fmt == "rgb8":
        return rgb
    if fmt.startswith("bayer_"):
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ch = np.array(["rgb".index(c) for c in fmt[6:]])[2 * (yy & 1) + (xx & 1)]
        return np.ascontiguousarray(np.take_along_axis(rgb, ch[..., None], axis=2)[..., 0])
    Y, U, V = rgb[..., 1], (rgb[..., 2] >> 1) + 64, (rgb[..., 0] >> 1) + 64
    if fmt == "mono8":
        return np.ascontiguousarray(Y)
    if fmt == "nv12":
        uv = np.stack([U[0::2, 0::2], V[0::2, 0::2]], axis=-1).reshape(H // 2, W)
        return np.ascontiguousarray(np.concatenate([Y, uv], axis=0))
    planes = [Y[:, 0::2], U[:, 0::2], Y[:, 1::2], V[:, 0::2]] if fmt == "yuyv" else [U[:, 0::2], Y[:, 0::2], V[:, 0::2], Y[:, 1::2]]
    return np.ascontiguousarray(np.stack(planes, axis=-1).reshape(H, 2 * W))


INGEST_WARM = 5  # --ingest-kernels: untimed launches in front of every block
INGEST_KERNEL = "ingest_kernel<"  # ingest_kernel<FMT, MAP> (ingest.hip); FMT 0 = rgb8


def ingest_schedule(formats, n):
    """The blocks of --ingest-kernels in launch order: (format, 'free' | 'rect', launches).  The rgb8 pair comes three
    times -- in front, in the middle and at the end -- so that its spread brackets the other formats."""
    rgb = [("rgb8", cfg, INGEST_WARM + n) for cfg in ("free", "rect")]
    rest = [(f, cfg, INGEST_WARM + n) for f in formats for cfg in ("free", "rect")]
    half = len(rest) // 2 // 2 * 2
    return rgb + rest[:half] + rgb + rest[half:] + rgb


def run_ingest_kernels(formats, n):
    """Only the ingest launches, block by block (for `rocprofv3 --kernel-trace`; read the trace with --parse-trace)."""
    from codd_amd import ops
    dev = torch.device("cuda:0")
    HP, WP = -(-H // 64) * 64, -(-W // 64) * 64
    left, right = frames(1)[0]
    maps = tuple(tuple(torch.from_numpy(m).to(dev) for m in p) for p in radial_maps())
    out = tuple(torch.empty(1, 3, HP, WP, device=dev) for _ in range(2))
    src = {f: tuple(torch.from_numpy(raw_of(v, f)).to(dev) for v in (left, right)) for f in ["rgb8"] + formats}
    for fmt, cfg, launches in ingest_schedule(formats, n):
        m = maps if cfg == "rect" else None
        for _ in range(launches):
            if fmt == "rgb8":
                ops.ingest_pair(*src[fmt], *out, bgr=False, maps=m)
            else:
                ops.ingest_frames(*src[fmt], *out, fmt, (H, W), maps=m)
        torch.cuda.synchronize()


def parse_ingest_trace(path, formats, n):
    """The kernel trace (csv) of an --ingest-kernels run with the same --pixel-format and count -> the table."""
    import csv
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path))
                if INGEST_KERNEL in r["Kernel_Name"])
    sched = ingest_schedule(formats, n)
    assert len(ev) == sum(b[2] for b in sched), f"{len(ev)} ingest dispatches in the trace, the schedule has {sum(b[2] for b in sched)}"
    from codd_amd.live import frame_layout
    blocks, i = {}, 0
    for fmt, cfg, launches in sched:
        us = np.array([(e - s) / 1e3 for s, e, _ in ev[i + INGEST_WARM:i + launches]])
        names = {k for _, _, k in ev[i:i + launches]}
        assert len(names) == 1 and ((INGEST_KERNEL + "0,") in next(iter(names))) == (fmt == "rgb8"), (fmt, names)
        blocks.setdefault((fmt, cfg), []).append(float(np.median(us)))
        i += launches
    lines = ["| format | upload bytes / frame | map-free median us | rectified median us |", "|---|---|---|---|"]
    for fmt in ["rgb8"] + formats:
        cells = [" / ".join(f"{v:.2f}" for v in blocks[(fmt, cfg)]) for cfg in ("free", "rect")]
        lines.append(f"| {fmt} | {2 * frame_layout(fmt, H, W)[3]} | {cells[0]} | {cells[1]} |")
    for cfg in ("free", "rect"):
        v = blocks[("rgb8", cfg)]
        lines.append(f"\nrgb8 {cfg}: spread of {len(v)} repetitions {min(v):.2f} .. {max(v):.2f} us")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    ap.add_argument("--trace", default=None, metavar="VARIANTS", help="run only 40 untimed frames of these live variants "
                    "(comma-separated from c, c_rect, d, d_rect) -- for a profiler trace")
    ap.add_argument("--pixel-format", default=None, metavar="FORMATS", help="raw camera formats (comma-separated from "
                    "ops.FRAME_FORMATS, or 'all'): adds a pipelined variant d:<format> per format next to rgb8's d, fed raw "
                    "frames of the same images; with --trace the traced variants run in these formats instead of rgb8")
    ap.add_argument("--ingest-kernels", type=int, default=0, metavar="N", help="run only the ingest launch, N timed launches "
                    "per block: rgb8 and every --pixel-format, map-free and rectified -- for a kernel trace")
    ap.add_argument("--parse-trace", default=None, metavar="CSV", help="print the table of an --ingest-kernels run from its "
                    "rocprofv3 kernel trace (same --pixel-format and --ingest-kernels as that run); needs no GPU")
    args = ap.parse_args()
    from codd_amd import configs, ops, synth
    formats = []
    if args.pixel_format:
        formats = list(ops.FRAME_FORMATS) if args.pixel_format == "all" else args.pixel_format.split(",")
        unknown = [f for f in formats if f not in ops.FRAME_FORMATS]
        if unknown:
            ap.error(f"--pixel-format: unknown {unknown}; known: {list(ops.FRAME_FORMATS)}")
    if args.parse_trace:
        return parse_ingest_trace(args.parse_trace, formats, args.ingest_kernels)
    if args.ingest_kernels:
        return run_ingest_kernels(formats, args.ingest_kernels)
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
    # variant -> pixel format: the live variants in rgb8, plus d:<format> per raw format (traced: the raw formats instead)
    if args.trace:
        fmt_of = {(k if f == "rgb8" else f"{k}:{f}"): f for f in (formats or ["rgb8"]) for k in args.trace.split(",")}
    else:
        fmt_of = {**{k: "rgb8" for k in ("c", "c_rect", "d", "d_rect")}, **{f"d:{f}": f for f in formats}}
    sess = {k: LiveSession(est, (H, W), output="disp", rectify=radial_maps() if k.split(":")[0].endswith("rect") else None,
                           pixel_format=f) for k, f in fmt_of.items()}
    raw = {f: [tuple(raw_of(v, f) for v in pair) for pair in src] for f in set(fmt_of.values())}

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

    def sync(s, src):
        def go(n, lat):
            for _ in range(n):
                a, b = src[nxt()]
                t0 = time.perf_counter()
                s.step(a, b)
                lat.append(time.perf_counter() - t0)
        return go

    def piped(s, src):
        def go(n, lat):
            for _ in range(n):
                if s.pending() == 2:
                    s.pop()
                s.push(*src[nxt()])
            while s.pending():
                s.pop()
        return go

    variants = {k: (sync if k.startswith("c") else piped)(s, raw[fmt_of[k]]) for k, s in sess.items()}
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
                         upload_bytes=0 if k == "a" else 2 * raw[fmt_of.get(k, "rgb8")][0][0].nbytes,
                         lat_mean_ms=float(lat.mean()) if lat.size else None,
                         lat_worst_ms=float(lat.max()) if lat.size else None))
    by = {r["variant"]: r for r in rows}
    spread = abs(by["b"]["ms_per_frame"] - by["b2"]["ms_per_frame"])
    res = dict(shape=[H, W], rounds=args.rounds, per_round=args.per_round, rows=rows, spread_b_ms=spread,
               d_ge_b=by["d"]["fps"] >= max(by["b"]["fps"], by["b2"]["fps"]),
               c_le_b_by_more_than_spread=by["c"]["lat_mean_ms"] < min(by["b"]["lat_mean_ms"], by["b2"]["lat_mean_ms"]) - spread)
    print(json.dumps(res))
    f2 = lambda v: "-" if v is None else f"{v:.2f}"  # noqa: E731
    lines = ["| variant | frames | frames/s | ms/frame | host-to-host mean ms | worst ms | upload bytes / frame |",
             "|---|---|---|---|---|---|---|"]
    lines += [f"| {r['variant']} | {r['frames']} | {r['fps']:.1f} | {f2(r['ms_per_frame'])} | {f2(r['lat_mean_ms'])} | "
              f"{f2(r['lat_worst_ms'])} | {r['upload_bytes']} |" for r in rows]
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
