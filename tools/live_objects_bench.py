"""Cost of LiveSession's obstacle objects (codd_objects), 540x960 in 576x960.

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, five repetitions of the replay (median, min, max): on the labels and the record codd_ground_plane
   gives for a scene of tests/live_ground_ref.py at that size (a pitched and rolled camera 1.2 above a floor with three
   boxes, sky, a NaN band and 0.05 px of noise) with and without the id map, and on two fabricated worst cases of
   tests/live_objects_ref.py at that size: the one-pixel serpentine through the whole crop (one component across every
   tile border, the longest parent chains) and the checkerboard of isolated pixels (259 200 components).
2. The host route this replaces, timed in the same process: the download of the padded disparity and the labels into
   pinned memory, then tests/live_objects_ref.py's foreground and edge masks and scipy.sparse.csgraph
   .connected_components on that edge list (the partition alone: no statistics), medians over --host-runs.
3. LiveSession.step frames/s with ground= and objects= against ground= alone and against neither: sessions on one
   estimator, alternated in rounds, median over the rounds.

    python tools/live_objects_bench.py [--calls 200 --rounds 5 --per-round 25] [--out profiles/live_objects.md]

CODD_LIB_AB=<another build of libcodd_hip.so> python tools/live_objects_bench.py --kernel-only measures that build's kernels
with the same tool (how profiles/live_objects.md compared the tile-local stage with a plain global-memory union-find).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, HP, WP = 540, 960, 576, 960
DEV = "cuda:0"
LAUNCHES = 7
SPEC = dict(crop=(H, W), padded=(HP, WP), K=(1050.0, 1050.0, 479.5, 269.5), calib=210.0, cam_h=1.2, pitch=0.15, roll=0.03,
            name="bench", scene="bench", par={}, seed=None, grid=None)
BOXES = [(60, 300, 150, 400), (380, 620, 190, 470), (700, 900, 170, 360)]


def time_calls(fn, n, warmup=20):
    """(eager us / call, graph-replayed us / call: median, min, max of 5 repetitions); the graph holds ONE call."""
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
    return eager, float(np.median(reps)), min(reps), max(reps)


def scenes():
    """[(name, disp [HP,WP] device, labels [H,W] device, record device, K, calib, parameters)]: the realistic frame's labels
    and record come from codd_ground_plane itself."""
    import live_ground_ref as lg
    import live_objects_ref as lo
    from codd_amd import ops
    lg.SCENES["bench"] = dict(boxes=BOXES)
    c = lg.case(SPEC)
    disp = torch.from_numpy(c["disp"]).to(DEV)
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    lab = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    ops.ground_plane(disp, c["K"], c["calib"], (H, W), rec, lab, **{k: v for k, v in c["par"].items() if k != "cell"})
    torch.cuda.synchronize()
    assert float(rec[3]) == 1.0
    out = [("three boxes on a floor (labels and record of codd_ground_plane), defaults", disp, lab, rec, c["K"], c["calib"], {})]
    for name, build in (("serpentine, one pixel wide, through the whole crop", lo._serpentine),
                        ("checkerboard of isolated pixels", lo._checker)):
        labels, d = build((H, W))
        m = lo.make(name, labels, d, rec=lo.record(K=SPEC["K"], calib=SPEC["calib"]), padded=(HP, WP), K=SPEC["K"],
                    calib=SPEC["calib"], min_pixels=1, min_height=lo.ANY_HEIGHT)
        out.append((name + " (min_pixels 1, any height)", torch.from_numpy(m["disp"]).to(DEV), torch.from_numpy(labels).to(DEV),
                    torch.from_numpy(m["rec"]).to(DEV), m["K"], m["calib"], dict(min_pixels=1, min_height=lo.ANY_HEIGHT)))
    return out


def kernel_part(n):
    from codd_amd import ops
    m = ops.OBJECT_PARAMS["max_objects"]
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    oi, of = torch.zeros(m, 8, dtype=torch.int32, device=DEV), torch.zeros(m, 8, device=DEV)
    ids = torch.empty(H, W, dtype=torch.uint16, device=DEV)
    scratch = torch.empty(ops.objects_scratch(H, W, m), dtype=torch.uint8, device=DEV)
    rows = []
    for name, disp, lab, rec, K, calib, par in scenes():
        for with_ids in (True, False):
            fn = lambda: ops.objects(disp, K, calib, (H, W), lab, rec, cnt, oi, of, ids=ids if with_ids else None,  # noqa: E731
                                     scratch=scratch, **par)
            eager, graph, lo_, hi_ = time_calls(fn, n)
            c = cnt.cpu().numpy()
            rows.append(dict(scene=name, ids=with_ids, launches=LAUNCHES - (0 if with_ids else 1), eager_us=eager, graph_us=graph,
                             graph_min=lo_, graph_max=hi_, count=c.tolist()))
    return rows


def host_part(runs):
    """The route a user had to write: download disparity and labels, foreground and edges in numpy, scipy's connected
    components -> median milliseconds of each."""
    import live_objects_ref as lo
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    name, disp, lab, rec, K, calib, par = scenes()[0]
    pd, pl = torch.empty(HP, WP, pin_memory=True), torch.empty(H, W, dtype=torch.uint8, pin_memory=True)
    record = rec.cpu().numpy()
    idx = np.arange(H * W).reshape(H, W)
    t = dict(download=[], masks=[], components=[])
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pd.copy_(disp, non_blocking=True)
        pl.copy_(lab, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        c = dict(crop=(H, W), disp=pd.numpy(), labels=pl.numpy(), rec=record, par=dict(lo.DEFAULTS, **par))
        fg = lo.foreground(c)
        right, down = lo.edges(c, fg)
        t2 = time.perf_counter()
        a = np.concatenate([idx[:, :-1][right], idx[:-1, :][down]])
        b = np.concatenate([idx[:, 1:][right], idx[1:, :][down]])
        ncomp, _ = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(H * W, H * W)), directed=False)
        t3 = time.perf_counter()
        for k, v in zip(t, (t1 - t0, t2 - t1, t3 - t2)):
            t[k].append(1e3 * v)
    return {k: float(np.median(v)) for k, v in t.items()}, int(ncomp - (~fg).sum())


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="part 1 only")
    ap.add_argument("--no-session", action="store_true", help="the kernel and host parts only")
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from codd_amd import _abi, ops
    ops.enable_autotune(False)
    krows = kernel_part(args.calls)
    host, ncomp = ({}, 0) if args.kernel_only else host_part(args.host_runs)
    srows = []
    if not (args.kernel_only or args.no_session):
        srows = session_part(args.rounds, args.per_round, {
            "neither": {}, "ground=True": dict(ground=True), "ground=True, objects=True": dict(ground=True, objects=True),
            "ground=True, objects=dict(map=True)": dict(ground=True, objects=dict(map=True))})
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], calls=args.calls, library=_abi.LOADED, kernel=krows, host=host,
                          session=srows)))
    lines = [f"codd_objects at {W}x{H} in {WP}x{HP}, HIP events over {args.calls} calls after 20 warm-ups, graph replay repeated five "
             f"times; library {os.path.relpath(_abi.LOADED, ROOT)}", "",
             "| scene | id map | launches | us / call, issued eagerly | us / call, graph replay (median) | min | max | us / launch | "
             "count (objects, passing, components, foreground) |", "|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {r['scene']} | {'yes' if r['ids'] else 'no'} | {r['launches']} | {r['eager_us']:.2f} | {r['graph_us']:.2f} | "
              f"{r['graph_min']:.2f} | {r['graph_max']:.2f} | {r['graph_us'] / r['launches']:.2f} | {r['count']} |" for r in krows]
    if host:
        total = sum(host.values())
        lines += ["", f"the host route it replaces, the first scene, medians over {args.host_runs} runs: download of the padded "
                  f"disparity and the labels {host['download']:.3f} ms, foreground and edge masks (numpy) {host['masks']:.3f} ms, "
                  f"scipy.sparse.csgraph.connected_components on the edge list {host['components']:.3f} ms ({ncomp} components; the "
                  f"partition only, no statistics): {total:.3f} ms per frame against {krows[0]['graph_us'] / 1e3:.3f} ms"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max | ms / frame |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} | "
                  f"{1e3 / r['fps_median']:.3f} |" for r in srows]
        g, o = srows[1]["fps_median"], srows[2]["fps_median"]
        lines += ["", f"cost of the objects output per synchronous frame: {1e3 / o - 1e3 / g:.3f} ms of {1e3 / o:.3f} ms "
                  f"({100 * (1 - o / g):.2f} %)"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
