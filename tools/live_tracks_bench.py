"""Cost of LiveSession's object tracks (codd_track_objects), 540x960 in 576x960.

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, five repetitions of the replay (median, min, max), on three synthetic frames: the three boxes of
   tools/live_objects_bench.py's realistic frame under a field that shifts them by (3, 1) pixels, with the ego record and
   the moving mask; one object covering the whole crop (every wave adds to the same nine words); and the checkerboard of
   one-pixel objects with max_objects = 1024 (no wave is uniform: one atomic per lane and value).  The id map is the same
   before and after (the call rolls it), so every call of a run does the same work.
2. The host route this replaces, timed in the same process: the download of both id maps and a flow_dd map into pinned
   memory, the numpy warp of one id map onto the other, np.add.at for the votes and the per-object sums of the flow;
   medians over --host-runs.
3. LiveSession.step frames/s with tracks= against the same session without it: sessions on one estimator, alternated in
   rounds, median over the rounds.

    python tools/live_tracks_bench.py [--calls 200 --rounds 5 --per-round 25] [--out profiles/live_tracks.md]

CODD_LIB_AB=<another build of libcodd_hip.so> python tools/live_tracks_bench.py --kernel-only measures that build's kernels
with the same tool: profiles/live_tracks.md compares the shipped per-pixel launch that way with a build whose lanes each
issue their own atomics (made for the measurement, not kept in the source).  --trace-run issues the calls eagerly and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/live_tracks_bench.py --trace-run`.
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
LAUNCHES = 4
K = (1050.0, 1050.0, 479.5, 269.5)
BOXES = [(60, 300, 150, 400), (380, 620, 190, 470), (700, 900, 170, 360)]  # (x0, x1, y0, y1) of tools/live_objects_bench.py
SHIFT = (3.0, 1.0)


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
    """[(name, ids uint16 [H,W], n, T [HP,WP,7], depth [HP,WP], max_objects, min_votes)], numpy."""
    import live_tracks_ref as lt
    T, depth = lt.field((H, W), (HP, WP), SHIFT, Z=10.0, K=K, q=lt.Q_SMALL)
    T, depth = np.nan_to_num(T), np.nan_to_num(depth, nan=10.0)
    three = lt.boxes((H, W), *((y0, y1, x0, x1) for x0, x1, y0, y1 in BOXES))
    whole = np.zeros((H, W), np.uint16)
    yy, xx = np.mgrid[:H, :W]
    checker = np.full(H * W, lt.NONE, np.uint16)
    where = np.flatnonzero(((yy + xx) % 2 == 0).ravel())
    checker[where] = np.arange(where.size) % 1024  # (every object: 253 scattered pixels)
    return [("three boxes shifted by (3, 1) px", three, 3, T, depth, 256, 16),
            ("one object covering the crop", whole, 1, T, depth, 256, 16),
            ("checkerboard of one-pixel pieces, 1024 objects", checker.reshape(H, W), 1024, T, depth, 1024, 1)]


class Call:
    """The device buffers of one scene and the call on them."""

    def __init__(self, scene):
        import live_tracks_ref as lt
        from codd_amd import ops
        self.name, ids, n, T, depth, self.m, self.min_votes = scene
        self.ids = torch.from_numpy(ids.view(np.int16)).to(DEV).view(torch.uint16)
        self.count = torch.tensor([n, n, n, int((ids != lt.NONE).sum())], dtype=torch.int32, device=DEV)
        self.T, self.depth = torch.from_numpy(T)[None].to(DEV), torch.from_numpy(depth).to(DEV)
        self.ego = torch.from_numpy(lt.EGO).to(DEV)
        self.moving = torch.from_numpy(np.random.default_rng(3).integers(0, 2, (H, W)).astype(np.uint8)).to(DEV)
        self.state = torch.zeros(ops.track_state_bytes(H, W, self.m), dtype=torch.uint8, device=DEV)
        self.scratch = torch.empty(ops.track_scratch(H, W, self.m), dtype=torch.uint8, device=DEV)
        self.cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.ti, self.tf = torch.zeros(self.m, 8, dtype=torch.int32, device=DEV), torch.zeros(self.m, 8, device=DEV)
        self(fresh=True)

    def __call__(self, fresh=False):
        from codd_amd import ops
        ops.track_objects(self.T, self.depth, K, (H, W), self.ids, self.count, self.state, self.cnt, self.ti, self.tf,
                          scratch=self.scratch, ego_record=self.ego, moving=self.moving, scale=0.37, fresh=fresh,
                          min_votes=self.min_votes, max_objects=self.m)


def kernel_part(n):
    rows = []
    for scene in scenes():
        call = Call(scene)
        eager, graph, lo_, hi_ = time_calls(call, n)
        rows.append(dict(scene=call.name, eager_us=eager, graph_us=graph, graph_min=lo_, graph_max=hi_,
                         count=call.cnt.cpu().numpy().tolist(), row0=call.ti[0].cpu().numpy().tolist()))
    return rows


def trace_run(n):
    for scene in scenes():
        call = Call(scene)
        for _ in range(n):
            call()
        torch.cuda.synchronize()


def host_part(runs):
    """The route a user had to write, on the first scene: download the two id maps and a flow_dd map, warp, count overlaps
    and average the flow per object in numpy -> median milliseconds of each."""
    import live_tracks_ref as lt
    from codd_amd import ops
    name, ids, n, T, depth, m, _ = scenes()[0]
    d_prev, d_cur = (torch.from_numpy(ids.view(np.int16)).to(DEV) for _ in range(2))
    disp = torch.full((HP, WP), 21.0, device=DEV)
    dp = torch.from_numpy(depth).to(DEV)
    flow = torch.empty(H, W, 3, device=DEV)
    ops.export_motion(torch.from_numpy(T)[None].to(DEV), disp, dp, flow, "flow_dd", K, 210.0)
    torch.cuda.synchronize()
    p_prev, p_cur = (torch.empty(H, W, dtype=torch.int16, pin_memory=True) for _ in range(2))
    p_flow = torch.empty(H, W, 3, pin_memory=True)
    yy, xx = np.mgrid[:H, :W]
    t = dict(download=[], warp=[], add_at=[])
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p_prev.copy_(d_prev, non_blocking=True)
        p_cur.copy_(d_cur, non_blocking=True)
        p_flow.copy_(flow, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        a, cur, fl = p_prev.numpy().view(np.uint16), p_cur.numpy().view(np.uint16), p_flow.numpy()
        with np.errstate(invalid="ignore"):
            u, v = np.floor(xx + fl[..., 0] + 0.5), np.floor(yy + fl[..., 1] + 0.5)
            ok = (a != lt.NONE) & np.isfinite(fl[..., 0]) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        b = np.full((H, W), lt.NONE, np.uint16)
        b[ok] = cur[v[ok].astype(np.int64), u[ok].astype(np.int64)]
        t2 = time.perf_counter()
        votes = np.zeros((m, m), np.int64)
        hit = ok & (b != lt.NONE)
        np.add.at(votes, (a[hit], b[hit]), 1)
        sums, cnt = np.zeros((m, 3)), np.zeros(m, np.int64)
        sel = a != lt.NONE
        np.add.at(cnt, a[sel], 1)
        np.add.at(sums, a[sel], fl[sel])
        t3 = time.perf_counter()
        for k, val in zip(t, (t1 - t0, t2 - t1, t3 - t2)):
            t[k].append(1e3 * val)
    return {k: float(np.median(v)) for k, v in t.items()}, int(votes.sum())


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
    ap.add_argument("--trace-run", action="store_true", help="--calls eager calls per scene and nothing else (for rocprofv3)")
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from codd_amd import _abi, ops
    ops.enable_autotune(False)
    if args.trace_run:
        trace_run(args.calls)
        return
    krows = kernel_part(args.calls)
    host, nvotes = ({}, 0) if args.kernel_only else host_part(args.host_runs)
    srows = []
    if not (args.kernel_only or args.no_session):
        base = dict(ground=True, objects=True, egomotion=True)
        srows = session_part(args.rounds, args.per_round, {"ground, objects, egomotion": base,
                                                           "ground, objects, egomotion, tracks": dict(base, tracks=True)})
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], calls=args.calls, library=_abi.LOADED, kernel=krows, host=host,
                          session=srows)))
    lines = [f"codd_track_objects at {W}x{H} in {WP}x{HP}, HIP events over {args.calls} calls after 20 warm-ups, graph replay "
             f"repeated five times; library {os.path.relpath(_abi.LOADED, ROOT)}", "",
             "| scene | launches | us / call, issued eagerly | us / call, graph replay (median) | min | max | us / launch | "
             "trk_count (n, continued, started, ended) | row 0 |", "|---|---|---|---|---|---|---|---|---|"]
    lines += [f"| {r['scene']} | {LAUNCHES} | {r['eager_us']:.2f} | {r['graph_us']:.2f} | {r['graph_min']:.2f} | "
              f"{r['graph_max']:.2f} | {r['graph_us'] / LAUNCHES:.2f} | {r['count']} | {r['row0']} |" for r in krows]
    if host:
        total = sum(host.values())
        lines += ["", f"the host route it replaces, the first scene, medians over {args.host_runs} runs: download of two id maps "
                  f"and a flow_dd map {host['download']:.3f} ms, the warp (numpy) {host['warp']:.3f} ms, np.add.at for the votes "
                  f"({nvotes}) and the per-object flow sums {host['add_at']:.3f} ms: {total:.3f} ms per frame against "
                  f"{krows[0]['graph_us'] / 1e3:.3f} ms"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max | ms / frame |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} | "
                  f"{1e3 / r['fps_median']:.3f} |" for r in srows]
        g, o = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the tracks output per synchronous frame: {1e3 / o - 1e3 / g:.3f} ms of {1e3 / o:.3f} ms "
                  f"({100 * (1 - o / g):.2f} %)"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
