"""Cost of LiveSession's elevation layer (codd_height_map), 540x960 in 576x960, default parameters, on codd_local_map's
default window (128 x 128 cells of 0.1 to a range of 12.8).

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, five repetitions of the replay (median, min, max), on the three inputs of tools/live_scan_bench.py:
   the realistic frame (three boxes on a noisy floor), a fronto-parallel wall filling the view (every pixel of the frame in
   one row of cells, the worst contention) and the floor alone.  Every timed call is codd_local_map followed by
   codd_height_map, as in a session (the layer's precondition); the map alone is timed on the same inputs in the same run,
   and the layer's cost is the difference.  The ego record is tools/live_localmap_bench.py's step of 0.03 forward.
2. The same with ONE ATOMIC PER LANE AND TABLE in the pixel launch: codd_amd/csrc/heightmap.hip compiled a second time with
   -DHEIGHTMAP_LANE_ATOMICS (and the entries renamed by -D) into build/live_heightmap_bench/ and loaded with ctypes -- the
   variant lives nowhere in the library.  Its layers, outputs and record must equal the shipped call's bytes, which the
   tool asserts on calls from equal states.
3. The host route this replaces, timed in the same process on the realistic frame: the download of the padded disparity
   and the labels into pinned memory, the projection and the heights in numpy, np.maximum.at / np.minimum.at / np.add.at
   and the update rule; medians over --host-runs.
4. LiveSession.step frames/s with heightmap= against the same session without it: sessions on one estimator, alternated
   in rounds, median over the rounds.

Every GPU part runs in a child process of its own under a time limit (--limit seconds each): a part that faults or hangs
ends the tool, which starts nothing after it.

    python tools/live_heightmap_bench.py [--calls 200 --rounds 5 --per-round 25] [--out profiles/live_heightmap.md]

--build-only compiles the per-lane variant and exits (no GPU needed).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GH = GW = 128
LAYERS = (("top", "int16"), ("bot", "int16"), ("ceil", "int16"), ("hage", "uint8"))
OUTPUTS = LAYERS + (("step", "uint16"), ("flags", "uint8"))


def build_variant(verbose=False):
    """Path of the shared library holding the per-lane variant (entries lane_height_map_scratch, lane_height_map), compiled
    from codd_amd/csrc/heightmap.hip when missing or older than it."""
    csrc = os.path.join(ROOT, "codd_amd", "csrc")
    src = os.path.join(csrc, "heightmap.hip")
    out_dir = os.path.join(ROOT, "build", "live_heightmap_bench")
    lib = os.path.join(out_dir, "libheightmap_lane.so")
    deps = [src] + [os.path.join(csrc, h) for h in ("map_window.h", "floor_frame.h", "common.h")] + [os.path.join(ROOT, "include", "codd_hip.h")]
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(d) for d in deps):
        return lib
    os.makedirs(out_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DHEIGHTMAP_LANE_ATOMICS",
           "-Dcodd_height_map_scratch=lane_height_map_scratch", "-Dcodd_height_map=lane_height_map",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, src, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return lib


def load_variant():
    from codd_amd import _abi
    lib = C.CDLL(build_variant())
    res, args = _abi.SIGNATURES["codd_height_map"]
    lib.lane_height_map.restype, lib.lane_height_map.argtypes = res, args
    return lib


class Call:
    """tools/live_localmap_bench.py's map call on one scene, and behind it the shipped layer call and the per-lane variant,
    each with layers and outputs of its own on the map's state."""

    def __init__(self, scene, variant):
        import torch
        import live_localmap_bench as mb
        from codd_amd import ops
        self.map = mb.Call(scene, None)
        self.sb, self.torch, self.variant = self.map.sb, torch, variant
        dev = self.sb.DEV
        new = lambda dt: torch.zeros(GH, GW, dtype=getattr(torch, dt), device=dev)  # noqa: E731
        self.sets = [dict(layers=[new(dt) for _, dt in LAYERS], outs=[new(dt) for _, dt in OUTPUTS],
                          rec=torch.zeros(16, dtype=torch.float64, device=dev)) for _ in range(2)]
        self.scratch = torch.empty(ops.height_map_scratch(GH, GW), dtype=torch.uint8, device=dev)
        self.state = self.map.sets[0]["state"]

    @property
    def name(self):
        return self.map.name

    def map_only(self, fresh=False):
        self.map.shipped(fresh=fresh)

    def layer(self, k=0):
        from codd_amd import ops
        s, sb, m = self.sets[k], self.sb, self.map
        if k == 0:
            ops.height_map(m.disp, sb.SPEC["K"], sb.SPEC["calib"], (sb.H, sb.W), m.lab, m.rec, self.state, *s["layers"], *s["outs"],
                           s["rec"], scratch=self.scratch)
            return
        p = ops.HEIGHT_PARAMS
        q = ops.height_thresholds(p["h_res"], p["max_step"], p["robot_height"], p["max_drop"])
        mp = ops.MAP_PARAMS
        rc = self.variant.lane_height_map(m.disp.data_ptr(), sb.HP, sb.WP, sb.H, sb.W, *[float(v) for v in sb.SPEC["K"]],
                                          float(sb.SPEC["calib"]), m.lab.data_ptr(), m.rec.data_ptr(), self.state.data_ptr(), GH, GW,
                                          mp["cell"], mp["range_min"], mp["range_max"], p["h_res"], p["select"], p["min_pixels"],
                                          p["alpha"], *q, *[t.data_ptr() for t in s["layers"]], self.scratch.data_ptr(),
                                          self.scratch.numel(), *[t.data_ptr() for t in s["outs"]], s["rec"].data_ptr(),
                                          self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def shipped(self, fresh=False):
        self.map_only(fresh)
        self.layer(0)

    def per_lane(self, fresh=False):
        self.map_only(fresh)
        self.layer(1)

    def same(self):
        a, b = self.sets
        u8 = self.torch.uint8
        return (all(self.torch.equal(x.view(u8), y.view(u8)) for k in ("layers", "outs") for x, y in zip(a[k], b[k]))
                and self.torch.equal(a["rec"].view(u8), b["rec"].view(u8)))


def kernel_part(n):
    import torch
    import live_scan_bench as sb
    from codd_amd import ops
    ops.enable_autotune(False)
    variant = load_variant()
    rows = []
    for scene in sb.scenes():
        call = Call(scene, variant)
        for k in range(3):  # a fresh frame and two steps: both layer calls behind ONE map call, from equal states
            call.map_only(fresh=k == 0)
            call.layer(0)
            call.layer(1)
            torch.cuda.synchronize()
            assert call.same(), f"{call.name}: the per-lane variant's bytes differ from the shipped call's (call {k})"
        row = dict(scene=call.name, record=call.sets[0]["rec"].cpu().numpy().tolist(), same_bytes=True)
        for key, fn in (("map", call.map_only), ("shipped", call.shipped), ("per_lane", call.per_lane)):
            eager, graph, lo_, hi_ = sb.time_calls(fn, n)
            row[key] = dict(eager_us=eager, graph_us=graph, graph_min=lo_, graph_max=hi_)
        rows.append(row)
    return rows


def host_part(runs):
    """The route a user had to write, on the realistic frame: download disparity and labels, project, heights, the three
    extremes and two counts per cell, the update rule -> median milliseconds of each."""
    import torch
    import live_scan_bench as sb
    from codd_amd import ops
    ops.enable_autotune(False)
    name, disp, lab, rec = sb.scenes()[0][:4]
    H, W, HP, WP = sb.H, sb.W, sb.HP, sb.WP
    pd, pl = torch.empty(HP, WP, pin_memory=True), torch.empty(H, W, dtype=torch.uint8, pin_memory=True)
    record = rec.cpu().numpy()
    fx, fy, cx, cy = sb.SPEC["K"]
    n_, f_ = record[8:11], record[22:25]
    r_ = np.cross(f_, n_)
    mp, p = ops.MAP_PARAMS, ops.HEIGHT_PARAMS
    yy, xx = np.mgrid[:H, :W]
    top, bot = np.full((GH, GW), -32768, np.int64), np.full((GH, GW), -32768, np.int64)
    ceil, age = np.full((GH, GW), 32767, np.int64), np.full((GH, GW), 255, np.int64)
    pose, head = np.zeros(2), np.array([0.0, 1.0])
    t = dict(download=[], project=[], tables=[])
    blend = lambda v, x: v + np.sign(x - v) * ((p["alpha"] * np.abs(x - v)) // 256)  # noqa: E731
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pd.copy_(disp, non_blocking=True)
        pl.copy_(lab, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d, labels = pd.numpy()[:H, :W], pl.numpy()
        pose = pose + 0.03 * head
        ix0, iz0 = np.floor(pose / mp["cell"]).astype(np.int64) - np.array([GW // 2, GH // 2])
        with np.errstate(all="ignore"):
            take = (labels < 4) & np.isfinite(d) & (d > 0)
            ys, xs = yy[take], xx[take]
            dd = d[take]
            Z = sb.SPEC["calib"] / dd
            X0, X1 = Z * (xs - cx) / fx, Z * (ys - cy) / fy
            gx, gz = r_[0] * X0 + r_[1] * X1 + r_[2] * Z, f_[0] * X0 + f_[1] * X1 + f_[2] * Z
            rho = np.hypot(gx, gz)
            wx, wz = gx * head[1] + gz * head[0] + pose[0], gz * head[1] - gx * head[0] + pose[1]
            jx, jz = np.floor(wx / mp["cell"]).astype(np.int64) - ix0, np.floor(wz / mp["cell"]).astype(np.int64) - iz0
            hgt = record[11] * (dd - (record[0] * (xs - cx) + record[1] * (ys - cy) + record[2])) / dd
            q = np.clip(np.rint(hgt / p["h_res"]), -32000, 32000)
            ok = (rho >= mp["range_min"]) & (rho < mp["range_max"]) & (jx >= 0) & (jx < GW) & (jz >= 0) & (jz < GH) & np.isfinite(hgt)
        t2 = time.perf_counter()
        q = q.astype(np.int64)
        ov = ok & (labels[take] == 2)
        su = ok & ~ov
        Tmax, Tmin = np.full((GH, GW), -2 ** 31, np.int64), np.full((GH, GW), 2 ** 31 - 1, np.int64)
        Cmin, Tn, Cn = np.full((GH, GW), 2 ** 31 - 1, np.int64), np.zeros((GH, GW), np.int64), np.zeros((GH, GW), np.int64)
        np.maximum.at(Tmax, (jz[su], jx[su]), q[su])
        np.minimum.at(Tmin, (jz[su], jx[su]), q[su])
        np.add.at(Tn, (jz[su], jx[su]), 1)
        np.minimum.at(Cmin, (jz[ov], jx[ov]), q[ov])
        np.add.at(Cn, (jz[ov], jx[ov]), 1)
        s, o = Tn >= p["min_pixels"], Cn >= p["min_pixels"]
        top = np.where(s, np.where(top == -32768, Tmax, blend(top, Tmax)), top)
        bot = np.where(s, np.where(bot == -32768, Tmin, blend(bot, Tmin)), bot)
        ceil = np.where(o, np.where(ceil == 32767, Cmin, blend(ceil, Cmin)), ceil)
        age = np.where(s | o, 0, np.where(age == 255, 255, np.minimum(age + 1, 254)))
        t3 = time.perf_counter()
        for key, v in zip(t, (t1 - t0, t2 - t1, t3 - t2)):
            t[key].append(1e3 * v)
    return {key: float(np.median(v)) for key, v in t.items()}


def session_part(rounds, per_round):
    import live_scan_bench as sb
    base = dict(ground=True, egomotion=True, localmap=True)
    return sb.session_part(rounds, per_round, {"ground, egomotion, localmap": base,
                                               "ground, egomotion, localmap, heightmap": dict(base, heightmap=True)})


def child(args):
    """One GPU part, in this process: prints one JSON line."""
    if args.part == "kernel":
        out = kernel_part(args.calls)
    elif args.part == "host":
        out = host_part(args.host_runs)
    else:
        out = session_part(args.rounds, args.per_round)
    print("RESULT " + json.dumps(out), flush=True)


def run_part(part, args):
    """A child process for one part, under the time limit; its result, or SystemExit: nothing runs after a part that failed."""
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--part", part, "--calls", str(args.calls),
           "--rounds", str(args.rounds), "--per-round", str(args.per_round), "--host-runs", str(args.host_runs)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.stdout.write(r.stdout)
        raise SystemExit(f"live_heightmap_bench: part {part!r} ended with status {r.returncode}; nothing else was started")
    return json.loads(lines[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU part")
    ap.add_argument("--kernel-only", action="store_true", help="part 1 and 2 only")
    ap.add_argument("--no-session", action="store_true", help="the kernel and host parts only")
    ap.add_argument("--build-only", action="store_true", help="compile the per-lane variant and exit")
    ap.add_argument("--part", choices=("kernel", "host", "session"), help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    if args.build_only:
        print(build_variant(verbose=True))
        return
    if args.part:
        child(args)
        return
    build_variant()
    krows = run_part("kernel", args)
    host = {} if args.kernel_only else run_part("host", args)
    srows = [] if (args.kernel_only or args.no_session) else run_part("session", args)
    print(json.dumps(dict(grid=[GH, GW], calls=args.calls, kernel=krows, host=host, session=srows)))
    lines = [f"codd_local_map + codd_height_map at 960x540 in 960x576, {GH} x {GW} cells, default parameters, HIP events over {args.calls} "
             f"calls after 20 warm-ups, graph replay repeated five times (median [min .. max]); the layer's cost is the pair minus the map",
             "", "| input | record of the last checked call (integrated, surface px, overhead px, observed, known, step, headroom, hole, "
             "top max, bot min, ix0, iz0, 0..) | map alone, 4 launches: us eager | graph replay | map + layer, 8 launches: eager | graph "
             "replay | map + layer with one atomic per lane and table: eager | graph replay | layer alone, shipped / per lane (graph "
             "medians) | same bytes |", "|---|---|---|---|---|---|---|---|---|---|"]
    fmt = lambda r: f"{r['graph_us']:.2f} [{r['graph_min']:.2f} .. {r['graph_max']:.2f}]"  # noqa: E731
    lines += [f"| {r['scene']} | {[round(v, 4) for v in r['record']]} | {r['map']['eager_us']:.2f} | {fmt(r['map'])} | "
              f"{r['shipped']['eager_us']:.2f} | {fmt(r['shipped'])} | {r['per_lane']['eager_us']:.2f} | {fmt(r['per_lane'])} | "
              f"{r['shipped']['graph_us'] - r['map']['graph_us']:.2f} / {r['per_lane']['graph_us'] - r['map']['graph_us']:.2f} | "
              f"{r['same_bytes']} |" for r in krows]
    if host:
        total = sum(host.values())
        layer = (krows[0]["shipped"]["graph_us"] - krows[0]["map"]["graph_us"]) / 1e3
        lines += ["", f"the host route it replaces, the first input, medians over {args.host_runs} runs: download of the disparity and "
                  f"the labels {host['download']:.3f} ms, projection, cells and heights (numpy) {host['project']:.3f} ms, the ufunc.at "
                  f"tables and the update rule {host['tables']:.3f} ms: {total:.3f} ms per frame against {layer:.3f} ms"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max | ms / frame |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} | "
                  f"{1e3 / r['fps_median']:.3f} |" for r in srows]
        g, o = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the elevation layer per synchronous frame: {1e3 / o - 1e3 / g:.3f} ms of {1e3 / o:.3f} ms ({100 * (1 - o / g):.2f} %)"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
