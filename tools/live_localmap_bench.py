"""Cost of LiveSession's local map (codd_local_map), 540x960 in 576x960, default parameters (128 x 128 cells of 0.1 to a range
of 12.8).

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, five repetitions of the replay (median, min, max), on the three inputs of tools/live_scan_bench.py:
   the realistic frame (three boxes on a noisy floor; labels and record from codd_ground_plane itself), a fronto-parallel
   wall filling the view (every pixel an obstacle at one depth: all of the frame in one row of cells, the worst
   contention) and the floor alone.  The ego record is a step of 0.03 forward with a small turn, so every call scrolls
   nothing or one row; the state, the storage and the outputs stay on the device between the calls, as in a session.
2. The same call with ONE ATOMIC PER LANE in the pixel launch: codd_amd/csrc/localmap.hip compiled a second time with
   -DLOCALMAP_LANE_ATOMICS (and the entries renamed by -D) into build/live_localmap_bench/ and loaded with ctypes -- the
   variant lives nowhere in the library.  Its outputs must equal the shipped call's bytes, which the tool asserts on a
   call from equal states.
3. The host route this replaces, timed in the same process on the realistic frame: the download of the padded disparity
   and the labels into pinned memory, the composition of the pose, the projection in numpy and np.add.at; medians over
   --host-runs.
4. LiveSession.step frames/s with localmap= against the same session without it: sessions on one estimator, alternated
   in rounds, median over the rounds.

Every GPU part runs in a child process of its own under a time limit (--limit seconds each): a part that faults or hangs
ends the tool, which starts nothing after it.

    python tools/live_localmap_bench.py [--calls 200 --rounds 5 --per-round 25] [--out profiles/live_localmap.md]

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
LAUNCHES = 4
GH = GW = 128


def build_variant(verbose=False):
    """Path of the shared library holding the per-lane variant (entries lane_local_map_scratch, lane_local_map), compiled
    from codd_amd/csrc/localmap.hip when missing or older than it."""
    csrc = os.path.join(ROOT, "codd_amd", "csrc")
    src = os.path.join(csrc, "localmap.hip")
    out_dir = os.path.join(ROOT, "build", "live_localmap_bench")
    lib = os.path.join(out_dir, "liblocalmap_lane.so")
    deps = [src, os.path.join(csrc, "map_window.h"), os.path.join(csrc, "floor_frame.h"), os.path.join(csrc, "common.h"),
            os.path.join(ROOT, "include", "codd_hip.h")]
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(d) for d in deps):
        return lib
    os.makedirs(out_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DLOCALMAP_LANE_ATOMICS",
           "-Dcodd_local_map_scratch=lane_local_map_scratch", "-Dcodd_local_map=lane_local_map",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, src, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return lib


def load_variant():
    from codd_amd import _abi
    lib = C.CDLL(build_variant())
    res, args = _abi.SIGNATURES["codd_local_map"]
    lib.lane_local_map.restype, lib.lane_local_map.argtypes = res, args
    return lib


class Call:
    """The device buffers of one scene and the shipped call and the per-lane variant on them, each with a state of its own."""

    def __init__(self, scene, variant):
        import torch
        import live_scan_bench as sb
        self.sb, self.torch = sb, torch
        self.name, self.disp, self.lab, self.rec = scene[:4]
        dev = sb.DEV
        ego = np.zeros(16, np.float32)
        ego[0:3], ego[3:7], ego[7] = (0.001, 0.0, -0.03), (0.0, 0.002, 0.0, 1.0), 1.0
        self.ego = torch.from_numpy(ego).to(dev)
        self.variant = variant
        self.sets = []
        for _ in range(2):
            self.sets.append(dict(state=torch.zeros(32, dtype=torch.float64, device=dev),
                                  L=torch.zeros(GH, GW, dtype=torch.int16, device=dev), age=torch.zeros(GH, GW, dtype=torch.uint8, device=dev),
                                  mo=torch.zeros(GH, GW, dtype=torch.int16, device=dev), ao=torch.zeros(GH, GW, dtype=torch.uint8, device=dev),
                                  rec=torch.zeros(16, dtype=torch.float64, device=dev)))
        from codd_amd import ops
        self.scratch = torch.empty(ops.local_map_scratch(GH, GW), dtype=torch.uint8, device=dev)

    def shipped(self, fresh=False):
        from codd_amd import ops
        s, sb = self.sets[0], self.sb
        ops.local_map(self.disp, sb.SPEC["K"], sb.SPEC["calib"], (sb.H, sb.W), self.lab, self.rec, self.ego, s["state"], s["L"], s["age"],
                      s["mo"], s["ao"], s["rec"], fresh=fresh, scratch=self.scratch)

    def per_lane(self, fresh=False):
        from codd_amd import ops
        s, sb, p = self.sets[1], self.sb, ops.MAP_PARAMS
        rc = self.variant.lane_local_map(self.disp.data_ptr(), sb.HP, sb.WP, sb.H, sb.W, *[float(v) for v in sb.SPEC["K"]],
                                         float(sb.SPEC["calib"]), self.lab.data_ptr(), self.rec.data_ptr(), self.ego.data_ptr(),
                                         1 if fresh else 0, GH, GW, p["cell"], p["range_min"], p["range_max"], p["select"], p["min_pixels"],
                                         p["l_occ"], p["l_free"], p["l_min"], p["l_max"], p["decay"], p["occ_level"], p["free_level"],
                                         p["lost"], s["state"].data_ptr(), s["L"].data_ptr(), s["age"].data_ptr(),
                                         self.scratch.data_ptr(), self.scratch.numel(), s["mo"].data_ptr(), s["ao"].data_ptr(),
                                         s["rec"].data_ptr(), self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def same(self):
        a, b = self.sets
        return all(self.torch.equal(a[k].view(self.torch.uint8), b[k].view(self.torch.uint8)) for k in a)


def kernel_part(n):
    import torch
    import live_scan_bench as sb
    from codd_amd import ops
    ops.enable_autotune(False)
    variant = load_variant()
    rows = []
    for scene in sb.scenes():
        call = Call(scene, variant)
        for k in range(3):  # a fresh frame and two steps, each from equal states
            call.shipped(fresh=k == 0)
            call.per_lane(fresh=k == 0)
            torch.cuda.synchronize()
            assert call.same(), f"{call.name}: the per-lane variant's outputs differ from the shipped call's (call {k})"
        row = dict(scene=call.name, record=call.sets[0]["rec"].cpu().numpy().tolist(), same_bytes=True)
        for key, fn in (("shipped", call.shipped), ("per_lane", call.per_lane)):
            eager, graph, lo_, hi_ = sb.time_calls(fn, n)
            row[key] = dict(eager_us=eager, graph_us=graph, graph_min=lo_, graph_max=hi_)
        rows.append(row)
    return rows


def host_part(runs):
    """The route a user had to write, on the realistic frame: download disparity and labels, compose the pose, project,
    np.add.at, the update rule -> median milliseconds of each."""
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
    p = ops.MAP_PARAMS
    yy, xx = np.mgrid[:H, :W]
    L, age = np.zeros((GH, GW), np.int64), np.full((GH, GW), 255, np.int64)
    pose, head = np.zeros(2), np.array([0.0, 1.0])
    t = dict(download=[], project=[], tables=[])
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pd.copy_(disp, non_blocking=True)
        pl.copy_(lab, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d, labels = pd.numpy()[:H, :W], pl.numpy()
        pose = pose + 0.03 * head  # (the composition itself is a few dozen operations)
        ix0, iz0 = np.floor(pose / p["cell"]).astype(np.int64) - np.array([GW // 2, GH // 2])
        with np.errstate(all="ignore"):
            take = ((labels == 0) | (labels == 1)) & np.isfinite(d) & (d > 0)
            ys, xs = yy[take], xx[take]
            Z = sb.SPEC["calib"] / d[take]
            X0, X1 = Z * (xs - cx) / fx, Z * (ys - cy) / fy
            gx, gz = r_[0] * X0 + r_[1] * X1 + r_[2] * Z, f_[0] * X0 + f_[1] * X1 + f_[2] * Z
            rho = np.hypot(gx, gz)
            wx, wz = gx * head[1] + gz * head[0] + pose[0], gz * head[1] - gx * head[0] + pose[1]
            jx, jz = np.floor(wx / p["cell"]).astype(np.int64) - ix0, np.floor(wz / p["cell"]).astype(np.int64) - iz0
            ok = (rho >= p["range_min"]) & (rho < p["range_max"]) & (jx >= 0) & (jx < GW) & (jz >= 0) & (jz < GH)
        t2 = time.perf_counter()
        ob = ok & (labels[take] == 1)
        fl = ok & ~ob
        O, F = np.zeros((GH, GW), np.int64), np.zeros((GH, GW), np.int64)
        np.add.at(O, (jz[ob], jx[ob]), 1)
        np.add.at(F, (jz[fl], jx[fl]), 1)
        occ = O >= p["min_pixels"]
        free = ~occ & (F >= p["min_pixels"])
        L = np.where(occ, np.minimum(L + p["l_occ"], p["l_max"]), np.where(free, np.maximum(L - p["l_free"], p["l_min"]), L))
        age = np.where(occ | free, 0, np.where(age == 255, 255, np.minimum(age + 1, 254)))
        t3 = time.perf_counter()
        for key, v in zip(t, (t1 - t0, t2 - t1, t3 - t2)):
            t[key].append(1e3 * v)
    return {key: float(np.median(v)) for key, v in t.items()}


def session_part(rounds, per_round):
    import live_scan_bench as sb
    base = dict(ground=True, egomotion=True)
    return sb.session_part(rounds, per_round, {"ground, egomotion": base, "ground, egomotion, localmap": dict(base, localmap=True)})


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
        raise SystemExit(f"live_localmap_bench: part {part!r} ended with status {r.returncode}; nothing else was started")
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
    lines = [f"codd_local_map at 960x540 in 960x576, {GH} x {GW} cells, default parameters, HIP events over {args.calls} calls after 20 "
             f"warm-ups, graph replay repeated five times (median [min .. max])", "",
             "| input | record of the last checked call (integrated, linked, restarts, frames, px, pz, hx, hz, ix0, iz0, pixels, occupied, "
             "free, never seen, dx, dz) | shipped, 4 launches: us / call eager | graph replay | one atomic per lane: eager | graph replay "
             "| same bytes |", "|---|---|---|---|---|---|---|"]
    fmt = lambda r: f"{r['graph_us']:.2f} [{r['graph_min']:.2f} .. {r['graph_max']:.2f}]"  # noqa: E731
    lines += [f"| {r['scene']} | {[round(v, 4) for v in r['record']]} | {r['shipped']['eager_us']:.2f} | {fmt(r['shipped'])} | "
              f"{r['per_lane']['eager_us']:.2f} | {fmt(r['per_lane'])} | {r['same_bytes']} |" for r in krows]
    if host:
        total = sum(host.values())
        lines += ["", f"the host route it replaces, the first input, medians over {args.host_runs} runs: download of the disparity and "
                  f"the labels {host['download']:.3f} ms, projection and cell indices (numpy) {host['project']:.3f} ms, np.add.at and the "
                  f"update rule {host['tables']:.3f} ms: {total:.3f} ms per frame against {krows[0]['shipped']['graph_us'] / 1e3:.3f} ms"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max | ms / frame |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} | "
                  f"{1e3 / r['fps_median']:.3f} |" for r in srows]
        g, o = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the local map per synchronous frame: {1e3 / o - 1e3 / g:.3f} ms of {1e3 / o:.3f} ms ({100 * (1 - o / g):.2f} %)"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
