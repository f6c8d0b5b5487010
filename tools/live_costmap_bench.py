"""Cost of LiveSession's cost map (codd_cost_map) and of the host route it replaces.

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, five repetitions of the replay (median, min, max), at 128 x 128 cells (R = 10) and at 512 x 512 (R = 10
   and R = 40), on three maps each: the local map of a session frame (tools/live_scan_bench.py's three boxes on a noisy floor,
   through codd_ground_plane and four calls of codd_local_map at that grid), an empty map (nothing occupied, everything
   free) and an all-occupied one.
2. For the small grid, both paths: codd_amd/csrc/costmap.hip compiled a second time with -DCOSTMAP_ONE_WORKGROUP (and the
   entries renamed by -D) into build/live_costmap_bench/ and loaded with ctypes -- the single-workgroup variant lives
   nowhere in the library.  Its outputs must equal the shipped call's bytes, which the tool asserts on every map.
3. The host route this replaces, timed in the same process: the download of map and age into pinned memory and the
   brute-force numpy restatement of tests/live_costmap_ref.py (numpy, not an optimised library; its outputs must equal the
   device's).  It visits every pair of a cell and an occupied cell, so it is skipped (null) where that is more than
   --host-pairs pairs.
4. LiveSession.step frames/s with costmap= against the same session without it: sessions on one estimator, alternated
   in rounds, median over the rounds.

Every GPU part runs in a child process of its own under a time limit (--limit seconds each): a part that faults or hangs
ends the tool, which starts nothing after it.

    python tools/live_costmap_bench.py [--calls 200 --rounds 5 --per-round 25] [--out profiles/live_costmap.md]

--build-only compiles the single-workgroup variant and exits (no GPU needed).
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
CONFIGS = ((128, 0.1, 10), (512, 0.025, 10), (512, 0.025, 40))  # (side, cell, R): the same 12.8 x 12.8 of floor
ROBOT_CELLS, SCALING, START_RADIUS = 3, 3.0, 1.5  # the robot's radius in cells: 0.3 at the default cell


def build_variant(verbose=False):
    """Path of the shared library holding the single-workgroup variant (entries one_cost_map_scratch, one_cost_map),
    compiled from codd_amd/csrc/costmap.hip when missing or older than it."""
    csrc = os.path.join(ROOT, "codd_amd", "csrc")
    src = os.path.join(csrc, "costmap.hip")
    out_dir = os.path.join(ROOT, "build", "live_costmap_bench")
    lib = os.path.join(out_dir, "libcostmap_one.so")
    deps = [src, os.path.join(csrc, "common.h"), os.path.join(ROOT, "include", "codd_hip.h")]
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(d) for d in deps):
        return lib
    os.makedirs(out_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DCOSTMAP_ONE_WORKGROUP",
           "-Dcodd_cost_map_scratch=one_cost_map_scratch", "-Dcodd_cost_map=one_cost_map",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, src, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return lib


def load_variant():
    from codd_amd import _abi
    lib = C.CDLL(build_variant())
    res, args = _abi.SIGNATURES["codd_cost_map"]
    lib.one_cost_map.restype, lib.one_cost_map.argtypes = res, args
    return lib


def session_map(side, cell):
    """(map int16, age uint8) [side,side] on the device: four frames of the realistic scene through codd_local_map."""
    import torch
    import live_scan_bench as sb
    from codd_amd import ops
    name, disp, lab, rec = sb.scenes()[0][:4]
    dev = sb.DEV
    ego = np.zeros(16, np.float32)
    ego[0:3], ego[3:7], ego[7] = (0.001, 0.0, -0.03), (0.0, 0.002, 0.0, 1.0), 1.0
    ego = torch.from_numpy(ego).to(dev)
    state = torch.zeros(32, dtype=torch.float64, device=dev)
    L, age = torch.zeros(side, side, dtype=torch.int16, device=dev), torch.zeros(side, side, dtype=torch.uint8, device=dev)
    mo, ao = torch.zeros_like(L), torch.zeros_like(age)
    out = torch.zeros(16, dtype=torch.float64, device=dev)
    for k in range(4):
        ops.local_map(disp, sb.SPEC["K"], sb.SPEC["calib"], (sb.H, sb.W), lab, rec, ego, state, L, age, mo, ao, out, fresh=k == 0,
                      cell=cell, min_pixels=1 if side > 128 else 4)
    torch.cuda.synchronize()
    return mo, ao


class Call:
    """The device buffers of one map and the shipped call and the single-workgroup variant on them, each with outputs of its own."""

    def __init__(self, name, m, age, cell, R, variant):
        import torch
        from codd_amd import ops
        self.torch, self.name, self.map, self.age, self.R, self.variant = torch, name, m, age, R, variant
        gh, gw = m.shape
        dev = m.device
        R_, lut = ops.cost_lut(cell, ROBOT_CELLS * cell, (R - 0.5) * cell, SCALING)  # (ceil: R)
        assert R_ == R, (R_, R)
        self.lut_host = lut
        self.lut = torch.from_numpy(lut).to(dev)
        self.start = (gw // 2, gh // 2)
        self.seed_r2 = int(np.floor((START_RADIUS / cell) ** 2))
        new = lambda: dict(dist2=torch.zeros(gh, gw, dtype=torch.int32, device=dev), nearest=torch.zeros(gh, gw, dtype=torch.int32, device=dev),  # noqa: E731
                           cost=torch.zeros(gh, gw, dtype=torch.uint8, device=dev), reach=torch.zeros(gh, gw, dtype=torch.uint8, device=dev),
                           record=torch.zeros(16, dtype=torch.float64, device=dev))
        self.sets = [new(), new()]
        self.scratch = torch.empty(ops.cost_map_scratch(gh, gw, R), dtype=torch.uint8, device=dev)

    def shipped(self):
        from codd_amd import ops
        s = self.sets[0]
        ops.cost_map(self.map, self.age, self.lut, self.R, self.start, s["dist2"], s["nearest"], s["cost"], s["reach"], s["record"],
                     seed_r2=self.seed_r2, scratch=self.scratch)

    def one(self):
        from codd_amd import ops
        s = self.sets[1]
        gh, gw = self.map.shape
        rc = self.variant.one_cost_map(self.map.data_ptr(), self.age.data_ptr(), gh, gw, ops.MAP_PARAMS["occ_level"],
                                           ops.MAP_PARAMS["free_level"], self.R, self.lut.data_ptr(), self.start[0], self.start[1],
                                           self.seed_r2, 0, self.scratch.data_ptr(), self.scratch.numel(), s["dist2"].data_ptr(),
                                           s["nearest"].data_ptr(), s["cost"].data_ptr(), s["reach"].data_ptr(), s["record"].data_ptr(),
                                           self.torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def same(self):
        a, b = self.sets
        return all(self.torch.equal(a[k].view(self.torch.uint8), b[k].view(self.torch.uint8)) for k in a)

    def host(self, runs, max_pairs):
        """Median ms of the download and of the numpy restatement, or None where it has too many pairs to visit."""
        import live_costmap_ref as cr
        from codd_amd import ops
        torch = self.torch
        gh, gw = self.map.shape
        occ = int((self.map >= ops.MAP_PARAMS["occ_level"]).sum())
        if occ * gh * gw > max_pairs:
            return None
        pm, pa = torch.empty(gh, gw, dtype=torch.int16, pin_memory=True), torch.empty(gh, gw, dtype=torch.uint8, pin_memory=True)
        down, work = [], []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pm.copy_(self.map, non_blocking=True)
            pa.copy_(self.age, non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = cr.cost_map(dict(map=pm.numpy(), age=pa.numpy(), R=self.R, lut=self.lut_host, start=self.start, seed_r2=self.seed_r2,
                                   through_unknown=False, occ_level=ops.MAP_PARAMS["occ_level"], free_level=ops.MAP_PARAMS["free_level"]))
            t2 = time.perf_counter()
            down.append(1e3 * (t1 - t0))
            work.append(1e3 * (t2 - t1))
        for k, v in self.sets[0].items():
            assert v.cpu().numpy().tobytes() == out[k].tobytes(), f"{self.name}: {k} differs from the restatement"
        return dict(download_ms=float(np.median(down)), numpy_ms=float(np.median(work)))


def kernel_part(n, host_runs, max_pairs):
    import torch
    import live_scan_bench as sb
    from codd_amd import ops
    ops.enable_autotune(False)
    variant = load_variant()
    rows = []
    for side, cell, R in CONFIGS:
        m, age = session_map(side, cell)
        maps = (("a session frame", m, age),
                ("empty", torch.full_like(m, ops.MAP_PARAMS["free_level"]), torch.zeros_like(age)),
                ("all occupied", torch.full_like(m, ops.MAP_PARAMS["occ_level"]), torch.zeros_like(age)))
        for name, mm, aa in maps:
            call = Call(name, mm, aa, cell, R, variant)
            call.shipped()
            call.one()  # (above its threshold the variant runs the five launches too)
            torch.cuda.synchronize()
            assert call.same(), f"{side} x {side}, R = {R}, {name}: the variant's outputs differ from the shipped call's"
            row = dict(side=side, R=R, map=name, record=call.sets[0]["record"].cpu().numpy()[:10].tolist(), same_bytes=True,
                       single=side * side <= 16384)
            for key, fn in (("shipped", call.shipped), ("one", call.one)):
                if key == "one" and not row["single"]:
                    continue  # (the variant IS the shipped path at this size)
                eager, graph, lo_, hi_ = sb.time_calls(fn, n)
                row[key] = dict(eager_us=eager, graph_us=graph, graph_min=lo_, graph_max=hi_)
            row["host"] = call.host(host_runs, max_pairs)
            rows.append(row)
    return rows


def session_part(rounds, per_round):
    import live_scan_bench as sb
    base = dict(ground=True, egomotion=True, localmap=True)
    return sb.session_part(rounds, per_round, {"ground, egomotion, localmap": base, "ground, egomotion, localmap, costmap": dict(base, costmap=True)})


def child(args):
    """One GPU part, in this process: prints one JSON line."""
    out = kernel_part(args.calls, args.host_runs, args.host_pairs) if args.part == "kernel" else session_part(args.rounds, args.per_round)
    print("RESULT " + json.dumps(out), flush=True)


def run_part(part, args):
    """A child process for one part, under the time limit; its result, or SystemExit: nothing runs after a part that failed."""
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--part", part, "--calls", str(args.calls),
           "--rounds", str(args.rounds), "--per-round", str(args.per_round), "--host-runs", str(args.host_runs),
           "--host-pairs", str(args.host_pairs)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        sys.stdout.write(r.stdout)
        raise SystemExit(f"live_costmap_bench: part {part!r} ended with status {r.returncode}; nothing else was started")
    return json.loads(lines[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-round", type=int, default=25)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=1 << 31, help="skip the numpy route above this many (cell, occupied cell) pairs")
    ap.add_argument("--limit", type=int, default=300, help="seconds per GPU part")
    ap.add_argument("--kernel-only", action="store_true", help="parts 1 to 3 only")
    ap.add_argument("--build-only", action="store_true", help="compile the single-workgroup variant and exit")
    ap.add_argument("--part", choices=("kernel", "session"), help=argparse.SUPPRESS)
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
    srows = [] if args.kernel_only else run_part("session", args)
    print(json.dumps(dict(calls=args.calls, kernel=krows, session=srows)))
    fmt = lambda r: "" if r is None else f"{r['eager_us']:.2f} / {r['graph_us']:.2f} [{r['graph_min']:.2f} .. {r['graph_max']:.2f}]"  # noqa: E731
    host = lambda h: "not run (too many pairs)" if h is None else f"{h['download_ms']:.3f} + {h['numpy_ms']:.1f}"  # noqa: E731
    lines = [f"codd_cost_map, robot radius {ROBOT_CELLS} cells, inflation radius R - 0.5 cells, scaling {SCALING}, start radius {START_RADIUS}, HIP events over {args.calls} calls after 20 "
             f"warm-ups, graph replay repeated five times: us / call eager / graph replay median [min .. max]", "",
             "| grid | R | map | record [0:10] (occupied, inscribed, no information, reachable, frontiers, start ok, start dist2, start "
             "nearest, nearest frontier, its dist2) | shipped, 5 launches | one workgroup, 1 launch (not in the library) | same bytes | host: download + numpy "
             "restatement, ms |", "|---|---|---|---|---|---|---|---|"]
    lines += [f"| {r['side']} x {r['side']} | {r['R']} | {r['map']} | {[int(v) for v in r['record']]} | {fmt(r['shipped'])} | "
              f"{fmt(r.get('one')) or 'above its 16384 cells'} | {r['same_bytes']} | {host(r['host'])} |"
              for r in krows]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max | ms / frame |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} | "
                  f"{1e3 / r['fps_median']:.3f} |" for r in srows]
        g, o = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the cost map per synchronous frame: {1e3 / o - 1e3 / g:.3f} ms of {1e3 / o:.3f} ms ({100 * (1 - o / g):.2f} %)"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
