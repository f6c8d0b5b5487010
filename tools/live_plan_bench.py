"""Cost of LiveSession's plan (codd_plan) and of the host route it replaces.

1. Microseconds per call, HIP events over N calls after 20 warm-ups, five repetitions (median, min, max), on four inputs: an
   open floor, rooms with doorways and the same rooms with a frontier goal at 128 x 128, and rooms at 160 x 160, the limit.
   Next to each the rounds the relaxation took (the entry leaves them in its scratch; no output holds them).
2. The same for the relaxation variants: codd_amd/csrc/plan.hip compiled again with -DPLAN_JACOBI and / or -DPLAN_THREADS=512
   (and the entries renamed by -D) into build/live_plan_bench/ and loaded with ctypes.  Every variant's outputs must equal the
   shipped call's bytes, which the tool asserts on every input.
3. The host route this replaces, on the same inputs: the download of cost and reach into pinned memory and the restatement
   of tests/live_plan_ref.py (a heap Dijkstra in Python; its outputs must equal the device's).
4. LiveSession.step milliseconds per frame with plan=True against the same session without it at the default grid:
   sessions on one estimator, alternated in rounds, median over the rounds.

Every GPU part runs in a child process of its own under a time limit (--limit seconds each): a part that faults or hangs
ends the tool, which starts nothing after it.

    python tools/live_plan_bench.py [--calls 100 --rounds 5 --per-round 20] [--out FILE.json]

--build-only compiles the variants and exits (no GPU needed).
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
VARIANTS = {"jacobi-512": ["-DPLAN_JACOBI", "-DPLAN_THREADS=512"], "jacobi-1024": ["-DPLAN_JACOBI"],
            "sweeps-512": ["-DPLAN_THREADS=512"]}  # (the library: two Gauss-Seidel sweeps, 1024 threads)


def build_variant(name, verbose=False):
    csrc = os.path.join(ROOT, "codd_amd", "csrc")
    src = os.path.join(csrc, "plan.hip")
    out_dir = os.path.join(ROOT, "build", "live_plan_bench")
    lib = os.path.join(out_dir, f"libplan_{name}.so")
    deps = [src, os.path.join(csrc, "common.h"), os.path.join(ROOT, "include", "codd_hip.h")]
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(d) for d in deps):
        return lib
    os.makedirs(out_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", *VARIANTS[name],
           "-Dcodd_plan_scratch=var_plan_scratch", "-Dcodd_plan=var_plan", "-I", os.path.join(ROOT, "include"), "-I", csrc, src, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return lib


def inputs():
    import live_plan_ref as pr
    rooms = pr.make("rooms-128", 128, 128, (66, 66), goal=(2, 2), max_path=1024, build=pr.rooms(1))
    far = int(np.flatnonzero(rooms["reach"].ravel())[-1])  # the last reachable cell stands in for the nearest frontier
    return [pr.make("open-128", 128, 128, (64, 64), goal=(120, 10), max_path=1024), rooms,
            pr.make("rooms-128-frontier", 128, 128, (66, 66), mode=pr.FRONTIER, cost_record=far, max_path=1024, build=pr.rooms(1)),
            pr.make("rooms-160", 160, 160, (80, 80), goal=(157, 3), max_path=1024, build=pr.rooms(2))]


class Call:
    def __init__(self, c, lib=None):
        import torch
        from codd_amd import _abi, ops
        self.c, self.torch = c, torch
        gh, gw = c["cost"].shape
        dev = "cuda:0"
        self.cost, self.reach = torch.from_numpy(c["cost"]).to(dev), torch.from_numpy(c["reach"]).to(dev)
        rec = lambda r: torch.from_numpy(r if r is not None else np.zeros(16)).to(dev)  # noqa: E731
        self.crec, self.mrec = rec(c["cost_record"]), rec(c["map_record"])
        self.pot, self.dir = torch.zeros(gh, gw, dtype=torch.int32, device=dev), torch.zeros(gh, gw, dtype=torch.uint8, device=dev)
        self.path, self.rec = torch.zeros(c["max_path"], dtype=torch.int32, device=dev), torch.zeros(16, dtype=torch.float64, device=dev)
        self.scratch = torch.zeros(ops.plan_scratch(gh, gw) + 16, dtype=torch.uint8, device=dev)
        self.fn = _abi.load().codd_plan
        if lib is not None:
            self.fn = C.CDLL(lib).var_plan
            self.fn.restype, self.fn.argtypes = _abi.SIGNATURES["codd_plan"]

    def __call__(self):
        c, t = self.c, self.torch
        gh, gw = c["cost"].shape
        rc = self.fn(self.cost.data_ptr(), self.reach.data_ptr(), self.crec.data_ptr(), self.mrec.data_ptr(), gh, gw, c["start"][0],
                     c["start"][1], c["mode"], c["goal_i"], c["goal_j"], c["goal_x"], c["goal_z"], c["cell"], c["goal_r2"], c["neutral"],
                     c["factor"], c["unknown_cost"], c["max_path"], self.scratch.data_ptr(), self.scratch.numel(), self.pot.data_ptr(),
                     self.dir.data_ptr(), self.path.data_ptr(), self.rec.data_ptr(), t.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def outputs(self):
        self.torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in (self.pot, self.dir, self.path, self.rec)]

    def rounds(self):
        off = (-self.scratch.data_ptr()) % 16
        return int(self.scratch[off:off + 4].cpu().numpy().view(np.int32)[0])

    def time(self, calls):
        t = self.torch
        for _ in range(20):
            self()
        reps = []
        for _ in range(5):
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                self()
            b.record()
            t.cuda.synchronize()
            reps.append(a.elapsed_time(b) * 1000.0 / calls)
        return dict(us=float(np.median(reps)), min=min(reps), max=max(reps), rounds=self.rounds())


def part_calls(args):
    import live_plan_ref as pr
    import torch
    out = {}
    for c in inputs():
        shipped = Call(c)
        row = dict(shipped=shipped.time(args.calls))
        want = shipped.outputs()
        for name in VARIANTS:
            v = Call(c, build_variant(name))
            row[name] = v.time(args.calls)
            assert v.outputs() == want, f"{c['name']}: variant {name} differs from the shipped call"
        host_cost, host_reach = (torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (shipped.cost, shipped.reach))
        t0 = time.perf_counter()
        host_cost.copy_(shipped.cost)
        host_reach.copy_(shipped.reach)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ref = pr.plan(dict(c, cost=host_cost.numpy(), reach=host_reach.numpy()))
        t2 = time.perf_counter()
        assert [ref["potential"].tobytes(), ref["dir"].tobytes(), ref["path"].tobytes(), ref["record"].tobytes()] == want, c["name"]
        row["host"] = dict(download_us=(t1 - t0) * 1e6, restatement_us=(t2 - t1) * 1e6)
        out[c["name"]] = row
        print(json.dumps({c["name"]: row}), flush=True)
    return out


def part_session(args):
    import test_gpu_live_motion as glm
    import test_gpu_live_objects as glo
    import torch
    from codd_amd import ops
    ops.enable_autotune(False)
    kw = dict(ground=glo.GROUND, egomotion=True, localmap=True, costmap=True)
    sessions = dict(without=glm._session(**kw), plan=glm._session(plan=True, **kw))
    frames = glm._frames()
    ms = {k: [] for k in sessions}
    for r in range(args.rounds + 1):
        for k, s in sessions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in range(args.per_round):
                s.step(*frames[n % len(frames)])
            torch.cuda.synchronize()
            if r:  # (round 0 warms up and captures)
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.per_round)
    for s in sessions.values():
        s.reset()
        s.close()
    out = {k: dict(ms=float(np.median(v)), min=min(v), max=max(v)) for k, v in ms.items()}
    print(json.dumps(dict(session=out)), flush=True)
    return dict(session=out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=100)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--per-round", type=int, default=20)
    p.add_argument("--limit", type=int, default=240, help="seconds for each GPU part")
    p.add_argument("--out")
    p.add_argument("--build-only", action="store_true")
    p.add_argument("--part", choices=("calls", "session"))
    args = p.parse_args()
    if args.part:
        (part_calls if args.part == "calls" else part_session)(args)
        return
    for name in VARIANTS:
        print(build_variant(name, verbose=True))
    if args.build_only:
        return
    results = {}
    for part in ("calls", "session"):  # each in a child of its own, under its own limit; nothing starts after a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--calls", str(args.calls), "--rounds", str(args.rounds),
               "--per-round", str(args.per_round)]
        done = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        print(done.stdout, end="", flush=True)
        if done.returncode != 0:
            sys.exit(f"part {part} ended with {done.returncode}: nothing more is started")
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                results.update(json.loads(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
