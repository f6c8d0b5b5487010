"""Cost of LiveSession's range scan (codd_range_scan), 540x960 in 576x960, default parameters (256 beams over the camera's
field, 128 bins to 12.8).

1. One call replayed from a captured graph (device time, launch gaps included) and issued eagerly, HIP events over N calls
   after 20 warm-ups, five repetitions of the replay (median, min, max), on three inputs: the realistic frame of
   tools/live_objects_bench.py (three boxes on a noisy floor; labels, record and id map from codd_ground_plane and
   codd_objects themselves); a fronto-parallel wall filling the view (every pixel an obstacle at one depth: all of the
   frame in one range bin of every beam, the worst contention); and the floor alone.  codd_objects is timed on the same
   frames by the same loop, for comparison.
2. The same call with ONE ATOMIC PER LANE in the pixel launch: a variant of codd_amd/csrc/scan.hip that this tool makes
   itself -- it replaces the wave's walk over its distinct keys by the lanes' own atomics, renames the entry, compiles the
   text with hipcc into build/live_scan_bench/ and loads it with ctypes -- so the variant lives nowhere in the library.
   Its outputs must equal the shipped call's bytes (the aggregation changes no byte), which the tool asserts.
3. The host route this replaces, timed in the same process on the realistic frame: the download of the padded disparity
   and the labels into pinned memory, then the projection, arctan2, the binning and np.add.at / np.minimum.at in numpy;
   medians over --host-runs.
4. LiveSession.step frames/s with scan= against the same session without it: sessions on one estimator, alternated in
   rounds, median over the rounds.

    python tools/live_scan_bench.py [--calls 200 --rounds 5 --per-round 25] [--out profiles/live_scan.md]

--build-only compiles the per-lane variant and exits (no GPU needed).  CODD_LIB_AB=<another build of libcodd_hip.so> python
tools/live_scan_bench.py --kernel-only measures that build's kernels with the same tool.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, HP, WP = 540, 960, 576, 960
DEV = "cuda:0"
LAUNCHES = 3
SPEC = dict(crop=(H, W), padded=(HP, WP), K=(1050.0, 1050.0, 479.5, 269.5), calib=210.0, cam_h=1.2, pitch=0.15, roll=0.03,
            name="bench", scene="bench", par={}, seed=None, grid=None)
BOXES = [(60, 300, 150, 400), (380, 620, 190, 470), (700, 900, 170, 360)]  # (x0, x1, y0, y1) of tools/live_objects_bench.py
WALL_DISP = 70.0  # calib / 70 = 3 units away
BEAMS, BINS = 256, 128

# ---- the one-atomic-per-lane variant ------------------------------------------------------------------------------------
AGG_BEGIN = "  unsigned long long rest = __ballot(key >= 0);\n"
AGG_END = "    rest &= ~m;\n  }\n"
PER_LANE = """  if (key >= 0) {  // (tools/live_scan_bench.py: one atomic per lane and value)
    const int cell = key >> 1;
    if (key & 1) {
      atomicAdd(a.O + cell, 1);
      atomicMin(a.N + cell, ((unsigned long long)rb << 32) | (unsigned)(y * a.w + x));
    } else {
      atomicAdd(a.F + cell, 1);
    }
  }
"""


def build_variant(verbose=False):
    """Path of the shared library holding the per-lane variant (entries lane_range_scan_scratch, lane_range_scan), compiled
    from the text of codd_amd/csrc/scan.hip when missing or older than it."""
    src = os.path.join(ROOT, "codd_amd", "csrc", "scan.hip")
    out_dir = os.path.join(ROOT, "build", "live_scan_bench")
    lib = os.path.join(out_dir, "libscan_lane.so")
    if os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(src), os.path.getmtime(__file__)):
        return lib
    text = open(src).read()
    i, j = text.index(AGG_BEGIN), text.index(AGG_END)
    assert 0 < i < j and text.count(AGG_BEGIN) == 1 and text.count(AGG_END) == 1, "scan.hip: the aggregation block moved"
    text = text[:i] + PER_LANE + text[j + len(AGG_END):]
    text = text.replace("codd_range_scan", "lane_range_scan")
    os.makedirs(out_dir, exist_ok=True)
    hip = os.path.join(out_dir, "scan_lane.hip")
    with open(hip, "w") as f:
        f.write(text)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "codd_amd", "csrc"), hip, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return lib


def load_variant():
    from codd_amd import _abi
    lib = C.CDLL(build_variant())
    res, args = _abi.SIGNATURES["codd_range_scan"]
    lib.lane_range_scan.restype, lib.lane_range_scan.argtypes = res, args
    return lib


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
    """[(name, disp [HP,WP], labels [H,W], record, ids [H,W] uint16, objects' (count, obj_i, obj_f, scratch))], device
    tensors; labels, record and ids come from codd_ground_plane and codd_objects themselves."""
    import live_ground_ref as lg
    import live_objects_ref as lo
    from codd_amd import ops
    lg.SCENES["bench"] = dict(boxes=BOXES)
    lg.SCENES["bench-floor"] = dict(boxes=[])
    out = []
    m = ops.OBJECT_PARAMS["max_objects"]
    for name, scene in (("three boxes on a floor", "bench"), ("the floor alone", "bench-floor")):
        c = lg.case(dict(SPEC, scene=scene))
        disp = torch.from_numpy(c["disp"]).to(DEV)
        rec = torch.zeros(32, dtype=torch.float64, device=DEV)
        lab = torch.empty(H, W, dtype=torch.uint8, device=DEV)
        ops.ground_plane(disp, c["K"], c["calib"], (H, W), rec, lab, **{k: v for k, v in c["par"].items() if k != "cell"})
        torch.cuda.synchronize()
        assert float(rec[3]) == 1.0
        out.append([name, disp, lab, rec])
    wall = np.full((HP, WP), WALL_DISP, np.float32)
    out.insert(1, ["a fronto-parallel wall filling the view", torch.from_numpy(wall).to(DEV),
                   torch.full((H, W), lo.OBSTACLE, dtype=torch.uint8, device=DEV),
                   torch.from_numpy(lo.record(cam_h=SPEC["cam_h"], pitch=0.0, roll=0.0, K=SPEC["K"], calib=SPEC["calib"])).to(DEV)])
    for s in out:
        bufs = (torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(m, 8, dtype=torch.int32, device=DEV),
                torch.zeros(m, 8, device=DEV), torch.empty(ops.objects_scratch(H, W, m), dtype=torch.uint8, device=DEV))
        ids = torch.empty(H, W, dtype=torch.uint16, device=DEV)
        ops.objects(s[1], SPEC["K"], SPEC["calib"], (H, W), s[2], s[3], *bufs[:3], ids=ids, scratch=bufs[3])
        s += [ids, bufs]
    torch.cuda.synchronize()
    return out


class Call:
    """The device buffers of one scene and the shipped call, the per-lane variant and codd_objects on them."""

    def __init__(self, scene, variant):
        from codd_amd import ops
        self.name, self.disp, self.lab, self.rec, self.ids, self.obj = scene
        K = SPEC["K"]
        lo_, hi_ = np.arctan((0.0 - K[2]) / K[0]), np.arctan((W - 1.0 - K[2]) / K[0])
        self.edges = torch.from_numpy(ops.scan_edges(BEAMS, lo_, hi_)).to(DEV)
        self.scratch = torch.empty(ops.range_scan_scratch(BEAMS, BINS), dtype=torch.uint8, device=DEV)
        new = lambda: (torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(BEAMS, 4, dtype=torch.int32, device=DEV),  # noqa: E731
                       torch.zeros(BEAMS, 4, device=DEV))
        self.out, self.out_lane = new(), new()
        self.variant = variant

    def shipped(self):
        from codd_amd import ops
        ops.range_scan(self.disp, SPEC["K"], SPEC["calib"], (H, W), self.lab, self.rec, self.edges, *self.out, ids=self.ids,
                       scratch=self.scratch, bins=BINS)

    def per_lane(self):
        from codd_amd import ops
        p = ops.SCAN_PARAMS
        rc = self.variant.lane_range_scan(self.disp.data_ptr(), HP, WP, H, W, *[float(v) for v in SPEC["K"]], float(SPEC["calib"]),
                                          self.lab.data_ptr(), self.rec.data_ptr(), self.ids.data_ptr(), self.edges.data_ptr(),
                                          BEAMS, BINS, p["range_min"], p["range_max"], p["select"], p["min_pixels"],
                                          self.scratch.data_ptr(), self.scratch.numel(), *(t.data_ptr() for t in self.out_lane),
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def objects(self):
        from codd_amd import ops
        ops.objects(self.disp, SPEC["K"], SPEC["calib"], (H, W), self.lab, self.rec, *self.obj[:3], ids=self.ids, scratch=self.obj[3])


def kernel_part(n):
    variant = load_variant()
    rows = []
    for scene in scenes():
        call = Call(scene, variant)
        call.shipped()
        call.per_lane()
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(call.out, call.out_lane))
        assert same, f"{call.name}: the per-lane variant's outputs differ from the shipped call's"
        row = dict(scene=call.name, count=call.out[0].cpu().numpy().tolist(), same_bytes=same)
        for key, fn in (("shipped", call.shipped), ("per_lane", call.per_lane), ("objects", call.objects)):
            eager, graph, lo_, hi_ = time_calls(fn, n)
            row[key] = dict(eager_us=eager, graph_us=graph, graph_min=lo_, graph_max=hi_)
        rows.append(row)
    return rows


def host_part(runs):
    """The route a user had to write, on the realistic frame: download disparity and labels, project, arctan2, bin,
    np.add.at and np.minimum.at -> (median milliseconds of each, hit beams)."""
    from codd_amd import ops
    name, disp, lab, rec, ids, _ = scenes()[0]
    pd, pl = torch.empty(HP, WP, pin_memory=True), torch.empty(H, W, dtype=torch.uint8, pin_memory=True)
    record = rec.cpu().numpy()
    fx, fy, cx, cy = SPEC["K"]
    n_, f_ = record[8:11], record[22:25]
    r_ = np.cross(f_, n_)
    a0, a1 = np.arctan((0.0 - cx) / fx), np.arctan((W - 1.0 - cx) / fx)
    p = ops.SCAN_PARAMS
    yy, xx = np.mgrid[:H, :W]
    t = dict(download=[], project=[], tables=[])
    hits = 0
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pd.copy_(disp, non_blocking=True)
        pl.copy_(lab, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d, labels = pd.numpy()[:H, :W], pl.numpy()
        with np.errstate(all="ignore"):
            take = ((labels == 0) | (labels == 1)) & np.isfinite(d) & (d > 0)
            ys, xs = yy[take], xx[take]
            Z = SPEC["calib"] / d[take]
            X0, X1 = Z * (xs - cx) / fx, Z * (ys - cy) / fy
            gx, gz = r_[0] * X0 + r_[1] * X1 + r_[2] * Z, f_[0] * X0 + f_[1] * X1 + f_[2] * Z
            rho, ang = np.hypot(gx, gz), np.arctan2(gx, gz)
            beam = np.floor((ang - a0) / ((a1 - a0) / BEAMS)).astype(np.int64)
            k = np.minimum(np.floor(rho / (p["range_max"] / BINS)).astype(np.int64), BINS - 1)
            ok = (gz > 0) & (rho >= p["range_min"]) & (rho < p["range_max"]) & (beam >= 0) & (beam < BEAMS)
        t2 = time.perf_counter()
        ob = ok & (labels[take] == 1)
        fl = ok & ~ob
        O, F = np.zeros((BEAMS, BINS), np.int64), np.zeros((BEAMS, BINS), np.int64)
        N = np.full((BEAMS, BINS), np.inf)
        np.add.at(O, (beam[ob], k[ob]), 1)
        np.add.at(F, (beam[fl], k[fl]), 1)
        np.minimum.at(N, (beam[ob], k[ob]), rho[ob])
        first = np.argmax(O >= p["min_pixels"], 1)
        hits = int((O >= p["min_pixels"]).any(1).sum())
        ranges = N[np.arange(BEAMS), first]  # noqa: F841  (the per-beam resolve is negligible next to the tables)
        t3 = time.perf_counter()
        for key, v in zip(t, (t1 - t0, t2 - t1, t3 - t2)):
            t[key].append(1e3 * v)
    return {key: float(np.median(v)) for key, v in t.items()}, hits


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
    ap.add_argument("--kernel-only", action="store_true", help="part 1 and 2 only")
    ap.add_argument("--no-session", action="store_true", help="the kernel and host parts only")
    ap.add_argument("--build-only", action="store_true", help="compile the per-lane variant and exit")
    ap.add_argument("--out", default=None, help="write the tables (markdown) here")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if args.build_only:
        print(build_variant(verbose=True))
        return
    from codd_amd import _abi, ops
    ops.enable_autotune(False)
    krows = kernel_part(args.calls)
    host, hits = ({}, 0) if args.kernel_only else host_part(args.host_runs)
    srows = []
    if not (args.kernel_only or args.no_session):
        base = dict(ground=True, objects=True)
        srows = session_part(args.rounds, args.per_round, {"ground, objects": base, "ground, objects, scan": dict(base, scan=True)})
    print(json.dumps(dict(shape=[H, W], padded=[HP, WP], beams=BEAMS, bins=BINS, calls=args.calls, library=_abi.LOADED, kernel=krows,
                          host=host, session=srows)))
    lines = [f"codd_range_scan at {W}x{H} in {WP}x{HP}, {BEAMS} beams x {BINS} bins, HIP events over {args.calls} calls after 20 "
             f"warm-ups, graph replay repeated five times (median [min .. max]); library {os.path.relpath(_abi.LOADED, ROOT)}", "",
             "| input | scan_count (hit, clear, unknown, obstacle pixels) | shipped, 3 launches: us / call eager | graph replay | "
             "one atomic per lane: eager | graph replay | same bytes | codd_objects on the frame, 7 launches: graph replay |",
             "|---|---|---|---|---|---|---|---|"]
    fmt = lambda r: f"{r['graph_us']:.2f} [{r['graph_min']:.2f} .. {r['graph_max']:.2f}]"  # noqa: E731
    lines += [f"| {r['scene']} | {r['count']} | {r['shipped']['eager_us']:.2f} | {fmt(r['shipped'])} | {r['per_lane']['eager_us']:.2f} | "
              f"{fmt(r['per_lane'])} | {r['same_bytes']} | {fmt(r['objects'])} |" for r in krows]
    if host:
        total = sum(host.values())
        lines += ["", f"the host route it replaces, the first input, medians over {args.host_runs} runs: download of the disparity "
                  f"and the labels {host['download']:.3f} ms, projection, arctan2 and binning (numpy) {host['project']:.3f} ms, "
                  f"np.add.at and np.minimum.at ({hits} hit beams) {host['tables']:.3f} ms: {total:.3f} ms per frame against "
                  f"{krows[0]['shipped']['graph_us'] / 1e3:.3f} ms"]
    if srows:
        lines += ["", "LiveSession.step, one process, sessions alternated in rounds", "",
                  "| session | rounds x frames | frames/s median | min | max | ms / frame |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['variant']} | {r['rounds']} x {r['per_round']} | {r['fps_median']:.2f} | {r['fps_min']:.2f} | {r['fps_max']:.2f} | "
                  f"{1e3 / r['fps_median']:.3f} |" for r in srows]
        g, o = srows[0]["fps_median"], srows[1]["fps_median"]
        lines += ["", f"cost of the scan output per synchronous frame: {1e3 / o - 1e3 / g:.3f} ms of {1e3 / o:.3f} ms "
                  f"({100 * (1 - o / g):.2f} %)"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
