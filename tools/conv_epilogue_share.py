#!/usr/bin/env python
"""dev (GPU box): what the epilogue of the exact-fp32 convolution kernels costs at the product shapes.

    python tools/conv_epilogue_share.py record /tmp/fp32_launches.json
        one eager steady-state frame of the headline workload (in-tree library): the parameters of every exact-fp32
        convolution launch (codd_conv2d with layout 0 | 1, codd_conv2d_multi), without their pointers
    CODD_LIB_AB=<lib> python tools/conv_epilogue_share.py time /tmp/fp32_launches.json /tmp/times_<tag>.json
        replays each distinct launch on fresh random tensors (weights packed for its configuration) with the library
        this process loads and times it with HIP events (us per launch, back-to-back launches)
    python tools/conv_epilogue_share.py table parent=<json> noepi=<json> new=<json>
        per kernel class (kind, layout, nw, npb, mb): us per frame of each build; the epilogue's share of the first
        build is (first - noepi) / first.  ``noepi`` is a build with CODD_EXTRA_FLAGS=-DCONV_NO_EPILOGUE (conv_kernel.h):
        it computes nothing usable and is only ever run by this replay, never through the network.  With a second run of
        the first build as ``parent2`` the classes that ``new`` made slower by more than |parent - parent2| are listed.
    python tools/conv_epilogue_share.py layers parent=<json> parent2=<json> noepi=<json> new=<json>
        the same per distinct launch (us per launch), with the launches ``new`` made slower by more than the spread."""
import collections
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VIEWS = ("in0", "in1", "res1", "res2", "post")
PTRS = ("wpacked", "bias", "out", "xs", "xso")


def _dump(p):
    from codd_amd._abi import ConvParams
    d = {}
    for name, _ in ConvParams._fields_:
        v = getattr(p, name)
        if name in VIEWS:
            d[name] = [v.ptr or 0, v.ctot, v.coff]
        else:
            d[name] = v or 0
    return d


def record(path):
    import torch
    import bench
    from codd_amd import ops, synth
    from codd_amd.runtime import FrameRunner
    sys.argv = [sys.argv[0]]
    args = bench.parse()
    dev = torch.device("cuda", 0)
    ops.enable_autotune(True, shipped=True)
    ops.set_conv_precision(args.precision)
    est = bench.build_model(args, dev)
    H, W = args.height, args.width
    img, r_img, _ = synth.stereo_sequence(H, W, 6, flow=(0.75, 0.25))
    img, r_img = img.to(dev), r_img.to(dev)
    raw = (bench.RAW_H, bench.RAW_W) if (H, W) == (bench.PAD_H, bench.PAD_W) else (H, W)
    runner = FrameRunner(est, synth.default_metas(H, W, img_shape=raw + (3,))[0], use_graph=False)
    for i in range(3):
        runner.step(img[:, i].contiguous(), r_img[:, i].contiguous())
    torch.cuda.synchronize()
    launches, orig, orig_multi = [], ops._launch_conv, ops._launch_conv_multi

    def one(lib, p, stream):
        if p.layout in (0, 1):
            launches.append([_dump(p)])
        return orig(lib, p, stream)

    def multi(lib, params, n, stream):
        launches.append([_dump(params[i]) for i in range(n)])
        return orig_multi(lib, params, n, stream)

    ops._launch_conv, ops._launch_conv_multi = one, multi
    try:
        runner.eager_frame_on_static_state(img[:, 3].contiguous(), r_img[:, 3].contiguous())
        torch.cuda.synchronize()
    finally:
        ops._launch_conv, ops._launch_conv_multi = orig, orig_multi
    json.dump(launches, open(path, "w"))
    print("%d exact-fp32 launches (%d multi) of one frame -> %s" % (len(launches), sum(len(l) > 1 for l in launches), path))


def _shape_key(job):
    return json.dumps([{k: (v[1:] + [bool(v[0])] if k in VIEWS else (bool(v) if k in PTRS else v)) for k, v in d.items()} for d in job])


def _build(d, torch, ops, keep):
    """ConvParams of a recorded launch on fresh tensors: one buffer per recorded pointer (so a recorded alias, e.g.
    out = post, stays one), random values, weights packed for the recorded configuration."""
    from codd_amd._abi import ConvParams, View
    p = ConvParams()
    deconv = bool(d["store_mode"])
    cin, cout_eff = d["C0"] + d["C1"], d["Cout"] * (4 if deconv else 1)
    bufs = {}

    def buf(ptr, n):
        if ptr not in bufs or bufs[ptr].numel() < n:
            bufs[ptr] = torch.randn(n, device="cuda")
        return bufs[ptr]

    need = collections.defaultdict(int)
    for name in VIEWS:
        ptr, ctot, _ = d[name]
        hw = d["Hin"] * d["Win"] if name in ("in0", "in1") else d["Hout"] * d["Wout"]
        if ptr:
            need[ptr] = max(need[ptr], d["B"] * ctot * hw)
    need[d["out"]] = max(need[d["out"]], d["B"] * d["out_ctot"] * d["Hout"] * d["Wout"] * (4 if deconv else 1))
    for name, _ in ConvParams._fields_:
        if name in VIEWS:
            ptr, ctot, coff = d[name]
            setattr(p, name, View(buf(ptr, need[ptr]).data_ptr() if ptr else None, ctot, coff))
        elif name not in PTRS:
            setattr(p, name, d[name])
    p.out = buf(d["out"], need[d["out"]]).data_ptr()
    w = torch.randn(cin, d["Cout"], 2, 2, device="cuda") if deconv else torch.randn(cout_eff, cin, d["kh"], d["kw"], device="cuda")
    pc = ops.PackedConv(w / (cin * d["kh"] * d["kw"]) ** 0.5, torch.randn(d["Cout"], device="cuda") if d["bias"] else None, deconv=deconv)
    p.wpacked = pc.packed(d["ck"], d["mb"], d["layout"]).data_ptr()
    p.bias = pc.bias.data_ptr() if d["bias"] else None
    keep.append((bufs, pc))
    return p


def time_(src, dst, reps=200):
    import torch
    from codd_amd import _abi, ops
    from codd_amd._abi import ConvParams
    lib = _abi.load()
    launches = json.load(open(src))
    groups = collections.OrderedDict()
    for job in launches:
        groups.setdefault(_shape_key(job), [job, 0])[1] += 1
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for key, (job, n) in groups.items():
        keep = []
        ps = [_build(d, torch, ops, keep) for d in job]
        if len(ps) > 1:
            arr = (ConvParams * len(ps))(*ps)
            go = lambda: lib.codd_conv2d_multi(arr, len(ps), stream)
        else:
            go = lambda: lib.codd_conv2d(C.byref(ps[0]), stream)
        for _ in range(10):
            _abi.check(go(), "replay")
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            go()
        e.record()
        torch.cuda.synchronize()
        d = job[0]
        rows.append(dict(kind="multi%d" % len(job) if len(job) > 1 else "single", layout=d["layout"], nw=d["nw"] or 4, npb=d["npb"], mb=d["mb"],
                         ck=d["ck"], layer="%dx%d %d->%d @%dx%d s%d%s" % (d["kh"], d["kw"], d["C0"] + d["C1"], d["Cout"], d["Hout"], d["Wout"], d["sy"],
                                                                          "T" if d["store_mode"] else ""),
                         operands="".join(c for c, k in (("b", "bias"), ("1", "res1"), ("2", "res2"), ("p", "post")) if (d[k][0] if k in VIEWS else d[k])),
                         act=d["act"], per_frame=n, us=round(s.elapsed_time(e) / reps * 1e3, 2)))
    json.dump(dict(library=os.path.relpath(_abi.LOADED, ROOT), rows=rows), open(dst, "w"), indent=0)
    print("%d distinct launches timed with %s -> %s" % (len(rows), os.path.relpath(_abi.LOADED, ROOT), dst))


def table(named):
    data = collections.OrderedDict((kv.split("=")[0], json.load(open(kv.split("=")[1]))["rows"]) for kv in named)
    tags = list(data)
    cls = collections.OrderedDict()
    for tag, rows in data.items():
        for r in rows:
            c = cls.setdefault((r["kind"], r["layout"], r["nw"], r["npb"], r["mb"]), {"n": 0, "launches": 0})
            c[tag] = c.get(tag, 0.0) + r["us"] * r["per_frame"]
            if tag == tags[0]:
                c["n"] += 1; c["launches"] += r["per_frame"]
    print("us per frame, back-to-back replay of the frame's exact-fp32 launches at their product shapes")
    print("%-34s %7s %8s " % ("class (kind, layout, nw, npb, mb)", "layers", "launches") + " ".join("%10s" % t for t in tags) + "  epilogue share of %s" % tags[0])
    tot = collections.defaultdict(float)
    for k, c in sorted(cls.items(), key=lambda kv: -kv[1].get(tags[0], 0)):
        share = "%5.1f %%" % (100 * (c[tags[0]] - c["noepi"]) / c[tags[0]]) if "noepi" in c else ""
        print("%-34s %7d %8d " % ("%s l%d nw%d npb%d mb%d" % k, c["n"], c["launches"]) + " ".join("%10.1f" % c.get(t, float("nan")) for t in tags) + "  " + share)
        for t in tags:
            tot[t] += c.get(t, 0.0)
    print("%-34s %7s %8s " % ("total", "", "") + " ".join("%10.1f" % tot[t] for t in tags) +
          ("  %5.1f %%" % (100 * (tot[tags[0]] - tot["noepi"]) / tot[tags[0]]) if "noepi" in tot else ""))
    if "parent2" in tags and "new" in tags:
        slow = ["%s l%d nw%d npb%d mb%d (%+.1f us, spread %.1f)" % (k + (c["new"] - (c[tags[0]] + c["parent2"]) / 2, abs(c[tags[0]] - c["parent2"])))
                for k, c in cls.items() if c["new"] - max(c[tags[0]], c["parent2"]) > abs(c[tags[0]] - c["parent2"])]
        print("classes slower in new by more than the spread of the two parent runs: " + ("; ".join(slow) or "none"))


def layers(named):
    data = collections.OrderedDict((kv.split("=")[0], json.load(open(kv.split("=")[1]))["rows"]) for kv in named)
    tags = list(data)
    first = data[tags[0]]
    assert all(len(rows) == len(first) for rows in data.values())
    print("%-7s %-22s %-30s %-8s %3s %3s " % ("kind", "class", "layer", "operands", "act", "n") + " ".join("%8s" % t for t in tags) + "   share")
    slow = []
    for i, r in enumerate(first):
        us = {t: data[t][i]["us"] for t in tags}
        assert all(data[t][i]["layer"] == r["layer"] for t in tags)
        share = "%5.1f%%" % (100 * (us[tags[0]] - us["noepi"]) / us[tags[0]]) if "noepi" in us else ""
        print("%-7s %-22s %-30s %-8s %3d %3d " % (r["kind"], "l%d nw%d npb%d mb%d ck%d" % (r["layout"], r["nw"], r["npb"], r["mb"], r["ck"]), r["layer"],
                                                 r["operands"], r["act"], r["per_frame"]) + " ".join("%8.2f" % us[t] for t in tags) + "  " + share)
        if "parent2" in us and "new" in us and us["new"] - max(us[tags[0]], us["parent2"]) > abs(us[tags[0]] - us["parent2"]):
            slow.append("%s %s (%+.2f us)" % (r["kind"], r["layer"], us["new"] - (us[tags[0]] + us["parent2"]) / 2))
    if "parent2" in tags and "new" in tags:
        print("launches slower in new by more than the spread of the two parent runs: " + ("; ".join(slow) or "none"))


if __name__ == "__main__":
    if sys.argv[1] == "record":
        record(sys.argv[2])
    elif sys.argv[1] == "time":
        time_(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "layers":
        layers(sys.argv[2:])
    else:
        table(sys.argv[2:])
