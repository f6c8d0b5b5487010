#!/usr/bin/env python
"""dev (GPU box): what the epilogue of the split-bf16 convolution kernel costs at the product shapes.

    python tools/convb_epilogue_share.py record /tmp/convb_launches.json
        one eager steady-state frame of the headline workload (in-tree library): the parameters of every split-bf16
        launch (codd_conv2d with layout 2), pointers kept only as identities (which fields name the same buffer)
    CODD_LIB_AB=<lib> python tools/convb_epilogue_share.py time /tmp/convb_launches.json /tmp/times_<tag>.json
        replays each distinct launch on fresh tensors of its own (weights packed for its configuration) with the library
        this process loads and times it with HIP events (us per launch, back-to-back launches)
    python tools/convb_epilogue_share.py table parent=<json> noepi=<json> [new=<json>]
        per instantiation <PGW,CGW,A,B,TERMS,OUTF,KS> and gate: us per frame of each build; the epilogue's share of the
        first build is (first - noepi) / first.  ``noepi`` is a build with CODD_EXTRA_FLAGS=-DCONVB_NO_EPILOGUE
        (conv_bf16_kernel.h): it computes nothing usable, writes one float per thread into `out` (the replay gives every
        launch an `out` large enough for that) and is only ever run by this replay, never through the network."""
import collections
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import conv_epilogue_share as S  # noqa: E402  (the exact-fp32 twin: _dump, _shape_key, VIEWS, PTRS)


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
    launches, orig = [], ops._launch_conv

    def one(lib, p, stream):
        rc = orig(lib, p, stream)
        if p.layout == 2 and rc == 0:  # (ops.conv2d retries on a private re-layout when a shared split tensor is refused)
            launches.append(S._dump(p))
        return rc

    ops._launch_conv = one
    try:
        runner.eager_frame_on_static_state(img[:, 3].contiguous(), r_img[:, 3].contiguous())
        torch.cuda.synchronize()
    finally:
        ops._launch_conv = orig
    json.dump(launches, open(path, "w"))
    print("%d split-bf16 launches of one frame -> %s" % (len(launches), path))


def _inst(d):
    """<PGW,CGW,A,B,TERMS,OUTF,KS> of a recorded launch (conv_bf16.hip: A = pixel units per wave, B = blocks per wave)."""
    pu = d["nw"] * d["npb"]
    return (d["pgw"], d["cgw"], -(-pu // d["pgw"]), d["mb"] // d["cgw"], d["terms"], 1 if (d["xso"] or d["gate"]) else 0,
            max(1, d["ksplit"]))


def _grid(d):
    cout_eff = d["Cout"] * (4 if d["store_mode"] else 1)
    return -(-d["Wout"] // (16 * d["npb"])) * -(-d["Hout"] // d["nw"]) * -(-cout_eff // (16 * d["mb"])) * d["B"]


def _build(d, torch, ops, keep):
    """ConvParams of a recorded launch on fresh tensors: one buffer per recorded pointer (a recorded alias, e.g. gate 3's
    out = post, stays one), sized for the largest use, weights packed for the recorded configuration."""
    from codd_amd._abi import ConvParams, View
    p = ConvParams()
    planes = 2 if d["terms"] in (3, 48) else 1
    hw = d["Hout"] * d["Wout"]
    need = collections.defaultdict(int)  # bytes per recorded pointer
    for name in ("res1", "res2", "post"):
        ptr, ctot, _ = d[name]
        if ptr:
            need[ptr] = max(need[ptr], 4 * d["B"] * ctot * hw)
    # `out`: the tensor itself, and room for the one float per thread the no-epilogue build writes
    need[d["out"] or -1] = max(need[d["out"] or -1], 4 * d["B"] * max(d["out_ctot"], 1) * hw * (4 if d["store_mode"] else 1),
                               4 * (_grid(d) + 4) * 256)
    need[d["xs"]] = max(need[d["xs"]], 16 * d["B"] * planes * d["xs_c8"] * d["xs_hp"] * d["xs_wp"])
    if d["xso"]:
        need[d["xso"]] = max(need[d["xso"]], 16 * d["B"] * planes * d["xso_c8"] * d["xso_hp"] * d["xso_wp"])
    bufs = {}
    for ptr, n in need.items():
        if ptr in (d["xs"], d["xso"]):  # records: small finite bf16 / fp16 values in every lane
            t = (torch.randn(n // 2, device="cuda") * 0.25).to(torch.float16 if d["terms"] in (16, 48) else torch.bfloat16)
        else:
            t = torch.rand(n // 4, device="cuda")
        bufs[ptr] = t
    for name, _ in ConvParams._fields_:
        if name in S.VIEWS:
            ptr, ctot, coff = d[name]
            setattr(p, name, View(bufs[ptr].data_ptr() if ptr and ptr in bufs else None, ctot, coff))
        elif name not in S.PTRS:
            setattr(p, name, d[name])
    p.out = bufs[d["out"] or -1].data_ptr()
    p.xs = bufs[d["xs"]].data_ptr()
    p.xso = bufs[d["xso"]].data_ptr() if d["xso"] else None
    cin, cout_eff = d["C0"] + d["C1"], d["Cout"] * (4 if d["store_mode"] else 1)
    deconv = bool(d["store_mode"])
    w = torch.randn(cin, d["Cout"], 2, 2, device="cuda") if deconv else torch.randn(cout_eff, cin, d["kh"], d["kw"], device="cuda")
    pc = ops.PackedConv(w / (cin * d["kh"] * d["kw"]) ** 0.5, torch.randn(d["Cout"], device="cuda") if d["bias"] else None, deconv=deconv)
    p.wpacked = pc.packed(d["ck"], d["mb"], 20 + d["terms"]).data_ptr()
    p.bias = pc.bias.data_ptr() if d["bias"] else None
    keep.append((bufs, pc))
    return p


def time_(src, dst, reps=200):
    import torch
    from codd_amd import _abi, ops
    lib = _abi.load()
    groups = collections.OrderedDict()
    for d in json.load(open(src)):
        groups.setdefault(S._shape_key([d]), [d, 0])[1] += 1
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for key, (d, n) in groups.items():
        keep = []
        p = _build(d, torch, ops, keep)
        _abi.check(lib.codd_conv2d_check(C.byref(p)), "replay check of %s" % (_inst(d),))
        go = lambda: lib.codd_conv2d(C.byref(p), stream)
        for _ in range(10):
            _abi.check(go(), "replay")
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            go()
        e.record()
        torch.cuda.synchronize()
        rows.append(dict(inst=list(_inst(d)), gate=d["gate"], per_frame=n, us=round(s.elapsed_time(e) / reps * 1e3, 2),
                         layer="%dx%d %d->%d @%dx%d%s%s" % (d["kh"], d["kw"], d["C0"] + d["C1"], d["Cout"], d["Hout"], d["Wout"],
                                                          " dil2" if d["dil2"] else "", "T" if d["store_mode"] else "")))
    json.dump(dict(library=os.path.relpath(_abi.LOADED, ROOT), rows=rows), open(dst, "w"), indent=0)
    print("%d distinct launches timed with %s -> %s" % (len(rows), os.path.relpath(_abi.LOADED, ROOT), dst))


def table(named):
    data = collections.OrderedDict((kv.split("=")[0], json.load(open(kv.split("=")[1]))["rows"]) for kv in named)
    tags = list(data)
    cls = collections.OrderedDict()
    for tag, rows in data.items():
        for r in rows:
            c = cls.setdefault((tuple(r["inst"]), r["gate"]), {"n": 0, "launches": 0})
            c[tag] = c.get(tag, 0.0) + r["us"] * r["per_frame"]
            if tag == tags[0]:
                c["n"] += 1; c["launches"] += r["per_frame"]
    print("us per frame, back-to-back replay of the frame's split-bf16 launches at their product shapes")
    print("%-30s %4s %6s %8s " % ("<PGW,CGW,A,B,TERMS,OUTF,KS>", "gate", "layers", "launches") + " ".join("%10s" % t for t in tags) +
          "  epilogue share of %s" % tags[0])
    tot = collections.defaultdict(float)
    for (inst, gate), c in sorted(cls.items(), key=lambda kv: -kv[1].get(tags[0], 0)):
        share = "%5.1f %%" % (100 * (c[tags[0]] - c["noepi"]) / c[tags[0]]) if "noepi" in c else ""
        print("%-30s %4d %6d %8d " % ("<%d,%d,%d,%d,%d,%d,%d>" % inst, gate, c["n"], c["launches"]) +
              " ".join("%10.1f" % c.get(t, float("nan")) for t in tags) + "  " + share)
        for t in tags:
            tot[t] += c.get(t, 0.0)
    print("%-30s %4s %6s %8s " % ("total", "", "", "") + " ".join("%10.1f" % tot[t] for t in tags) +
          ("  %5.1f %%" % (100 * (tot[tags[0]] - tot["noepi"]) / tot[tags[0]]) if "noepi" in tot else ""))


if __name__ == "__main__":
    if sys.argv[1] == "record":
        record(sys.argv[2])
    elif sys.argv[1] == "time":
        time_(sys.argv[2], sys.argv[3])
    else:
        table(sys.argv[2:])
