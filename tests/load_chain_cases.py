"""The launches whose output bits tests/golden/load_chain_bits.json records (sha256 of the output bytes), shared by the
generator tools/parent_bits.py --cases load_chain, by tests/test_gpu_load_chain_bits.py and by tests/test_load_chain_cases.py.  They cover
the five kernels of motion.hip whose loads were re-ordered (instnorm_stats / instnorm_apply / instnorm_apply_xs,
se3_gn_solve, splat_gather); the recorded bits are those of the library BEFORE the re-ordering: no floating-point operation,
operand or order changed, so every output byte stays.

* ``inorm/<B>x<C>x<H>x<W>[/<plant>]/plain/relu<r>res<s>``: ops.instnorm, plain form -> y.
  ``inorm/.../xs/relu<r>res<s>relu2<t>fp32<f>``: the record-writing form -> y (when fp32) and the WHOLE record buffer.
  Shapes (STATS_DEPTH = 8 loads in flight per thread of the statistics pass; trips = loads of thread 0 of a part):
    1 x 8 x 1 x 1       HW = 1, parts = 1, trips 1
    2 x 128 x 24 x 40   C = 128 at B = 2, parts = 1
    2 x 64 x 37 x 61    HW % 4 != 0 (the scalar apply path), parts = 3
    1 x 8 x 226 x 238   parts = 32, trips 7 = D - 1, the last part shorter than the others
    1 x 8 x 240 x 256   trips 8 = D
    1 x 8 x 256 x 272   trips 9 = D + 1
    1 x 8 x 288 x 480   trips 17 = 2 D + 1 (the product's largest plane at an eighth of its channels)
  and 1 x 16 x 40 x 52 with a NaN planted in one plane / with one constant plane.
* ``gn/<h>x<w>r<radius>[q<q4>]/B<B>/builder<n>/steps<k>``: T after k = 1 and 3 calls of ops.se3_gn_step.
    16 x 24 r 4: G = 1 in every tile; 37 x 61 r 8: partial tiles; 72 x 80 r 32: an unclipped tile (G = 27) beside clipped
    ones; 24 x 40 r 8 with gn_q4 = 16: G reaches 36 (more than two batches of the solve).
* ``splat/<geometry>/flow<f>A<CA>B<CB>bf<0|1>``: ops.splat -> out and z, on the 2 x (8 * 37) x (8 * 61) sources of
  motion_fp64.geometry_case: ds 1 radius 2, ds 4 radius 4, ds 4 radius 8 (far more than 8 candidates per pixel) and ds 4
  radius 4 under a sideways translation that leaves a band of pixels without a candidate.  featA[:, 0, 0, 0] is NaN: slot
  values of empty slots are read from pixel 0 and must not reach the sum."""
import functools

import numpy as np
import torch

import motion_fp64 as M
from parent_bits import DEV, digest

NAME = "load_chain"
SOURCES = ("codd_amd/csrc/motion.hip",)
STATS_DEPTH = 8  # IN_STATS_DEPTH of motion.hip
SOLVE_BATCH = 16  # GN_SOLVE_BATCH of motion.hip


# ------------------------------------------------------------------------------------------------ instance norm
INORM_SHAPES = ((1, 8, 1, 1), (2, 128, 24, 40), (2, 64, 37, 61), (1, 8, 226, 238), (1, 8, 240, 256), (1, 8, 256, 272),
                (1, 8, 288, 480))
INORM_PLANTED = ((1, 16, 40, 52, "nan"), (1, 16, 40, 52, "const"))
INORM_PLAIN = tuple((r, s) for r in (1, 0) for s in (1, 0))                      # (relu, res)
INORM_XS = tuple((r, s, t, f) for r in (1, 0) for (s, t) in ((0, 0), (1, 0), (1, 1)) for f in (1, 0))  # (relu, res, relu2, fp32)


def inorm_parts(B, C, HW):
    """parts of codd_instnorm / codd_instnorm_xs, and the loads of thread 0 of a full part and the size of the last part."""
    cdiv = lambda a, b: -(-a // b)
    parts = min(max(cdiv(2048, B * C), 1), 32)
    parts = min(parts, cdiv(HW, 1024))
    per = cdiv(HW, parts)
    return parts, cdiv(per, 256), HW - (parts - 1) * per, per


def inorm_id(shape):
    return "x".join(str(v) for v in shape[:4]) + ("/" + shape[4] if len(shape) > 4 else "")


def inorm_keys(shape):
    s = "inorm/" + inorm_id(shape)
    return (["%s/plain/relu%dres%d" % ((s,) + v) for v in INORM_PLAIN] +
            ["%s/xs/relu%dres%drelu2%dfp32%d" % ((s,) + v) for v in INORM_XS])


@functools.lru_cache(maxsize=2)
def inorm_inputs(shape):
    """(x, res): planes of mean up to +-30 and std 0.1 .. 3; ``nan``: one NaN in plane 5; ``const``: plane 3 constant."""
    B, C, H, W = shape[:4]
    g = torch.Generator().manual_seed(101 + 7 * B + 11 * C + 13 * H + 17 * W)
    x = torch.randn(B, C, H, W, generator=g) * (0.1 + 2.9 * torch.rand(B, C, 1, 1, generator=g)) + 60.0 * (torch.rand(B, C, 1, 1, generator=g) - 0.5)
    res = torch.randn(B, C, H, W, generator=g)
    if len(shape) > 4:
        if shape[4] == "nan":
            x[B - 1, 5, H // 2, W // 3] = float("nan")
        else:
            x[B - 1, 3] = 2.5
    return x, res


def inorm_digests(shape):
    from codd_amd import ops
    B, C, H, W = shape[:4]
    x, res = inorm_inputs(shape)
    xd, rd = x.to(DEV), res.to(DEV)
    keys, out = inorm_keys(shape), {}
    for key, (relu, s) in zip(keys, INORM_PLAIN):
        out[key] = digest(ops.instnorm(xd, relu=bool(relu), res=rd if s else None).cpu())
    prev = ops.set_conv_precision("split")
    try:
        xs = ops.split_buffer(("load_chain", "inorm"), B, C, H, W, 1, DEV)
        for key, (relu, s, relu2, f) in zip(keys[len(INORM_PLAIN):], INORM_XS):
            xs.buf.zero_()
            y = ops.instnorm(xd, relu=bool(relu), res=rd if s else None, res_relu=bool(relu2), xs_out=xs, want_fp32=bool(f))
            assert (y is not None) == bool(f)
            out[key] = digest(*([y.cpu()] if f else []), xs.buf.cpu())
    finally:
        ops.set_conv_precision(prev)
    return out


# ------------------------------------------------------------------------------------------------ Gauss-Newton step
GN_CASES = ((16, 24, 4, 0), (37, 61, 8, 0), (72, 80, 32, 0), (24, 40, 8, 16))  # (h, w, radius, gn_q4 or 0 = the default)
GN_BATCHES = (1, 2)
GN_BUILDERS = (5, 3)
GN_STEPS = (1, 3)


def gn_id(case):
    h, w, radius, q4 = case
    return "%dx%dr%d%s" % (h, w, radius, "q%d" % q4 if q4 else "")


def gn_keys(case):
    return ["gn/%s/B%d/builder%d/steps%d" % (gn_id(case), B, n, k) for B in GN_BATCHES for n in GN_BUILDERS for k in GN_STEPS]


def gn_groups(case):
    """G of every 8 x 8 tile (motion.hip gn_span / gn_groups restated)."""
    h, w, radius, q4 = case
    q4 = max(q4 or 192, 16)
    span = lambda t0, size: min(t0 + 7 + radius, size - 1) - max(t0 - radius, 0) + 1
    full = 8 + 2 * radius
    gmax = max((full * full + q4 // 2) // q4, 1)
    return [min(max((span(ty, h) * span(tx, w) + q4 // 2) // q4, 1), gmax) for ty in range(0, h, 8) for tx in range(0, w, 8)], gmax


def gn_inputs(case, B):
    h, w, radius, _ = case
    g = torch.Generator().manual_seed(5 + 3 * h + 7 * w + B)
    T = torch.zeros(B, h, w, 7)
    T[..., 6] = 1
    T[..., :3] = torch.randn(B, h, w, 3, generator=g) * 0.02
    d1 = torch.rand(B, h, w, generator=g) * 30 + 3
    ae = torch.randn(B, 32, h, w, generator=g) * 3
    xyz = torch.rand(B, h, w, 3, generator=g) * 40
    delta = torch.randn(B, 3, h, w, generator=g) * 0.2
    wgt = torch.sigmoid(torch.randn(B, 3, h, w, generator=g))
    return T, (ae, xyz, delta, wgt, d1), [40.0, 42.0, w / 2.0, h / 2.0]


def gn_digests(case):
    from codd_amd import _abi, ops
    h, w, radius, q4 = case
    out = {}
    prev_q4 = _abi.set_option("gn_q4", q4) if q4 else None  # (before the scratch is sized)
    try:
        for B in GN_BATCHES:
            T0, args, K8 = gn_inputs(case, B)
            args = [a.to(DEV) for a in args]
            for builder in GN_BUILDERS:
                _abi.set_option("gn_builder", builder)
                T = T0.to(DEV).clone()
                for k in range(1, max(GN_STEPS) + 1):
                    ops.se3_gn_step(T, *args, K8, radius=radius)
                    if k in GN_STEPS:
                        out["gn/%s/B%d/builder%d/steps%d" % (gn_id(case), B, builder, k)] = digest(T.cpu())
    finally:
        _abi.set_option("gn_builder", 5)
        if q4:
            _abi.set_option("gn_q4", prev_q4)
    return {k: out[k] for k in gn_keys(case)}


# ------------------------------------------------------------------------------------------------ splat
SPLAT_GEOMETRIES = {"ds1r2": (1, 2.0, 0.0), "ds4r4": (4, 4.0, 0.0), "ds4r8": (4, 8.0, 0.0), "ds4r4shift": (4, 4.0, 6.0)}  # ds, radius, t.x
# (flow, CA, CB, bf > 0); without flow and without features there is no output tensor and codd_splat rejects the call
SPLAT_VARIANTS = tuple((f, ca, cb, bf) for f in (1, 0) for (ca, cb) in ((0, 0), (1, 0), (3, 2), (9, 0)) for bf in (0, 1)
                       if f or ca or cb)


def splat_keys(name):
    return ["splat/%s/flow%dA%dB%dbf%d" % ((name,) + v) for v in SPLAT_VARIANTS]


@functools.lru_cache(maxsize=None)
def splat_inputs(name):
    """dict(T, depth [B,HT,WT], H, W, o, ds, K, radius, feat [B,11,H,W]) of a geometry."""
    ds, radius, shift = SPLAT_GEOMETRIES[name]
    c = M.geometry_case(2, 37, 61, scale=8, tag=8)
    T, depth = c["T"].clone(), c["d1"].clone()
    T[..., 0] += shift
    B, HT, WT = depth.shape
    H, W = HT // ds, WT // ds
    g = torch.Generator().manual_seed(40 + ds)
    feat = torch.randn(B, 11, H, W, generator=g)
    feat[:, 0, 0, 0] = float("nan")
    return dict(T=T, depth=depth, H=H, W=W, o=ds // 2 - 1 if ds > 1 else 0, ds=ds, K=[v / ds for v in c["K"]], radius=radius, feat=feat)


@functools.lru_cache(maxsize=None)
def splat_candidate_counts(name):
    """Candidates per output pixel [B,H,W], restated in numpy (fp64): project every sampled source point, count it on the
    pixel centres strictly inside its disc of R = radius * min(H, W) / (2 H) pixels."""
    c = splat_inputs(name)
    H, W, o, ds = c["H"], c["W"], c["o"], c["ds"]
    fx, fy, cx, cy = c["K"]
    T = c["T"][:, o::ds, o::ds][:, :H, :W].double().numpy()
    d = c["depth"][:, o::ds, o::ds][:, :H, :W].double().numpy()
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X0 = np.stack([d * ((xs - cx) / fx), d * ((ys - cy) / fy), d], -1)
    t, qv, qw = T[..., :3], T[..., 3:6], T[..., 6:7]
    c1 = np.cross(qv, X0)
    X1 = X0 + 2.0 * (qw * c1 + np.cross(qv, c1)) + t
    z = X1[..., 2]
    with np.errstate(all="ignore"):
        u, v = fx * X1[..., 0] / z + cx, fy * X1[..., 1] / z + cy
    ok = (z > 0) & (np.abs(u) < 1e7) & (np.abs(v) < 1e7)
    R = c["radius"] * min(H, W) / (2.0 * H)
    span = int(R + 1.5)
    cnt = np.zeros(T.shape[:3], dtype=np.int64)
    bi = np.broadcast_to(np.arange(T.shape[0])[:, None, None], ok.shape)[ok]
    u, v = u[ok], v[ok]
    bx, by = np.floor(u - 0.5).astype(np.int64), np.floor(v - 0.5).astype(np.int64)
    for oy in range(-span + 1, span + 1):
        for ox in range(-span + 1, span + 1):
            xx, yy = bx + ox, by + oy
            du, dv = u - (xx + 0.5), v - (yy + 0.5)
            hit = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (du * du + dv * dv < R * R)
            np.add.at(cnt, (bi[hit], yy[hit], xx[hit]), 1)
    return cnt


@functools.lru_cache(maxsize=None)
def splat_candidate_classes():
    """{geometry: (pixels with 0, 1 .. 7, 8, more than 8 candidates)}; asserts that the set holds what the gather pass
    branches on: empty pixels (a whole band of them under the translation), partly filled slot lists, and lists longer than
    one batch of 8."""
    out = {}
    for n in SPLAT_GEOMETRIES:
        c = splat_candidate_counts(n)
        out[n] = (int((c == 0).sum()), int(((c > 0) & (c < 8)).sum()), int((c == 8).sum()), int((c > 8).sum()))
    for n in ("ds1r2", "ds4r4"):
        assert out[n][0] > 0 and out[n][1] > 0 and out[n][3] > 0, (n, out[n])
    assert out["ds4r8"][3] > out["ds4r8"][0] + out["ds4r8"][1] + out["ds4r8"][2], out["ds4r8"]
    band = (splat_candidate_counts("ds4r4shift") == 0).all(axis=1)  # whole columns without a candidate
    assert band.any(axis=1).all(), "no empty band"
    return out


def splat_digests(name):
    from codd_amd import ops
    splat_candidate_classes()
    c = splat_inputs(name)
    T, depth, feat = c["T"].to(DEV), c["depth"].to(DEV), c["feat"].to(DEV)
    out = {}
    for key, (flow, ca, cb, bf) in zip(splat_keys(name), SPLAT_VARIANTS):
        fa = feat[:, :ca].contiguous() if ca else None
        fb = feat[:, 9:9 + cb].contiguous() if cb else None
        o, z = ops.splat(T, depth, fa, fb, bool(flow), c["H"], c["W"], c["o"], c["o"], c["ds"], c["K"], c["radius"],
                         bf=M.BF if bf else 0.0)
        assert tuple(o.shape) == (2, ca + 3 * flow + cb, c["H"], c["W"])
        out[key] = digest(o.cpu(), z.cpu())
    return out


# ------------------------------------------------------------------------------------------------ all of it
def groups():
    """[(group id, keys, function -> {key: digest})] in the fixture's order."""
    return ([("inorm/" + inorm_id(s), inorm_keys(s), functools.partial(inorm_digests, s)) for s in INORM_SHAPES + INORM_PLANTED] +
            [("gn/" + gn_id(c), gn_keys(c), functools.partial(gn_digests, c)) for c in GN_CASES] +
            [("splat/" + n, splat_keys(n), functools.partial(splat_digests, n)) for n in SPLAT_GEOMETRIES])
