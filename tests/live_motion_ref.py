"""fp64 restatement of codd_export_motion (include/codd_hip.h): the three motion modes, the validity rule and the depth
roll, with per-element bounds, for tests/test_live_motion.py (CPU: self-checks, and the fp32 evaluation that sets the
two constants below) and tests/test_gpu_live_motion.py (the HIP kernel and LiveSession).

Built on tests/motion_fp64.py (geometry_case, induced_flow, disp_to_depth, C, U) and oracle.se3 / oracle.motion, and
following that module's protocol: the bound of an output element is |got - ref64| <= c * 2^-24 * M with M the
first-order magnitude of the arithmetic that forms it and one scalar c per quantity:

    flow2d, flow_dd[..., :2]   M of motion_fp64.induced_flow, c = C["induced_flow"] as they stand
    flow_dd[..., 2]            M = bf * M_z + |value| (M_z: induced_flow's third magnitude; the product's own rounding)
    sceneflow                  M = |scale| * (|X0|_1 + |t|_1): X1 - X0 = (R - I) X0 + t is summed from terms of that size

c of the last two = 4 x the worst |eval32 - ref64| / (2^-24 M) of an fp32 torch-CPU evaluation (oracle.se3.act,
oracle.motion.inv_project / project on fp32 tensors) over CASES, rounded up to two digits (MEASURED holds the measured
values; test_fp32_evaluation_within_a_quarter_of_every_bound re-measures them).

Validity: a pixel is valid iff Z0 >= MIN_DEPTH and Z1 >= MIN_DEPTH; invalid pixels are NaN in every channel.  A pixel
whose fp64 Z0 or Z1 lies within UNDECIDED of MIN_DEPTH may fall either way in fp32 and is left out of every comparison;
compare() asserts that at most 0.1 % of a case's pixels are."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_fp64 as mf  # noqa: E402

from oracle import motion as om  # noqa: E402
from oracle import se3  # noqa: E402

F64 = torch.float64
MIN_DEPTH = om.MIN_DEPTH
UNDECIDED = 1e-5
DEPTH_CAP = 210.0  # the clip of codd_disp_to_depth
MODES = ("flow2d", "flow_dd", "sceneflow")
CHANNELS = dict(flow2d=2, flow_dd=3, sceneflow=3)
# ((h, w) crop, (H, W) padded): odd width, misaligned output rows, crop on both axes; a row longer than one workgroup
# run, with a tail; no crop, everything aligned
CASES = [((37, 53), (64, 64)), ((40, 301), (64, 320)), ((128, 192), (128, 192))]
SCALE = 0.37

# worst |eval32 - ref64| / (2^-24 M) of the fp32 CPU evaluation over CASES (inside the crops) ...
MEASURED = {"flow_dd_z": 1.1, "sceneflow": 2.49}
# ... and c = 4 x that, rounded up to two digits
C = {"induced_flow": mf.C["induced_flow"], "flow_dd_z": 4.4, "sceneflow": 10.0}


def bf_of(fx):
    """Motion._bf: depth_scale * fx evaluated in fp32 (reference motion.py:154-159)."""
    fx = np.float32(fx)
    return float(np.float32(np.float32(om.BF_DEFAULT) / fx) * fx)


def case(H, W):
    """geometry_case at H x W (T over all five rotation regimes, d1 = depth_prev with its planted invalid pixels) + bf."""
    g = mf.geometry_case(1, H // 8, W // 8, scale=8)
    return dict(T=g["T"], depth=g["d1"], regime=g["regime"], K=g["K"], bf=bf_of(g["K"][0]))


def disparity(H, W, seed=11):
    """A random disparity map [1,1,H,W] holding 0, a negative value, NaN and +inf (inside the smallest crop)."""
    g = torch.Generator().manual_seed(seed + 7 * H + W)
    d = torch.rand(1, 1, H, W, generator=g) * 300.0 + 0.01
    d[0, 0, 1, 2], d[0, 0, 3, 5], d[0, 0, 7, 11], d[0, 0, 13, 17] = 0.0, -0.75, float("nan"), float("inf")
    return d


def _points(T, depth, K, dtype):
    Kt = torch.tensor([list(K)] * depth.shape[0], dtype=dtype)
    X0 = om.inv_project(depth.to(dtype), Kt)
    return X0, se3.act(T.to(dtype), X0), Kt


def reference(T, depth, K, bf, scale):
    """T [1,H,W,7], depth [1,H,W] (fp32) -> dict: per mode (value [H,W,C], M [H,W,C]) in fp64, ``invalid`` [H,W] (the
    pixels that are NaN) and ``undecided`` [H,W]."""
    X0, X1, _ = _points(T, depth, K, F64)
    flow, Mf, _ = mf.induced_flow(T, depth, K)
    dd = bf * flow[..., 2:]
    sf = scale * (X1 - X0)
    Ms = abs(scale) * (X0.abs().sum(-1) + T.to(F64)[..., :3].abs().sum(-1))
    Z0, Z1 = X0[..., 2], X1[..., 2]
    return dict(flow2d=(flow[0, ..., :2], Mf[0, ..., :2]),
                flow_dd=(torch.cat([flow[..., :2], dd], -1)[0], torch.cat([Mf[..., :2], bf * Mf[..., 2:] + dd.abs()], -1)[0]),
                sceneflow=(sf[0], Ms[0, ..., None].expand(*sf.shape[1:])),
                invalid=~((Z0 >= MIN_DEPTH) & (Z1 >= MIN_DEPTH))[0],
                undecided=(((Z0 - MIN_DEPTH).abs() < UNDECIDED) | ((Z1 - MIN_DEPTH).abs() < UNDECIDED))[0])


def evaluate32(T, depth, K, bf, scale, mode):
    """The same quantities from the project's fp32 CPU oracle -> [H,W,C] fp32, NaN where invalid."""
    X0, X1, Kt = _points(T, depth, K, torch.float32)
    if mode == "sceneflow":
        v = np.float32(scale) * (X1 - X0)
    else:
        v = om.project(X1, Kt) - om.project(X0, Kt)
        v = v[..., :2] if mode == "flow2d" else torch.cat([v[..., :2], np.float32(bf) * v[..., 2:]], -1)
    valid = (X0[..., 2] >= np.float32(MIN_DEPTH)) & (X1[..., 2] >= np.float32(MIN_DEPTH))
    return torch.where(valid[..., None], v, torch.full_like(v, float("nan")))[0]


def roll(disp, bf):
    """clip(bf / (disp + 1e-5), 0, 210) in fp64; a NaN (which fmaxf(NaN, 0) turns into 0 in the kernel) gives 0."""
    v = bf / (disp.to(F64) + 1e-5)
    return torch.where(torch.isnan(v), torch.zeros_like(v), v).clamp(0.0, DEPTH_CAP)


def compare(got, ref, mode, h, w, name, regime=None):
    """got [h,w,C] against reference(...) cropped to h x w -> {key of C: worst err / (2^-24 M)} over the decided valid
    pixels.  Asserts the undecided share (<= 0.1 %) and, on every decided pixel, that NaN-ness equals the reference's."""
    val, M = (a[:h, :w] for a in ref[mode])
    invalid, undecided = ref["invalid"][:h, :w], ref["undecided"][:h, :w]
    assert tuple(got.shape) == (h, w, CHANNELS[mode]), (tuple(got.shape), mode)
    assert int(undecided.sum()) <= 1e-3 * h * w, f"{name}: {int(undecided.sum())} undecided pixels of {h * w}"
    nan = torch.isnan(got)
    decided = ~undecided
    assert torch.equal(nan.all(-1)[decided], invalid[decided]) and torch.equal(nan.any(-1)[decided], invalid[decided]), \
        f"{name} {mode}: NaN pixels differ from the reference's invalid ones"
    keep = (decided & ~invalid)[..., None]
    g = torch.where(keep, got.to(F64), val)
    r = mf.ratio(g, val, M, 1.0)
    rg = None if regime is None else regime[0, :h, :w]
    if mode == "sceneflow":
        return {"sceneflow": mf.worst(f"{name} sceneflow", r, keep, rg)[0]}
    res = {"induced_flow": mf.worst(f"{name} {mode} flow", r[..., :2], keep, rg)[0]}
    if mode == "flow_dd":
        res["flow_dd_z"] = mf.worst(f"{name} flow_dd dz", r[..., 2:], keep, rg)[0]
    return res


def within(res, frac=1.0, what=""):
    bad = {k: (v, frac * C[k]) for k, v in res.items() if not v <= frac * C[k]}
    assert not bad, (what, bad)
