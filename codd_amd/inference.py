"""Command-line launcher: ``python -m codd_amd.inference <checkpoint> --img-dir L --r-img-dir R ...``

reference inference.py:12-135 (arguments, dist init, dataloader, checkpoint, DP/DDP wrap) and
datasets/custom_stereo_mf.py (folder of frames -> one multi-frame sample), configs/datasets/custom.py
(pseudo intrinsics / calib / disp range).  One process per GPU (``--launcher pytorch`` under torchrun,
RCCL); each rank takes every world_size-th video; images are decoded on the host (PIL), uploaded as
uint8 and normalised + reflect-padded on the GPU by ``codd_preprocess``.
"""
import argparse
import os
import os.path as osp
import re

import numpy as np
import torch

from . import apis, configs, ops
from .registry import build_estimator

CUSTOM = dict(intrinsics=[640, 360, 1050, 1050], calib=210, disp_range=(1, 210))  # configs/datasets/custom.py:4-7


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="CODD inference on MI355X")
    p.add_argument("checkpoint", nargs="?", default=None, help="published .pth (omit: synthetic weights)")
    p.add_argument("--iters", type=int, default=16, help="RAFT3D update iterations (configs/models/motion.py)")
    p.add_argument("--stereo-only", action="store_true")
    p.add_argument("--img-dir", help="left frames, or a directory of per-video sub-directories")
    p.add_argument("--r-img-dir", help="right frames, same layout as --img-dir")
    p.add_argument("--img-suffix", default=".png")
    p.add_argument("--num-frames", type=int, default=-1, help="frames per sample (reference caps at 50)")
    p.add_argument("--show", action="store_true", help="write <name>.disp.pred.npz per video")
    p.add_argument("--show-dir", default="./work_dirs/output")
    p.add_argument("--eval", action="store_true", help="needs --disp-dir with .npy ground truth")
    p.add_argument("--disp-dir")
    p.add_argument("--launcher", choices=["none", "pytorch"], default="none")
    p.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay of the frame")
    p.add_argument("--no-autotune", action="store_true", help="static launch heuristics (bit-reproducible runs)")
    p.add_argument("--live", action="store_true", help="feed each video frame by frame through a codd_amd.live.LiveSession "
                   "(no --num-frames cap, no whole-clip tensor: host memory does not grow with the video)")
    p.add_argument("--output", choices=["disp", "depth", "disp_u16"], default="disp", help="--live: what is written")
    p.add_argument("--motion", choices=["flow2d", "flow_dd", "sceneflow"], default=None,
                   help="--live: also write <name>.motion.pred.npz, key motion, [1, frames, h, w, C] fp32: the per-pixel motion "
                   "from the previous frame to this one on the previous frame's grid (flow2d: pixels; flow_dd: + disparity "
                   "change; sceneflow: 3-D, in the unit of calib); NaN where invalid and in frames without a field")
    p.add_argument("--ego", action="store_true",
                   help="--live: also write <name>.ego.pred.npz: pose [1, frames, 7] (t in the unit of calib, q_xyzw: the rigid "
                   "motion of static points from the previous camera frame to this one; its inverse is the camera's motion), "
                   "stats [1, frames, 4] (ok, valid pixels, inliers, inlier rms in pixels), camera_to_world [1, frames, 4, 4] "
                   "and moving [1, frames, h, w] uint8 (0 static, 1 moving, 255 invalid); a frame without a field is NaN / 255")
    p.add_argument("--confidence", action="store_true",
                   help="--live: also write <name>.conf.pred.npz: flags [1, frames, h, w] uint8 (the OR of 1 out of view, 2 "
                   "occluded in the right image, 4 photometric mismatch; 128 invalid disparity; 0: a pixel to trust) and "
                   "residual [1, frames, h, w] fp32 (grey levels; NaN where the flags are 1 or 128)")
    p.add_argument("--occ-px", type=float, default=None, help="--confidence: occlusion tolerance in pixels (default 1.0)")
    p.add_argument("--tau", type=float, default=None, help="--confidence: mismatch threshold in grey levels (default 24.0)")
    p.add_argument("--align", default=None, metavar="left|right|FILE",
                   help="--live: also write <name>.aligned.pred.npz, key depth, [1, frames, ht, wt] fp32: the depth map "
                   "(unit of calib) registered to another calibrated camera, +inf where nothing lands: `left` / `right`, the "
                   "rig's own physical cameras (need --calibration), or a .json / .npz file of a "
                   "codd_amd.calibration.AlignTarget, see INTEGRATION.md (without --calibration the session's pseudo "
                   "intrinsics have two focal lengths, which the session rejects)")
    p.add_argument("--epipolar", action="store_true",
                   help="--live: rectification health check; also write <name>.epi.pred.npz: coef [1, frames, 4] (the fitted "
                        "vertical disparity: a rotation of the right view by (-c0, c1, c2) rad and a focal error c3), stats "
                        "[1, frames, 5] (ok, measurable, inliers, rms_px, rms_fit_px), A [1, frames, 4, 4] and b [1, frames, 4] "
                        "(each frame's normal equations), combined [4] and combined_ok (live.combine_epipolar over the video)")
    p.add_argument("--ground", action="store_true",
                   help="--live: find the floor; also write <name>.ground.pred.npz: coef [1, frames, 3] (the plane d = c0 (x - "
                        "cx) + c1 (y - cy) + c2 in disparity space), ok [1, frames], normal [1, frames, 3] (from the floor to "
                        "the camera), camera_height [1, frames] (unit of calib / fx), labels [1, frames, h, w] uint8 (0 floor, 1 "
                        "obstacle, 2 overhead, 3 below, 255 invalid) and, with --ground-grid, grid_count [1, frames, 2, GH, GW] "
                        "(floor and obstacle pixels per cell) and grid_height [1, frames, GH, GW]")
    p.add_argument("--ground-height", type=float, default=None,
                   help="--ground: the camera's mounting height above the floor (unit of calib / fx): seeds the fit")
    p.add_argument("--ground-grid", default=None, metavar="GHxGW",
                   help="--ground: also a top-down grid of GH rows (forward) x GW columns (right) on the floor")
    p.add_argument("--ground-cell", type=float, default=None, help="--ground-grid: the side of a cell (default 0.1)")
    p.add_argument("--objects", action="store_true",
                   help="--ground: the obstacles as objects (connected components of the obstacle pixels); also write "
                        "<name>.objects.pred.npz: n and found [1, frames] and, padded with zeros to MAX = the session's "
                        "max_objects, pixels [1, frames, MAX], box [1, frames, MAX, 4] (x0, y0, x1, y1), near_px [1, frames, MAX, 2], "
                        "key [1, frames, MAX], extent [1, frames, MAX, 4] (gx_min, gx_max, gz_min, gz_max), height and "
                        "disparity [1, frames, MAX, 2] (min, max); with --show also ids [1, frames, h, w] uint16 (the object "
                        "number of every pixel, 65535 for none)")
    p.add_argument("--tracks", action="store_true",
                   help="--objects, with a model that has a motion stage: persistent track ids and the motion of every "
                        "object; also write <name>.tracks.pred.npz: n, continued, started and ended [1, frames] and, padded "
                        "with zeros to MAX = the session's max_objects, track, age, prev, votes, pixels, moving and "
                        "own_pixels [1, frames, MAX] and motion and own [1, frames, MAX, 3] (row k belongs to object k of "
                        "<name>.objects.pred.npz; NaN: a started track, own also without --ego)")
    p.add_argument("--scan", action="store_true",
                   help="--ground: a planar range scan over the camera's horizontal field (how far to the first obstacle in "
                        "every direction); also write <name>.scan.pred.npz: ranges and free fp32 and object int32 [1, frames, "
                        "beams] (range +inf: clear as far as the floor was seen, NaN: unknown; object -1: none, or no "
                        "--objects), hits, clear, unknown and obstacle_pixels [1, frames], angle_min, angle_increment "
                        "(radians), range_min and range_max")
    p.add_argument("--localmap", action="store_true",
                   help="--ground --ego: a rolling occupancy map around the camera, kept across the frames; also write "
                        "<name>.localmap.pred.npz: logodds int16 and age uint8 [1, frames, gh, gw] (age 255: never seen), pose "
                        "float64 [1, frames, 4] (x, z and the unit heading in the map), origin int64 [1, frames, 2] (the world "
                        "cell of [0,0]), integrated, linked, restarts, occupied, free and unknown int32 [1, frames], cell, "
                        "occ_level and free_level")
    p.add_argument("--costmap", action="store_true",
                   help="--localmap: clearance, inflated cost, reachable cells and frontiers of every frame's local map; also "
                        "write <name>.costmap.pred.npz: cost and reach uint8 and dist2 int32 [1, frames, gh, gw] (cost as ROS "
                        "costmap_2d: 254 lethal, 253 inscribed, 255 no information; dist2 2^31 - 1: far; reach 1: reachable, 2: "
                        "a frontier), occupied, inscribed, unknown, reachable, frontiers, start_ok, start_dist2 and frontier_dist2 "
                        "int32 [1, frames], frontier_cell int32 [1, frames, 2] (j, i; -1: none), start (i, j), cell, robot_radius "
                        "and inflation_radius")
    p.add_argument("--plan", action="store_true",
                   help="--costmap: the navigation function and the path to the goal on every frame's cost map; also write "
                        "<name>.plan.pred.npz: potential uint32 [1, frames, gh, gw] (0xffffffff: no path), path int32 [1, frames, "
                        "max_path, 2] (j, i; -1 behind the last cell), found, cost, length_cells, truncated, clamped, snapped, "
                        "reached and max_cost_on_path int32 [1, frames], goal_cell and end_cell int32 [1, frames, 2] (j, i; -1: none), "
                        "length float64 [1, frames], start (i, j) and cell")
    p.add_argument("--plan-goal", default="frontier", metavar="frontier|X,Z",
                   help="--plan: the nearest frontier (default) or a point X,Z of the map frame")
    p.add_argument("--heightmap", action="store_true",
                   help="--localmap: a rolling elevation layer on the local map's cells, kept across the frames; also write "
                        "<name>.heightmap.pred.npz: top, bot and ceil int16 [1, frames, gh, gw] in units of h_res above the "
                        "floor (-32768: no surface, 32767: no overhead), age uint8 (255: never seen), step uint16 and flags "
                        "uint8 [1, frames, gh, gw] (1 step, 2 headroom, 4 hole; 255: unknown), integrated, surface_pixels, "
                        "overhead_pixels, observed, known, steps, headroom and holes int32 [1, frames], origin int64 [1, frames, "
                        "2], cell and h_res")
    p.add_argument("--align-footprint", type=int, default=None, choices=[1, 2, 3, 4],
                   help="--align: target pixels per source pixel and axis (default: the smallest that leaves no hole lines)")
    p.add_argument("--rectify-maps", help="--live: .npz with left_x, left_y, right_x, right_y (fp32 [h,w]) applied on the GPU")
    p.add_argument("--calibration", help="--live: .json / .npz stereo calibration (or rectification) of the rig, see "
                   "INTEGRATION.md; the frames are rectified from it on the GPU, and intrinsics and calib are those of the "
                   "rectified camera.  Exclusive with --rectify-maps")
    p.add_argument("--zoom", type=float, default=None, help="--calibration: scale of the rectified focal length (default 1.0)")
    p.add_argument("--net-size", default=None, metavar="HxW", help="--calibration: height x width of the rectified image "
                   "the network sees (default: the size of the source frames)")
    p.add_argument("--pixel-format", choices=list(ops.FRAME_FORMATS), default=None,
                   help="--live: the frame files are raw byte dumps in this camera format (what `v4l2-ctl --stream-to` "
                   "writes, one frame per file, selected by --img-suffix), decoded on the GPU; needs --frame-size")
    p.add_argument("--frame-size", default=None, metavar="HxW", help="--pixel-format: height x width of a frame in pixels")
    p.add_argument("--pitch", type=int, default=None, help="--pixel-format: bytes per source row (default: tight)")
    p.add_argument("--yuv", choices=list(ops.YUV_MATRICES), default=None,
                   help="--pixel-format yuyv / uyvy / nv12: the YUV -> RGB matrix (default bt601; bt709 for HD video range, "
                   "jpeg for full range)")
    args = p.parse_args(argv)
    if args.pixel_format is not None:
        if not args.live:
            p.error("--pixel-format needs --live")
        m = re.fullmatch(r"(\d+)x(\d+)", args.frame_size or "")
        if not m:
            p.error("--pixel-format needs --frame-size HxW")
        args.frame_size = (int(m.group(1)), int(m.group(2)))
    elif args.frame_size is not None or args.pitch is not None or args.yuv is not None:
        p.error("--frame-size / --pitch / --yuv need --pixel-format")
    if args.calibration is not None:
        if not args.live:
            p.error("--calibration needs --live")
        if args.rectify_maps:
            p.error("--calibration and --rectify-maps exclude each other")
        if args.net_size is not None:
            m = re.fullmatch(r"(\d+)x(\d+)", args.net_size)
            if not m:
                p.error("--net-size: HxW expected")
            args.net_size = (int(m.group(1)), int(m.group(2)))
    elif args.zoom is not None or args.net_size is not None:
        p.error("--zoom / --net-size need --calibration")
    if args.motion is not None and not args.live:
        p.error("--motion needs --live")
    if args.ego and not args.live:
        p.error("--ego needs --live")
    if args.confidence and not args.live:
        p.error("--confidence needs --live")
    if (args.occ_px is not None or args.tau is not None) and not args.confidence:
        p.error("--occ-px / --tau need --confidence")
    if args.epipolar and not args.live:
        p.error("--epipolar needs --live")
    if args.ground and not args.live:
        p.error("--ground needs --live")
    if (args.ground_height is not None or args.ground_grid is not None) and not args.ground:
        p.error("--ground-height / --ground-grid need --ground")
    if args.objects and not args.ground:
        p.error("--objects needs --ground")
    if args.tracks and not args.objects:
        p.error("--tracks needs --objects")
    if args.scan and not args.ground:
        p.error("--scan needs --ground")
    if args.localmap and not (args.ground and args.ego):
        p.error("--localmap needs --ground and --ego")
    if args.costmap and not args.localmap:
        p.error("--costmap needs --localmap")
    if args.plan and not args.costmap:
        p.error("--plan needs --costmap")
    if args.heightmap and not args.localmap:
        p.error("--heightmap needs --localmap")
    if args.plan_goal != "frontier":
        m = re.fullmatch(r"([^,]+),([^,]+)", args.plan_goal)
        try:
            args.plan_goal = (float(m.group(1)), float(m.group(2)))
            if not all(np.isfinite(args.plan_goal)):
                raise ValueError
        except (AttributeError, ValueError):
            p.error("--plan-goal: frontier or X,Z expected")
    if args.ground_grid is not None:
        m = re.fullmatch(r"(\d+)x(\d+)", args.ground_grid)
        if not m or not int(m.group(1)) or not int(m.group(2)):
            p.error("--ground-grid: GHxGW expected")
        args.ground_grid = (int(m.group(1)), int(m.group(2)))
    elif args.ground_cell is not None:
        p.error("--ground-cell needs --ground-grid")
    if args.align is not None:
        if not args.live:
            p.error("--align needs --live")
        if args.align in ("left", "right") and args.calibration is None:
            p.error(f"--align {args.align} names a camera of the rig: it needs --calibration")
    elif args.align_footprint is not None:
        p.error("--align-footprint needs --align")
    return args


def _natural(names):
    return sorted(names, key=lambda s: [int(c) if c.isdigit() else c.lower() for c in re.split("([0-9]+)", s)])


def list_videos(img_dir, r_img_dir, suffix):
    """[(name, [left paths], [right paths])]: sub-directories are videos, else the directory is one."""
    subs = _natural([d for d in os.listdir(img_dir) if osp.isdir(osp.join(img_dir, d))])
    out = []
    for name, ld, rd in ([(s, osp.join(img_dir, s), osp.join(r_img_dir, s)) for s in subs] or
                         [(osp.basename(osp.normpath(img_dir)), img_dir, r_img_dir)]):
        lf = _natural([f for f in os.listdir(ld) if f.endswith(suffix)])
        rf = _natural([f for f in os.listdir(rd) if f.endswith(suffix)])
        assert len(lf) == len(rf) and lf, "left / right frame lists differ in %s" % name
        out.append((name, [osp.join(ld, f) for f in lf], [osp.join(rd, f) for f in rf]))
    return out


def _load_rgb(path, device):
    from PIL import Image
    arr = np.array(Image.open(path).convert("RGB"))
    return ops.preprocess(torch.from_numpy(np.ascontiguousarray(arr)).to(device), bgr=False)


def make_sample(name, lefts, rights, device, num_frames=-1, disp_paths=None):
    """One data dict in the layout the estimator's forward_test expects (datasets/formating.py:65-85)."""
    if num_frames > 0:
        lefts, rights = lefts[:num_frames], rights[:num_frames]
    img = torch.stack([_load_rgb(p, device)[0] for p in lefts])[None]
    r_img = torch.stack([_load_rgb(p, device)[0] for p in rights])[None]
    from PIL import Image
    w, h = Image.open(lefts[0]).size
    H, W = img.shape[-2:]
    meta = dict(filename=lefts[0], ori_filename=name + ".png", ori_shape=(h, w, 3), img_shape=(h, w, 3),
                pad_shape=(H, W, 3), **CUSTOM)
    data = dict(img=[img], r_img=[r_img], img_metas=[[meta]])
    if disp_paths:
        gt = torch.zeros(1, len(lefts), 1, H, W, device=device)
        for i, p in enumerate(disp_paths[:len(lefts)]):
            gt[0, i, 0, :h, :w] = torch.from_numpy(np.load(p).astype(np.float32)).to(device)
        data["gt_disp"] = [gt]
    return data


def iter_frames(lefts, rights):
    """(left, right) uint8 RGB [h,w,3] pairs in the order given, each decoded only when asked for."""
    from PIL import Image
    for lp, rp in zip(lefts, rights):
        yield tuple(np.ascontiguousarray(np.array(Image.open(p).convert("RGB"))) for p in (lp, rp))


def iter_raw_frames(lefts, rights, fmt, shape, pitch=None):
    """(left, right) uint8 [rows, pitch] pairs of raw ``fmt`` frames (live.frame_layout), each file read only when asked
    for; a file that is not exactly one frame long is a ValueError."""
    from .live import frame_layout
    rows, _, p, nbytes = frame_layout(fmt, shape[0], shape[1], pitch)
    for lp, rp in zip(lefts, rights):
        pair = []
        for path in (lp, rp):
            a = np.fromfile(path, dtype=np.uint8)
            if a.size != nbytes:
                raise ValueError(f"{path}: {a.size} bytes, expected one {fmt} frame of {shape[0]}x{shape[1]} "
                                 f"(pitch {p}) = {nbytes} bytes")
            pair.append(a.reshape(rows, p))
        yield tuple(pair)


def live_results(session, frames, depth=2):
    """Push ``frames`` through ``session`` keeping at most ``depth`` of them in flight; yields the results in order."""
    frames = iter(frames)
    while True:
        if session.pending() >= depth:  # (before the next frame is decoded: never more than ``depth`` frames alive)
            yield session.pop()
        pair = next(frames, None)
        if pair is None:
            break
        session.push(*pair)
    while session.pending():
        yield session.pop()


class _NpzStream:
    """Writes ``<key>.npy`` of a known shape into a compressed .npz one frame at a time (what np.savez_compressed
    writes, without holding the whole array)."""

    def __init__(self, path, key, shape, dtype):
        import zipfile
        self.spooled = None
        self.zip = zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, allowZip64=True)
        self.f = self.zip.open(key + ".npy", "w", force_zip64=True)
        np.lib.format.write_array_header_1_0(self.f, dict(descr=np.lib.format.dtype_to_descr(np.dtype(dtype)),
                                                          fortran_order=False, shape=tuple(shape)))

    def write(self, a):
        self.f.write(np.ascontiguousarray(a).tobytes())

    def spool(self, key, shape, dtype):
        """A second member that grows alongside the first (a zip archive takes one member at a time): its frames go to an
        anonymous temporary file next to the archive, which ``close`` copies into the archive in chunks; the file
        vanishes with the process if ``close`` is never reached.  Returns the object to ``write`` frames to."""
        import tempfile
        tmp = tempfile.TemporaryFile(dir=osp.dirname(osp.abspath(self.zip.filename)))
        self.spooled = (key, tuple(shape), np.dtype(dtype), tmp)
        return _Spool(tmp, dtype)

    def close(self, extra=None):
        """``extra``: {key: array} of further (small) members written whole."""
        self.f.close()
        if self.spooled:
            key, shape, dtype, tmp = self.spooled
            try:
                tmp.seek(0)
                with self.zip.open(key + ".npy", "w", force_zip64=True) as f:
                    np.lib.format.write_array_header_1_0(f, dict(descr=np.lib.format.dtype_to_descr(dtype),
                                                                 fortran_order=False, shape=shape))
                    for chunk in iter(lambda: tmp.read(1 << 22), b""):
                        f.write(chunk)
            finally:
                tmp.close()
        for key, a in (extra or {}).items():
            with self.zip.open(key + ".npy", "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(a), allow_pickle=False)
        self.zip.close()

    def abort(self):
        """Give up on a half-written archive: close what is open and remove the file, so that no truncated result is
        left where a complete one is expected."""
        try:
            self.f.close()
            if self.spooled:
                self.spooled[3].close()
            self.zip.close()
        finally:
            if osp.exists(self.zip.filename):
                os.remove(self.zip.filename)


class _Spool:
    def __init__(self, f, dtype):
        self.f, self.dtype = f, np.dtype(dtype)

    def write(self, a):
        self.f.write(np.ascontiguousarray(a, dtype=self.dtype).tobytes())


def run_live(args, model, videos):
    """--live: one LiveSession per frame size, every video pushed through it frame by frame; with --show each video's
    results go to <show-dir>/<name>.disp.pred.npz ([1, frames, h, w], as the default path writes) and, with --motion,
    <name>.motion.pred.npz ([1, frames, h, w, C]; a frame without a field is all NaN) and, with --ego,
    <name>.ego.pred.npz (pose, stats, camera_to_world, moving; a frame without a field is NaN, 255 in moving) and, with
    --confidence, <name>.conf.pred.npz (flags and residual, [1, frames, h, w] each) and, with --align,
    <name>.aligned.pred.npz (depth, [1, frames, ht, wt] on the target camera's grid) and, with --epipolar,
    <name>.epi.pred.npz (per-frame coefficients, counts, rms and normal equations plus the combined coefficients; one line
    with the rms vertical disparity and the combined rotation is printed with or without --show) and, with --ground,
    <name>.ground.pred.npz (per-frame plane, ok, normal, camera height and labels, and the grids with --ground-grid; one
    line with the frames in which a floor was found is printed with or without --show) and, with --objects,
    <name>.objects.pred.npz (per-frame n, found and the object tables padded to max_objects, written with or without
    --show; the id maps with --show only) and, with --tracks, <name>.tracks.pred.npz (per-frame n, continued, started, ended
    and the track tables padded to max_objects, written with or without --show) and, with --scan, <name>.scan.pred.npz
    (per-frame ranges, free ranges, objects and counts, written with or without --show) and, with --localmap,
    <name>.localmap.pred.npz (per-frame map, age plane, pose and counts, written with or without --show) and, with --costmap,
    <name>.costmap.pred.npz (per-frame cost, dist2, reach, counts and nearest frontier, likewise) and, with --plan,
    <name>.plan.pred.npz (per-frame potential, path and counts, likewise) and, with --heightmap,
    <name>.heightmap.pred.npz (per-frame elevation layers, flags and counts, likewise).  With --pixel-format the
    frame files are raw byte dumps of --frame-size in that camera format (iter_raw_frames) and are decoded on the GPU.  With
    --calibration the frames (files or --frame-size) have the calibration's source size and every result has --net-size."""
    from PIL import Image
    from .live import LiveSession, combine_epipolar
    maps = None
    if args.rectify_maps:
        z = np.load(args.rectify_maps)
        maps = ((z["left_x"], z["left_y"]), (z["right_x"], z["right_y"]))
    extra = dict(egomotion=True) if args.ego else {}
    if args.confidence:
        extra["confidence"] = {k: v for k, v in (("occ_px", args.occ_px), ("tau", args.tau)) if v is not None} or True
    align_to = getattr(args, "align", None)
    if align_to:
        extra["align_to"] = align_to
        if args.align_footprint is not None:
            extra["align"] = dict(footprint=args.align_footprint)
    if getattr(args, "epipolar", False):
        extra["epipolar"] = True
    if getattr(args, "ground", False):
        g = dict(height=args.ground_height, grid=args.ground_grid)
        if args.ground_cell is not None:
            g["cell"] = args.ground_cell
        extra["ground"] = g
    if getattr(args, "objects", False):
        extra["objects"] = dict(map=bool(args.show))
    if getattr(args, "tracks", False):
        extra["tracks"] = True
    if getattr(args, "scan", False):
        extra["scan"] = True
    if getattr(args, "localmap", False):
        extra["localmap"] = True
    if getattr(args, "costmap", False):
        extra["costmap"] = True
    if getattr(args, "plan", False):
        extra["plan"] = dict(goal=getattr(args, "plan_goal", "frontier"))
    if getattr(args, "heightmap", False):
        extra["heightmap"] = True
    raw = getattr(args, "pixel_format", None)
    if raw:
        extra.update(pixel_format=raw, pitch=args.pitch, yuv=args.yuv or "bt601")
    sessions = {}
    for name, lefts, rights in videos:
        src = h, w = args.frame_size if raw else Image.open(lefts[0]).size[::-1]
        cal = getattr(args, "calibration", None)
        if cal:
            h, w = args.net_size or src
            rig = dict(calibration=cal, zoom=1.0 if args.zoom is None else args.zoom)
        else:
            rig = dict(intrinsics=CUSTOM["intrinsics"], calib=CUSTOM["calib"], rectify=maps)
        s = sessions.get((h, w))
        if s is None:
            s = sessions[(h, w)] = LiveSession(model, (h, w), output=args.output, bgr=False, use_graph=not args.no_graph,
                                               motion=args.motion, **rig, **extra)
        if cal and s.src_shape != tuple(src):
            raise ValueError(f"{name}: frames of {src[0]}x{src[1]}, the calibration is for {s.src_shape[0]}x{s.src_shape[1]}")
        s.reset()
        out = mot = ego = cflags = cres = aligned = None
        nf = len(lefts)
        pose, stats, world = (np.full((1, nf) + t, np.nan, dt) for t, dt in (((7,), np.float32), ((4,), np.float32),
                                                                             ((4, 4), np.float64)))
        if args.show:
            os.makedirs(args.show_dir, exist_ok=True)
            out = _NpzStream(osp.join(args.show_dir, name + ".disp.pred.npz"), "disp", (1, len(lefts), h, w),
                             np.uint16 if args.output == "disp_u16" else np.float32)
            if args.motion:
                ch = ops.MOTION_CHANNELS[args.motion]
                mot = _NpzStream(osp.join(args.show_dir, name + ".motion.pred.npz"), "motion", (1, len(lefts), h, w, ch),
                                 np.float32)
            if args.ego:
                ego = _NpzStream(osp.join(args.show_dir, name + ".ego.pred.npz"), "moving", (1, nf, h, w), np.uint8)
            if args.confidence:
                cflags = _NpzStream(osp.join(args.show_dir, name + ".conf.pred.npz"), "flags", (1, nf, h, w), np.uint8)
                cres = cflags.spool("residual", (1, nf, h, w), np.float32)
            if align_to:
                aligned = _NpzStream(osp.join(args.show_dir, name + ".aligned.pred.npz"), "depth",
                                     (1, nf) + s.align_target.camera.size, np.float32)
        n, epis, grounds, objs, trks, scans, maps, costs, plans = 0, [], [], [], [], [], [], [], []
        heights = []
        try:
            frames = iter_raw_frames(lefts, rights, raw, src, args.pitch) if raw else iter_frames(lefts, rights)
            for res in live_results(s, frames):
                n += 1
                if "heightmap" in extra:
                    res, hm = res[:-1], res[-1]  # (a LocalMap precedes it: still a tuple)
                    heights.append(hm)
                if "plan" in extra:
                    res, pl = res[:-1], res[-1]  # (a CostMap precedes it: still a tuple)
                    plans.append(pl)
                if "costmap" in extra:
                    res, cm = res[:-1], res[-1]  # (a LocalMap precedes it: still a tuple)
                    costs.append(cm)
                if "localmap" in extra:
                    res, lm = res[:-1], res[-1]  # (an Ego and a Ground precede it: still a tuple)
                    maps.append(lm)
                if "scan" in extra:
                    res, sc = res[:-1], res[-1]  # (a Ground precedes it: still a tuple)
                    scans.append(sc)
                if "tracks" in extra:
                    res, tr = res[:-1], res[-1]  # (a Ground and an Objects precede it: still a tuple)
                    trks.append(tr)
                if "objects" in extra:
                    res, ob = res[:-1], res[-1]  # (a Ground precedes it: still a tuple)
                    objs.append(ob)
                if "ground" in extra:
                    res, g = res[:-1] if (args.motion or args.ego or args.confidence or align_to
                                          or "epipolar" in extra) else res[0], res[-1]
                    grounds.append(g if args.show else g._replace(labels=None, grid_count=None, grid_height=None))
                if "epipolar" in extra:
                    res, ep = res[:-1] if (args.motion or args.ego or args.confidence or align_to) else res[0], res[-1]
                    epis.append(ep)
                if align_to:
                    res, al = res[:-1] if (args.motion or args.ego or args.confidence) else res[0], res[-1]
                    if aligned is not None:
                        aligned.write(al.depth)
                if args.confidence:
                    res, c = res[:-1] if (args.motion or args.ego) else res[0], res[-1]
                    if cflags is not None:
                        cflags.write(c.flags)
                        cres.write(c.residual)
                if args.ego:
                    res, e = res[:-1] if args.motion else res[0], res[-1]
                    if e is not None:
                        pose[0, n - 1], world[0, n - 1] = e.pose, e.camera_to_world
                        stats[0, n - 1] = (e.ok, e.valid, e.inliers, e.rms_px)
                    if ego is not None:
                        ego.write(np.full((h, w), 255, np.uint8) if e is None else e.moving)
                if args.motion:
                    res, field = res
                    if mot is not None:
                        mot.write(np.full((h, w, ch), np.nan, np.float32) if field is None else field)
                if out is not None:
                    out.write(res)
        except BaseException:  # (no truncated <name>.conf.pred.npz behind a failed run)
            if cflags is not None:
                cflags.abort()
            raise
        for stream in (out, mot, aligned):
            if stream is not None:
                stream.close()
        if ego is not None:
            ego.close(dict(pose=pose, stats=stats, camera_to_world=world))
        if cflags is not None:
            cflags.close()
        if "epipolar" in extra:
            coef, ok = combine_epipolar(epis)
            if args.show:
                np.savez(osp.join(args.show_dir, name + ".epi.pred.npz"), coef=np.array([[e.coef for e in epis]]),
                         stats=np.array([[(e.ok, e.valid, e.inliers, e.rms_px, e.rms_fit_px) for e in epis]], np.float64),
                         A=np.array([[e.A for e in epis]]), b=np.array([[e.b for e in epis]]), combined=coef,
                         combined_ok=np.array(ok))
            nv = sum(e.valid for e in epis)
            mean = float(np.sqrt(sum(e.valid * e.rms_px ** 2 for e in epis) / nv)) if nv else 0.0
            mdeg = np.degrees([-coef[0], coef[1], coef[2]]) * 1e3
            print(f"{name}: epipolar: rms vertical disparity {mean:.3f} px over {nv} pixels; combined rotation of the right "
                  f"view ({mdeg[0]:+.1f}, {mdeg[1]:+.1f}, {mdeg[2]:+.1f}) millidegrees, focal ratio {1 + coef[3]:.5f}"
                  f"{'' if ok else ' (not determined: too little texture)'}")
        if "ground" in extra:
            if args.show:
                grids = {}
                if args.ground_grid is not None:
                    grids = dict(grid_count=np.array([[g.grid_count for g in grounds]]),
                                 grid_height=np.array([[g.grid_height for g in grounds]]))
                np.savez(osp.join(args.show_dir, name + ".ground.pred.npz"), coef=np.array([[g.coef for g in grounds]]),
                         ok=np.array([[g.ok for g in grounds]]), normal=np.array([[g.normal for g in grounds]]),
                         camera_height=np.array([[g.camera_height for g in grounds]]),
                         labels=np.array([[g.labels for g in grounds]]), **grids)
            good = [g for g in grounds if g.ok]
            hs, ts = [g.camera_height for g in good], [g.tilt_deg for g in good]
            print(f"{name}: ground: floor found in {len(good)} of {len(grounds)} frames"
                  + (f"; camera height {np.mean(hs):.3f} (min {min(hs):.3f}, max {max(hs):.3f}), tilt against up "
                     f"{np.mean(ts):.1f} degrees" if good else ""))
        if "objects" in extra:
            m = s.objects["max_objects"]

            def table(field, tail, dt):
                t = np.zeros((1, len(objs), m) + tail, dt)
                for i, ob in enumerate(objs):
                    t[0, i, :ob.n] = getattr(ob, field)
                return t

            os.makedirs(args.show_dir, exist_ok=True)
            np.savez(osp.join(args.show_dir, name + ".objects.pred.npz"), n=np.array([[ob.n for ob in objs]], np.int32),
                     found=np.array([[ob.found for ob in objs]], np.int32), pixels=table("pixels", (), np.int32),
                     box=table("box", (4,), np.int32), near_px=table("near_px", (2,), np.int32), key=table("key", (), np.int32),
                     extent=table("extent", (4,), np.float32), height=table("height", (2,), np.float32),
                     disparity=table("disparity", (2,), np.float32),
                     **(dict(ids=np.array([[ob.ids for ob in objs]])) if args.show else {}))
            print(f"{name}: objects: {sum(ob.n for ob in objs)} in {len(objs)} frames"
                  + (f", most in one frame {max(ob.n for ob in objs)}" if objs else ""))
        if "tracks" in extra:
            m = s.objects["max_objects"]

            def padded(field, tail, dt):
                t = np.zeros((1, len(trks), m) + tail, dt)
                for i, tr in enumerate(trks):
                    t[0, i, :tr.n] = getattr(tr, field)
                return t

            os.makedirs(args.show_dir, exist_ok=True)
            np.savez(osp.join(args.show_dir, name + ".tracks.pred.npz"),
                     **{k: np.array([[getattr(tr, k) for tr in trks]], np.int32) for k in ("n", "continued", "started", "ended")},
                     **{k: padded(k, (), np.int32) for k in ("track", "age", "prev", "votes", "pixels", "moving", "own_pixels")},
                     motion=padded("motion", (3,), np.float32), own=padded("own", (3,), np.float32))
            print(f"{name}: tracks: {sum(tr.started for tr in trks)} started, {sum(tr.continued for tr in trks)} continued, "
                  f"{sum(tr.ended for tr in trks)} ended in {len(trks)} frames"
                  + (f", oldest {max((int(tr.age.max()) for tr in trks if tr.n), default=0)} frames" if trks else ""))
        if "scan" in extra:
            os.makedirs(args.show_dir, exist_ok=True)
            beams = s.scan["beams"]
            np.savez(osp.join(args.show_dir, name + ".scan.pred.npz"),
                     ranges=np.array([[sc.ranges for sc in scans]], np.float32).reshape(1, len(scans), beams),
                     free=np.array([[sc.free for sc in scans]], np.float32).reshape(1, len(scans), beams),
                     object=np.array([[sc.object for sc in scans]], np.int32).reshape(1, len(scans), beams),
                     **{k: np.array([[getattr(sc, k) for sc in scans]], np.int32) for k in ("hits", "clear", "unknown",
                                                                                           "obstacle_pixels")},
                     **{k: np.array(v, np.float64) for k, v in zip(("angle_min", "angle_increment", "range_min", "range_max"),
                                                                   s._scan_meta)})
            near = [float(sc.ranges[np.isfinite(sc.ranges)].min()) for sc in scans if sc.hits]
            print(f"{name}: scan: {beams} beams; {sum(sc.hits for sc in scans)} hits, {sum(sc.clear for sc in scans)} clear, "
                  f"{sum(sc.unknown for sc in scans)} unknown in {len(scans)} frames"
                  + (f", nearest hit {min(near):.3f}" if near else ""))
        if "localmap" in extra:
            os.makedirs(args.show_dir, exist_ok=True)
            np.savez(osp.join(args.show_dir, name + ".localmap.pred.npz"),
                     logodds=np.array([[lm.logodds for lm in maps]], np.int16), age=np.array([[lm.age for lm in maps]], np.uint8),
                     pose=np.array([[lm.pose[:2] + lm.pose[2] for lm in maps]], np.float64).reshape(1, len(maps), 4),
                     origin=np.array([[lm.origin for lm in maps]], np.int64).reshape(1, len(maps), 2),
                     **{k: np.array([[int(getattr(lm, k)) for lm in maps]], np.int32)
                        for k in ("integrated", "linked", "restarts", "occupied", "free", "unknown")},
                     cell=np.array(s.localmap["cell"], np.float64), occ_level=np.array(s.localmap["occ_level"], np.int32),
                     free_level=np.array(s.localmap["free_level"], np.int32))
            gh, gw = s.localmap["grid"]
            print(f"{name}: localmap: {gh} x {gw} cells; {sum(lm.integrated for lm in maps)} integrated, "
                  f"{sum(lm.linked for lm in maps)} linked in {len(maps)} frames, {maps[-1].restarts if maps else 0} restarts"
                  + (f", {maps[-1].occupied} occupied and {maps[-1].free} free cells at the end" if maps else ""))
        if "costmap" in extra:
            os.makedirs(args.show_dir, exist_ok=True)
            np.savez(osp.join(args.show_dir, name + ".costmap.pred.npz"),
                     cost=np.array([[cm.cost for cm in costs]], np.uint8), dist2=np.array([[cm.dist2 for cm in costs]], np.int32),
                     reach=np.array([[cm.reach for cm in costs]], np.uint8),
                     **{k: np.array([[int(getattr(cm, k)) for cm in costs]], np.int32)
                        for k in ("occupied", "inscribed", "unknown", "reachable", "frontiers", "start_ok", "start_dist2",
                                  "frontier_dist2")},
                     frontier_cell=np.array([[cm.frontier_cell or (-1, -1) for cm in costs]], np.int32).reshape(1, len(costs), 2),
                     start=np.array(costs[0].start if costs else (-1, -1), np.int32), cell=np.array(s.localmap["cell"], np.float64),
                     robot_radius=np.array(s.costmap["robot_radius"], np.float64),
                     inflation_radius=np.array(s.costmap["inflation_radius"], np.float64))
            near = [cm.frontier_dist2 for cm in costs if cm.frontier_cell is not None]
            print(f"{name}: costmap: start traversable in {sum(cm.start_ok for cm in costs)} of {len(costs)} frames"
                  + (f", {costs[-1].reachable} reachable cells and {costs[-1].frontiers} frontiers at the end" if costs else "")
                  + (f", nearest frontier {np.sqrt(min(near)) * s.localmap['cell']:.3f}" if near else ""))
        if "plan" in extra:
            os.makedirs(args.show_dir, exist_ok=True)
            paths = np.full((1, len(plans), s.plan["max_path"], 2), -1, np.int32)
            for k, pl in enumerate(plans):
                paths[0, k, :len(pl.path)] = pl.path
            np.savez(osp.join(args.show_dir, name + ".plan.pred.npz"),
                     potential=np.array([[pl.potential for pl in plans]], np.uint32), path=paths,
                     **{k: np.array([[int(getattr(pl, k)) for pl in plans]], np.int32)
                        for k in ("found", "cost", "length_cells", "truncated", "clamped", "snapped", "reached", "max_cost_on_path")},
                     goal_cell=np.array([[pl.goal_cell or (-1, -1) for pl in plans]], np.int32).reshape(1, len(plans), 2),
                     end_cell=np.array([[pl.end_cell or (-1, -1) for pl in plans]], np.int32).reshape(1, len(plans), 2),
                     length=np.array([[pl.length for pl in plans]], np.float64),
                     start=np.array(plans[0].start if plans else (-1, -1), np.int32), cell=np.array(s.localmap["cell"], np.float64))
            found = [pl for pl in plans if pl.found]
            print(f"{name}: plan: a path to {'the nearest frontier' if s.plan['goal'] == 'frontier' else s.plan['goal']} in "
                  f"{len(found)} of {len(plans)} frames"
                  + (f", the last {found[-1].length:.3f} long over {found[-1].length_cells} cells at cost {found[-1].cost}, at most "
                     f"cost {found[-1].max_cost_on_path} on it, {found[-1].reached} cells reached" if found else ""))
        if "heightmap" in extra:
            os.makedirs(args.show_dir, exist_ok=True)
            np.savez(osp.join(args.show_dir, name + ".heightmap.pred.npz"),
                     top=np.array([[hm.top_q for hm in heights]], np.int16), bot=np.array([[hm.bot_q for hm in heights]], np.int16),
                     ceil=np.array([[hm.ceil_q for hm in heights]], np.int16), age=np.array([[hm.age for hm in heights]], np.uint8),
                     step=np.array([[hm.step for hm in heights]], np.uint16), flags=np.array([[hm.flags for hm in heights]], np.uint8),
                     origin=np.array([[hm.origin for hm in heights]], np.int64).reshape(1, len(heights), 2),
                     **{k: np.array([[int(getattr(hm, k)) for hm in heights]], np.int32)
                        for k in ("integrated", "surface_pixels", "overhead_pixels", "observed", "known", "steps", "headroom",
                                  "holes")},
                     cell=np.array(s.localmap["cell"], np.float64), h_res=np.array(s.heightmap["h_res"], np.float64))
            print(f"{name}: heightmap: {sum(hm.integrated for hm in heights)} integrated in {len(heights)} frames"
                  + (f", {heights[-1].known} known cells at the end: {heights[-1].steps} steps, {heights[-1].headroom} without "
                     f"headroom, {heights[-1].holes} holes, top up to {heights[-1].top_max:.3f}, bot down to "
                     f"{heights[-1].bot_min:.3f}" if heights else ""))
        print(f"{name}: {n} frames")
    for s in sessions.values():
        s.close()


def main(argv=None):
    args = parse_args(argv)
    distributed = args.launcher != "none"
    if distributed:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group("nccl")  # RCCL on ROCm
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_estimator(configs.stereo_only() if args.stereo_only else configs.codd(iters=args.iters))
    if args.checkpoint:
        apis.load_checkpoint(model, args.checkpoint, map_location="cpu")
    else:
        from . import synth
        print("no checkpoint given: synthetic weights (outputs are meaningless, timing is not)")
        synth.load_synthetic_weights(model, gain=1.4)
    model = model.to(device).eval()
    model.use_graph = not args.no_graph  # steady-state frames by hipGraph replay (estimator.inference / FrameRunner)
    ops.enable_autotune(not args.no_autotune)  # time the conv launch configurations once per layer shape
    videos = list_videos(args.img_dir, args.r_img_dir, args.img_suffix)
    mine = apis.shard_loader(videos) if distributed else videos
    if args.live:
        assert not args.eval, "--live writes results (--show); metrics need the default path"
        with torch.no_grad():
            run_live(args, model, mine)
        if distributed:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return None

    def loader():
        for name, lf, rf in mine:
            dp = None
            if args.eval:
                assert args.disp_dir, "--eval needs --disp-dir"
                dd = osp.join(args.disp_dir, name) if osp.isdir(osp.join(args.disp_dir, name)) else args.disp_dir
                dp = [osp.join(dd, f) for f in _natural([f for f in os.listdir(dd) if f.endswith(".npy")])]
            yield make_sample(name, lf, rf, device, args.num_frames, dp)

    fn = apis.multi_gpu_inference if distributed else apis.single_gpu_inference
    res = fn(model, loader(), args.show_dir, show=args.show, evaluate=args.eval)
    if distributed:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
