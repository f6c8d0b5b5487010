"""Live stereo session: host ``uint8`` camera frames in, host depth maps out, one frame at a time.

The reference has no online entry: datasets/custom_stereo_mf.py cuts a video into multi-frame samples and
model/codd.py:290-398 walks a whole resident clip.  ``LiveSession`` owns everything between a frame in host memory
and a result the caller may keep, around the FrameRunner's captured frame graph:

    pinned host slot --(copy stream)--> device uint8 slot --codd_ingest_pair--> the graph's own static inputs
    --graph replay--> padded disparity --codd_export_depth--> device staging --(copy stream)--> pinned host slot

Ingest and export run on the compute stream, outside the graph, right before and after the replay; both copies run on
streams of their own, ordered against the compute stream with events, so the upload of frame t+1 and the download of
frame t-1 overlap the compute of frame t.  Every buffer is allocated once, at the first frame.

With ``motion=`` the session also hands out the dense SE3 motion field the network estimates on every steady-state
frame, as per-pixel optical flow, flow + disparity change, or metric 3-D scene flow: ``codd_export_motion`` runs right
after ``codd_export_depth``, reads the field where the frame graph left it, and keeps the previous frame's depth map the
field refers to in a buffer of the session's own, which it rolls forward in the same launch.

With ``egomotion=`` the session separates that field into the camera's own motion and the pixels that moved on their
own: ``codd_ego_motion`` runs between the two exports (it reads the previous depth map before ``codd_export_motion``
rolls it), fits one rigid motion to the field robustly and marks the pixels whose flow disagrees with it; the camera
trajectory is composed on the host when a result is collected.

With ``confidence=`` the session says which depth pixels to trust: ``codd_export_confidence`` runs right after
``codd_export_depth`` on the frame's disparity and on the two normalised images the frame graph read -- the buffers the
``fill`` closure below was handed for this frame, which the graph only reads -- and returns per-pixel flags (out of view,
occluded in the right image, photometric mismatch, invalid) and the photometric residual.  It needs no motion stage.

With ``pixel_format=`` the session takes frames as a camera hands them out -- mono8, YUYV / UYVY, NV12 or a Bayer mosaic,
with a row pitch -- uploads those bytes (1 to 2 per pixel instead of 3) and decodes them inside the ingest launch:
``codd_ingest_frames`` stands where ``codd_ingest_pair`` stands above and writes the bits ``codd_ingest_pair`` writes on
the decoded RGB images, so that everything behind it is unchanged.

With ``calibration=`` the session rectifies from the rig's calibration (codd_amd/calibration.py): ``shape`` is the size
of the rectified image the network sees, frames arrive at the calibration's own source size in either family of formats,
and ``codd_ingest_calibrated`` stands where the two entries above stand -- it evaluates the rectifying map in registers
(no map arrays) -- while ``intrinsics`` and ``calib`` of the rectified virtual camera come from the rectification.

With ``align_to=`` the session also hands out the depth map on the grid of another calibrated camera -- a physical camera
of the rig or a separate colour camera (``calibration.AlignTarget``): ``codd_align_depth`` runs right after
``codd_export_depth`` on the frame's disparity, forward-warps it into the target camera with a z-buffer (the nearest
surface wins) and, on request, returns where every pixel of the session's own grid lands in the target image.

With ``epipolar=`` the session checks the assumption all of the above rests on, that the calibration still describes the
rig: ``codd_epipolar_check`` runs right after ``codd_export_confidence`` on the same disparity and normalised images,
measures per pixel the row offset at which the right image really matches, and fits a small rotation of the right view
plus a focal ratio to that map; ``combine_epipolar`` pools the frames' normal equations and ``calibration.Rectification
.corrected`` applies the result.  It needs no motion stage and no ``calibration=``.

With ``ground=`` the session finds the floor: ``codd_ground_plane`` runs after the other export stages on the frame's
disparity, fits one plane robustly in disparity space and returns per pixel the height above it and a label (floor,
obstacle, overhead, below), plus, on request, a top-down grid of the floor and obstacle pixels a planner can read.  It
needs no motion stage and no ``calibration=``.

With ``objects=`` (which needs ``ground=``) the session says what the obstacles are: ``codd_objects`` runs right after
``codd_ground_plane`` on its device labels and record, joins the labelled pixels into connected components along
4-neighbour edges whose disparity step is small, and returns a short table -- per object the pixel count, the image
box, the nearest pixel and the extents in the ground grid's frame, in height and in disparity -- and, on request, the
per-pixel object number.

With ``tracks=`` (which needs ``objects=`` and an estimator with a motion stage) the session says which object is which
across frames and how each one moves: ``codd_track_objects`` runs after ``codd_ego_motion`` and before
``codd_export_motion`` rolls the previous depth map, carries every pixel of the previous frame's objects along the SE3
field onto this frame's id map, lets it vote, and keeps a track id where the best matches are mutual; per object it
returns the mean 3-D displacement of its pixels and, with ``egomotion=``, what is left of it after the camera's own motion.

With ``scan=`` (which needs ``ground=``) the session says how far one can go in every direction in front of the camera:
``codd_range_scan`` runs right after ``codd_objects`` (after ``codd_ground_plane`` without ``objects=``) on the same device
labels, record and id map, bins the floor and obstacle pixels by bearing and range in the frame of the objects' extents,
and returns a planar laser scan -- per beam the range of the first obstacle, the pixel and the object that made it, and
how far the floor was seen in front of it.

With ``localmap=`` (which needs ``ground=`` and ``egomotion=``) the session keeps a map across frames: ``codd_local_map``
runs after ``codd_ground_plane`` and ``codd_ego_motion`` on their device records and labels, advances the camera's planar
pose by the ego fit levelled with each frame's own floor normal, and adds the frame's floor and obstacle pixels to a rolling
occupancy grid of integer log-odds that follows the camera.  The map, its age plane and the pose state stay on the device.

With ``costmap=`` (which needs ``localmap=``) the session says where the robot can go: ``codd_cost_map`` runs right after
``codd_local_map`` on the unrolled map it left on the device and returns, per cell, the squared distance to the nearest
occupied cell, an inflated cost in the convention of ROS costmap_2d, whether the cell can be reached from the camera's cell,
and whether the known space ends there (a frontier).  Integers only: equal maps give equal bytes.

With ``plan=`` (which needs ``costmap=``) the session says which way to go: ``codd_plan`` runs right after
``codd_cost_map`` on the cost and reach it left on the device and returns the navigation function -- the least cost to reach
the goal from every reachable cell -- and the path from the camera's cell to the goal.  The goal is the nearest frontier
(exploring) or a point of the map frame, changed between frames with ``set_goal``.  Integers only, one launch.

With ``heightmap=`` (which needs ``localmap=``) the session also says how high things are: ``codd_height_map`` runs right
behind ``codd_local_map`` on the pose and window it left and keeps a 2.5-D elevation layer on the map's cells -- the highest
and lowest surface and the lowest overhead thing per cell, with step, headroom and hole flags.  Integers only, 4 launches.
"""
from collections import deque, namedtuple

import numpy as np
import torch

from . import _abi, calibration as _calibration, ops, synth
from .runtime import FrameRunner

OUTPUTS = ("disp", "depth", "disp_u16")
MOTIONS = ("flow2d", "flow_dd", "sceneflow")
PIXEL_FORMATS = ("rgb8",) + tuple(ops.FRAME_FORMATS)  # rgb8: packed [h,w,3] through codd_ingest_pair; the others raw
YUVS = tuple(ops.YUV_MATRICES)
DEPTH = 2  # frames in flight: input, device and host output slots are double-buffered
DEFAULT_INTRINSICS, DEFAULT_CALIB = (1050.0, 1050.0, 480.0, 270.0), 210.0  # without calibration= and not passed
EGO_DEFAULTS = dict(iters=5, delta_px=1.0, tau_px=2.0, min_valid=16)
CONF_DEFAULTS = dict(occ_px=1.0, tau=24.0)
ALIGN_DEFAULTS = dict(footprint=None, uv=False)  # footprint None: calibration.auto_footprint
EPI_DEFAULTS = dict(range_px=2, step=2, tau=24.0, min_curv=0.5, iters=4, delta_px=0.25, min_valid=256, map=False)
GROUND_DEFAULTS = dict(step=2, iters=8, delta_px=0.25, delta0_px=4.0, asym=4.0, min_valid=256, max_tilt_deg=45.0, tol_px=0.5,
                       ground_tol=0.05, clearance=2.0, height=None, pitch_deg=0.0, up=(0, -1, 0), map=False, grid=None,
                       cell=0.1)
OBJECT_DEFAULTS = dict(select=("obstacle",), gap_px=1.0, gap_rel=0.05, min_pixels=64, min_height=0.15, max_objects=256,
                       map=False)
TRACK_DEFAULTS = dict(min_votes=16)
SCAN_DEFAULTS = dict(beams=256, angles_deg=None, range_min=0.0, range_max=12.8, bins=128, select=("obstacle",), min_pixels=8)
# The increments and levels of ops.MAP_PARAMS are chosen by reasoning, not measured on real footage (see there).
LOCALMAP_DEFAULTS = dict(grid=(128, 128), cell=0.1, range_min=0.0, range_max=12.8, select=("obstacle",), min_pixels=4, l_occ=4,
                         l_free=2, l_min=-32, l_max=64, decay=0, occ_level=8, free_level=-4, lost="reset")
LOCALMAP_LOST = dict(reset=ops.MAP_RESET, hold=ops.MAP_HOLD)
# Chosen by reasoning, not measured on real footage: a robot of 0.3 radius; costs that decay out to 1.0, where scaling 3.0
# leaves 252 exp(-2.1) = 30, a visible slope across the seven cells of 0.1 in between; start_radius covers the blind zone of
# a camera about 1 m above the floor, whose lower image edge meets the floor more than a metre ahead, so the cells under
# and right around the robot are never observed.
COSTMAP_DEFAULTS = dict(robot_radius=0.3, inflation_radius=1.0, scaling=3.0, start_radius=1.5, through_unknown=False, nearest=False)
# Chosen by reasoning, not measured on real footage: neutral 50 and factor 0.8 (205 / 256) are the defaults of ROS navfn, so
# a free cell costs 50 per step and an inscribed one 50 + 202 -- five free cells of detour buy one cell away from a wall;
# an unknown cell (crossed only with the cost map's through_unknown) counts as cost 128, half way up; the goal is the
# nearest frontier, which is what a robot without orders does; 1024 path cells cover the diagonal of the default window
# more than five times.
PLAN_DEFAULTS = dict(goal="frontier", goal_radius=0.0, neutral=50, factor=205, unknown_cost=128, max_path=1024, dir=False)
# Chosen by reasoning, not measured on real footage (ops.HEIGHT_PARAMS says why): 5 mm units, every surface label, four
# pixels as the map's, half way to each new observation, a platform that climbs and drops 10 cm and stands 1 m tall.
HEIGHTMAP_DEFAULTS = dict(h_res=0.005, select=("floor", "obstacle", "below"), min_pixels=4, alpha=128, max_step=0.10,
                          robot_height=1.0, max_drop=0.10)
OBJECT_LABELS = dict(floor=ops.GROUND_FLOOR, obstacle=ops.GROUND_OBSTACLE, overhead=ops.GROUND_OVERHEAD,
                     below=ops.GROUND_BELOW)  # the names ``select`` takes

# One frame's ego-motion, caller-owned: pose fp32 [7] = (t, q_xyzw) of G, the rigid motion that maps static points from
# the previous camera frame to the current one (t in the unit of calib; the camera itself moved by G^-1); ok (False: the
# fit was degenerate and pose is its last good iterate); valid / inliers pixel counts; rms_px of the inliers; moving
# uint8 [h,w] (0 static, 1 moving, 255 invalid) and residual fp32 [h,w] (pixels, NaN where invalid) on the previous
# frame's grid; camera_to_world float64 [4,4], the current camera's pose in the frame of the sequence's first field.
Ego = namedtuple("Ego", "pose ok valid inliers rms_px moving residual camera_to_world")


# One frame's stereo confidence on the CURRENT frame's grid, caller-owned: flags uint8 [h,w], the OR of 1 (out of view: the
# match falls left of the right image), 2 (occluded in the right image), 4 (photometric mismatch: residual > tau) and 128
# (disparity not finite or not positive; alone) -- 0 is a pixel to trust; residual fp32 [h,w], the mean absolute
# difference of the left pixel and its match in the right image in grey levels of the 8-bit source, NaN where the flags
# are 1 or 128.
Confidence = namedtuple("Confidence", "flags residual")


# One frame's depth on the grid of the align_to camera, caller-owned: depth fp32 [ht,wt] in the unit of calib, the nearest
# surface that lands on each target pixel, +inf where nothing lands; uv fp32 [h,w,2] (None unless align=dict(uv=True)): the
# position (sx, sy) in the target image of every pixel of the session's own grid, NaN where the pixel has no valid
# disparity or does not project into the target camera.
Aligned = namedtuple("Aligned", "depth uv")


# One frame's rectification check, caller-owned: coef float64 [4] = (c0, c1, c2, c3) of the fitted vertical disparity
# dy = fy (c0 (1 + yn^2) + c1 xr yn + c2 xr + c3 yn) -- the right view is rotated by (-c0, c1, c2) radians and its focal
# length is off by the ratio c3; ok (False: the frame alone does not determine the fit and coef is its last good iterate);
# valid measurable pixels, inliers of the fit; rms_px of the measured dy and rms_fit_px of the inliers' residual;
# A float64 [4,4] and b float64 [4], the last step's normal equations (combine_epipolar adds them over frames); dy fp32
# [h,w] (None unless epipolar=dict(map=True)): the measured row offset, L(x, y) ~ R(x - d, y + dy), NaN where not measured.
Epipolar = namedtuple("Epipolar", "coef ok valid inliers rms_px rms_fit_px A b dy")


def epipolar_from_record(rec, dy=None):
    """The 32 doubles of codd_epipolar_check (include/codd_hip.h) -> ``Epipolar``."""
    rec = np.asarray(rec, np.float64)
    A = np.zeros((4, 4))
    A[np.triu_indices(4)] = rec[10:20]
    A = A + np.triu(A, 1).T
    return Epipolar(rec[0:4].copy(), bool(rec[4] != 0), int(rec[5]), int(rec[6]), float(rec[7]), float(rec[8]), A,
                    rec[20:24].copy(), dy)


# One frame's ground plane, caller-owned: coef float64 [3] of the fitted plane d = c0 (x - cx) + c1 (y - cy) + c2 in
# disparity space; ok (False: no floor was found -- the fit was degenerate, tilted by more than max_tilt_deg against up,
# had too few inliers, or the camera looks straight down -- and labels are all 255, heights NaN, grids zero); normal
# float64 [3], the unit normal from the floor towards the camera in camera coordinates; camera_height above the plane and
# every height in the unit of calib / fx (metres for a metric baseline); tilt_deg between normal and up; forward float64
# [3], the grid's forward axis (the optical axis projected onto the plane); valid fit pixels, inliers (|e| <= delta_px)
# and their rms_px; steps taken; labels uint8 [h,w] (0 floor, 1 obstacle, 2 overhead, 3 below the floor, 255 invalid);
# height fp32 [h,w] above the plane, NaN where invalid (None unless ground=dict(map=True)); grid_count int32 [2,gh,gw]
# (floor and obstacle pixels per cell) and grid_height fp32 [gh,gw] (the tallest obstacle pixel of a cell, 0 without one),
# None unless ground=dict(grid=(gh, gw)): row iz = 0 lies under the camera, iz grows forward, column gw / 2 is straight
# ahead and ix grows to the right, cells of `cell` units.
Ground = namedtuple("Ground", "coef ok normal camera_height tilt_deg forward valid inliers rms_px steps labels height "
                              "grid_count grid_height")


def ground_from_record(rec, labels, height=None, grid_count=None, grid_height=None):
    """The 32 doubles of codd_ground_plane (include/codd_hip.h) and its maps -> ``Ground``."""
    rec = np.asarray(rec, np.float64)
    return Ground(rec[0:3].copy(), bool(rec[3] != 0), rec[8:11].copy(), float(rec[11]), float(rec[12]), rec[22:25].copy(),
                  int(rec[4]), int(rec[5]), float(rec[6]), int(rec[7]), labels, height, grid_count, grid_height)


# One frame's obstacle objects, caller-owned: n objects (at most max_objects), in raster order of their first pixel; found
# components that passed min_pixels and min_height (> n: the list was truncated); components and foreground pixels in
# all; pixels int32 [n]; box int32 [n,4] (x0, y0, x1, y1, inclusive); near_px int32 [n,2] (x, y) of the pixel with the
# largest disparity; key int32 [n], the raster index y * w + x of the object's first pixel; extent fp32 [n,4] (gx_min, gx_max,
# gz_min, gz_max) in the frame of Ground.grid_count (gx to the right, gz forward, the camera above the origin); height
# fp32 [n,2] (lowest, highest pixel above the floor); disparity fp32 [n,2] (smallest, largest: depth = calib / disparity);
# ids uint16 [h,w] (None unless objects=dict(map=True)): the object number of every pixel, 0xFFFF for none.
Objects = namedtuple("Objects", "n found components foreground pixels box near_px key extent height disparity ids")


def objects_from_buffers(count, obj_i, obj_f, ids=None):
    """count int32 [4], obj_i int32 [max_objects,8] and obj_f fp32 [max_objects,8] of codd_objects (include/codd_hip.h) and
    its id map -> ``Objects``, the tables sliced to the n objects (copies: the buffers may be reused)."""
    count, obj_i, obj_f = np.asarray(count, np.int32), np.asarray(obj_i, np.int32), np.asarray(obj_f, np.float32)
    n = int(count[0])
    return Objects(n, int(count[1]), int(count[2]), int(count[3]), obj_i[:n, 0].copy(), obj_i[:n, 1:5].copy(),
                   obj_i[:n, 5:7].copy(), obj_i[:n, 7].copy(), obj_f[:n, 0:4].copy(), obj_f[:n, 4:6].copy(),
                   obj_f[:n, 6:8].copy(), ids)


# One frame's object tracks, caller-owned, row k belonging to object k of the frame's ``Objects``: n objects; continued of
# them carry on a track of the previous frame, started begin one, and ended tracks of the previous frame found no
# successor; track int32 [n], the persistent id (from 1; never reused within 2^31 ids); age int32 [n], the frames the track
# has lived (1: started here); prev int32 [n], the object's number in the PREVIOUS frame's ``Objects`` (-1: started); votes
# int32 [n], the previous object's pixels that the field carried onto this one; pixels int32 [n], the previous object's
# pixels with a valid motion, moving of them marked by the ego stage's mask, own_pixels of them counted in ``own``;
# motion fp32 [n,3], the mean 3-D displacement (X, Y, Z) of those pixels from the previous frame to this one in the unit
# of calib, and own fp32 [n,3], the same after the camera's own motion is taken out (NaN rows: a started track; own also
# without ``egomotion=`` or without a good ego fit).
Tracks = namedtuple("Tracks", "n continued started ended track age prev votes pixels moving own_pixels motion own")


def tracks_from_buffers(trk_count, trk_i, trk_f):
    """trk_count int32 [4], trk_i int32 [max_objects,8] and trk_f fp32 [max_objects,8] of codd_track_objects
    (include/codd_hip.h) -> ``Tracks``, the tables sliced to the n objects (copies: the buffers may be reused)."""
    c, ti, tf = np.asarray(trk_count, np.int32), np.asarray(trk_i, np.int32), np.asarray(trk_f, np.float32)
    n = int(c[0])
    return Tracks(n, int(c[1]), int(c[2]), int(c[3]), *(ti[:n, k].copy() for k in range(7)), tf[:n, 0:3].copy(),
                  tf[:n, 3:6].copy())


# One frame's range scan, caller-owned, in the convention of a planar laser scan: beam k covers the bearings angle_min + k *
# angle_increment .. angle_min + (k + 1) * angle_increment (radians from the ground grid's forward axis, positive to the
# right); ranges fp32 [beams] in the unit of calib / fx, measured on the floor from the point under the camera: the range of
# the nearest pixel of the first range bin holding at least min_pixels obstacle pixels, +inf where the beam is clear as far
# as the floor was seen, NaN where nothing is known; free fp32 [beams], the range up to which the floor was seen in front of
# the hit (0: not at all); hit_xz fp32 [beams,2], (gx, gz) of the hit pixel in the frame of Objects.extent (zeros without a
# hit); pixel int32 [beams], its raster index y * w + x (-1 without); object int32 [beams], its number in the frame's
# ``Objects`` (-1: none, or no objects=); track int32 [beams], the track id of that object (0: none; None without tracks=);
# support int32 [beams], the obstacle pixels of the hit bin; floor int32 [beams], the floor pixels in front of the hit;
# hits, clear and unknown beams (they add up to the beams) and obstacle_pixels binned in all.
Scan = namedtuple("Scan", "angle_min angle_increment range_min range_max ranges free hit_xz pixel object track support floor "
                          "hits clear unknown obstacle_pixels")


def scan_from_buffers(count, scan_i, scan_f, edges_meta, tracks=None):
    """count int32 [4], scan_i int32 [beams,4] and scan_f fp32 [beams,4] of codd_range_scan (include/codd_hip.h) ->
    ``Scan`` (copies: the buffers may be reused).  ``edges_meta`` = (angle_min, angle_increment, range_min, range_max);
    ``tracks``: the frame's ``Tracks`` or None -- with it ``track`` is ``tracks.track[object]``, 0 where there is no object."""
    count, si, sf = np.asarray(count, np.int32), np.asarray(scan_i, np.int32), np.asarray(scan_f, np.float32)
    obj = si[:, 1].copy()
    track = None
    if tracks is not None:
        known = (obj >= 0) & (obj < tracks.n)
        track = np.zeros(obj.shape, np.int32)
        track[known] = np.asarray(tracks.track, np.int32)[obj[known]]
    a0, da, r0, r1 = (float(v) for v in edges_meta)
    return Scan(a0, da, r0, r1, sf[:, 0].copy(), sf[:, 1].copy(), sf[:, 2:4].copy(), si[:, 0].copy(), obj, track,
                si[:, 2].copy(), si[:, 3].copy(), int(count[0]), int(count[1]), int(count[2]), int(count[3]))


# One frame's view of the rolling occupancy map, caller-owned.  logodds int16 [gh,gw] and age uint8 [gh,gw]: the window
# unrolled, [j,i] = world cell (origin[0] + i, origin[1] + j) of the map frame -- the floor frame of the first integrated
# frame, x to its right, z forward, cells of ``cell`` units (the unit of calib / fx); age 255: never observed inside the
# window, otherwise frames since the last observation (254: that or more).  pose = (x, z, (hx, hz)): the camera's foot point
# and unit heading in the map; origin = (ix0, iz0); integrated: the frame had a floor and its pixels were added; linked: the
# pose was advanced by the ego fit (False on the first frame of a sequence and on a LOST one); restarts; frames since the
# last reset; occupied, free and unknown: cells with logodds >= occ_level, <= free_level and with age 255; pixels: the
# pixels added; step = (dx, dz): the camera's planar step in its previous floor frame; occ_level and free_level as given.
_LocalMap = namedtuple("LocalMap", "logodds age pose origin cell integrated linked restarts frames occupied free unknown pixels "
                                   "step occ_level free_level")
MAP_FREE, MAP_OCCUPIED, MAP_UNKNOWN = 0, 1, 2  # the values of LocalMap.state()


class LocalMap(_LocalMap):
    __slots__ = ()

    def state(self):
        """uint8 [gh,gw]: ``MAP_OCCUPIED`` where logodds >= occ_level, ``MAP_FREE`` where logodds <= free_level (and not
        occupied), ``MAP_UNKNOWN`` elsewhere."""
        out = np.full(self.logodds.shape, MAP_UNKNOWN, np.uint8)
        out[self.logodds <= self.free_level] = MAP_FREE
        out[self.logodds >= self.occ_level] = MAP_OCCUPIED
        return out

    def world_xz(self, j, i):
        """The centre (x, z) of cell [j,i] in the map frame (float64; arrays broadcast)."""
        j, i = np.broadcast_arrays(np.asarray(j, np.float64), np.asarray(i, np.float64))
        x, z = (self.origin[0] + i + 0.5) * self.cell, (self.origin[1] + j + 0.5) * self.cell
        return (float(x), float(z)) if x.ndim == 0 else (x, z)


def localmap_from_buffers(record, map_out, age_out, cell, occ_level, free_level):
    """record float64 [16], map_out int16 [gh,gw] and age_out uint8 [gh,gw] of codd_local_map (include/codd_hip.h) ->
    ``LocalMap`` (copies: the buffers may be reused)."""
    r = np.asarray(record, np.float64)
    return LocalMap(np.array(map_out, np.int16), np.array(age_out, np.uint8), (float(r[4]), float(r[5]), (float(r[6]), float(r[7]))),
                    (int(r[8]), int(r[9])), float(cell), bool(r[0] != 0), bool(r[1] != 0), int(r[2]), int(r[3]), int(r[11]),
                    int(r[12]), int(r[13]), int(r[10]), (float(r[14]), float(r[15])), int(occ_level), int(free_level))


# One frame's cost map of the LocalMap of the same frame, caller-owned; [j,i] is the LocalMap's cell [j,i].  cost uint8
# [gh,gw] in the convention of ROS costmap_2d (ops.COST_LETHAL 254: occupied, ops.COST_INSCRIBED 253: within robot_radius of
# an occupied cell, 1 .. 252 decaying to inflation_radius, 0 free, ops.COST_NO_INFO 255: unknown and not inscribed); dist2
# int32 [gh,gw]: the squared distance in cells to the nearest occupied cell of the window, ops.COST_FAR beyond R =
# ceil(inflation_radius / cell) cells; nearest int32 [gh,gw] (the raster index j gw + i of that cell, -1 for none) or None
# without ``nearest``; reach uint8 [gh,gw]: REACH_NO 0, REACH_YES 1, REACH_FRONTIER 2 (reachable, next to unknown cells that
# are not); origin and cell as the LocalMap's; start = (i, j): the camera's cell; occupied, inscribed (cost 253 or 254),
# unknown (cost 255), reachable (frontiers included) and frontiers: cell counts; start_ok: the start cell is traversable;
# start_dist2: dist2 there (-1: far); frontier_cell = (j, i) of the frontier nearest to the start, or None; frontier_dist2:
# its squared distance in cells (-1).
_CostMap = namedtuple("CostMap", "cost dist2 nearest reach origin cell start occupied inscribed unknown reachable frontiers "
                                 "start_ok start_dist2 frontier_cell frontier_dist2")
REACH_NO, REACH_YES, REACH_FRONTIER = 0, 1, 2  # the values of CostMap.reach


class CostMap(_CostMap):
    __slots__ = ()

    def clearance(self):
        """fp32 [gh,gw]: the distance to the nearest occupied cell, sqrt(dist2) * cell, +inf where dist2 is far."""
        far = self.dist2 == ops.COST_FAR
        out = (np.sqrt(np.where(far, 0, self.dist2).astype(np.float64)) * self.cell).astype(np.float32)
        out[far] = np.inf
        return out

    world_xz = LocalMap.world_xz  # (the same cells: it reads ``origin`` and ``cell`` alone)

    def frontier_xz(self):
        """The centre (x, z) of ``frontier_cell`` in the map frame, or None without a frontier."""
        return None if self.frontier_cell is None else self.world_xz(*self.frontier_cell)


def costmap_from_buffers(record, dist2, cost, reach, nearest, origin, cell, start):
    """record float64 [16], dist2 int32, cost and reach uint8 [gh,gw] and nearest int32 [gh,gw] or None of codd_cost_map
    (include/codd_hip.h), the LocalMap's ``origin`` and ``cell`` and start = (i, j) -> ``CostMap`` (copies: the buffers may be
    reused)."""
    r = np.asarray(record, np.float64)
    gw = int(np.asarray(cost).shape[1])
    front = int(r[8])
    return CostMap(np.array(cost, np.uint8), np.array(dist2, np.int32), None if nearest is None else np.array(nearest, np.int32),
                   np.array(reach, np.uint8), (int(origin[0]), int(origin[1])), float(cell), (int(start[0]), int(start[1])),
                   int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), bool(r[5] != 0), int(r[6]),
                   None if front < 0 else (front // gw, front % gw), int(r[9]))


# One frame's plan on the CostMap of the same frame, caller-owned; [j,i] is the LocalMap's cell [j,i].  potential uint32
# [gh,gw]: the least cost to reach the goal from the cell (ops.PLAN_UNREACHED: no path), the sum over the cells entered of
# the step's length (5 straight, 7 diagonal) times neutral + factor cost / 256; dir uint8 [gh,gw] or None without ``dir``: the
# move to make there (0 .. 7: (di, dj) = PLAN_MOVES[k], 8: in the goal set, 255: no path); path int32 [n,2]: the cells (j, i)
# from the start cell to the goal, the written entries only; found: the start cell has a path; cost: the potential there
# (-1); length_cells: the cells of the full path; truncated: it is longer than max_path; goal_cell = (j, i) after clamping,
# or None without a goal; clamped: the goal lay outside the window; snapped: no reachable cell lay within goal_radius of the
# goal cell and the nearest reachable one took its place; end_cell = (j, i) of the path's last cell, or None; reached: the
# cells with a path; max_cost_on_path: the largest cost byte other than 255 on the path (-1); length: the path's length in
# the map's unit; origin and cell as the LocalMap's; start = (i, j): the camera's cell.
_Plan = namedtuple("Plan", "potential dir path found cost length_cells truncated goal_cell clamped snapped end_cell reached "
                           "max_cost_on_path length origin cell start")
PLAN_MOVES = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))  # (di, dj) of Plan.dir's k


class Plan(_Plan):
    __slots__ = ()

    world_xz = LocalMap.world_xz  # (the same cells: it reads ``origin`` and ``cell`` alone)

    def path_xz(self):
        """float64 [n,2]: the centres (x, z) of the path's cells in the map frame."""
        if not len(self.path):
            return np.zeros((0, 2), np.float64)
        return np.stack(self.world_xz(self.path[:, 0], self.path[:, 1]), axis=1)

    def lookahead(self, dist):
        """The centre (x, z) of the first path cell at least ``dist`` from the start cell along the path (a straight step is
        one cell long, a diagonal one 7 / 5), or of the last cell if none is; None without a path.  The point a pure-pursuit
        controller steers at."""
        if not len(self.path):
            return None
        step = np.abs(np.diff(self.path, axis=0)).sum(axis=1)  # 1: straight, 2: diagonal
        along = np.concatenate(([0.0], np.cumsum(np.where(step == 1, 5, 7)) * (self.cell / 5.0)))
        k = int(np.argmax(along >= dist)) if (along >= dist).any() else len(along) - 1
        return self.world_xz(int(self.path[k, 0]), int(self.path[k, 1]))


def plan_from_buffers(record, potential, dir, path, origin, cell, start):
    """record float64 [16], potential [gh,gw] (its 32 bits, signed or not), dir uint8 [gh,gw] or None and path int32 [max_path]
    of codd_plan (include/codd_hip.h), the LocalMap's ``origin`` and ``cell`` and start = (i, j) -> ``Plan`` (copies: the
    buffers may be reused)."""
    r = np.asarray(record, np.float64)
    pot = np.array(np.asarray(potential).view(np.uint32))
    gw = int(pot.shape[1])
    n = int(r[3])
    cells = np.array(np.asarray(path, np.int32)[:n])
    at = lambda v: None if v < 0 else (int(v) // gw, int(v) % gw)  # noqa: E731
    return Plan(pot, None if dir is None else np.array(dir, np.uint8), np.stack([cells // gw, cells % gw], axis=1).astype(np.int32),
                bool(r[0] != 0), int(r[1]), int(r[2]), bool(r[2] > r[3]), at(r[4]), bool(r[5] != 0), bool(r[6] != 0), at(r[8]),
                int(r[9]), int(r[11]), float(r[12]) * float(cell) / 5.0, (int(origin[0]), int(origin[1])), float(cell),
                (int(start[0]), int(start[1])))


# One frame's view of the rolling elevation layer, caller-owned; [j,i] is the LocalMap's cell [j,i].  top, bot and ceil fp32
# [gh,gw]: the highest and the lowest surface seen in the cell and the lowest thing hanging over it, in the unit of
# calib / fx above the floor plane of the frame that saw them (not a global datum), NaN where nothing was seen; top_q, bot_q
# and ceil_q int16 [gh,gw]: the same in units of h_res as the device keeps them (ops.HEIGHT_NONE -32768: no surface,
# ops.HEIGHT_NO_CEIL 32767: no overhead); age uint8 [gh,gw]: 255 never observed inside the window, otherwise frames since the
# last observation (254: that or more); step uint16 [gh,gw]: how far the cell's top stands above its lowest known
# 8-neighbour, in units of h_res; flags uint8 [gh,gw]: ops.HEIGHT_UNKNOWN 255 for a cell without a surface, otherwise the
# bits ops.HEIGHT_STEP (step > max_step), ops.HEIGHT_HEADROOM (ceil - top < robot_height), ops.HEIGHT_HOLE (bot < -max_drop);
# integrated: the frame's pixels were added; surface_pixels and overhead_pixels: the pixels added; observed: cells
# updated by this frame; known: cells with a surface; steps, headroom, holes: cells with each flag; top_max and bot_min:
# the largest top and the smallest bot over the known cells, in the layer's unit (0.0 without one); origin and cell as the
# LocalMap's; h_res.
_HeightMap = namedtuple("HeightMap", "top bot ceil top_q bot_q ceil_q age step flags integrated surface_pixels overhead_pixels "
                                     "observed known steps headroom holes top_max bot_min origin cell h_res")


class HeightMap(_HeightMap):
    __slots__ = ()

    world_xz = LocalMap.world_xz  # (the same cells: it reads ``origin`` and ``cell`` alone)

    def traversable(self):
        """bool [gh,gw]: ``flags == 0`` -- a known cell without a step, with headroom and without a hole."""
        return self.flags == 0


def heightmap_from_buffers(record, top, bot, ceil, age, step, flags, cell, h_res):
    """record float64 [16], top_out, bot_out, ceil_out int16, hage_out uint8, step_out uint16 and flags_out uint8 [gh,gw] of
    codd_height_map (include/codd_hip.h), the LocalMap's ``cell`` and ``h_res`` -> ``HeightMap`` (copies: the buffers may be
    reused)."""
    r = np.asarray(record, np.float64)
    res = np.float32(h_res)
    tq, bq, cq = (np.array(v, np.int16) for v in (top, bot, ceil))

    def metres(q, none):
        out = q.astype(np.float32) * res
        out[q == none] = np.nan
        return out

    return HeightMap(metres(tq, ops.HEIGHT_NONE), metres(bq, ops.HEIGHT_NONE), metres(cq, ops.HEIGHT_NO_CEIL), tq, bq, cq,
                     np.array(age, np.uint8), np.array(np.asarray(step).view(np.uint16)), np.array(flags, np.uint8), bool(r[0] != 0),
                     int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5]), int(r[6]), int(r[7]), float(r[8]) * float(h_res),
                     float(r[9]) * float(h_res), (int(r[10]), int(r[11])), float(cell), float(h_res))


def _unit_up(up, pitch_deg=0.0):
    """The unit up vector in camera coordinates after pitching the camera DOWN by ``pitch_deg`` (a rotation about the
    camera's x axis: a level camera's (0, -1, 0) becomes (0, -cos, -sin))."""
    u = np.array([float(v) for v in up], np.float64)
    n = float(np.sqrt(u @ u))
    if u.shape != (3,) or not (n > 0 and np.isfinite(n)):
        raise ValueError(f"up: three finite numbers, not all zero, expected, got {up!r}")
    u = u / n
    t = np.deg2rad(float(pitch_deg))
    return np.array([u[0], u[1] * np.cos(t) - u[2] * np.sin(t), u[1] * np.sin(t) + u[2] * np.cos(t)])


def ground_seed(height, K, calib, up=(0, -1, 0), pitch_deg=0.0):
    """The coefficients (float64 [3]) of the floor a camera mounted ``height`` above it sees: the plane N.X = calib with
    N = -(calib / height) u, u the unit up vector after the pitch (``_unit_up``), is c = -(calib / height) (u_x / fx,
    u_y / fy, u_z).  ``height`` is in the unit of calib / fx."""
    if not (float(height) > 0 and np.isfinite(float(height))):
        raise ValueError(f"ground_seed: a positive height expected, got {height!r}")
    fx, fy = float(K[0]), float(K[1])
    u = _unit_up(up, pitch_deg)
    return -(float(calib) / float(height)) * np.array([u[0] / fx, u[1] / fy, u[2]])


def solve_epipolar(A, b):
    """``(coef, ok)`` of the normal equations ``A c = b``: the 4x4 Cholesky and the pivot rule of codd_epipolar_check
    (a pivot <= 1e-12 trace(A), or anything not finite: zeros and False)."""
    A, b = np.array(A, np.float64), np.array(b, np.float64)
    if A.shape != (4, 4) or b.shape != (4,) or not (np.all(np.isfinite(A)) and np.all(np.isfinite(b))):
        return np.zeros(4), False
    floor_ = 1e-12 * np.trace(A)
    L = np.zeros((4, 4))
    for j in range(4):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > floor_:
            return np.zeros(4), False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 4):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(4)
    for i in range(4):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    c = np.zeros(4)
    for i in range(3, -1, -1):
        c[i] = (y[i] - L[i + 1:, i] @ c[i + 1:]) / L[i, i]
    if not np.all(np.isfinite(c)):
        return np.zeros(4), False
    return c, True


def combine_epipolar(results):
    """``(coef, ok)`` over several frames: the ``Epipolar``s' normal equations ``A``, ``b`` summed in float64 and solved
    once.  Every frame takes part, those whose own ``ok`` is False too: a single frame often lacks the texture or the
    spread of disparities that the sequence has.  None entries (and an empty list: ok False) are allowed."""
    A, b = np.zeros((4, 4)), np.zeros(4)
    for r in results:
        if r is not None:
            A += np.asarray(r.A, np.float64)
            b += np.asarray(r.b, np.float64)
    return solve_epipolar(A, b)


def pose_matrix(pose):
    """[t(3), q_xyzw(4)] -> the 4x4 float64 matrix of the rigid motion."""
    t, (x, y, z, w) = np.asarray(pose[:3], np.float64), np.asarray(pose[3:7], np.float64)
    n = x * x + y * y + z * z + w * w
    s = 2.0 / n
    M = np.eye(4)
    M[:3, :3] = [[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                 [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                 [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]]
    M[:3, 3] = t
    return M


def trajectory_step(world, pose, ok=True):
    """camera_to_world after one more frame: W_t = W_{t-1} G_t^-1.  ``pose`` None (a frame without a field) restarts
    the trajectory at identity; ``ok`` False (a degenerate fit) carries ``world`` forward unchanged."""
    if pose is None:
        return np.eye(4)
    if not ok:
        return np.array(world, np.float64)
    G = pose_matrix(pose)
    Ginv = np.eye(4)
    Ginv[:3, :3] = G[:3, :3].T
    Ginv[:3, 3] = -G[:3, :3].T @ G[:3, 3]
    return np.asarray(world, np.float64) @ Ginv


def _check_ego(egomotion):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise (no device call)."""
    if egomotion is None or egomotion is False:
        return None
    if egomotion is True:
        return dict(EGO_DEFAULTS)
    if not isinstance(egomotion, dict):
        raise ValueError(f"egomotion: False, True or a dict of {tuple(EGO_DEFAULTS)} expected, got {egomotion!r}")
    unknown = set(egomotion) - set(EGO_DEFAULTS)
    if unknown:
        raise ValueError(f"egomotion: unknown keys {sorted(unknown)}; known: {tuple(EGO_DEFAULTS)}")
    p = dict(EGO_DEFAULTS, **egomotion)
    if not (isinstance(p["iters"], int) and 1 <= p["iters"] <= 32):
        raise ValueError(f"egomotion: iters in [1, 32] expected, got {p['iters']!r}")
    for k in ("delta_px", "tau_px"):
        if not float(p[k]) > 0:
            raise ValueError(f"egomotion: positive {k} expected, got {p[k]!r}")
    p["min_valid"] = int(p["min_valid"])
    return p


def _check_conf(confidence):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise (no device call)."""
    if confidence is None or confidence is False:
        return None
    if confidence is True:
        return dict(CONF_DEFAULTS)
    if not isinstance(confidence, dict):
        raise ValueError(f"confidence: False, True or a dict of {tuple(CONF_DEFAULTS)} expected, got {confidence!r}")
    unknown = set(confidence) - set(CONF_DEFAULTS)
    if unknown:
        raise ValueError(f"confidence: unknown keys {sorted(unknown)}; known: {tuple(CONF_DEFAULTS)}")
    p = {}
    for k, v in dict(CONF_DEFAULTS, **confidence).items():
        try:
            p[k] = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"confidence: a number expected for {k}, got {v!r}") from None
    if not p["occ_px"] >= 0:  # (NaN compares false)
        raise ValueError(f"confidence: occ_px >= 0 expected, got {confidence['occ_px']!r}")
    if p["tau"] != p["tau"]:
        raise ValueError("confidence: tau must not be NaN")
    return p


def _check_epi(epipolar):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise (no device call)."""
    if epipolar is None or epipolar is False:
        return None
    if epipolar is True:
        return dict(EPI_DEFAULTS)
    if not isinstance(epipolar, dict):
        raise ValueError(f"epipolar: False, True or a dict of {tuple(EPI_DEFAULTS)} expected, got {epipolar!r}")
    unknown = set(epipolar) - set(EPI_DEFAULTS)
    if unknown:
        raise ValueError(f"epipolar: unknown keys {sorted(unknown)}; known: {tuple(EPI_DEFAULTS)}")
    p = dict(EPI_DEFAULTS, **epipolar)
    for k, lo, hi in (("range_px", 1, 4), ("step", 1, 8), ("iters", 1, 32)):
        if not (isinstance(p[k], int) and not isinstance(p[k], bool) and lo <= p[k] <= hi):
            raise ValueError(f"epipolar: an integer {k} in [{lo}, {hi}] expected, got {p[k]!r}")
    if not (isinstance(p["min_valid"], int) and not isinstance(p["min_valid"], bool)):
        raise ValueError(f"epipolar: an integer min_valid expected, got {p['min_valid']!r}")
    for k in ("tau", "min_curv", "delta_px"):
        try:
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError(f"epipolar: a number expected for {k}, got {p[k]!r}") from None
        if p[k] != p[k]:
            raise ValueError(f"epipolar: {k} must not be NaN")
    if not p["delta_px"] > 0:
        raise ValueError(f"epipolar: positive delta_px expected, got {p['delta_px']!r}")
    if not isinstance(p["map"], bool):
        raise ValueError(f"epipolar: map True or False expected, got {p['map']!r}")
    return p


def _check_ground(ground):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise (no device call)."""
    if ground is None or ground is False:
        return None
    if ground is True:
        return dict(GROUND_DEFAULTS)
    if not isinstance(ground, dict):
        raise ValueError(f"ground: False, True or a dict of {tuple(GROUND_DEFAULTS)} expected, got {ground!r}")
    unknown = set(ground) - set(GROUND_DEFAULTS)
    if unknown:
        raise ValueError(f"ground: unknown keys {sorted(unknown)}; known: {tuple(GROUND_DEFAULTS)}")
    p = dict(GROUND_DEFAULTS, **ground)
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)  # noqa: E731
    for k, lo, hi in (("step", 1, 8), ("iters", 1, 32)):
        if not (is_int(p[k]) and lo <= p[k] <= hi):
            raise ValueError(f"ground: an integer {k} in [{lo}, {hi}] expected, got {p[k]!r}")
    if not is_int(p["min_valid"]):
        raise ValueError(f"ground: an integer min_valid expected, got {p['min_valid']!r}")
    for k in ("delta_px", "delta0_px", "asym", "max_tilt_deg", "tol_px", "ground_tol", "clearance", "pitch_deg", "cell"):
        try:
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError(f"ground: a number expected for {k}, got {p[k]!r}") from None
        if not np.isfinite(p[k]):
            raise ValueError(f"ground: a finite {k} expected, got {p[k]!r}")
    for k in ("delta_px", "delta0_px", "cell"):
        if not p[k] > 0:
            raise ValueError(f"ground: positive {k} expected, got {p[k]!r}")
    if not p["asym"] >= 1:
        raise ValueError(f"ground: asym >= 1 expected, got {p['asym']!r}")
    for k in ("max_tilt_deg", "tol_px", "ground_tol"):
        if not p[k] >= 0:
            raise ValueError(f"ground: {k} >= 0 expected, got {p[k]!r}")
    if not p["clearance"] >= p["ground_tol"]:
        raise ValueError(f"ground: clearance >= ground_tol expected, got {p['clearance']!r} < {p['ground_tol']!r}")
    if p["height"] is not None:
        try:
            p["height"] = float(p["height"])
        except (TypeError, ValueError):
            raise ValueError(f"ground: height None or a number expected, got {p['height']!r}") from None
        if not (p["height"] > 0 and np.isfinite(p["height"])):
            raise ValueError(f"ground: a positive height expected, got {p['height']!r}")
    try:
        p["up"] = tuple(float(v) for v in p["up"])
        _unit_up(p["up"])
    except (TypeError, ValueError):
        raise ValueError(f"ground: up: three finite numbers, not all zero, expected, got {p['up']!r}") from None
    if not isinstance(p["map"], bool):
        raise ValueError(f"ground: map True or False expected, got {p['map']!r}")
    if p["grid"] is not None:
        g = p["grid"]
        if not (isinstance(g, (tuple, list)) and len(g) == 2 and all(is_int(v) and v > 0 for v in g)
                and g[0] * g[1] < 2 ** 30):
            raise ValueError(f"ground: grid None or positive integers (gh, gw) with gh gw < 2^30 expected, got {g!r}")
        p["grid"] = (g[0], g[1])
    return p


def _check_objects(objects, ground=True):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise, and for ``objects``
    without ``ground`` (no device call)."""
    if objects is None or objects is False:
        return None
    if not (objects is True or isinstance(objects, dict)):
        raise ValueError(f"objects: False, True or a dict of {tuple(OBJECT_DEFAULTS)} expected, got {objects!r}")
    if ground is None or ground is False:
        raise ValueError("objects: needs ground= (the components are those of the ground stage's labels)")
    if objects is True:
        return dict(OBJECT_DEFAULTS)
    unknown = set(objects) - set(OBJECT_DEFAULTS)
    if unknown:
        raise ValueError(f"objects: unknown keys {sorted(unknown)}; known: {tuple(OBJECT_DEFAULTS)}")
    p = dict(OBJECT_DEFAULTS, **objects)
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)  # noqa: E731
    sel = p["select"]
    if isinstance(sel, str):
        sel = (sel,)
    if not (isinstance(sel, (tuple, list)) and len(sel) > 0 and all(isinstance(v, str) and v in OBJECT_LABELS for v in sel)):
        raise ValueError(f"objects: select: one or more of {tuple(OBJECT_LABELS)} expected, got {p['select']!r}")
    p["select"] = tuple(sel)
    if not (is_int(p["max_objects"]) and 1 <= p["max_objects"] <= ops.OBJECT_MAX):
        raise ValueError(f"objects: an integer max_objects in [1, {ops.OBJECT_MAX}] expected, got {p['max_objects']!r}")
    if not (is_int(p["min_pixels"]) and p["min_pixels"] >= 1):
        raise ValueError(f"objects: an integer min_pixels >= 1 expected, got {p['min_pixels']!r}")
    for k in ("gap_px", "gap_rel", "min_height"):
        try:
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError(f"objects: a number expected for {k}, got {p[k]!r}") from None
        if not np.isfinite(p[k]):
            raise ValueError(f"objects: a finite {k} expected, got {p[k]!r}")
    if not p["gap_px"] > 0:
        raise ValueError(f"objects: positive gap_px expected, got {p['gap_px']!r}")
    if not p["gap_rel"] >= 0:
        raise ValueError(f"objects: gap_rel >= 0 expected, got {p['gap_rel']!r}")
    if not isinstance(p["map"], bool):
        raise ValueError(f"objects: map True or False expected, got {p['map']!r}")
    return p


def _check_tracks(tracks, objects=None, estimator=None):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise, for ``tracks`` without
    ``objects`` (the checked dict of ``_check_objects``) or with more than ``ops.TRACK_MAX`` objects, and for an
    estimator without a motion stage (no device call)."""
    if tracks is None or tracks is False:
        return None
    if not (tracks is True or isinstance(tracks, dict)):
        raise ValueError(f"tracks: False, True or a dict of {tuple(TRACK_DEFAULTS)} expected, got {tracks!r}")
    if objects is None or objects is False:
        raise ValueError("tracks: needs objects= (the tracks are those of the objects stage's objects)")
    if getattr(estimator, "motion", None) is None:
        raise ValueError(f"tracks={tracks!r} needs an estimator with a motion stage (this one has none)")
    m = OBJECT_DEFAULTS["max_objects"] if objects is True else objects.get("max_objects", OBJECT_DEFAULTS["max_objects"])
    if m > ops.TRACK_MAX:
        raise ValueError(f"tracks: objects max_objects <= {ops.TRACK_MAX} expected, got {m!r}")
    if tracks is True:
        return dict(TRACK_DEFAULTS)
    unknown = set(tracks) - set(TRACK_DEFAULTS)
    if unknown:
        raise ValueError(f"tracks: unknown keys {sorted(unknown)}; known: {tuple(TRACK_DEFAULTS)}")
    p = dict(TRACK_DEFAULTS, **tracks)
    if not (isinstance(p["min_votes"], int) and not isinstance(p["min_votes"], bool) and p["min_votes"] >= 1):
        raise ValueError(f"tracks: an integer min_votes >= 1 expected, got {p['min_votes']!r}")
    return p


def _check_scan(scan, ground=True):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise, and for ``scan`` without
    ``ground`` (no device call)."""
    if scan is None or scan is False:
        return None
    if not (scan is True or isinstance(scan, dict)):
        raise ValueError(f"scan: False, True or a dict of {tuple(SCAN_DEFAULTS)} expected, got {scan!r}")
    if ground is None or ground is False:
        raise ValueError("scan: needs ground= (the scan is that of the ground stage's labels, in its frame)")
    if scan is True:
        return dict(SCAN_DEFAULTS)
    unknown = set(scan) - set(SCAN_DEFAULTS)
    if unknown:
        raise ValueError(f"scan: unknown keys {sorted(unknown)}; known: {tuple(SCAN_DEFAULTS)}")
    p = dict(SCAN_DEFAULTS, **scan)
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)  # noqa: E731
    for k, hi in (("beams", ops.SCAN_MAX_BEAMS), ("bins", ops.SCAN_MAX_BINS)):
        if not (is_int(p[k]) and 1 <= p[k] <= hi):
            raise ValueError(f"scan: an integer {k} in [1, {hi}] expected, got {p[k]!r}")
    if p["beams"] * p["bins"] > ops.SCAN_MAX_CELLS:
        raise ValueError(f"scan: beams * bins <= {ops.SCAN_MAX_CELLS} expected, got {p['beams']} * {p['bins']}")
    if not (is_int(p["min_pixels"]) and p["min_pixels"] >= 1):
        raise ValueError(f"scan: an integer min_pixels >= 1 expected, got {p['min_pixels']!r}")
    for k in ("range_min", "range_max"):
        try:
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError(f"scan: a number expected for {k}, got {p[k]!r}") from None
        if not np.isfinite(p[k]):
            raise ValueError(f"scan: a finite {k} expected, got {p[k]!r}")
    if not p["range_max"] > 0:
        raise ValueError(f"scan: positive range_max expected, got {p['range_max']!r}")
    if not 0 <= p["range_min"] < p["range_max"]:
        raise ValueError(f"scan: 0 <= range_min < range_max expected, got {p['range_min']!r}, {p['range_max']!r}")
    sel = p["select"]
    if isinstance(sel, str):
        sel = (sel,)
    if not (isinstance(sel, (tuple, list)) and len(sel) > 0 and all(isinstance(v, str) and v in OBJECT_LABELS for v in sel)):
        raise ValueError(f"scan: select: one or more of {tuple(OBJECT_LABELS)} expected, got {p['select']!r}")
    if "floor" in sel:
        raise ValueError("scan: select: the floor is what the beams run over, not an obstacle")
    p["select"] = tuple(sel)
    if p["angles_deg"] is not None:
        a = p["angles_deg"]
        try:
            a = tuple(float(v) for v in a)
        except (TypeError, ValueError):
            raise ValueError(f"scan: angles_deg None or two numbers expected, got {p['angles_deg']!r}") from None
        if not (len(a) == 2 and -90.0 <= a[0] < a[1] <= 90.0):  # (NaN compares false)
            raise ValueError(f"scan: angles_deg None or -90 <= min < max <= 90 expected, got {p['angles_deg']!r}")
        p["angles_deg"] = a
    return p


def _check_localmap(localmap, ground=True, egomotion=True):
    """False / None -> None; True -> the defaults; a dict overrides them.  ValueError otherwise, and for ``localmap``
    without ``ground`` or without ``egomotion`` (no device call)."""
    if localmap is None or localmap is False:
        return None
    if not (localmap is True or isinstance(localmap, dict)):
        raise ValueError(f"localmap: False, True or a dict of {tuple(LOCALMAP_DEFAULTS)} expected, got {localmap!r}")
    if ground is None or ground is False:
        raise ValueError("localmap: needs ground= (the map is built from the ground stage's labels, in its floor frame)")
    if egomotion is None or egomotion is False:
        raise ValueError("localmap: needs egomotion= (the pose is advanced by the ego stage's fit)")
    if localmap is True:
        return dict(LOCALMAP_DEFAULTS)
    unknown = set(localmap) - set(LOCALMAP_DEFAULTS)
    if unknown:
        raise ValueError(f"localmap: unknown keys {sorted(unknown)}; known: {tuple(LOCALMAP_DEFAULTS)}")
    p = dict(LOCALMAP_DEFAULTS, **localmap)
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)  # noqa: E731
    g = p["grid"]
    if not (isinstance(g, (tuple, list)) and len(g) == 2 and all(is_int(v) and 1 <= v <= ops.MAP_MAX_SIDE for v in g)
            and g[0] * g[1] <= ops.MAP_MAX_CELLS):
        raise ValueError(f"localmap: grid = (gh, gw), integers in [1, {ops.MAP_MAX_SIDE}] with gh gw <= {ops.MAP_MAX_CELLS} "
                         f"expected, got {g!r}")
    p["grid"] = (int(g[0]), int(g[1]))
    for k in ("cell", "range_min", "range_max"):
        try:
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError(f"localmap: a number expected for {k}, got {p[k]!r}") from None
        if not np.isfinite(p[k]):
            raise ValueError(f"localmap: a finite {k} expected, got {p[k]!r}")
    if not p["cell"] > 0:
        raise ValueError(f"localmap: positive cell expected, got {p['cell']!r}")
    if not p["range_max"] > 0:
        raise ValueError(f"localmap: positive range_max expected, got {p['range_max']!r}")
    if not 0 <= p["range_min"] < p["range_max"]:
        raise ValueError(f"localmap: 0 <= range_min < range_max expected, got {p['range_min']!r}, {p['range_max']!r}")
    for k, lo_, hi_ in (("min_pixels", 1, 2 ** 31 - 1), ("l_occ", 0, 32767), ("l_free", 0, 32767), ("decay", 0, 32767),
                        ("l_min", -32768, 0), ("l_max", 0, 32767), ("occ_level", -32768, 32767), ("free_level", -32768, 32767)):
        if not (is_int(p[k]) and lo_ <= p[k] <= hi_):
            raise ValueError(f"localmap: an integer {k} in [{lo_}, {hi_}] expected, got {p[k]!r}")
        p[k] = int(p[k])
    if not p["free_level"] < p["occ_level"]:
        raise ValueError(f"localmap: free_level < occ_level expected, got {p['free_level']!r}, {p['occ_level']!r}")
    sel = p["select"]
    if isinstance(sel, str):
        sel = (sel,)
    if not (isinstance(sel, (tuple, list)) and all(isinstance(v, str) and v in OBJECT_LABELS for v in sel)):
        raise ValueError(f"localmap: select: names of {tuple(OBJECT_LABELS)} expected, got {p['select']!r}")
    if "floor" in sel:
        raise ValueError("localmap: select: the floor is the free evidence, not an obstacle")
    p["select"] = tuple(sel)
    if not (isinstance(p["lost"], str) and p["lost"] in LOCALMAP_LOST):
        raise ValueError(f"localmap: lost: one of {tuple(LOCALMAP_LOST)} expected, got {p['lost']!r}")
    return p


def _check_costmap(costmap, localmap=True):
    """False / None -> None; True -> the defaults; a dict overrides them.  ``localmap``: the checked ``localmap`` dict.
    ValueError otherwise, and for ``costmap`` without ``localmap`` (no device call)."""
    if costmap is None or costmap is False:
        return None
    if not (costmap is True or isinstance(costmap, dict)):
        raise ValueError(f"costmap: False, True or a dict of {tuple(COSTMAP_DEFAULTS)} expected, got {costmap!r}")
    if localmap is None or localmap is False:
        raise ValueError("costmap: needs localmap= (the cost map is computed from the local map's cells)")
    cell = float(localmap["cell"]) if isinstance(localmap, dict) else LOCALMAP_DEFAULTS["cell"]
    unknown = set(costmap) - set(COSTMAP_DEFAULTS) if isinstance(costmap, dict) else ()
    if unknown:
        raise ValueError(f"costmap: unknown keys {sorted(unknown)}; known: {tuple(COSTMAP_DEFAULTS)}")
    p = dict(COSTMAP_DEFAULTS, **(costmap if isinstance(costmap, dict) else {}))
    for k in ("robot_radius", "inflation_radius", "scaling", "start_radius"):
        try:
            if isinstance(p[k], bool):
                raise TypeError
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError(f"costmap: a number expected for {k}, got {p[k]!r}") from None
        if not np.isfinite(p[k]):
            raise ValueError(f"costmap: a finite {k} expected, got {p[k]!r}")
    if not p["inflation_radius"] > 0:
        raise ValueError(f"costmap: positive inflation_radius expected, got {p['inflation_radius']!r}")
    if not 0 <= p["robot_radius"] <= p["inflation_radius"]:
        raise ValueError(f"costmap: 0 <= robot_radius <= inflation_radius expected, got {p['robot_radius']!r}, "
                         f"{p['inflation_radius']!r}")
    if not p["scaling"] >= 0:
        raise ValueError(f"costmap: scaling >= 0 expected, got {p['scaling']!r}")
    if not p["start_radius"] >= 0:
        raise ValueError(f"costmap: start_radius >= 0 expected, got {p['start_radius']!r}")
    for k in ("through_unknown", "nearest"):
        if not isinstance(p[k], (bool, np.bool_)):
            raise ValueError(f"costmap: a boolean expected for {k}, got {p[k]!r}")
        p[k] = bool(p[k])
    if np.ceil(p["inflation_radius"] / cell) > ops.COST_MAX_R:
        raise ValueError(f"costmap: ceil(inflation_radius / cell) <= {ops.COST_MAX_R} expected, got {p['inflation_radius']!r} / {cell!r}")
    if not (p["start_radius"] / cell) ** 2 < 2 ** 31:
        raise ValueError(f"costmap: (start_radius / cell)^2 < 2^31 expected, got {p['start_radius']!r} / {cell!r}")
    return p


def _check_goal(goal):
    """"frontier" or a finite (x, z) of the map frame -> "frontier" or (float, float).  ValueError otherwise."""
    if isinstance(goal, str) and goal == "frontier":
        return goal
    try:
        if isinstance(goal, str) or any(isinstance(v, bool) for v in goal):
            raise TypeError
        x, z = (float(v) for v in goal)
    except (TypeError, ValueError):
        raise ValueError(f'plan: goal "frontier" or (x, z) in the map frame expected, got {goal!r}') from None
    if not (np.isfinite(x) and np.isfinite(z)):
        raise ValueError(f"plan: a finite goal (x, z) expected, got {goal!r}")
    return (x, z)


def _check_plan(plan, costmap=True, localmap=True):
    """False / None -> None; True -> the defaults; a dict overrides them.  ``costmap`` and ``localmap``: the checked dicts.
    ValueError otherwise, for ``plan`` without ``costmap`` and for a grid above ``ops.PLAN_MAX_CELLS`` (no device call)."""
    if plan is None or plan is False:
        return None
    if not (plan is True or isinstance(plan, dict)):
        raise ValueError(f"plan: False, True or a dict of {tuple(PLAN_DEFAULTS)} expected, got {plan!r}")
    if costmap is None or costmap is False:
        raise ValueError("plan: needs costmap= (the plan is computed on the cost map's cost and reach)")
    grid, cell = ((localmap["grid"], float(localmap["cell"])) if isinstance(localmap, dict)
                  else (LOCALMAP_DEFAULTS["grid"], LOCALMAP_DEFAULTS["cell"]))
    if int(grid[0]) * int(grid[1]) > ops.PLAN_MAX_CELLS:
        raise ValueError(f"plan: a localmap grid of at most {ops.PLAN_MAX_CELLS} cells expected (the whole window is planned in "
                         f"the LDS of one CU), got {tuple(grid)}")
    unknown = set(plan) - set(PLAN_DEFAULTS) if isinstance(plan, dict) else ()
    if unknown:
        raise ValueError(f"plan: unknown keys {sorted(unknown)}; known: {tuple(PLAN_DEFAULTS)}")
    p = dict(PLAN_DEFAULTS, **(plan if isinstance(plan, dict) else {}))
    p["goal"] = _check_goal(p["goal"])
    try:
        if isinstance(p["goal_radius"], bool):
            raise TypeError
        p["goal_radius"] = float(p["goal_radius"])
    except (TypeError, ValueError):
        raise ValueError(f"plan: a number expected for goal_radius, got {p['goal_radius']!r}") from None
    if not (np.isfinite(p["goal_radius"]) and p["goal_radius"] >= 0 and (p["goal_radius"] / cell) ** 2 < 2 ** 31):
        raise ValueError(f"plan: finite goal_radius >= 0 with (goal_radius / cell)^2 < 2^31 expected, got {p['goal_radius']!r}")
    for k, lo, hi in (("neutral", 1, 255), ("factor", 0, 1024), ("unknown_cost", 0, 254), ("max_path", 1, 2 ** 31 - 1)):
        if isinstance(p[k], (bool, np.bool_)) or not isinstance(p[k], (int, np.integer)) or not lo <= p[k] <= hi:
            raise ValueError(f"plan: an integer in [{lo}, {hi}] expected for {k}, got {p[k]!r}")
        p[k] = int(p[k])
    if not isinstance(p["dir"], (bool, np.bool_)):
        raise ValueError(f"plan: a boolean expected for dir, got {p['dir']!r}")
    p["dir"] = bool(p["dir"])
    return p


def _check_heightmap(heightmap, localmap=True):
    """False / None -> None; True -> the defaults; a dict overrides them.  ``localmap``: the checked ``localmap`` dict.
    ValueError otherwise, and for ``heightmap`` without ``localmap`` (no device call)."""
    if heightmap is None or heightmap is False:
        return None
    if not (heightmap is True or isinstance(heightmap, dict)):
        raise ValueError(f"heightmap: False, True or a dict of {tuple(HEIGHTMAP_DEFAULTS)} expected, got {heightmap!r}")
    if localmap is None or localmap is False:
        raise ValueError("heightmap: needs localmap= (the layer lives on the local map's window and reads its pose)")
    unknown = set(heightmap) - set(HEIGHTMAP_DEFAULTS) if isinstance(heightmap, dict) else ()
    if unknown:
        raise ValueError(f"heightmap: unknown keys {sorted(unknown)}; known: {tuple(HEIGHTMAP_DEFAULTS)}")
    p = dict(HEIGHTMAP_DEFAULTS, **(heightmap if isinstance(heightmap, dict) else {}))
    for k in ("h_res", "max_step", "robot_height", "max_drop"):
        try:
            if isinstance(p[k], (bool, np.bool_)):
                raise TypeError
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError(f"heightmap: a number expected for {k}, got {p[k]!r}") from None
        if not np.isfinite(p[k]):
            raise ValueError(f"heightmap: a finite {k} expected, got {p[k]!r}")
    if not p["h_res"] > 0:
        raise ValueError(f"heightmap: positive h_res expected, got {p['h_res']!r}")
    for k in ("max_step", "robot_height", "max_drop"):
        if not 0 <= np.rint(p[k] / p["h_res"]) <= ops.HEIGHT_Q_MAX:
            raise ValueError(f"heightmap: 0 <= {k} / h_res <= {ops.HEIGHT_Q_MAX} expected, got {p[k]!r} / {p['h_res']!r}")
    for k, lo_, hi_ in (("min_pixels", 1, 2 ** 31 - 1), ("alpha", 1, 256)):
        if isinstance(p[k], (bool, np.bool_)) or not isinstance(p[k], (int, np.integer)) or not lo_ <= p[k] <= hi_:
            raise ValueError(f"heightmap: an integer {k} in [{lo_}, {hi_}] expected, got {p[k]!r}")
        p[k] = int(p[k])
    sel = p["select"]
    if isinstance(sel, str):
        sel = (sel,)
    if not (isinstance(sel, (tuple, list)) and all(isinstance(v, str) and v in OBJECT_LABELS for v in sel)):
        raise ValueError(f"heightmap: select: names of {tuple(OBJECT_LABELS)} expected, got {p['select']!r}")
    if "overhead" in sel:
        raise ValueError("heightmap: select: overhead pixels go to the ceil layer, they are not a surface")
    p["select"] = tuple(sel)
    return p


def scan_span(p, K, w):
    """(angle_min, angle_max) in radians of the checked ``scan`` dict: ``angles_deg``, or the camera's own horizontal field
    atan((0 - cx) / fx) .. atan((w - 1 - cx) / fx)."""
    if p["angles_deg"] is not None:
        return float(np.deg2rad(p["angles_deg"][0])), float(np.deg2rad(p["angles_deg"][1]))  # (90 degrees: np.pi / 2 exactly)
    fx, cx = float(K[0]), float(K[2])
    return float(np.arctan((0.0 - cx) / fx)), float(np.arctan((float(w) - 1.0 - cx) / fx))


def select_mask(names):
    """The ``select`` bit set of codd_objects for label names of ``OBJECT_LABELS``."""
    return sum({1 << OBJECT_LABELS[v] for v in names})


def _check_align(align, align_to):
    """None -> the defaults; a dict overrides them.  ValueError otherwise, and for ``align`` without ``align_to``."""
    if align is None:
        return dict(ALIGN_DEFAULTS)
    if align_to is None:
        raise ValueError("align: needs align_to=")
    if not isinstance(align, dict):
        raise ValueError(f"align: None or a dict of {tuple(ALIGN_DEFAULTS)} expected, got {align!r}")
    unknown = set(align) - set(ALIGN_DEFAULTS)
    if unknown:
        raise ValueError(f"align: unknown keys {sorted(unknown)}; known: {tuple(ALIGN_DEFAULTS)}")
    p = dict(ALIGN_DEFAULTS, **align)
    k = p["footprint"]
    if k is not None and not (isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= ops.ALIGN_MAX_FOOTPRINT):
        raise ValueError(f"align: footprint None or an integer in [1, {ops.ALIGN_MAX_FOOTPRINT}] expected, got {k!r}")
    if not isinstance(p["uv"], bool):
        raise ValueError(f"align: uv True or False expected, got {p['uv']!r}")
    return p


def check_frame(a, shape, name="frame"):
    """A C-contiguous uint8 [h,w,3] numpy array or CPU tensor, else TypeError / ValueError (no device call)."""
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise TypeError(f"{name}: a host (CPU) tensor is expected, got one on {a.device}")
        dtype_ok, contiguous, shp = a.dtype == torch.uint8, a.is_contiguous(), tuple(a.shape)
    elif isinstance(a, np.ndarray):
        dtype_ok, contiguous, shp = a.dtype == np.uint8, a.flags["C_CONTIGUOUS"], tuple(a.shape)
    else:
        raise TypeError(f"{name}: numpy array or CPU tensor expected, got {type(a).__name__}")
    if not dtype_ok:
        raise ValueError(f"{name}: dtype uint8 expected, got {a.dtype}")
    if shp != (shape[0], shape[1], 3):
        raise ValueError(f"{name}: shape {(shape[0], shape[1], 3)} expected, got {shp}")
    if not contiguous:
        raise ValueError(f"{name}: a C-contiguous array is expected")
    return a


def frame_layout(fmt, h, w, pitch=None):
    """``(rows, row_bytes, pitch, nbytes)`` of one view of an h x w frame in pixel format ``fmt``: a host frame is
    ``rows x pitch`` bytes, of which the first ``row_bytes`` of a row carry pixels (nv12: ``rows`` = 3h/2, the Y plane
    and the interleaved U V plane behind it).  ``pitch`` None is tight.  ValueError for an unknown format, a violated
    size rule (yuyv / uyvy: w even; nv12: w and h even; Bayer: h, w >= 2) or a pitch below ``row_bytes``; ``rgb8`` is
    tight only.  The same rules as codd_frame_bytes, restated here so that no library is needed to validate."""
    if fmt not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format: one of {PIXEL_FORMATS} expected, got {fmt!r}")
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError(f"shape: positive (h, w) expected, got {(h, w)}")
    if fmt in ("yuyv", "uyvy", "nv12") and w % 2:
        raise ValueError(f"{fmt}: an even width is expected, got {w}")
    if fmt == "nv12" and h % 2:
        raise ValueError(f"nv12: an even height is expected, got {h}")
    if fmt.startswith("bayer_") and (h < 2 or w < 2):
        raise ValueError(f"{fmt}: at least 2 x 2 pixels are expected, got {h} x {w}")
    row_bytes = w * {"rgb8": 3, "yuyv": 2, "uyvy": 2}.get(fmt, 1)
    if fmt == "rgb8" and pitch is not None:
        raise ValueError("pitch: not supported for rgb8 (packed 3-byte frames are tight)")
    p = row_bytes if pitch is None else int(pitch)
    if p < row_bytes:
        raise ValueError(f"pitch: at least the row's {row_bytes} bytes expected for {fmt} of width {w}, got {pitch}")
    rows = h + h // 2 if fmt == "nv12" else h
    return rows, row_bytes, p, rows * p


def check_raw_frame(a, fmt, shape, pitch=None, name="frame"):
    """A C-contiguous uint8 numpy array or CPU tensor holding one raw ``fmt`` frame: shape ``(rows, pitch)`` of
    ``frame_layout`` or, for tight yuyv / uyvy, ``(h, w, 2)``; else TypeError / ValueError (no device call)."""
    rows, _, p, _ = frame_layout(fmt, shape[0], shape[1], pitch)
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise TypeError(f"{name}: a host (CPU) tensor is expected, got one on {a.device}")
        dtype_ok, contiguous, shp = a.dtype == torch.uint8, a.is_contiguous(), tuple(a.shape)
    elif isinstance(a, np.ndarray):
        dtype_ok, contiguous, shp = a.dtype == np.uint8, a.flags["C_CONTIGUOUS"], tuple(a.shape)
    else:
        raise TypeError(f"{name}: numpy array or CPU tensor expected, got {type(a).__name__}")
    if not dtype_ok:
        raise ValueError(f"{name}: dtype uint8 expected, got {a.dtype}")
    accepted = [(rows, p)]
    if fmt in ("yuyv", "uyvy") and p == 2 * shape[1]:
        accepted.append((shape[0], shape[1], 2))
    if shp not in accepted:
        raise ValueError(f"{name}: {fmt} frame of shape {' or '.join(map(str, accepted))} expected, got {shp}")
    if not contiguous:
        raise ValueError(f"{name}: a C-contiguous array is expected")
    return a


def _check_maps(rectify, shape):
    if rectify is None:
        return None
    if len(rectify) != 2:
        raise ValueError("rectify: ((left_x, left_y), (right_x, right_y)) expected")
    out = []
    for view, pair in zip(("left", "right"), rectify):
        if pair is None:
            out.append(None)
            continue
        if len(pair) != 2 or pair[0] is None or pair[1] is None:
            raise ValueError(f"rectify: the {view} view needs both map_x and map_y")
        maps = []
        for m in pair:
            m = np.ascontiguousarray(m, dtype=np.float32)
            if m.shape != tuple(shape):
                raise ValueError(f"rectify: {view} map of shape {m.shape}, expected {tuple(shape)}")
            maps.append(m)
        out.append(tuple(maps))
    return tuple(out)


class LiveSession:
    """``step(left, right)`` is synchronous; ``push`` / ``pop`` pipeline two frames.

    Ownership: ``push`` copies both images into the session's pinned slots before it returns, so the caller may reuse
    its arrays at once; every result is a fresh numpy array owned by the caller.  At most ``DEPTH`` (2) frames are in
    flight: a further ``push`` first waits for the OLDEST frame's download and parks its result in an internal queue,
    which ``pop`` drains first -- results always come out in push order and no slot in flight is overwritten.

    ``motion`` (None, "flow2d", "flow_dd" or "sceneflow"): with a mode set, ``pop`` and ``step`` return ``(result,
    motion)``; ``motion`` is a caller-owned fp32 numpy [h,w,C] or None for a frame without a field (the first frame of a
    sequence).  The vectors live on the PREVIOUS frame's pixel grid and point to the current frame (the convention of
    RAFT-3D and of the scene-flow benchmarks): "flow2d" (C=2) optical flow in pixels; "flow_dd" (C=3) the same plus the
    change of disparity in pixels; "sceneflow" (C=3) the 3-D displacement (X, Y, Z) in the unit of ``calib`` = fx *
    baseline (metres for a metric baseline).  Pixels whose point is not in front of the camera before and after the
    motion (depth below 0.05 normalised units) are NaN in every channel.

    ``egomotion`` (False, True, or a dict overriding ``iters``, ``delta_px``, ``tau_px``, ``min_valid``): ``pop`` and
    ``step`` also return an ``Ego`` (or None for a frame without a field).  The tuple order is fixed:
    ``result[, motion][, ego][, confidence][, aligned][, epipolar][, ground][, objects][, tracks][, scan][, localmap]
    [, costmap][, plan][, heightmap]``, each part present iff requested.

    ``confidence`` (False, True, or a dict overriding ``occ_px`` (1.0 pixel) and ``tau`` (24.0 grey levels)): ``pop`` and
    ``step`` also return a ``Confidence(flags, residual)`` on the CURRENT frame's grid, for every frame (never None).  It
    needs no motion stage.

    ``pixel_format`` (one of ``PIXEL_FORMATS``; "rgb8", the default, is the packed [h,w,3] frame above, with ``bgr``):
    with a raw format a frame is a C-contiguous uint8 array or CPU tensor of ``rows x pitch`` bytes (``frame_layout``):
    mono8 and Bayer ``(h, pitch)``; yuyv / uyvy ``(h, pitch)`` or, when tight, ``(h, w, 2)``; nv12 ``(3h/2, pitch)``, the
    Y plane and the interleaved U V plane behind it.  ``pitch`` (bytes per row, None: tight) and ``yuv`` ("bt601" and
    "bt709" video range, "jpeg" full range) describe the source; ``bgr`` and ``pitch`` do not combine with the other
    family of formats (ValueError).  The decode is defined in include/codd_hip.h (codd_ingest_frames).

    ``calibration`` (a ``calibration.StereoCalibration``, a ``calibration.Rectification``, or a path to a ``.json`` /
    ``.npz`` file of either) with ``zoom``: ``shape`` is then the size of the RECTIFIED image (what the network sees and
    what every result has), frames have the calibration's source size (``src_shape``; ``pitch`` and the format's size
    rules apply to it), and ``intrinsics`` and ``calib`` are those of the rectified virtual camera -- passing either, or
    ``rectify=``, next to ``calibration`` is a ValueError.  The map is defined in include/codd_hip.h (THE MAP FUNCTION).

    ``align_to`` (a ``calibration.AlignTarget``, a path to a ``.json`` / ``.npz`` file of one, or "left" / "right", the
    rig's own physical cameras, which need ``calibration=``): ``pop`` and ``step`` also return an ``Aligned(depth, uv)``,
    for every frame (never None), last in the tuple: ``depth`` fp32 [ht,wt] on the target camera's grid (its
    ``camera.size``) in the unit of ``calib``, the nearest surface per pixel and +inf where nothing lands, whatever
    ``output`` is.  The target's pose ``X_target = R X_left + T`` starts from the physical left camera when the session
    has ``calibration=`` and from the session's own (rectified) camera otherwise, which must then have one focal length
    (``intrinsics[0] == intrinsics[1]``).  ``align`` (None or a dict overriding ``ALIGN_DEFAULTS``): ``footprint`` (1 .. 4;
    None: ``calibration.auto_footprint``, the smallest that leaves no hole lines) is the side of the square of target
    pixels each source pixel covers -- 1 leaves lines of holes where the target magnifies, more widens foreground
    edges; ``uv`` True also returns ``uv`` fp32 [h,w,2], where each pixel of the session's grid lands in the target image
    (NaN: nowhere).  ``align`` without ``align_to`` is a ValueError.  Defined in include/codd_hip.h (codd_align_depth).

    ``epipolar`` (False, True, or a dict overriding ``EPI_DEFAULTS``): ``pop`` and ``step`` also return an ``Epipolar``,
    for every frame (never None), last in the tuple: the vertical disparity the frame's own images show under the frame's
    disparity, fitted by a rotation of the right view and a focal ratio.  ``range_px`` (1 .. 4) rows are searched either
    way at every ``step``-th (1 .. 8) column and row; a pixel counts when its best match costs at most ``tau`` grey levels
    per pixel and the cost's curvature across rows exceeds ``min_curv``; ``iters`` (1 .. 32) re-weighted steps with the
    Cauchy scale ``delta_px``; fewer than ``min_valid`` pixels make ``ok`` False; ``map`` True also returns the per-pixel
    ``dy``.  It needs no motion stage and no ``calibration=``.  Defined in include/codd_hip.h (codd_epipolar_check).

    ``ground`` (False, True, or a dict overriding ``GROUND_DEFAULTS``): ``pop`` and ``step`` also return a ``Ground``, for
    every frame (never None), last in the tuple: the floor plane fitted to the frame's disparity (``coef``, ``normal``,
    ``camera_height``), per-pixel ``labels`` (0 floor, 1 obstacle, 2 overhead, 3 below, 255 invalid) and, on request, the
    per-pixel ``height`` above the floor (``map`` True) and a top-down obstacle grid (``grid`` (gh, gw) cells of ``cell``
    units; row 0 under the camera, rows forward, column gw / 2 straight ahead).  The fit runs over every ``step``-th (1 .. 8)
    column and row in ``iters`` (1 .. 32) re-weighted steps whose Cauchy scale anneals from ``delta0_px`` to ``delta_px``
    and is ``asym`` times tighter above the plane than below it, so that the floor is the lower envelope; ``height``
    (the camera's mounting height) with ``pitch_deg`` (positive: looking down) and ``up`` seeds it (``ground_seed``),
    without it the first step takes the lower half of the image; fewer than ``min_valid`` fit pixels or inliers, or a
    plane tilted by more than ``max_tilt_deg`` against the pitched ``up``, make ``ok`` False -- then no pixel is labelled.
    A pixel within ``tol_px`` of disparity or ``ground_tol`` of height of the plane is floor; above it, up to
    ``clearance``, an obstacle.  Heights are in the unit of ``calib`` / fx.  It needs no motion stage and no
    ``calibration=``; it uses the session's ``intrinsics`` and ``calib``.  Defined in include/codd_hip.h (codd_ground_plane).

    ``objects`` (False, True, or a dict overriding ``OBJECT_DEFAULTS``; needs ``ground``, ValueError without): ``pop`` and
    ``step`` also return an ``Objects``, for every frame (never None), last in the tuple: the connected components of the
    pixels whose label is one of ``select`` (names of ``OBJECT_LABELS``; by default the obstacles), two 4-neighbours being
    joined when their disparities differ by at most ``max(gap_px, gap_rel * the smaller one)``.  A component with at least
    ``min_pixels`` pixels whose top is at least ``min_height`` above the floor is an object; objects are numbered in
    raster order of their first pixel and the first ``max_objects`` (1 .. 4096) are returned (``found`` > ``n``: there were
    more).  Per object: ``pixels``, the image ``box``, the nearest pixel ``near_px``, the ``extent`` in the ground grid's
    frame, the ``height`` range above the floor and the ``disparity`` range; ``map`` True also returns ``ids`` uint16
    [h,w], the object number of every pixel (0xFFFF: none).  A frame without a floor has no objects.  Defined in
    include/codd_hip.h (codd_objects).

    ``tracks`` (False, True, or a dict overriding ``TRACK_DEFAULTS``; needs ``objects`` with ``max_objects`` <= 1024 and an
    estimator with a motion stage, ValueError without): ``pop`` and ``step`` also return a ``Tracks``, for every frame
    (never None), last in the tuple; its rows belong to the rows of the frame's ``Objects``.  Every pixel of a previous
    object is carried by the frame's SE3 field onto this frame's objects and votes; object b continues the track of the
    previous object a iff each is the other's best match and at least ``min_votes`` pixels say so, so that a split or a
    merge leaves the id with the larger part; every other object starts a track with a new id.  ``motion`` is the mean
    3-D displacement of the previous object's pixels in the unit of ``calib`` and, with ``egomotion``, ``own`` is what is
    left after the camera's motion and ``moving`` counts the pixels of the ego stage's mask.  On a frame without a
    field (the first of a sequence) every object starts a track; ``reset()`` also restarts the ids at 1.  It needs
    neither ``motion=`` nor ``egomotion=``.  Defined in include/codd_hip.h (codd_track_objects).

    ``scan`` (False, True, or a dict overriding ``SCAN_DEFAULTS``; needs ``ground``, ValueError without): ``pop`` and
    ``step`` also return a ``Scan``, for every frame (never None), last in the tuple: a planar range scan of ``beams``
    (1 .. 2048) equal beams over ``angles_deg`` = (min, max) degrees from the ground grid's forward axis, positive to the
    right, within -90 .. 90 (None: the camera's own horizontal field).  Every floor pixel and every pixel labelled one of
    ``select`` (names of ``OBJECT_LABELS`` other than the floor) with a range in [``range_min``, ``range_max``) on the floor
    falls into one of ``bins`` (1 .. 1024; beams * bins <= 2^20) range bins of its beam; the first bin with at least
    ``min_pixels`` obstacle pixels is the hit -- a lone speckle nearer than that does not stop the beam -- and ``ranges``
    is the range of its nearest pixel; ``free`` says how far floor was seen in front of it.  With ``objects`` the hit names
    its object, with ``tracks`` its track.  A frame without a floor has only unknown beams.  Defined in include/codd_hip.h
    (codd_range_scan).

    ``localmap`` (False, True, or a dict overriding ``LOCALMAP_DEFAULTS``; needs ``ground`` and ``egomotion``, ValueError
    without either): ``pop`` and ``step`` also return a ``LocalMap``, for every frame (never None), last in the tuple: a
    rolling occupancy map of ``grid`` = (gh, gw) cells of ``cell`` units, centred on the camera's cell and moving by whole
    cells, in the floor frame of the first integrated frame (it never rotates).  The pose advances by the ego stage's fit,
    levelled by each frame's own floor normal.  Every floor pixel and every pixel labelled one of ``select`` with a range
    in [``range_min``, ``range_max``) on the floor falls into a cell; a cell with ``min_pixels`` obstacle pixels gains
    ``l_occ`` (up to ``l_max``), else one with ``min_pixels`` floor pixels loses ``l_free`` (down to ``l_min``), every
    other cell ages and moves ``decay`` towards 0.  ``occ_level`` and ``free_level`` are the levels of
    ``LocalMap.state()`` and of the counts.  ``lost`` says what a frame does whose pose cannot be advanced (no field, an
    ego fit that failed): ``"reset"`` starts a new map there, ``"hold"`` keeps map and pose as if the camera stood still.
    The first frame of a sequence starts a new map.  The defaults are reasoned, not measured on real footage.  Moving
    things are not excluded; free evidence and ``decay`` erase them.  Defined in include/codd_hip.h (codd_local_map).

    ``costmap`` (False, True, or a dict overriding ``COSTMAP_DEFAULTS``; needs ``localmap``, ValueError without it): ``pop``
    and ``step`` also return a ``CostMap`` of the frame's ``LocalMap``, for every frame (never None), last in the tuple.
    Per cell: ``dist2``, the squared distance in cells to the nearest occupied cell within ``inflation_radius``; ``cost`` in
    the convention of ROS costmap_2d -- 254 on an occupied cell, 253 within ``robot_radius`` of one, 252 exp(-``scaling``
    (distance - ``robot_radius``)) (at least 1) out to ``inflation_radius``, 0 beyond, 255 on a cell that is neither
    occupied nor free and not inscribed --; ``reach``, whether a robot at the camera's cell gets there over 4-neighbour
    steps through free cells of cost below 253 (and unknown ones with ``through_unknown``), and whether the cell is a
    frontier.  The cells within ``start_radius`` of the camera count as traversable unless occupied: the camera never
    sees the floor under itself.  ``nearest`` also returns the nearest occupied cell's index.  The defaults are
    reasoned, not measured on real footage.  Defined in include/codd_hip.h (codd_cost_map).

    ``plan`` (False, True, or a dict overriding ``PLAN_DEFAULTS``; needs ``costmap``, ValueError without it and for a
    ``localmap`` grid above ``ops.PLAN_MAX_CELLS`` cells): ``pop`` and ``step`` also return a ``Plan`` on the frame's
    ``CostMap``, for every frame (never None), last in the tuple.  ``goal`` is ``"frontier"`` (the frontier nearest to the
    camera, for exploring) or a point ``(x, z)`` of the map frame, which is clamped into the window when it lies outside;
    ``set_goal`` changes it for the frames pushed afterwards.  The goal set is the reachable cells within ``goal_radius``
    of the goal cell, or the reachable cell nearest to it when there are none.  ``potential`` is the least cost from every
    reachable cell to the goal set over 8-neighbour moves that cut no corner, a step of length 5 (straight) or 7
    (diagonal) into a cell costing ``neutral`` + ``factor`` cost / 256 (``unknown_cost`` for cost 255); ``path`` the cells
    from the camera's cell to the goal, at most ``max_path``; ``dir`` also returns the move to make at every cell.  The
    defaults are navfn's and are reasoned, not measured on real footage.  Defined in include/codd_hip.h (codd_plan).

    ``heightmap`` (False, True, or a dict overriding ``HEIGHTMAP_DEFAULTS``; needs ``localmap``, ValueError without it and
    for ``"overhead"`` in ``select``): ``pop`` and ``step`` also return a ``HeightMap`` on the frame's ``LocalMap`` cells,
    for every frame (never None), last in the tuple, after the ``Plan``.  ``codd_height_map`` runs right behind
    ``codd_local_map`` and keeps, per cell and across frames, the highest and the lowest surface seen (``top``, ``bot``)
    and the lowest overhead thing (``ceil``) in units of ``h_res`` above the floor plane of the frame that saw them: a
    blend ``alpha`` / 256 of the way to each frame's extreme over the pixels of the ``select`` labels (overhead pixels
    for ``ceil``), for cells with at least ``min_pixels`` of them.  ``flags`` marks the upper cell of a step above
    ``max_step``, a cell with less than ``robot_height`` between ``top`` and ``ceil``, and a cell whose ``bot`` lies more
    than ``max_drop`` below the floor; ``traversable()`` is ``flags == 0``.  The layers restart with the map (``reset``, a
    LOST frame under ``lost="reset"``).  The defaults are reasoned, not measured on real footage.  Defined in
    include/codd_hip.h (codd_height_map).
    """

    def __init__(self, estimator, shape, intrinsics=None, calib=None, output="depth",
                 bgr=False, rectify=None, use_graph=True, divisor=64, motion=None, egomotion=False, confidence=False,
                 pixel_format="rgb8", yuv="bt601", pitch=None, calibration=None, zoom=1.0, align_to=None, align=None,
                 epipolar=False, ground=False, objects=False, tracks=False, scan=False, localmap=False,
                 costmap=False, plan=False, heightmap=False):
        if output not in OUTPUTS:
            raise ValueError(f"output: one of {OUTPUTS} expected, got {output!r}")
        if motion is not None and motion not in MOTIONS:
            raise ValueError(f"motion: None or one of {MOTIONS} expected, got {motion!r}")
        if motion is not None and getattr(estimator, "motion", None) is None:
            raise ValueError(f"motion={motion!r} needs an estimator with a motion stage (this one has none)")
        self.ego = _check_ego(egomotion)
        if self.ego is not None and getattr(estimator, "motion", None) is None:
            raise ValueError(f"egomotion={egomotion!r} needs an estimator with a motion stage (this one has none)")
        self.conf = _check_conf(confidence)
        self.epi = _check_epi(epipolar)
        self.ground = _check_ground(ground)
        self.objects = _check_objects(objects, self.ground)
        self.tracks = _check_tracks(tracks, self.objects, estimator)
        self.scan = _check_scan(scan, self.ground)
        self.localmap = _check_localmap(localmap, self.ground, self.ego)
        self.costmap = _check_costmap(costmap, self.localmap)
        self.plan = _check_plan(plan, self.costmap, self.localmap)
        self.heightmap = _check_heightmap(heightmap, self.localmap)
        h, w = int(shape[0]), int(shape[1])
        if h <= 0 or w <= 0:
            raise ValueError(f"shape: positive (h, w) expected, got {shape}")
        if yuv not in YUVS:
            raise ValueError(f"yuv: one of {YUVS} expected, got {yuv!r}")
        self.rect = None
        if calibration is not None:
            for name, given in (("intrinsics", intrinsics), ("calib", calib), ("rectify", rectify)):
                if given is not None:
                    raise ValueError(f"{name}: not together with calibration= (the rectification provides it)")
            self.rect = _calibration.resolve(calibration, (h, w), zoom)
            intrinsics, calib = self.rect.intrinsics, self.rect.calib
            self._calib_views = ops.calib_structs(self.rect)  # (ctypes structs: no device call)
        elif float(zoom) != 1.0:
            raise ValueError("zoom: needs calibration=")
        intrinsics = DEFAULT_INTRINSICS if intrinsics is None else intrinsics
        calib = DEFAULT_CALIB if calib is None else calib
        self.align = _check_align(align, align_to)
        self.align_target = None
        if align_to is not None:
            self.align_target = _calibration.AlignTarget.resolve(align_to, self.rect)
            if float(intrinsics[0]) != float(intrinsics[1]):
                raise ValueError(f"align_to: the session's camera must have one focal length (fx == fy), got intrinsics "
                                 f"{tuple(intrinsics)}")
            self._align_K = tuple(float(v) for v in intrinsics)
            self._align_view = ops.align_view(self.align_target, self.rect)  # (a ctypes struct: no device call)
            if self.align["footprint"] is None:
                R = np.array(self._align_view.R[:], np.float64).reshape(3, 3)
                self.align["footprint"] = _calibration.auto_footprint(R, self.align_target.camera, (h, w), self._align_K,
                                                                      r2_max=self._align_view.r2_max)
        self._epi_K = tuple(float(v) for v in intrinsics)
        if self.ground is not None:
            g = self.ground
            self._ground_up = tuple(_unit_up(g["up"], g["pitch_deg"]))  # (the mount's pitch turns the expected normal too)
            self._ground_seed = None if g["height"] is None else ground_seed(g["height"], self._epi_K, calib, g["up"],
                                                                             g["pitch_deg"])
            self._ground_par = {k: g[k] for k in ops.GROUND_PARAMS}
        if self.objects is not None:
            self._objects_par = dict({k: self.objects[k] for k in ops.OBJECT_PARAMS}, select=select_mask(self.objects["select"]))
        if self.scan is not None:
            sc = self.scan
            lo, hi = scan_span(sc, self._epi_K, w)
            self._scan_edges_host = ops.scan_edges(sc["beams"], lo, hi)  # (numpy: no device call; ValueError for an empty span)
            self._scan_meta = (lo, (hi - lo) / sc["beams"], sc["range_min"], sc["range_max"])
            self._scan_par = dict(range_min=sc["range_min"], range_max=sc["range_max"], bins=sc["bins"],
                                  select=select_mask(sc["select"]), min_pixels=sc["min_pixels"])
        if self.localmap is not None:
            lm = self.localmap
            self._map_par = dict({k: lm[k] for k in ops.MAP_PARAMS if k not in ("select", "lost")},
                                 select=select_mask(lm["select"]), lost=LOCALMAP_LOST[lm["lost"]])
        if self.costmap is not None:
            cm, (gh, gw) = self.costmap, self.localmap["grid"]
            self._cost_R, self._cost_lut_host = ops.cost_lut(self.localmap["cell"], cm["robot_radius"], cm["inflation_radius"],
                                                             cm["scaling"])
            self._cost_start = (gw // 2, gh // 2)  # the camera's cell, by the definition of ix0 and iz0
            self._cost_par = dict(occ_level=self.localmap["occ_level"], free_level=self.localmap["free_level"],
                                  seed_r2=int(np.floor((cm["start_radius"] / self.localmap["cell"]) ** 2)),
                                  through_unknown=cm["through_unknown"])
        if self.plan is not None:
            pl = self.plan
            self._plan_goal = pl["goal"]
            self._plan_par = dict(goal_r2=int(np.floor((pl["goal_radius"] / self.localmap["cell"]) ** 2)), neutral=pl["neutral"],
                                  factor=pl["factor"], unknown_cost=pl["unknown_cost"])
        if self.heightmap is not None:
            hm = self.heightmap
            self._height_par = dict({k: hm[k] for k in ops.HEIGHT_PARAMS if k != "select"}, select=select_mask(hm["select"]),
                                    **{k: self.localmap[k] for k in ("cell", "range_min", "range_max")})
        self.src_shape = (h, w) if self.rect is None else self.rect.size  # the size of a frame as the camera hands it out
        # (rows, row_bytes, pitch, nbytes) of a source frame; ValueError if invalid
        self._layout = frame_layout(pixel_format, self.src_shape[0], self.src_shape[1], pitch)
        if pixel_format != "rgb8" and bgr:
            raise ValueError(f"bgr=True is for rgb8 frames only (pixel_format={pixel_format!r} names its own byte order)")
        self.pixel_format, self.yuv, self.pitch = pixel_format, yuv, None if pitch is None else int(pitch)
        self.est, self.shape, self.output, self.bgr, self.calib = estimator, (h, w), output, bool(bgr), float(calib)
        self.padded = (-(-h // divisor) * divisor, -(-w // divisor) * divisor)
        self._maps_host = _check_maps(rectify, (h, w))
        # one sample's img_metas (the list the estimator's inference() is handed): [dict]
        self.metas = synth.default_metas(*self.padded, img_shape=(h, w, 3), intrinsics=tuple(intrinsics))[0]
        self.metas[0]["calib"] = self.calib
        self.motion = motion
        self._world = np.eye(4)  # camera_to_world of the last collected frame
        if motion is not None or self.ego is not None or self.tracks is not None:
            from .motion import Motion
            self._K = [float(np.float32(v)) for v in self.metas[0]["intrinsics"]]  # as Motion.forward passes them
            self._bf = Motion._bf(self.metas)
        self.runner = FrameRunner(estimator, self.metas, use_graph=use_graph)
        self._open_done = False
        self._pushed = 0
        self._track_fresh = True  # the next frame is the first of a sequence for the tracks' state
        self._map_fresh = True  # and for the local map's
        self._inflight = deque()  # slots, oldest first
        self._ready = deque()  # results popped on the caller's behalf by a push that found the pipeline full

    # ---- one-time allocation ------------------------------------------------------------------------
    def _open(self):
        dev = next(self.est.parameters()).device
        if dev.type != "cuda":
            raise _abi.CoddHipError("LiveSession needs an estimator on a ROCm device (no CPU fallback in the product path)")
        _abi.load()
        h, w = self.shape
        H, W = self.padded
        self.dev = dev
        odt = torch.int16 if self.output == "disp_u16" else torch.float32  # (uint16 bits; handed out as numpy uint16)
        with torch.cuda.device(dev):
            # rgb8: [h,w,3]; a raw format: the frame's bytes, flat (frame_layout: rows x pitch)
            slot = self.src_shape + (3,) if self.pixel_format == "rgb8" else (self._layout[3],)
            self._h_in = [[torch.empty(slot, dtype=torch.uint8, pin_memory=True) for _ in range(2)] for _ in range(DEPTH)]
            self._d_in = [[torch.empty(slot, dtype=torch.uint8, device=dev) for _ in range(2)] for _ in range(DEPTH)]
            self._scratch = tuple(torch.empty(1, 3, H, W, dtype=torch.float32, device=dev) for _ in range(2))
            self._maps = None
            if self._maps_host is not None:
                self._maps = tuple(None if p is None else tuple(torch.from_numpy(m).to(dev) for m in p)
                                   for p in self._maps_host)
            self._d_out = torch.empty(h, w, dtype=odt, device=dev)
            self._h_out = [torch.empty(h, w, dtype=odt, pin_memory=True) for _ in range(DEPTH)]
            if self.motion is not None or self.ego is not None or self.tracks is not None:
                self._depth_prev = torch.zeros(H, W, dtype=torch.float32, device=dev)  # (rolled before it is ever read)
            if self.ego is not None:
                self._d_ego = (torch.zeros(16, dtype=torch.float32, device=dev),
                               torch.empty(h, w, dtype=torch.uint8, device=dev),
                               torch.empty(h, w, dtype=torch.float32, device=dev))
                self._h_ego = [(torch.empty(16, dtype=torch.float32, pin_memory=True),
                                torch.empty(h, w, dtype=torch.uint8, pin_memory=True),
                                torch.empty(h, w, dtype=torch.float32, pin_memory=True)) for _ in range(DEPTH)]
                self._ego_scratch = torch.empty(ops.ego_motion_scratch(h, w), dtype=torch.uint8, device=dev)
                self._has_ego = [False] * DEPTH
            if self.motion is not None:
                ch = ops.MOTION_CHANNELS[self.motion]
                self._d_mot = torch.empty(h, w, ch, dtype=torch.float32, device=dev)
                self._h_mot = [torch.empty(h, w, ch, dtype=torch.float32, pin_memory=True) for _ in range(DEPTH)]
                self._has_mot = [False] * DEPTH
            if self.conf is not None:
                self._d_conf = (torch.empty(h, w, dtype=torch.uint8, device=dev),
                                torch.empty(h, w, dtype=torch.float32, device=dev))
                self._h_conf = [(torch.empty(h, w, dtype=torch.uint8, pin_memory=True),
                                 torch.empty(h, w, dtype=torch.float32, pin_memory=True)) for _ in range(DEPTH)]
            if self.align_target is not None:
                shapes = (self.align_target.camera.size,) + (((h, w, 2),) if self.align["uv"] else ())
                self._d_align = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in shapes)
                self._h_align = [tuple(torch.empty(s, dtype=torch.float32, pin_memory=True) for s in shapes)
                                 for _ in range(DEPTH)]
            if self.epi is not None:
                self._d_epi = (torch.zeros(32, dtype=torch.float64, device=dev),) + (
                    (torch.empty(h, w, dtype=torch.float32, device=dev),) if self.epi["map"] else ())
                self._h_epi = [tuple(torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_epi)
                               for _ in range(DEPTH)]
                self._epi_scratch = torch.empty(ops.epipolar_scratch(h, w), dtype=torch.uint8, device=dev)
            if self.ground is not None:
                grid = self.ground["grid"]
                self._d_ground = [torch.zeros(32, dtype=torch.float64, device=dev),
                                  torch.empty(h, w, dtype=torch.uint8, device=dev)]
                if self.ground["map"]:
                    self._d_ground.append(torch.empty(h, w, dtype=torch.float32, device=dev))
                if grid is not None:
                    self._d_ground += [torch.empty((2,) + grid, dtype=torch.int32, device=dev),
                                       torch.empty(grid, dtype=torch.float32, device=dev)]
                self._h_ground = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_ground]
                                  for _ in range(DEPTH)]
                self._ground_scratch = torch.empty(ops.ground_scratch(h, w, grid), dtype=torch.uint8, device=dev)
            if self.objects is not None:
                m = self.objects["max_objects"]
                self._d_objects = [torch.zeros(4, dtype=torch.int32, device=dev),
                                   torch.zeros(m, 8, dtype=torch.int32, device=dev),
                                   torch.zeros(m, 8, dtype=torch.float32, device=dev)]
                if self.objects["map"]:
                    self._d_objects.append(torch.empty(h, w, dtype=torch.uint16, device=dev))
                elif self.tracks is not None or self.scan is not None:  # (read on the device; it is not downloaded)
                    self._track_ids = torch.empty(h, w, dtype=torch.uint16, device=dev)
                self._h_objects = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_objects]
                                   for _ in range(DEPTH)]
                self._objects_scratch = torch.empty(ops.objects_scratch(h, w, m), dtype=torch.uint8, device=dev)
            if self.tracks is not None:
                m = self.objects["max_objects"]
                self._d_tracks = [torch.zeros(4, dtype=torch.int32, device=dev),
                                  torch.zeros(m, 8, dtype=torch.int32, device=dev),
                                  torch.zeros(m, 8, dtype=torch.float32, device=dev)]
                self._h_tracks = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_tracks]
                                  for _ in range(DEPTH)]
                self._track_state = torch.zeros(ops.track_state_bytes(h, w, m), dtype=torch.uint8, device=dev)
                self._track_scratch = torch.empty(ops.track_scratch(h, w, m), dtype=torch.uint8, device=dev)
            if self.scan is not None:
                beams = self.scan["beams"]
                self._d_scan = [torch.zeros(4, dtype=torch.int32, device=dev),
                                torch.zeros(beams, 4, dtype=torch.int32, device=dev),
                                torch.zeros(beams, 4, dtype=torch.float32, device=dev)]
                self._h_scan = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_scan]
                                for _ in range(DEPTH)]
                self._scan_edges = torch.from_numpy(self._scan_edges_host).to(dev)
                self._scan_scratch = torch.empty(ops.range_scan_scratch(beams, self.scan["bins"]), dtype=torch.uint8, device=dev)
            if self.localmap is not None:
                gh, gw = self.localmap["grid"]
                self._d_map = [torch.zeros(16, dtype=torch.float64, device=dev), torch.zeros(gh, gw, dtype=torch.int16, device=dev),
                               torch.zeros(gh, gw, dtype=torch.uint8, device=dev)]  # record, map_out, age_out
                self._h_map = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_map]
                               for _ in range(DEPTH)]
                self._map_state = [torch.zeros(32, dtype=torch.float64, device=dev), torch.zeros(gh, gw, dtype=torch.int16, device=dev),
                                   torch.full((gh, gw), 255, dtype=torch.uint8, device=dev)]  # state, logodds, age
                self._map_scratch = torch.empty(ops.local_map_scratch(gh, gw), dtype=torch.uint8, device=dev)
            if self.costmap is not None:
                gh, gw = self.localmap["grid"]
                self._d_cost = [torch.zeros(16, dtype=torch.float64, device=dev), torch.zeros(gh, gw, dtype=torch.int32, device=dev),
                                torch.zeros(gh, gw, dtype=torch.uint8, device=dev), torch.zeros(gh, gw, dtype=torch.uint8, device=dev)]
                if self.costmap["nearest"]:  # record, dist2, cost, reach[, nearest]
                    self._d_cost.append(torch.zeros(gh, gw, dtype=torch.int32, device=dev))
                self._h_cost = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_cost]
                                for _ in range(DEPTH)]
                self._cost_lut = torch.from_numpy(self._cost_lut_host).to(dev)
                self._cost_scratch = torch.empty(ops.cost_map_scratch(gh, gw, self._cost_R), dtype=torch.uint8, device=dev)
            if self.plan is not None:
                gh, gw = self.localmap["grid"]  # record, potential (the bits of a uint32), path[, dir]
                self._d_plan = [torch.zeros(16, dtype=torch.float64, device=dev), torch.zeros(gh, gw, dtype=torch.int32, device=dev),
                                torch.full((self.plan["max_path"],), -1, dtype=torch.int32, device=dev)]
                if self.plan["dir"]:
                    self._d_plan.append(torch.zeros(gh, gw, dtype=torch.uint8, device=dev))
                self._h_plan = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_plan]
                                for _ in range(DEPTH)]
                self._plan_scratch = torch.empty(ops.plan_scratch(gh, gw), dtype=torch.uint8, device=dev)
            if self.heightmap is not None:
                gh, gw = self.localmap["grid"]  # record, top_out, bot_out, ceil_out, hage_out, step_out, flags_out
                i16, u8 = torch.int16, torch.uint8
                self._d_height = [torch.zeros(16, dtype=torch.float64, device=dev)] + [
                    torch.zeros(gh, gw, dtype=dt, device=dev) for dt in (i16, i16, i16, u8, torch.uint16, u8)]
                self._h_height = [[torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in self._d_height]
                                  for _ in range(DEPTH)]
                # top, bot, ceil, hage: the map's first call is CLEARED and gives every cell its sentinels
                self._height_state = [torch.zeros(gh, gw, dtype=dt, device=dev) for dt in (i16, i16, i16, u8)]
                self._height_scratch = torch.empty(ops.height_map_scratch(gh, gw), dtype=torch.uint8, device=dev)
            self._s_up, self._s_down = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
            ev = lambda: [torch.cuda.Event() for _ in range(DEPTH)]  # noqa: E731
            self._e_up, self._e_ingest, self._e_export, self._e_down = ev(), ev(), ev(), ev()
        self._open_done = True

    # ---- pipeline -----------------------------------------------------------------------------------
    def push(self, left_u8, right_u8):
        """Enqueue one frame.  Returns once both images sit in the session's pinned slot."""
        raw = self.pixel_format != "rgb8"
        for a, name in ((left_u8, "left"), (right_u8, "right")):
            if raw:
                check_raw_frame(a, self.pixel_format, self.src_shape, self.pitch, name)
            else:
                check_frame(a, self.src_shape, name)
        if not self._open_done:
            self._open()
        if len(self._inflight) == DEPTH:
            self._ready.append(self._collect())
        k = self._pushed % DEPTH
        first_use = self._pushed < DEPTH
        if not first_use:
            self._e_up[k].synchronize()  # the slot's previous upload has left the pinned memory
        with torch.cuda.device(self.dev), torch.no_grad():
            compute = torch.cuda.current_stream(self.dev)
            with torch.cuda.stream(self._s_up):
                if not first_use:
                    self._s_up.wait_event(self._e_ingest[k])  # the slot's previous frame has been read by its ingest
                # view by view: the left image's upload runs while the host copies the right one into its slot
                for dev_slot, host_slot, src in zip(self._d_in[k], self._h_in[k], (left_u8, right_u8)):
                    if raw:
                        src = src.reshape(-1)  # (C-contiguous: a view)
                    if isinstance(src, torch.Tensor):
                        host_slot.copy_(src)
                    else:
                        np.copyto(host_slot.numpy(), src)
                    dev_slot.copy_(host_slot, non_blocking=True)
                self._e_up[k].record(self._s_up)
            compute.wait_event(self._e_up[k])

            images = []  # (emptied per frame: a fill that is skipped cannot leave the previous frame's buffers here)

            def fill(left, right):
                images[:] = (left, right)  # (the frame's normalised images: export_confidence and epipolar_check read them)
                if self.rect is not None:
                    ops.ingest_calibrated(self._d_in[k][0], self._d_in[k][1], left, right, self._calib_views,
                                          self.pixel_format, self.src_shape, self.shape, bgr=self.bgr, yuv=self.yuv,
                                          pitch=self.pitch)
                elif raw:
                    ops.ingest_frames(self._d_in[k][0], self._d_in[k][1], left, right, self.pixel_format, self.shape,
                                      yuv=self.yuv, pitch=self.pitch, maps=self._maps)
                else:
                    ops.ingest_pair(self._d_in[k][0], self._d_in[k][1], left, right, bgr=self.bgr, maps=self._maps)
                self._e_ingest[k].record(compute)

            disp = self.runner.step_fill(fill, self._scratch)
            if self._pushed > 0:
                compute.wait_event(self._e_down[(self._pushed - 1) % DEPTH])  # one device staging buffer
            ops.export_depth(disp, self._d_out, mode=self.output, calib=self.calib)
            if self.align_target is not None:
                ops.align_depth(disp, self.shape, self._align_K, self.calib, self._align_view, self.align_target.camera.size,
                                self.align["footprint"], self._d_align[0], self._d_align[1] if self.align["uv"] else None)
            if self.conf is not None:
                # step_fill calls fill exactly once per frame, on every path: the buffers it was handed are this frame's
                assert len(images) == 2, "FrameRunner.step_fill did not call fill(left, right)"
                ops.export_confidence(disp, self._d_conf[0], self._d_conf[1], images[0], images[1], **self.conf)
            if self.epi is not None:
                assert len(images) == 2, "FrameRunner.step_fill did not call fill(left, right)"
                ops.epipolar_check(disp, images[0], images[1], self._epi_K, self.shape, self._d_epi[0],
                                   self._d_epi[1] if self.epi["map"] else None, scratch=self._epi_scratch,
                                   **{k: v for k, v in self.epi.items() if k != "map"})
            if self.ground is not None:
                ops.ground_plane(disp, self._epi_K, self.calib, self.shape, *self._ground_bufs(self._d_ground),
                                 scratch=self._ground_scratch, seed=self._ground_seed, up=self._ground_up,
                                 **self._ground_par)
            if self.objects is not None:
                ops.objects(disp, self._epi_K, self.calib, self.shape, self._d_ground[1], self._d_ground[0],
                            *self._d_objects[:3], ids=self._object_ids(), scratch=self._objects_scratch,
                            **self._objects_par)
            if self.scan is not None:
                ops.range_scan(disp, self._epi_K, self.calib, self.shape, self._d_ground[1], self._d_ground[0],
                               self._scan_edges, *self._d_scan, ids=None if self.objects is None else self._object_ids(),
                               scratch=self._scan_scratch, **self._scan_par)
            Ts = None
            if self.motion is not None or self.ego is not None or self.tracks is not None:
                Ts = self.runner.last.get("Ts")  # None: the frame has no field (first of a sequence) -- roll only
            if self.ego is not None:
                if Ts is not None:  # (before export_motion rolls the depth map the field refers to)
                    rec, mov, res = self._d_ego
                    ops.ego_motion(Ts, self._depth_prev, self._K, self.shape, rec, mov, res, scale=self.calib / self._bf,
                                   scratch=self._ego_scratch, **self.ego)
                self._has_ego[k] = Ts is not None
            if self.localmap is not None:  # (after the ground stage and the ego fit whose records it reads on the device)
                ops.local_map(disp, self._epi_K, self.calib, self.shape, self._d_ground[1], self._d_ground[0],
                              self._d_ego[0] if Ts is not None else None, *self._map_state, self._d_map[1], self._d_map[2],
                              self._d_map[0], fresh=self._map_fresh, scratch=self._map_scratch, **self._map_par)
                self._map_fresh = False
                if self.heightmap is not None:  # (right behind the map: it reads the pose and the window that call left)
                    ops.height_map(disp, self._epi_K, self.calib, self.shape, self._d_ground[1], self._d_ground[0],
                                   self._map_state[0], *self._height_state, *self._d_height[1:], self._d_height[0],
                                   scratch=self._height_scratch, **self._height_par)
                if self.costmap is not None:  # (on the unrolled map and age plane the call above left on the device)
                    ops.cost_map(self._d_map[1], self._d_map[2], self._cost_lut, self._cost_R, self._cost_start, self._d_cost[1],
                                 self._d_cost[4] if self.costmap["nearest"] else None, self._d_cost[2], self._d_cost[3],
                                 self._d_cost[0], scratch=self._cost_scratch, **self._cost_par)
                if self.plan is not None:  # (on the cost, reach and records the two calls above left on the device)
                    goal = self._plan_goal
                    ops.plan(self._d_cost[2], self._d_cost[3], self._cost_start, self._d_plan[1], self._d_plan[2], self._d_plan[0],
                             dir=self._d_plan[3] if self.plan["dir"] else None,
                             goal=goal if goal == "frontier" else ("world",) + goal, cost_record=self._d_cost[0],
                             map_record=self._d_map[0], cell=self.localmap["cell"], scratch=self._plan_scratch, **self._plan_par)
            if self.tracks is not None:  # (after the ego fit it reads, before export_motion rolls the depth map)
                with_ego = self.ego is not None and Ts is not None
                ops.track_objects(Ts, self._depth_prev, self._K, self.shape, self._object_ids(), self._d_objects[0],
                                  self._track_state, *self._d_tracks, scratch=self._track_scratch,
                                  ego_record=self._d_ego[0] if with_ego else None,
                                  moving=self._d_ego[1] if with_ego else None, scale=self.calib / self._bf,
                                  fresh=self._track_fresh, min_votes=self.tracks["min_votes"],
                                  max_objects=self.objects["max_objects"])
                self._track_fresh = False
            if self.motion is not None:
                ops.export_motion(Ts, disp, self._depth_prev, self._d_mot, self.motion, self._K, self._bf,
                                  scale=self.calib / self._bf)
                self._has_mot[k] = Ts is not None
            elif self.ego is not None or self.tracks is not None:
                ops.export_motion(None, disp, self._depth_prev, None, "sceneflow", self._K, self._bf, crop=self.shape)
            self._e_export[k].record(compute)
            with torch.cuda.stream(self._s_down):
                self._s_down.wait_event(self._e_export[k])
                self._h_out[k].copy_(self._d_out, non_blocking=True)
                if self.motion is not None and self._has_mot[k]:
                    self._h_mot[k].copy_(self._d_mot, non_blocking=True)
                if self.ego is not None and self._has_ego[k]:
                    for host, dev_buf in zip(self._h_ego[k], self._d_ego):
                        host.copy_(dev_buf, non_blocking=True)
                if self.conf is not None:
                    for host, dev_buf in zip(self._h_conf[k], self._d_conf):
                        host.copy_(dev_buf, non_blocking=True)
                if self.align_target is not None:
                    for host, dev_buf in zip(self._h_align[k], self._d_align):
                        host.copy_(dev_buf, non_blocking=True)
                if self.epi is not None:
                    for host, dev_buf in zip(self._h_epi[k], self._d_epi):
                        host.copy_(dev_buf, non_blocking=True)
                if self.ground is not None:
                    for host, dev_buf in zip(self._h_ground[k], self._d_ground):
                        host.copy_(dev_buf, non_blocking=True)
                if self.objects is not None:
                    for host, dev_buf in zip(self._h_objects[k], self._d_objects):
                        host.copy_(dev_buf, non_blocking=True)
                if self.tracks is not None:
                    for host, dev_buf in zip(self._h_tracks[k], self._d_tracks):
                        host.copy_(dev_buf, non_blocking=True)
                if self.scan is not None:
                    for host, dev_buf in zip(self._h_scan[k], self._d_scan):
                        host.copy_(dev_buf, non_blocking=True)
                if self.localmap is not None:
                    for host, dev_buf in zip(self._h_map[k], self._d_map):
                        host.copy_(dev_buf, non_blocking=True)
                if self.costmap is not None:
                    for host, dev_buf in zip(self._h_cost[k], self._d_cost):
                        host.copy_(dev_buf, non_blocking=True)
                if self.plan is not None:
                    for host, dev_buf in zip(self._h_plan[k], self._d_plan):
                        host.copy_(dev_buf, non_blocking=True)
                if self.heightmap is not None:
                    for host, dev_buf in zip(self._h_height[k], self._d_height):
                        host.copy_(dev_buf, non_blocking=True)
                self._e_down[k].record(self._s_down)
        self._inflight.append(k)
        self._pushed += 1

    def _collect(self):
        k = self._inflight.popleft()
        self._e_down[k].synchronize()  # this frame's download only
        res = self._h_out[k].numpy().copy()
        res = res.view(np.uint16) if self.output == "disp_u16" else res
        out = [res]
        if self.motion is not None:
            out.append(self._h_mot[k].numpy().copy() if self._has_mot[k] else None)
        if self.ego is not None:
            out.append(self._collect_ego(k))
        if self.conf is not None:
            out.append(Confidence(*(t.numpy().copy() for t in self._h_conf[k])))
        if self.align_target is not None:
            got = [t.numpy().copy() for t in self._h_align[k]]
            out.append(Aligned(got[0], got[1] if self.align["uv"] else None))
        if self.epi is not None:
            got = [t.numpy().copy() for t in self._h_epi[k]]
            out.append(epipolar_from_record(got[0], got[1] if self.epi["map"] else None))
        if self.ground is not None:
            out.append(ground_from_record(*self._ground_bufs([t.numpy().copy() for t in self._h_ground[k]])))
        if self.objects is not None:
            got = [t.numpy() for t in self._h_objects[k]]  # (objects_from_buffers copies what it keeps)
            out.append(objects_from_buffers(got[0], got[1], got[2], got[3].copy() if self.objects["map"] else None))
        tracks = None
        if self.tracks is not None:
            tracks = tracks_from_buffers(*(t.numpy() for t in self._h_tracks[k]))  # (copies what it keeps)
            out.append(tracks)
        if self.scan is not None:
            out.append(scan_from_buffers(*(t.numpy() for t in self._h_scan[k]), self._scan_meta, tracks))  # (copies too)
        if self.localmap is not None:
            lm = self.localmap
            out.append(localmap_from_buffers(*(t.numpy() for t in self._h_map[k]), lm["cell"], lm["occ_level"], lm["free_level"]))
        if self.costmap is not None:
            hc = [t.numpy() for t in self._h_cost[k]]
            out.append(costmap_from_buffers(hc[0], hc[1], hc[2], hc[3], hc[4] if len(hc) > 4 else None, out[-1].origin,
                                            self.localmap["cell"], self._cost_start))
        if self.plan is not None:
            hp = [t.numpy() for t in self._h_plan[k]]
            out.append(plan_from_buffers(hp[0], hp[1], hp[3] if len(hp) > 3 else None, hp[2], out[-1].origin,
                                         self.localmap["cell"], self._cost_start))
        if self.heightmap is not None:  # (last: the cost map and the plan index out[-1] above)
            out.append(heightmap_from_buffers(*(t.numpy() for t in self._h_height[k]), self.localmap["cell"],
                                              self.heightmap["h_res"]))
        return out[0] if len(out) == 1 else tuple(out)

    def _object_ids(self):
        """The device id map codd_objects writes: the downloaded one, the one the tracks and the scan read, or None."""
        if self.objects["map"]:
            return self._d_objects[3]
        return self._track_ids if self.tracks is not None or self.scan is not None else None

    def _ground_bufs(self, bufs):
        """(record, labels, height, grid_count, grid_height) of the buffers present, None for the others."""
        rest = list(bufs[2:])
        height = rest.pop(0) if self.ground["map"] else None
        return (bufs[0], bufs[1], height) + (tuple(rest) if self.ground["grid"] is not None else (None, None))

    def _collect_ego(self, k):
        if not self._has_ego[k]:
            self._world = trajectory_step(self._world, None)
            return None
        rec, moving, residual = (t.numpy().copy() for t in self._h_ego[k])
        pose, ok = rec[:7].copy(), bool(rec[7] != 0)
        self._world = trajectory_step(self._world, pose, ok)
        return Ego(pose, ok, int(rec[8]), int(rec[9]), float(rec[10]), moving, residual, self._world.copy())

    def pop(self):
        """The oldest frame's result: numpy [h,w] (fp32, or uint16 for ``disp_u16``), owned by the caller; with a
        ``motion`` mode, ``(result, motion)`` with motion fp32 [h,w,C] or None; with ``egomotion``, an ``Ego`` or None
        follows; with ``confidence``, a ``Confidence``; with ``align_to``, an ``Aligned``; with ``epipolar``, an
        ``Epipolar``; with ``ground``, a ``Ground``; with ``objects``, an ``Objects``; with ``tracks``, a ``Tracks``; with
        ``scan``, a ``Scan``; with ``localmap``, a ``LocalMap``; with ``costmap``, a ``CostMap``; with ``plan``, a ``Plan``;
        with ``heightmap``, a ``HeightMap`` comes last."""
        if self._ready:
            return self._ready.popleft()
        if not self._inflight:
            raise IndexError("pop from an empty LiveSession")
        return self._collect()

    def pending(self):
        """Frames pushed and not yet popped (in flight or parked)."""
        return len(self._ready) + len(self._inflight)

    def step(self, left_u8, right_u8):
        """One frame, synchronously (any frames already pushed are returned first by ``pop``, so drain them before): what
        ``pop`` returns, a ``Plan`` last with ``plan``."""
        if self.pending():
            raise RuntimeError("step() on a session with frames in flight: pop() them first")
        self.push(left_u8, right_u8)
        return self.pop()

    def set_goal(self, goal):
        """The goal of ``plan`` for the frames pushed from now on: ``"frontier"`` or a point ``(x, z)`` of the map frame.
        ValueError otherwise, and without ``plan=``.  No device call and no wait: the goal is an argument of the next
        frame's ``codd_plan``."""
        if self.plan is None:
            raise ValueError("set_goal: the session has no plan=")
        self._plan_goal = _check_goal(goal)

    def reset(self):
        """New sequence (reference reset_inference_state, model/codd.py:400-433).  Frames in flight stay poppable; the
        captured graph is kept."""
        self.runner.reset()
        self.est.reset_inference_state()
        self._track_fresh = True
        self._map_fresh = True

    def close(self):
        if self._open_done:
            self._s_up.synchronize()
            torch.cuda.current_stream(self.dev).synchronize()
            self._s_down.synchronize()
            for name in ("_h_in", "_d_in", "_scratch", "_maps", "_d_out", "_h_out", "_depth_prev", "_d_mot", "_h_mot",
                         "_d_ego", "_h_ego", "_ego_scratch", "_d_conf", "_h_conf", "_d_align", "_h_align",
                         "_d_epi", "_h_epi", "_epi_scratch", "_d_ground", "_h_ground", "_ground_scratch",
                         "_d_objects", "_h_objects", "_objects_scratch", "_track_ids", "_d_tracks", "_h_tracks",
                         "_track_state", "_track_scratch", "_d_scan", "_h_scan", "_scan_edges", "_scan_scratch",
                         "_d_map", "_h_map", "_map_state", "_map_scratch", "_d_cost", "_h_cost", "_cost_lut",
                         "_cost_scratch", "_d_plan", "_h_plan", "_plan_scratch", "_d_height", "_h_height", "_height_state",
                         "_height_scratch"):
                setattr(self, name, None)
            self._open_done = False
        self._inflight.clear()
        self._ready.clear()
        self.runner = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
