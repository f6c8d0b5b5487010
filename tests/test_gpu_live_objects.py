"""LiveSession obstacle objects on the GPU: codd_objects against the restatement of tests/live_objects_ref.py, bit for bit
on count, both tables in full (zero rows included) and the id map, with no excluded pixel and no tolerance (what each
case is built to show is asserted on the restatement in tests/test_live_objects.py); guard regions, dirty buffers,
unaligned pointers, determinism, untouched inputs; codd_ground_plane chained into codd_objects on a scene with planted
boxes; LiveSession(ground=..., objects=...) against the two entries called by hand on the disparity of the route a user
had to write; and the --live --ground --objects command line.
The crop of the cases is 70 x 150 in 128 x 192: the tile of codd_objects is 16 x 64, so there are five tile rows and three
tile columns, the last of each partial.
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ground_ref as lg  # noqa: E402
import live_objects_ref as lo  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every output
K_DEV = 5.0  # x the ground restatement's own deviation, as tests/test_gpu_live_ground.py bounds heights
_CACHE = {}
IDS = [lo.case_id(c) for c in lo.CASES]


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _case(name):
    """(inputs, reference), computed once and never modified."""
    if name not in _CACHE:
        c = lo.CASES[lo.NAMES[name]]
        _CACHE[name] = (c, lo.reference(c))
    return _CACHE[name]


def _guarded(n, dtype, fill, off):
    buf = torch.full((n + 2 * GUARD + 4,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD + off:GUARD + off + n]


class Run:
    """One call of ops.objects on the case ``c``: every output and the scratch between guard regions; ``off`` shifts every
    fp32 / int32 / uint16 pointer by that many elements off a 16-byte boundary and the byte buffers by as many bytes.  The
    id buffer exists whether the call asks for ids or not (``with_ids`` False: the call gets None and must leave it)."""
    FILLS = dict(count=-7, obj_i=-7, obj_f=-7.0, ids=0x5A5A, scratch=0x5A)

    def __init__(self, c, with_ids=True, off=0):
        from codd_amd import ops
        h, w = c["crop"]
        m = c["par"]["max_objects"]
        self.c, self.off, self.h, self.w, self.m, self.with_ids = c, off, h, w, m, with_ids
        H, W = c["padded"]
        buf = torch.zeros(H * W + 4, device=DEV)
        self.disp = buf[off:off + H * W].view(H, W)
        lbuf = torch.zeros(h * w + 4, dtype=torch.uint8, device=DEV)
        self.lab = lbuf[off:off + h * w].view(h, w)
        self.rec = torch.zeros(32, dtype=torch.float64, device=DEV)
        self.bcnt, self.cnt = _guarded(4, torch.int32, -7, off)
        self.boi, self.oi = _guarded(m * 8, torch.int32, -7, off)
        self.bof, self.of = _guarded(m * 8, torch.float32, -7.0, off)
        self.bids, self.ids = _guarded(h * w, torch.int16, 0x5A5A, off)  # (uint16 bits: torch compares int16 on the device)
        self.bscr, self.scr = _guarded(ops.objects_scratch(h, w, m), torch.uint8, 0x5A, off)
        self.oi, self.of, self.ids = self.oi.view(m, 8), self.of.view(m, 8), self.ids.view(h, w)
        assert self.bof.data_ptr() % 16 == 0 and self.of.data_ptr() % 16 == 4 * off and self.ids.data_ptr() % 16 == 2 * off
        self.launch(c)

    def launch(self, c):
        """(again, with another case of the same shapes: into the buffers and the scratch as the last call left them)"""
        from codd_amd import ops
        assert c["crop"] == (self.h, self.w) and c["par"]["max_objects"] == self.m
        self.c = c
        self.disp.copy_(torch.from_numpy(c["disp"]))
        self.lab.copy_(torch.from_numpy(c["labels"]))
        self.rec.copy_(torch.from_numpy(c["rec"]))
        self.inputs = (self.disp.clone(), self.lab.clone(), self.rec.clone())
        par = {k: v for k, v in c["par"].items() if k != "max_objects"}
        ops.objects(self.disp, c["K"], c["calib"], c["crop"], self.lab, self.rec, self.cnt, self.oi, self.of,
                    ids=self.ids.view(torch.uint16) if self.with_ids else None, scratch=self.scr, **par)
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        lo_ = GUARD + self.off
        for name, buf, view, used in (("count", self.bcnt, self.cnt, True), ("obj_i", self.boi, self.oi, True),
                                      ("obj_f", self.bof, self.of, True), ("ids", self.bids, self.ids, self.with_ids),
                                      ("scratch", self.bscr, self.scr, True)):
            fill, n = self.FILLS[name], view.numel()
            if used:
                assert bool((buf[:lo_] == fill).all()) and bool((buf[lo_ + n:] == fill).all()), f"{what}: {name} guard overwritten"
            else:
                assert bool((buf == fill).all()), f"{what}: no {name} asked for and its buffer was written"
        assert torch.equal(glm._bits(self.disp), glm._bits(self.inputs[0])) and torch.equal(self.lab, self.inputs[1]) \
            and torch.equal(self.rec.view(torch.int64), self.inputs[2].view(torch.int64)), f"{what}: an input was modified"

    def outputs(self):
        return dict(count=self.cnt.cpu().numpy(), obj_i=self.oi.cpu().numpy(), obj_f=self.of.cpu().numpy(),
                    ids=self.ids.cpu().numpy().view(np.uint16))

    def same_bytes(self, other):
        ok = torch.equal(self.cnt, other.cnt) and torch.equal(self.oi, other.oi) and torch.equal(glm._bits(self.of), glm._bits(other.of))
        if self.with_ids and other.with_ids:
            ok = ok and torch.equal(self.ids, other.ids)
        return ok


def _assert_equal(out, ref, name, ids=True):
    """count, both tables in full and the ids against the restatement: bytes, not values (-0 is not +0)."""
    print(f"{name}: count {out['count'].tolist()} (restatement {ref['count'].tolist()})")
    assert out["count"].tolist() == ref["count"].tolist(), name
    bad = np.argwhere(out["obj_i"] != ref["obj_i"])
    assert bad.size == 0, f"{name}: obj_i differs at {bad[:8].tolist()}: {out['obj_i'][bad[0][0]].tolist()} vs {ref['obj_i'][bad[0][0]].tolist()}"
    a, b = out["obj_f"].view(np.uint32), ref["obj_f"].view(np.uint32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{name}: obj_f differs at {bad[:8].tolist()}: {out['obj_f'][bad[0][0]].tolist()} vs {ref['obj_f'][bad[0][0]].tolist()}"
    if ids:
        bad = np.argwhere(out["ids"] != ref["ids"])
        assert bad.size == 0, f"{name}: {bad.shape[0]} ids differ, first at {bad[:8].tolist()}"


@pytest.mark.parametrize("name", IDS)
def test_objects_against_reference(name):
    c, ref = _case(name)
    a = Run(c)
    a.check_guards(name)
    _assert_equal(a.outputs(), ref, name)
    b = Run(c)  # determinism: a second run gives equal bytes
    assert a.same_bytes(b)


def test_dirty_buffers_and_scratch_give_the_same_bytes():
    """A call into outputs and a scratch that still hold another case's results: the chunk rows, the cleared rows, the
    parents and slots of the earlier image.  All 70 x 150 with 256 rows."""
    order = ["checkerboard", "no-floor", "min-pixels", "serpentine", "no-foreground", "all-foreground", "comb", "two-labels"]
    r = Run(_case(order[0])[0])
    for name in order[1:]:
        c, ref = _case(name)
        r.launch(c)
        r.check_guards(name)
        _assert_equal(r.outputs(), ref, name + " into used buffers")


@pytest.mark.parametrize("name", ("serpentine", "checkerboard", "both-signs", "five-by-seven"))
def test_objects_unaligned_views_and_no_ids(name):
    """Every fp32 / int32 pointer 4, 8, 12 bytes off a 16-byte boundary (ids 2, 4, 6; labels and scratch 1, 2, 3 bytes):
    the bytes of the restatement, nothing written outside the views; without ids the other outputs have the same bytes
    and the id buffer is untouched."""
    c, ref = _case(name)
    for off in (1, 2, 3):
        got = Run(c, off=off)
        assert got.disp.data_ptr() % 16 == 4 * off and got.cnt.data_ptr() % 16 == 4 * off and got.lab.data_ptr() % 16 == off
        got.check_guards(f"offset {off}")
        _assert_equal(got.outputs(), ref, f"{name} offset {off}")
    for kw in (dict(with_ids=False), dict(with_ids=False, off=1)):
        part = Run(c, **kw)
        part.check_guards(str(kw))
        _assert_equal(part.outputs(), ref, f"{name} {kw}", ids=False)


def test_ops_reject_bad_arguments():
    from codd_amd import _abi, ops
    c, _ = _case("five-by-seven")
    with pytest.raises(ValueError):
        ops.objects_scratch(0, 5)
    with pytest.raises(ValueError):
        ops.objects_scratch(4, 5, 4097)
    a = Run(c)
    args = (a.disp, c["K"], c["calib"], c["crop"], a.lab, a.rec, a.cnt, a.oi, a.of)
    with pytest.raises(TypeError):
        ops.objects(*args, scratch=a.scr, speed=3)
    for bad in (dict(select=0), dict(gap_px=0.0), dict(gap_rel=-1.0), dict(min_pixels=0), dict(min_height=float("nan"))):
        before = a.cnt.clone()
        with pytest.raises(_abi.CoddHipError):
            ops.objects(*args, scratch=a.scr, **bad)
        assert torch.equal(before, a.cnt)
    with pytest.raises(_abi.CoddHipError):  # scratch too small
        ops.objects(*args, scratch=a.scr[:-1])
    with pytest.raises(AssertionError):  # max_objects is the tables' row count
        ops.objects(*args, scratch=a.scr, max_objects=c["par"]["max_objects"] + 1)


# ---- codd_ground_plane chained into codd_objects ----------------------------------------------------------------------
def test_ground_plane_into_objects():
    """tests/live_ground_ref.py's "clutter": three fronto-parallel boxes on a noisy floor.  ops.ground_plane's device labels
    and record go to ops.objects as they are.  Each planted box comes back as one object: every obstacle pixel inside the
    planted rectangle carries one id and that object's image box lies inside the rectangle and spans its columns; its
    hgt_min and hgt_max are, bit for bit, the smallest and largest entry of codd_ground_plane's own height map over the
    object's pixels, and hgt_max is within the ground test's own bound (K_DEV x the deviation of the fp32 restatement from
    the fp64 reference) of the fp64 reference's largest height over the same pixels; its extents contain the box's true
    footprint: the noise-free gx and gz, at the planted depth, of the box's first and last column over the object's rows,
    up to what the noise can move a measured extreme inwards -- a pixel's gx and gz scale with 1 / d, so 5 sigma = 0.25 px of
    disparity move them by 0.25 / d of their size -- plus the ground test's bound on the frame itself (K_DEV x the
    deviation of the restatement's cell coordinates, in units of the cell, here 1).  Components are also compared with
    the restatement run on the labels and record the device produced."""
    from codd_amd import ops
    spec = next(s for s in lg.CASES if s["name"] == "clutter")
    c = lg.case(spec)
    gref = lg.reference(c)
    h, w = c["crop"]
    disp = torch.from_numpy(c["disp"]).to(DEV)
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    lab, hmap = torch.empty(h, w, dtype=torch.uint8, device=DEV), torch.empty(h, w, device=DEV)
    ops.ground_plane(disp, c["K"], c["calib"], c["crop"], rec, lab, hmap, seed=c["seed"], up=lg.UP,
                     **{k: v for k, v in c["par"].items() if k != "cell"})
    m = 64
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    oi, of = torch.zeros(m, 8, dtype=torch.int32, device=DEV), torch.zeros(m, 8, device=DEV)
    ids = torch.zeros(h, w, dtype=torch.int16, device=DEV)
    par = dict(min_pixels=64, min_height=0.15)
    ops.objects(disp, c["K"], c["calib"], c["crop"], lab, rec, cnt, oi, of, ids=ids.view(torch.uint16), **par)
    torch.cuda.synchronize()
    out = dict(count=cnt.cpu().numpy(), obj_i=oi.cpu().numpy(), obj_f=of.cpu().numpy(), ids=ids.cpu().numpy().view(np.uint16))
    labels, record, heights = lab.cpu().numpy(), rec.cpu().numpy(), hmap.cpu().numpy()
    assert record[3] == 1.0
    mine = lo.make("chained", labels, c["disp"][:h, :w], rec=record, padded=c["padded"], K=c["K"], calib=c["calib"],
                   max_objects=m, **par)
    _assert_equal(out, lo.reference(mine), "chained")
    n = int(out["count"][0])
    print(f"chained: {n} objects, pixels {out['obj_i'][:n, 0].tolist()}, hgt_max {out['obj_f'][:n, 5].tolist()}")
    p64, plane = gref["r64"]["pix"], gref["r64"]["plane"]
    fx, fy, cx, cy = c["K"]
    seen = set()
    for x0, x1, y0, y1 in lg.SCENES["clutter"]["boxes"]:
        inside = np.zeros((h, w), bool)
        inside[y0:y1, x0:x1] = True
        px = inside & (labels == lg.OBSTACLE)
        got = np.unique(out["ids"][px])
        assert px.sum() > 500 and got.size == 1 and got[0] != lo.NONE, f"box {(x0, x1, y0, y1)}: ids {got.tolist()}"
        k = int(got[0])
        assert k not in seen
        seen.add(k)
        row_i, row_f = out["obj_i"][k], out["obj_f"][k]
        assert x0 == row_i[1] and row_i[3] == x1 - 1 and y0 <= row_i[2] and row_i[4] < y1 and row_i[0] == int((out["ids"] == k).sum())
        mask = out["ids"] == k
        assert heights[mask].min().tobytes() == row_f[4].tobytes() and heights[mask].max().tobytes() == row_f[5].tobytes(), \
            f"box {(x0, x1, y0, y1)}: hgt_min / hgt_max {row_f[4:6].tolist()} are not the bits of the height map's " \
            f"{[float(heights[mask].min()), float(heights[mask].max())]}"
        want_top = float(np.nanmax(p64["height"][mask]))
        print(f"  box {(x0, x1, y0, y1)}: object {k}, hgt_max {row_f[5]:.6f} (fp64 reference {want_top:.6f}, bound "
              f"{K_DEV * gref['dev_h']:.3e}), extent {row_f[:4].tolist()}")
        assert abs(float(row_f[5]) - want_top) <= K_DEV * gref["dev_h"]
        db = lg.plane_disp(c["plant"], c["K"], 0.5 * (x0 + x1 - 1), y1 - 1)  # the planted disparity of the box
        Z = c["calib"] / db
        ys, xs = np.meshgrid(np.arange(row_i[2], row_i[4] + 1), np.array([x0, x1 - 1]), indexing="ij")
        X = Z * np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones(xs.shape)])  # [3, rows, 2], noise-free
        gx, gz = np.tensordot(plane["right"], X, 1), np.tensordot(plane["forward"], X, 1)
        slack = lambda v: 5 * lg.NOISE_PX / db * np.abs(v).max() + K_DEV * gref["dev_u"]  # noqa: E731
        print(f"    true footprint gx {gx.min():.4f} .. {gx.max():.4f}, gz {gz.min():.4f} .. {gz.max():.4f}; slack {slack(gx):.4f}, {slack(gz):.4f}")
        assert row_f[0] <= gx.min() + slack(gx) and gx.max() - slack(gx) <= row_f[1]
        assert row_f[2] <= gz.min() + slack(gz) and gz.max() - slack(gz) <= row_f[3]


# ---- the session against the entries on the tensors of the existing route -------------------------------------------
GROUND = dict(height=0.5, pitch_deg=12.0, map=True, grid=(16, 24), cell=0.05, min_valid=64, max_tilt_deg=90.0)
OBJECTS = dict(select=("obstacle", "overhead"), min_pixels=16, min_height=0.0, max_objects=32, map=True)
FIELDS = ("pixels", "box", "near_px", "key", "extent", "height", "disparity", "ids")


def _same_objects(a, b):
    return ((a.n, a.found, a.components, a.foreground) == (b.n, b.found, b.components, b.foreground)
            and all(getattr(a, k).dtype == getattr(b, k).dtype and getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in FIELDS))


def _direct(disp):
    """ops.ground_plane and ops.objects as a user calls them on the route's (padded) disparity, with the session's
    parameters."""
    from codd_amd import live, ops
    h, w = glm.H0, glm.W0
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    lab, hgt = torch.empty(h, w, dtype=torch.uint8, device=DEV), torch.empty(h, w, device=DEV)
    cnt, gh = torch.empty((2,) + GROUND["grid"], dtype=torch.int32, device=DEV), torch.empty(GROUND["grid"], device=DEV)
    par = {k: GROUND.get(k, live.GROUND_DEFAULTS[k]) for k in ops.GROUND_PARAMS}
    ops.ground_plane(disp, glm.INTRINSICS, glm.CALIB, (h, w), rec, lab, hgt, cnt, gh,
                     seed=live.ground_seed(GROUND["height"], glm.INTRINSICS, glm.CALIB, pitch_deg=GROUND["pitch_deg"]),
                     up=live._unit_up((0, -1, 0), GROUND["pitch_deg"]), **par)
    m = OBJECTS["max_objects"]
    count = torch.empty(4, dtype=torch.int32, device=DEV)
    oi, of = torch.empty(m, 8, dtype=torch.int32, device=DEV), torch.empty(m, 8, device=DEV)
    ids = torch.empty(h, w, dtype=torch.uint16, device=DEV)
    opar = {k: OBJECTS[k] for k in ("gap_px", "gap_rel", "min_pixels", "min_height") if k in OBJECTS}
    ops.objects(disp, glm.INTRINSICS, glm.CALIB, (h, w), lab, rec, count, oi, of, ids=ids,
                select=live.select_mask(OBJECTS["select"]), **opar)
    return live.objects_from_buffers(count.cpu().numpy(), oi.cpu().numpy(), of.cpu().numpy(), ids.cpu().numpy())


def test_session_objects_against_the_existing_route():
    import test_gpu_live_ground as glg
    from codd_amd import live
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()
    s, g_only = glm._session(ground=GROUND, objects=OBJECTS), glm._session(ground=GROUND)
    first = []
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 3
        res, g, ob = got
        res1, g1 = g_only.step(left, right)
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i]), f"frame {i}: the depth result changed"
        assert glg._same_ground(g, g1), f"frame {i}: Ground changed with objects= on"
        assert isinstance(ob, live.Objects) and ob.ids.dtype == np.uint16 and ob.ids.shape == (glm.H0, glm.W0) and ob.ids.flags["OWNDATA"]
        assert ob.pixels.shape == (ob.n,) and ob.box.shape == (ob.n, 4) and ob.extent.shape == (ob.n, 4) and ob.n <= 32
        want = _direct(parent[i][0])
        print(f"frame {i}: floor {g.ok}; {ob.n} objects of {ob.found} passing, {ob.components} components, {ob.foreground} "
              f"foreground pixels; pixels {ob.pixels.tolist()[:8]}")
        assert _same_objects(ob, want), f"frame {i}: Objects differ from the direct calls"
        first.append(ob)
    kept = [(ob.pixels.copy(), ob.ids.copy()) for ob in first]
    for ob in first:  # the results are the caller's: scribbling on them changes no later frame
        ob.pixels[...] = -1
        ob.ids[...] = 7
    s.reset()
    g_only.reset()
    g_only.close()
    second = []
    for left, right in frames:  # a new sequence, pipelined: push, push, pop, pop
        s.push(left.copy(), right.copy())
        if s.pending() == 2:
            second.append(s.pop())
    while s.pending():
        second.append(s.pop())
    assert len(second) == glm.FRAMES
    for i in range(glm.FRAMES):
        assert np.array_equal(second[i][0], plain[i]), f"pipelined frame {i}: the result differs"
        ob = second[i][2]
        assert np.array_equal(ob.pixels, kept[i][0]) and np.array_equal(ob.ids, kept[i][1]), f"pipelined frame {i}: Objects differ from step()'s"
    s.reset()
    s.close()
    assert s._d_objects is None and s._h_objects is None and s._objects_scratch is None


def test_cli_live_objects(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 4
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    common = ["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
              "--live", "--ground"]
    inference.main(common + ["--show", "--show-dir", str(tmp_path / "show"), "--objects"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "objects:" in ln]
    assert len(lines) == 1 and f"in {n} frames" in lines[0]
    assert sorted(os.listdir(tmp_path / "show")) == ["left.disp.pred.npz", "left.ground.pred.npz", "left.objects.pred.npz"]
    z = np.load(tmp_path / "show" / "left.objects.pred.npz")
    assert sorted(z.files) == ["box", "disparity", "extent", "found", "height", "ids", "key", "n", "near_px", "pixels"]
    m = 256
    assert z["n"].shape == z["found"].shape == (1, n) and z["pixels"].shape == z["key"].shape == (1, n, m)
    assert z["box"].shape == z["extent"].shape == (1, n, m, 4) and z["near_px"].shape == z["height"].shape == z["disparity"].shape == (1, n, m, 2)
    assert z["ids"].shape == (1, n, h, w) and z["ids"].dtype == np.uint16 and z["extent"].dtype == np.float32 and z["box"].dtype == np.int32
    inference.main(common + ["--show-dir", str(tmp_path / "quiet"), "--objects"])  # without --show: the tables only
    q = np.load(tmp_path / "quiet" / "left.objects.pred.npz")
    assert sorted(q.files) == ["box", "disparity", "extent", "found", "height", "key", "n", "near_px", "pixels"]
    assert all(q[k].tobytes() == z[k].tobytes() for k in q.files)
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, ground=True, objects=dict(map=True))
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        _, _, ob = s.step(left, right)
        assert ob.n == z["n"][0, i] and ob.found == z["found"][0, i] and np.array_equal(ob.ids, z["ids"][0, i])
        assert np.array_equal(ob.pixels, z["pixels"][0, i, :ob.n]) and not z["pixels"][0, i, ob.n:].any()
        assert ob.extent.tobytes() == z["extent"][0, i, :ob.n].tobytes() and np.array_equal(ob.box, z["box"][0, i, :ob.n])
    s.reset()
    s.close()
