"""LiveSession range scan on the GPU: codd_range_scan against the restatement of tests/live_scan_ref.py, bit for bit on
scan_count and both tables in full, with no excluded pixel and no tolerance (what each case is built to show is asserted
on the restatement in tests/test_live_scan.py); guard regions, dirty buffers and scratch, unaligned pointers, determinism,
untouched inputs, rejected arguments; codd_ground_plane -> codd_objects -> codd_range_scan chained on a scene with planted
boxes; LiveSession(ground=..., objects=..., scan=...) with and without tracks= against the entries called by hand on the
disparity of the route a user had to write; and the --live --ground --objects --scan command line.
The crop of the cases is 70 x 150 in 128 x 192: the pixel launch works on 32 x 8 tiles of four 8 x 8 blocks, so there are
nine tile rows and five tile columns, the last of each partial (the last tile column holds 22 of 32 columns: its third
block is partial and its fourth empty).
Autotune is off in every test, so launch configurations are the deterministic heuristics and runs are reproducible."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ground_ref as lg  # noqa: E402
import live_scan_ref as ls  # noqa: E402
import test_gpu_live_motion as glm  # noqa: E402  (its frames, estimator and FrameRunner route, computed once per process)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # guard elements on either side of every output
_CACHE = {}
IDS = [ls.case_id(c) for c in ls.CASES]


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


def _case(name):
    """(inputs, reference), computed once and never modified."""
    if name not in _CACHE:
        c = ls.CASES[ls.NAMES[name]]
        _CACHE[name] = (c, ls.reference(c))
    return _CACHE[name]


def _guarded(n, dtype, fill, off):
    buf = torch.full((n + 2 * GUARD + 4,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD + off:GUARD + off + n]


def _par(c):
    return {k: c["scan"][k] for k in ("bins", "range_min", "range_max", "select", "min_pixels")}


class Run:
    """One call of ops.range_scan on the case ``c``: every output and the scratch between guard regions; ``off`` shifts
    every fp32 / int32 / uint16 pointer by that many elements off a 16-byte boundary, the byte buffers by as many bytes and
    the record by ``off % 2`` doubles."""
    FILLS = dict(count=-7, scan_i=-7, scan_f=-7.0, scratch=0x5A)

    def __init__(self, c, off=0):
        from codd_amd import ops
        h, w = c["crop"]
        beams, bins = c["scan"]["beams"], c["scan"]["bins"]
        self.c, self.off, self.h, self.w, self.beams, self.bins = c, off, h, w, beams, bins
        H, W = c["padded"]
        self.disp = torch.zeros(H * W + 4, device=DEV)[off:off + H * W].view(H, W)
        self.lab = torch.zeros(h * w + 4, dtype=torch.uint8, device=DEV)[off:off + h * w].view(h, w)
        self.rec = torch.zeros(34, dtype=torch.float64, device=DEV)[off % 2:off % 2 + 32]
        self.ids = torch.zeros(h * w + 4, dtype=torch.int16, device=DEV)[off:off + h * w].view(h, w)  # (uint16 bits)
        self.edges = torch.zeros(2 * (beams + 1) + 4, device=DEV)[off:off + 2 * (beams + 1)].view(beams + 1, 2)
        self.bcnt, self.cnt = _guarded(4, torch.int32, -7, off)
        self.bsi, self.si = _guarded(beams * 4, torch.int32, -7, off)
        self.bsf, self.sf = _guarded(beams * 4, torch.float32, -7.0, off)
        self.bscr, self.scr = _guarded(ops.range_scan_scratch(beams, bins), torch.uint8, 0x5A, off)
        self.si, self.sf = self.si.view(beams, 4), self.sf.view(beams, 4)
        assert self.bsf.data_ptr() % 16 == 0 and self.sf.data_ptr() % 16 == 4 * off and self.ids.data_ptr() % 16 == 2 * off
        assert self.rec.data_ptr() % 16 == 8 * (off % 2) and self.edges.data_ptr() % 16 == 4 * off
        self.launch(c)

    def launch(self, c, **over):
        """(again, with another case of the same shapes: into the buffers and the scratch as the last call left them)"""
        from codd_amd import ops
        assert c["crop"] == (self.h, self.w) and (c["scan"]["beams"], c["scan"]["bins"]) == (self.beams, self.bins)
        self.c = c
        self.disp.copy_(torch.from_numpy(c["disp"]))
        self.lab.copy_(torch.from_numpy(c["labels"]))
        self.rec.copy_(torch.from_numpy(c["rec"]))
        self.edges.copy_(torch.from_numpy(c["edges"]))
        if c["ids"] is not None:
            self.ids.copy_(torch.from_numpy(c["ids"].view(np.int16)))
        self.inputs = tuple(t.clone() for t in (self.disp, self.lab, self.rec, self.edges, self.ids))
        ops.range_scan(self.disp, c["K"], c["calib"], c["crop"], self.lab, self.rec, self.edges, self.cnt, self.si, self.sf,
                       ids=None if c["ids"] is None else self.ids.view(torch.uint16), scratch=self.scr, **dict(_par(c), **over))
        torch.cuda.synchronize()

    def check_guards(self, what=""):
        lo_ = GUARD + self.off
        for name, buf, view in (("count", self.bcnt, self.cnt), ("scan_i", self.bsi, self.si), ("scan_f", self.bsf, self.sf),
                                ("scratch", self.bscr, self.scr)):
            fill, n = self.FILLS[name], view.numel()
            assert bool((buf[:lo_] == fill).all()) and bool((buf[lo_ + n:] == fill).all()), f"{what}: {name} guard overwritten"
        now = (glm._bits(self.disp), self.lab, self.rec.view(torch.int64), glm._bits(self.edges), self.ids)
        was = (glm._bits(self.inputs[0]), self.inputs[1], self.inputs[2].view(torch.int64), glm._bits(self.inputs[3]), self.inputs[4])
        assert all(torch.equal(a, b) for a, b in zip(now, was)), f"{what}: an input was modified"

    def outputs(self):
        return dict(count=self.cnt.cpu().numpy(), scan_i=self.si.cpu().numpy(), scan_f=self.sf.cpu().numpy())

    def same_bytes(self, other):
        return torch.equal(self.cnt, other.cnt) and torch.equal(self.si, other.si) and torch.equal(glm._bits(self.sf), glm._bits(other.sf))


def _assert_equal(out, ref, name):
    """scan_count and both tables in full against the restatement: bytes, not values (a NaN has one bit pattern)."""
    print(f"{name}: count {out['count'].tolist()} (restatement {ref['count'].tolist()})")
    assert out["count"].tolist() == ref["count"].tolist(), name
    bad = np.argwhere(out["scan_i"] != ref["scan_i"])
    assert bad.size == 0, f"{name}: scan_i differs at {bad[:8].tolist()}: {out['scan_i'][bad[0][0]].tolist()} vs {ref['scan_i'][bad[0][0]].tolist()}"
    a, b = out["scan_f"].view(np.uint32), ref["scan_f"].view(np.uint32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{name}: scan_f differs at {bad[:8].tolist()}: {out['scan_f'][bad[0][0]].tolist()} vs {ref['scan_f'][bad[0][0]].tolist()}"


@pytest.mark.parametrize("name", IDS)
def test_scan_against_reference(name):
    c, ref = _case(name)
    a = Run(c)
    a.check_guards(name)
    _assert_equal(a.outputs(), ref, name)
    b = Run(c)  # determinism: a second run gives equal bytes
    assert a.same_bytes(b)


@pytest.mark.parametrize("order", (("boxes", "no-floor", "boxes-no-ids", "boxes"),
                                   ("wall", "beam-edges", "floor-and-nothing", "wall-none-id"),
                                   ("speckle", "threshold-missed", "rho-tie", "range-max-excluded", "threshold-met", "range-edges")),
                         ids=("256x128", "4x16", "1x16"))
def test_dirty_buffers_and_scratch_give_the_same_bytes(order):
    """A call into outputs and a scratch that still hold another case's results: its tables, its rows, its counts."""
    r = Run(_case(order[0])[0])
    for name in order[1:]:
        c, ref = _case(name)
        r.launch(c)
        r.check_guards(name)
        _assert_equal(r.outputs(), ref, name + " into used buffers")


@pytest.mark.parametrize("name", ("boxes", "boxes-7x16", "wall", "own-beam", "behind"))
def test_scan_unaligned_views(name):
    """Every fp32 / int32 pointer 4, 8, 12 bytes off a 16-byte boundary (ids 2, 4, 6; labels and scratch 1, 2, 3 bytes; the
    record 8 bytes): the bytes of the restatement, nothing written outside the views."""
    c, ref = _case(name)
    for off in (1, 2, 3):
        got = Run(c, off=off)
        assert got.disp.data_ptr() % 16 == 4 * off and got.cnt.data_ptr() % 16 == 4 * off and got.lab.data_ptr() % 16 == off
        assert got.scr.data_ptr() % 16 == off
        got.check_guards(f"offset {off}")
        _assert_equal(got.outputs(), ref, f"{name} offset {off}")


def test_ops_reject_bad_arguments():
    from codd_amd import _abi, ops
    c, ref = _case("boxes-7x16")
    for bad in ((0, 4), (4, 0), (2049, 1), (1, 1025), (2048, 1024)):
        with pytest.raises(ValueError):
            ops.range_scan_scratch(*bad)
    a = Run(c)
    args = (a.disp, c["K"], c["calib"], c["crop"], a.lab, a.rec, a.edges, a.cnt, a.si, a.sf)
    with pytest.raises(TypeError):
        ops.range_scan(*args, scratch=a.scr, speed=3)
    before = (a.bcnt.clone(), a.bsi.clone(), a.bsf.clone(), a.bscr.clone())
    par = _par(c)
    for bad in (dict(select=0), dict(select=1), dict(select=3), dict(min_pixels=0), dict(range_max=0.0), dict(range_max=float("inf")),
                dict(range_max=float("nan")), dict(range_min=-1.0), dict(range_min=float("nan")), dict(range_min=par["range_max"]),
                dict(bins=0), dict(bins=1025)):
        with pytest.raises(_abi.CoddHipError):
            ops.range_scan(*args, scratch=a.scr, **dict(par, **bad))
    for K, calib in (((0.0,) + tuple(c["K"][1:]), c["calib"]), (c["K"][:2] + (float("nan"),) + c["K"][3:], c["calib"]),
                     (c["K"], float("inf"))):
        with pytest.raises(_abi.CoddHipError):
            ops.range_scan(a.disp, K, calib, *args[3:], scratch=a.scr, **par)
    with pytest.raises(_abi.CoddHipError):  # scratch too small
        ops.range_scan(*args, scratch=a.scr[:-1], **par)
    with pytest.raises(_abi.CoddHipError):  # the crop does not fit the padded map
        ops.range_scan(a.disp, c["K"], c["calib"], (c["padded"][0] + 1, c["crop"][1]), torch.zeros(c["padded"][0] + 1, c["crop"][1],
                       dtype=torch.uint8, device=DEV), *args[5:], scratch=a.scr, **par)
    torch.cuda.synchronize()
    now = (a.bcnt, a.bsi, a.bsf, a.bscr)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(now, before)), "a rejected call wrote something"
    with pytest.raises(AssertionError):  # the table's rows are the beams
        ops.range_scan(*args[:6], a.edges[:-1], *args[7:], scratch=a.scr, **par)
    _assert_equal(a.outputs(), ref, "after the rejected calls")


# ---- codd_ground_plane -> codd_objects -> codd_range_scan ---------------------------------------------------------------
def test_ground_plane_into_objects_into_scan():
    """tests/live_ground_ref.py's "clutter": three fronto-parallel boxes on a noisy floor.  The device labels, record and id
    map go from entry to entry as they are.  The scan has the bytes of the restatement run on what the device produced;
    every hit's object owns the hit pixel in the id map; every planted box stops at least ten beams (it spans 44 of 160
    columns and there are 96 beams) at a pixel inside its planted rectangle; and a hit's range is sqrtf(gx gx + gz gz) of
    the hit position it reports, to the bit."""
    from codd_amd import ops
    spec = next(s for s in lg.CASES if s["name"] == "clutter")
    c = lg.case(spec)
    h, w = c["crop"]
    disp = torch.from_numpy(c["disp"]).to(DEV)
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    lab = torch.empty(h, w, dtype=torch.uint8, device=DEV)
    ops.ground_plane(disp, c["K"], c["calib"], c["crop"], rec, lab, seed=c["seed"], up=lg.UP,
                     **{k: v for k, v in c["par"].items() if k != "cell"})
    m = 64
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    oi, of = torch.zeros(m, 8, dtype=torch.int32, device=DEV), torch.zeros(m, 8, device=DEV)
    ids = torch.zeros(h, w, dtype=torch.uint16, device=DEV)
    ops.objects(disp, c["K"], c["calib"], c["crop"], lab, rec, cnt, oi, of, ids=ids, min_pixels=64, min_height=0.15)
    beams, bins = 96, 64
    span = ls.camera_span(c["K"], w)
    edges = torch.from_numpy(ops.scan_edges(beams, *span)).to(DEV)
    sc = torch.zeros(4, dtype=torch.int32, device=DEV)
    si, sf = torch.zeros(beams, 4, dtype=torch.int32, device=DEV), torch.zeros(beams, 4, device=DEV)
    ops.range_scan(disp, c["K"], c["calib"], c["crop"], lab, rec, edges, sc, si, sf, ids=ids, bins=bins, range_max=6.4)
    torch.cuda.synchronize()
    out = dict(count=sc.cpu().numpy(), scan_i=si.cpu().numpy(), scan_f=sf.cpu().numpy())
    labels, record, idmap = lab.cpu().numpy(), rec.cpu().numpy(), ids.cpu().numpy()
    assert record[3] == 1.0 and int(cnt[0]) >= 3
    mine = ls.make("chained", labels, c["disp"][:h, :w], rec=record, ids=idmap, K=c["K"], calib=c["calib"], padded=c["padded"],
                   beams=beams, bins=bins, angles=span, range_max=6.4)
    _assert_equal(out, ls.reference(mine), "chained")
    hit = out["scan_i"][:, 0] >= 0
    print(f"chained: count {out['count'].tolist()}, objects at the hits {sorted(set(out['scan_i'][hit, 1].tolist()))}")
    at_hit = idmap.ravel()[out["scan_i"][hit, 0]].astype(np.int64)
    assert out["scan_i"][hit, 1].tolist() == np.where(at_hit == ls.NONE, -1, at_hit).tolist()
    rho = np.sqrt((out["scan_f"][:, 2] * out["scan_f"][:, 2]) + (out["scan_f"][:, 3] * out["scan_f"][:, 3]))
    assert rho[hit].tobytes() == out["scan_f"][hit, 0].tobytes()
    for x0, x1, y0, y1 in lg.SCENES["clutter"]["boxes"]:
        inside = np.zeros((h, w), bool)
        inside[y0:y1, x0:x1] = True
        obj = np.unique(idmap[inside & (labels == lg.OBSTACLE)])
        obj = obj[obj != ls.NONE]
        assert obj.size == 1
        rows = np.nonzero(hit & (out["scan_i"][:, 1] == obj[0]))[0]
        ys, xs = np.divmod(out["scan_i"][rows, 0], w)
        print(f"  box {(x0, x1, y0, y1)}: object {obj[0]}, {rows.size} beams, ranges {out['scan_f'][rows, 0].min():.4f} .. "
              f"{out['scan_f'][rows, 0].max():.4f}")
        assert rows.size >= 10 and np.all((xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1))


# ---- the session against the entries on the tensors of the existing route -------------------------------------------
SCAN = dict(beams=48, bins=64, range_max=25.6, min_pixels=16, select=("obstacle", "overhead"))
FIELDS = ("ranges", "free", "hit_xz", "pixel", "object", "support", "floor")


def _objects():
    """The objects= of tests/test_gpu_live_objects.py with room for every passing component of the frames (some 400): with
    its 32 rows the list is cut short in raster order and the nearest surfaces, low in the image, get no number."""
    import test_gpu_live_objects as glo
    return dict(glo.OBJECTS, max_objects=1024)


def _same_scan(a, b, track=True):
    names = FIELDS + (("track",) if track and a.track is not None else ())
    return (tuple(a[:4]) == tuple(b[:4]) and tuple(a[-4:]) == tuple(b[-4:]) and (not track or (a.track is None) == (b.track is None))
            and all(getattr(a, k).dtype == getattr(b, k).dtype and getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in names))


def _direct(disp, with_objects=True):
    """ops.ground_plane, ops.objects and ops.range_scan as a user calls them on the route's (padded) disparity, with the
    session's parameters -> (Scan, Objects or None)."""
    import test_gpu_live_objects as glo
    OBJECTS = _objects()
    from codd_amd import live, ops
    h, w = glm.H0, glm.W0
    rec = torch.zeros(32, dtype=torch.float64, device=DEV)
    lab, hgt = torch.empty(h, w, dtype=torch.uint8, device=DEV), torch.empty(h, w, device=DEV)
    cnt, gh = torch.empty((2,) + glo.GROUND["grid"], dtype=torch.int32, device=DEV), torch.empty(glo.GROUND["grid"], device=DEV)
    par = {k: glo.GROUND.get(k, live.GROUND_DEFAULTS[k]) for k in ops.GROUND_PARAMS}
    ops.ground_plane(disp, glm.INTRINSICS, glm.CALIB, (h, w), rec, lab, hgt, cnt, gh,
                     seed=live.ground_seed(glo.GROUND["height"], glm.INTRINSICS, glm.CALIB, pitch_deg=glo.GROUND["pitch_deg"]),
                     up=live._unit_up((0, -1, 0), glo.GROUND["pitch_deg"]), **par)
    ids, ob = None, None
    if with_objects:
        m = OBJECTS["max_objects"]
        count = torch.empty(4, dtype=torch.int32, device=DEV)
        oi, of = torch.empty(m, 8, dtype=torch.int32, device=DEV), torch.empty(m, 8, device=DEV)
        ids = torch.empty(h, w, dtype=torch.uint16, device=DEV)
        opar = {k: OBJECTS[k] for k in ("gap_px", "gap_rel", "min_pixels", "min_height") if k in OBJECTS}
        ops.objects(disp, glm.INTRINSICS, glm.CALIB, (h, w), lab, rec, count, oi, of, ids=ids,
                    select=live.select_mask(OBJECTS["select"]), **opar)
        ob = live.objects_from_buffers(count.cpu().numpy(), oi.cpu().numpy(), of.cpu().numpy(), ids.cpu().numpy())
    beams = SCAN["beams"]
    lo_, hi_ = np.arctan((0.0 - glm.INTRINSICS[2]) / glm.INTRINSICS[0]), np.arctan((w - 1.0 - glm.INTRINSICS[2]) / glm.INTRINSICS[0])
    edges = torch.from_numpy(ops.scan_edges(beams, lo_, hi_)).to(DEV)
    sc = torch.empty(4, dtype=torch.int32, device=DEV)
    si, sf = torch.empty(beams, 4, dtype=torch.int32, device=DEV), torch.empty(beams, 4, device=DEV)
    ops.range_scan(disp, glm.INTRINSICS, glm.CALIB, (h, w), lab, rec, edges, sc, si, sf, ids=ids, bins=SCAN["bins"],
                   range_max=SCAN["range_max"], min_pixels=SCAN["min_pixels"], select=live.select_mask(SCAN["select"]))
    meta = (float(lo_), float((hi_ - lo_) / beams), 0.0, SCAN["range_max"])
    return live.scan_from_buffers(sc.cpu().numpy(), si.cpu().numpy(), sf.cpu().numpy(), meta), ob


def test_session_scan_against_the_entries_by_hand():
    import test_gpu_live_ground as glg
    import test_gpu_live_objects as glo
    from codd_amd import live
    parent, plain = glm._parent_route(), glm._plain_results()
    frames = glm._frames()
    s = glm._session(ground=glo.GROUND, objects=_objects(), scan=SCAN)
    base = glm._session(ground=glo.GROUND, objects=_objects())  # without scan=: the parent's tuple and bytes
    lone = glm._session(ground=glo.GROUND, scan=SCAN)  # without objects=: no id map, every object -1
    hidden = glm._session(ground=glo.GROUND, objects=dict(_objects(), map=False), scan=SCAN)  # the id map stays on the device
    first = []
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 4
        res, g, ob, sc = got
        got1 = base.step(left, right)
        assert isinstance(got1, tuple) and len(got1) == 3
        res1, g1, ob1 = got1
        assert np.array_equal(res, plain[i]) and np.array_equal(res1, plain[i]), f"frame {i}: the depth result changed"
        assert glg._same_ground(g, g1) and glo._same_objects(ob, ob1), f"frame {i}: Ground or Objects changed with scan= on"
        assert isinstance(sc, live.Scan) and sc.ranges.shape == (48,) and sc.hit_xz.shape == (48, 2) and sc.ranges.flags["OWNDATA"]
        assert sc.hits + sc.clear + sc.unknown == 48 and sc.track is None
        want, want_ob = _direct(parent[i][0])
        print(f"frame {i}: floor {g.ok}; {sc.hits} hits, {sc.clear} clear, {sc.unknown} unknown beams, {sc.obstacle_pixels} obstacle "
              f"pixels; nearest {np.nanmin(np.where(np.isfinite(sc.ranges), sc.ranges, np.nan)) if sc.hits else None}; objects "
              f"{sorted(set(sc.object.tolist()))}")
        assert glo._same_objects(ob, want_ob) and _same_scan(sc, want), f"frame {i}: Scan differs from the direct calls"
        hit = sc.pixel >= 0
        at_hit = ob.ids.ravel()[sc.pixel[hit]].astype(np.int64)
        assert sc.object[hit].tolist() == np.where(at_hit == 0xFFFF, -1, at_hit).tolist()
        res2, g2, sc2 = lone.step(left, right)
        want2, _ = _direct(parent[i][0], with_objects=False)
        assert (sc2.object == -1).all() and _same_scan(sc2, want2), f"frame {i}: Scan without objects= differs from the direct calls"
        assert all(getattr(sc2, k).tobytes() == getattr(sc, k).tobytes() for k in FIELDS if k != "object")
        res3, g3, ob3, sc3 = hidden.step(left, right)
        assert ob3.ids is None and _same_scan(sc3, sc), f"frame {i}: Scan differs without objects=dict(map=True)"
        first.append(sc)
    kept = [tuple(getattr(sc, k).copy() for k in FIELDS) for sc in first]
    for sc in first:  # the results are the caller's: scribbling on them changes no later frame
        sc.ranges[...] = -1
        sc.object[...] = 7
    for t in (base, lone, hidden):
        t.reset()
        t.close()
    s.reset()
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
        sc = second[i][3]
        assert all(getattr(sc, k).tobytes() == v.tobytes() for k, v in zip(FIELDS, kept[i])), f"pipelined frame {i}: Scan differs from step()'s"
    s.reset()
    s.close()
    assert s._d_scan is None and s._h_scan is None and s._scan_scratch is None and s._scan_edges is None


def test_session_scan_with_tracks():
    """With tracks= the Scan's track is the Tracks' id of the hit's object, 0 where the beam names none; everything else
    has the bytes of the session without tracks=."""
    import test_gpu_live_objects as glo
    from codd_amd import live
    frames = glm._frames()
    s = glm._session(ground=glo.GROUND, objects=_objects(), tracks=dict(min_votes=4), scan=SCAN)
    base = glm._session(ground=glo.GROUND, objects=_objects(), scan=SCAN)
    plain_tracks = glm._session(ground=glo.GROUND, objects=_objects(), tracks=dict(min_votes=4))
    named = 0
    for i, (left, right) in enumerate(frames):
        got = s.step(left, right)
        assert isinstance(got, tuple) and len(got) == 5
        res, g, ob, tr, sc = got
        _, _, _, sc0 = base.step(left, right)
        _, _, _, tr0 = plain_tracks.step(left, right)
        assert isinstance(tr, live.Tracks) and isinstance(sc, live.Scan) and _same_scan(sc, sc0, track=False)
        assert tr.track.tobytes() == tr0.track.tobytes() and tuple(tr[:4]) == tuple(tr0[:4]), f"frame {i}: Tracks changed with scan= on"
        assert sc.track is not None and sc.track.dtype == np.int32 and sc.track.shape == (48,)
        want = np.where(sc.object >= 0, tr.track[np.clip(sc.object, 0, max(tr.n - 1, 0))] if tr.n else 0, 0)
        assert sc.track.tolist() == want.tolist(), f"frame {i}: track is not Tracks.track[object]"
        named += int((sc.track > 0).sum())
        print(f"frame {i}: {sc.hits} hits, objects {sorted(set(sc.object.tolist()))}, tracks {sorted(set(sc.track.tolist()))}")
    print(f"{named} beams named a track in {len(frames)} frames")
    for t in (s, base, plain_tracks):
        t.reset()
        t.close()


def test_cli_live_scan(tmp_path, capsys):
    from PIL import Image
    from codd_amd import inference
    from codd_amd.live import LiveSession
    h, w, n = 100, 200, 4
    for side, k in (("left", 0), ("right", 1)):
        os.makedirs(tmp_path / side)
        for i, pair in enumerate(glm._frames(h, w, n)):
            Image.fromarray(pair[k]).save(tmp_path / side / f"{i:03d}.png")
    inference.main(["--img-dir", str(tmp_path / "left"), "--r-img-dir", str(tmp_path / "right"), "--iters", "4", "--no-autotune",
                    "--live", "--ground", "--objects", "--scan", "--show-dir", str(tmp_path / "out")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "scan:" in ln]
    assert len(lines) == 1 and f"in {n} frames" in lines[0] and "256 beams" in lines[0]
    assert sorted(os.listdir(tmp_path / "out")) == ["left.objects.pred.npz", "left.scan.pred.npz"]
    z = np.load(tmp_path / "out" / "left.scan.pred.npz")
    assert sorted(z.files) == ["angle_increment", "angle_min", "clear", "free", "hits", "object", "obstacle_pixels", "range_max",
                               "range_min", "ranges", "unknown"]
    beams = 256
    assert z["ranges"].shape == z["free"].shape == z["object"].shape == (1, n, beams)
    assert z["ranges"].dtype == z["free"].dtype == np.float32 and z["object"].dtype == np.int32
    assert all(z[k].shape == (1, n) and z[k].dtype == np.int32 for k in ("hits", "clear", "unknown", "obstacle_pixels"))
    assert np.array_equal(z["hits"] + z["clear"] + z["unknown"], np.full((1, n), beams))
    assert float(z["range_min"]) == 0.0 and float(z["range_max"]) == 12.8
    fx, _, cx, _ = inference.CUSTOM["intrinsics"]
    assert float(z["angle_min"]) == np.arctan((0.0 - cx) / fx)
    assert abs(float(z["angle_min"]) + beams * float(z["angle_increment"]) - np.arctan((w - 1.0 - cx) / fx)) < 1e-12
    s = LiveSession(glm._estimator(iters=4), (h, w), intrinsics=inference.CUSTOM["intrinsics"], calib=inference.CUSTOM["calib"],
                    output="disp", bgr=False, ground=True, objects=True, scan=True)
    for i, (left, right) in enumerate(glm._frames(h, w, n)):
        sc = s.step(left, right)[-1]
        assert sc.ranges.tobytes() == z["ranges"][0, i].tobytes() and sc.free.tobytes() == z["free"][0, i].tobytes()
        assert np.array_equal(sc.object, z["object"][0, i]) and sc.hits == z["hits"][0, i]
    s.reset()
    s.close()
