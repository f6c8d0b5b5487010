"""LiveSession object tracks without a device: the restatement of codd_track_objects (tests/live_tracks_ref.py) on hand-made
6 x 8 id maps with the answers written out here -- a shift, a swap of raster order, a split, a merge, exact ties, votes
below and at min_votes, a frame without a field, a fresh state, the wrap of next_id and an object that leaves the image;
the restatement's mean motion against plain fp64 means; and what live.py, ops.py and the command line check before any
device call.  tests/test_gpu_live_tracks.py compares the kernels with the same restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_tracks_ref as lt  # noqa: E402

f32 = np.float32
N = lt.NONE
CROP, PADDED = (6, 8), (8, 16)
KS = (100.0, 100.0, 3.5, 2.5)
Z = 10.0


def ids_map(*boxes):
    """uint16 [6,8]: box k = (y0, y1, x0, x1), half-open, carries the id k."""
    m = np.full(CROP, N, np.uint16)
    for k, (y0, y1, x0, x1) in enumerate(boxes):
        m[y0:y1, x0:x1] = k
    return m


def two_frames(prev, cur, shift=(0.0, 0.0), min_votes=1, m=4, **kw):
    """Frame 0 (no field, fresh) on the id map ``prev``, then a frame with the field on ``cur``."""
    n_prev, n_cur = (int(v[v != N].max()) + 1 if (v != N).any() else 0 for v in (prev, cur))
    r0 = lt.track(lt.new_state(*CROP, m), None, None, KS, CROP, prev, [n_prev], max_objects=m, fresh=True)
    assert r0["count"].tolist() == [n_prev, 0, n_prev, 0]
    assert r0["trk_i"][:n_prev, 0].tolist() == list(range(1, n_prev + 1)) and r0["state"]["hdr"][:3].tolist() == [n_prev, n_prev + 1, 1]
    T, depth = lt.field(CROP, PADDED, shift, Z=Z, K=KS)
    return lt.track(r0["state"], T, depth, KS, CROP, cur, [n_cur], min_votes=min_votes, max_objects=m, **kw)


def test_shift_by_one_pixel():
    prev, cur = ids_map((1, 5, 1, 4)), ids_map((1, 5, 2, 5))
    r = two_frames(prev, cur, shift=(1.0, 0.0))
    assert r["count"].tolist() == [1, 1, 0, 0]
    assert r["trk_i"][0].tolist() == [1, 2, 0, 12, 12, 0, 0, 0]  # track 1, age 2, all 12 pixels land on the object
    tol = 2.0 ** -19 + 8 * Z * 2.0 ** -24  # the quantum's half, and a few fp32 roundings of coordinates up to Z
    assert abs(r["trk_f"][0, 0] - Z / KS[0]) < tol and abs(r["trk_f"][0, 1]) < tol and abs(r["trk_f"][0, 2]) < tol
    assert np.isnan(r["trk_f"][0, 3:6]).all() and not r["trk_i"][1:].any() and not r["trk_f"][1:].any()
    assert r["state"]["hdr"].tolist() == [1, 2, 2, 0, 0, 0, 0, 0] and r["state"]["table"].tolist() == [[1, 2], [0, 0], [0, 0], [0, 0]]
    assert np.array_equal(r["state"]["ids"], cur)
    still = two_frames(prev, cur)  # without the shift only the 8 overlapping pixels vote
    assert still["trk_i"][0].tolist() == [1, 2, 0, 8, 12, 0, 0, 0]


def test_ids_follow_objects_that_swap_raster_order():
    prev = ids_map((0, 2, 0, 3), (3, 5, 4, 7))  # A is object 0 (track 1), B object 1 (track 2)
    cur = ids_map((0, 2, 4, 7), (4, 6, 0, 3))   # B moved up and is now object 0, A moved down and is object 1
    dy = np.zeros(CROP)
    dy[prev == 0], dy[prev == 1] = 4.0, -3.0
    r = two_frames(prev, cur, shift=(0.0, dy))
    assert r["count"].tolist() == [2, 2, 0, 0]
    assert r["trk_i"][:2, :5].tolist() == [[2, 2, 1, 6, 6], [1, 2, 0, 6, 6]]
    assert r["state"]["table"][:2].tolist() == [[2, 2], [1, 2]] and r["state"]["hdr"][1] == 3


def test_split_and_merge_leave_the_id_with_the_larger_part():
    whole = ids_map((2, 4, 0, 8))
    parts = ids_map((2, 4, 0, 5), (2, 4, 6, 8))  # 10 and 4 pixels, column 5 empty
    r = two_frames(whole, parts)
    assert r["count"].tolist() == [2, 1, 1, 0]
    assert r["trk_i"][:2, :5].tolist() == [[1, 2, 0, 10, 16], [2, 1, -1, 0, 0]] and np.isnan(r["trk_f"][1, :6]).all()
    two = ids_map((2, 4, 0, 3), (2, 4, 4, 8))  # 6 and 8 pixels
    r = two_frames(two, whole)
    assert r["count"].tolist() == [1, 1, 0, 1]  # the smaller object's track ends
    assert r["trk_i"][0, :5].tolist() == [2, 2, 1, 8, 8]


def test_exact_ties_go_to_the_smaller_index():
    two = ids_map((2, 4, 0, 2), (2, 4, 4, 6))  # 4 and 4 pixels
    r = two_frames(two, ids_map((2, 4, 0, 8)))
    assert r["V"][:2, 0].tolist() == [4, 4] and r["count"].tolist() == [1, 1, 0, 1] and r["trk_i"][0, :4].tolist() == [1, 2, 0, 4]
    r = two_frames(ids_map((2, 4, 0, 4)), ids_map((2, 4, 0, 2), (2, 4, 2, 4)))  # one object, halves of 4 and 4
    assert r["V"][0, :2].tolist() == [4, 4] and r["count"].tolist() == [2, 1, 1, 0]
    assert r["trk_i"][:2, :4].tolist() == [[1, 2, 0, 4], [2, 1, -1, 0]]


def test_min_votes_below_and_at():
    prev, cur = ids_map((0, 1, 0, 5)), ids_map((0, 1, 0, 8))  # 5 votes
    assert two_frames(prev, cur, min_votes=6)["count"].tolist() == [1, 0, 1, 1]
    r = two_frames(prev, cur, min_votes=5)
    assert r["count"].tolist() == [1, 1, 0, 0] and r["trk_i"][0, :4].tolist() == [1, 2, 0, 5]


def test_no_field_fresh_and_wrap():
    m = 4
    prev = ids_map((0, 2, 0, 3), (3, 5, 4, 7))
    r0 = lt.track(lt.new_state(*CROP, m), None, None, KS, CROP, prev, [2], max_objects=m, fresh=True)
    r1 = lt.track(r0["state"], None, None, KS, CROP, prev, [2], max_objects=m)  # T = None: nothing is associated
    assert r1["count"].tolist() == [2, 0, 2, 2] and r1["trk_i"][:2, :3].tolist() == [[3, 1, -1], [4, 1, -1]]
    assert r1["state"]["hdr"][:3].tolist() == [2, 5, 2]
    T, depth = lt.field(CROP, PADDED, Z=Z, K=KS)
    r2 = lt.track(r1["state"], T, depth, KS, CROP, prev, [2], min_votes=1, max_objects=m, fresh=True)  # contents irrelevant
    assert r2["count"].tolist() == [2, 0, 2, 0] and r2["trk_i"][:2, 0].tolist() == [1, 2] and r2["state"]["hdr"][:3].tolist() == [2, 3, 1]
    top = 2 ** 31 - 1 - m
    for nid, want in ((top, [top, top + 1]), (top + 1, [1, 2])):  # the last ids before the wrap, and the wrap
        st = dict(r0["state"], hdr=np.array([0, nid, 7, 0, 0, 0, 0, 0], np.int32))
        r = lt.track(st, T, depth, KS, CROP, prev, [2], max_objects=m)
        assert r["trk_i"][:2, 0].tolist() == want and r["state"]["hdr"][:3].tolist() == [2, want[1] + 1, 8]
    r = lt.track(r0["state"], T, depth, KS, CROP, prev, [9], min_votes=1, max_objects=m)  # count[0] > max_objects
    assert r["count"][0] == m


def test_object_that_leaves_the_image_ends():
    prev, cur = ids_map((1, 3, 5, 8)), ids_map((3, 5, 0, 3))
    r = two_frames(prev, cur, shift=(100.0, 0.0))
    assert r["count"].tolist() == [1, 0, 1, 1] and r["n"][0] == 6 and not r["V"].any()
    assert r["trk_i"][0].tolist() == [2, 1, -1, 0, 0, 0, 0, 0]


def test_mean_motion_against_fp64():
    """motion and own of the restatement against plain fp64 means over the same pixels.
    (a) Against the fp64 mean of the fp32 displacements the bound is 2^-19 + 2^-23 |mean| per component: each term is
    quantised to a multiple of 2^-18 (error <= 2^-19, and so is the error of the mean), the int64 sum is exact, the fp64
    divisions add ~2^-52 relative and the result is rounded to fp32 once (2^-24 |mean|, counted twice for slack).
    (b) Against displacements whose geometry runs in fp64 from the same fp32 inputs the fp32 geometry adds its own
    rounding: with M the largest |coordinate| of X0 and X1 (at least 1) every intermediate of inv_project and qrot (uv = 2 u
    x X0, w uv, u x uv for a unit q) is below 4 sqrt(3) M < 7 M, and a coordinate of X1 - X0 passes through fewer than 24
    roundings of such values plus the subtraction's own (2 M): fewer than 24 * 7 + 2 < 200 roundings of M 2^-24 each, times
    scale.  So the bound of (b) is that of (a) plus 200 scale M 2^-24, derived from the operation count, not measured."""
    h, w, m = 37, 53, 8
    crop, padded = (h, w), (64, 64)
    rng = np.random.default_rng(5)
    K = (80.0, 75.0, 25.25, 18.5)
    T = np.full(padded + (7,), np.nan, f32)
    depth = np.full(padded, np.nan, f32)
    depth[:h, :w] = rng.uniform(2.0, 9.0, (h, w))
    q = np.array([0.01, -0.02, 0.015, 1.0])
    T[:h, :w, 3:7] = (q / np.linalg.norm(q)).astype(f32)
    T[:h, :w, 0:3] = np.array([0.05, -0.02, 0.3], f32) + rng.normal(0, 0.01, (h, w, 3)).astype(f32)
    prev = np.full(crop, N, np.uint16)
    prev[3:30, 4:25], prev[8:35, 30:50] = 0, 1
    ego = np.zeros(16, f32)
    eq = np.array([0.002, 0.001, -0.003, 1.0])
    ego[0:3], ego[3:7], ego[7] = (0.01, 0.0, 0.05), eq / np.linalg.norm(eq), 1.0
    scale = 0.37
    st = lt.track(lt.new_state(h, w, m), None, None, K, crop, prev, [2], max_objects=m, fresh=True)["state"]
    r = lt.track(st, T, depth, K, crop, prev, [2], ego=ego, scale=scale, max_objects=m)
    assert r["count"].tolist() == [2, 2, 0, 0]
    a, valid, _, _, D32, O32 = lt.pixels(st, T, depth, K, crop, prev, 2, 2, ego, scale)
    X0, X1, _ = lt.geometry(T, depth, K, crop, np.float64)
    Y = lt.qrot(tuple(np.float64(v) for v in ego[3:7]), X0, np.float64)
    s64 = np.float64(f32(scale))
    D64 = np.stack([s64 * (X1[k] - X0[k]) for k in range(3)])
    O64 = np.stack([s64 * (X1[k] - Y[k]) - np.float64(ego[k]) for k in range(3)])
    M = max(1.0, max(float(np.abs(v[:h, :w]).max()) for v in X0 + X1))
    geo = 200.0 * scale * M * 2.0 ** -24
    for obj in range(2):
        sel = valid & (a == obj)
        assert sel.sum() == r["trk_i"][obj, 4] == r["trk_i"][obj, 6] > 400
        for got, v32, v64 in ((r["trk_f"][obj, 0:3], D32, D64), (r["trk_f"][obj, 3:6], O32, O64)):
            for k in range(3):
                plain32, plain64 = float(v32[k][sel].astype(np.float64).mean()), float(v64[k][sel].mean())
                b = 2.0 ** -19 + 2.0 ** -23 * abs(plain32)
                print(f"object {obj} component {k}: {got[k]!r} vs fp64 mean of the fp32 terms {plain32!r} (|diff| "
                      f"{abs(got[k] - plain32):.3e}, bound {b:.3e}), of fp64 terms {plain64!r} (|diff| {abs(got[k] - plain64):.3e}, "
                      f"bound {b + geo:.3e})")
                assert abs(float(got[k]) - plain32) <= b
                assert abs(float(got[k]) - plain64) <= 2.0 ** -19 + 2.0 ** -23 * abs(plain64) + geo


def test_quantise_and_state_layout():
    v = np.array([0.0, 1.0, -1.0, 2.0 ** -19, 3 * 2.0 ** -19, 5000.0, -np.inf, np.nan, 1e-30], f32)
    assert lt.quantise(v).tolist() == [0, 262144, -262144, 0, 2, 4096 * 262144, -4096 * 262144, -4096 * 262144, 0]
    st = lt.new_state(2, 3, 2)
    st["hdr"][:3], st["table"][0], st["ids"][0, 1] = (1, 5, 9), (4, 2), 0
    raw = lt.state_bytes(st)
    assert len(raw) == 32 + 16 + 12 and np.frombuffer(raw, np.int32, 12)[[0, 1, 2, 8, 9]].tolist() == [1, 5, 9, 4, 2]
    assert np.frombuffer(raw, np.uint16, 6, 48).tolist() == [N, 0, N, N, N, N]


def test_gpu_cases_show_what_they_are_built_for():
    """The cases tests/test_gpu_live_tracks.py runs on the device, on the restatement: what each is there to show."""
    refs = {c["name"]: (c, lt.reference(c)) for c in lt.CASES}
    for name in ("shift-3.5", "shift0", "shift+7.25", "ego-moving", "ego-not-ok"):
        r = refs[name][1]
        assert [x["count"].tolist() for x in r] == [[3, 0, 3, 0], [3, 3, 0, 0], [3, 3, 0, 0]], name
        assert r[2]["trk_i"][:3, :3].tolist() == [[1, 3, 0], [2, 3, 1], [3, 3, 2]]
        assert r[1]["trk_i"][:3, 4].tolist() == [1040, 2000, 910]
        if name in ("shift0", "ego-moving"):  # a small rotation on top: the boxes' borders land beside their objects
            assert (r[1]["trk_i"][:3, 3] < r[1]["trk_i"][:3, 4]).all() and (r[1]["trk_i"][:3, 3] > 800).all()
        else:  # every pixel lands on its object
            assert r[1]["trk_i"][:3, 3].tolist() == [1040, 2000, 910], name
    c, r = refs["shift-3.5"]
    _, _, cxy = lt.geometry(c["frames"][1]["T"], c["frames"][1]["depth"], c["K"], c["crop"])
    frac = (cxy[0] + f32(0.5)) % 1
    assert (frac == 0).any() and (frac > 0.99).any() and (frac < 0.01).any()  # c.x + 0.5 on integers and on either side
    r = refs["ego-moving"][1][1]
    assert (r["trk_i"][:3, 6] == r["trk_i"][:3, 4]).all() and (r["trk_i"][:3, 5] > 200).all() and np.isfinite(r["trk_f"][:3, :6]).all()
    r = refs["ego-not-ok"][1][1]
    assert not r["trk_i"][:3, 6].any() and np.isnan(r["trk_f"][:3, 3:6]).all() and (r["trk_i"][:3, 5] > 200).all()
    r = refs["leaving"][1][1]  # object 0 partly out on the right, 1 wholly out (its track ends), 2 partly out on the left
    assert r["count"].tolist() == [2, 2, 0, 1] and r["trk_i"][:2, :5].tolist() == [[3, 2, 2, 700, 800], [1, 2, 0, 300, 750]]
    assert r["n"][:3].tolist() == [750, 800, 800] and not r["V"][1].any()
    r = refs["invalid"][1][1]  # 7 of the 8 depth rows and 6 of the 8 field rows are invalid (0.05 and t_z = -9.94 are not)
    assert r["trk_i"][:2, 4].tolist() == [30 * 50 - 7 * 28, 30 * 70 - 6 * 55] and r["count"].tolist() == [2, 2, 0, 0]
    r = refs["whole-crop"][1]
    assert r[1]["trk_i"][0, 4] == 70 * 150 == r[1]["trk_i"][0, 5] and r[2]["trk_i"][0, :3].tolist() == [1, 3, 0]
    r = refs["checkerboard"][1][1]  # every 1-pixel object lands on its right neighbour; the last of a row leaves the image
    assert r["count"].tolist() == [1024, 1010, 14, 14] and r["trk_i"][1, :5].tolist() == [1, 2, 0, 1, 1]
    assert [x["count"].tolist() for x in refs["n-cur-0"][1]] == [[2, 0, 2, 0], [0, 0, 0, 2], [2, 0, 2, 0]]
    assert [x["count"].tolist() for x in refs["n-prev-0"][1]] == [[0, 0, 0, 0], [2, 0, 2, 0], [2, 2, 0, 0]]
    r = refs["truncated"][1]
    assert r[2]["count"].tolist() == [4, 4, 0, 0] and r[2]["trk_i"][:, 0].tolist() == [1, 2, 3, 4] and r[2]["n"].sum() == 1600
    r = refs["split-merge-tie"][1]
    # frame 1: objects 0, 1 = the halves of old 3 (a tie: the first keeps track 4), 2, 3 = the parts of old 0 (the larger
    # keeps track 1), 4 = old 1 and old 2 merged (a tie: track 2 stays); frame 2: back again
    assert r[1]["count"].tolist() == [5, 3, 2, 1] and r[1]["trk_i"][:5, 0].tolist() == [4, 5, 1, 6, 2]
    assert r[1]["trk_i"][:5, 2].tolist() == [3, -1, 0, -1, 1] and r[1]["V"][1, 4] == r[1]["V"][2, 4] == 800
    assert r[2]["count"].tolist() == [4, 3, 1, 2] and r[2]["trk_i"][:4, :3].tolist() == [[1, 3, 2], [2, 3, 4], [7, 1, -1], [4, 3, 0]]
    r = refs["min-votes"][1][1]  # 15 votes start a track, 16 continue one
    assert r["count"].tolist() == [2, 1, 1, 1] and r["trk_i"][:2, :4].tolist() == [[3, 1, -1, 0], [2, 2, 1, 16]]
    r = refs["wrap"][1][0]
    assert r["trk_i"][:3, :2].tolist() == [[2 ** 31 - 257, 8], [5, 4], [1, 1]] and r["state"]["hdr"][:3].tolist() == [3, 2, 42]
    for name in ("crop-1x150", "crop-70x1", "crop-5x7"):
        r = refs[name][1][1]
        assert r["count"][1] >= 2 and r["trk_i"][:, 6].sum() == r["trk_i"][:, 4].sum() > 0, name


# ---- live.py, ops.py, the command line: what is checked before any device call ---------------------------------------
class _Est:
    def __init__(self, motion=True):
        self.motion = object() if motion else None


def test_check_tracks():
    from codd_amd import live, ops
    objs = live._check_objects(True)
    assert live._check_tracks(False) is None and live._check_tracks(None) is None
    assert live._check_tracks(True, objs, _Est()) == live.TRACK_DEFAULTS == ops.TRACK_PARAMS == dict(min_votes=16)
    assert live._check_tracks(dict(min_votes=3), objs, _Est()) == dict(min_votes=3)
    assert ops.TRACK_MAX == 1024
    for bad, o, est in ((True, None, _Est()), (True, objs, _Est(False)), (True, dict(objs, max_objects=1025), _Est()),
                        (dict(speed=1), objs, _Est()), (dict(min_votes=0), objs, _Est()), (dict(min_votes=2.5), objs, _Est()),
                        (dict(min_votes=True), objs, _Est()), ("yes", objs, _Est()), (3, objs, _Est())):
        with pytest.raises(ValueError):
            live._check_tracks(bad, o, est)
    with pytest.raises(ValueError):  # the session: tracks without objects, before anything is built
        live.LiveSession(_Est(), (64, 64), tracks=True)
    with pytest.raises(ValueError):
        live.LiveSession(_Est(False), (64, 64), ground=True, objects=True, tracks=True)


def test_tracks_from_buffers():
    from codd_amd import live
    m = 4
    ti, tf = np.zeros((m, 8), np.int32), np.zeros((m, 8), f32)
    ti[0], ti[1] = (7, 3, 1, 40, 44, 5, 44, 0), (9, 1, -1, 0, 0, 0, 0, 0)
    tf[0, :6], tf[1, :6] = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6), np.nan
    t = live.tracks_from_buffers(np.array([2, 1, 1, 3], np.int32), ti, tf)
    assert t._fields == ("n", "continued", "started", "ended", "track", "age", "prev", "votes", "pixels", "moving", "own_pixels",
                         "motion", "own")
    assert (t.n, t.continued, t.started, t.ended) == (2, 1, 1, 3)
    assert t.track.tolist() == [7, 9] and t.age.tolist() == [3, 1] and t.prev.tolist() == [1, -1] and t.votes.tolist() == [40, 0]
    assert t.pixels.tolist() == [44, 0] and t.moving.tolist() == [5, 0] and t.own_pixels.tolist() == [44, 0]
    assert t.motion.shape == t.own.shape == (2, 3) and t.motion.dtype == np.float32 and np.isnan(t.motion[1]).all()
    assert t.motion[0].tolist() == tf[0, :3].tolist() and t.own[0].tolist() == tf[0, 3:6].tolist()
    ti[...] = -1  # copies: the buffers may be reused
    assert t.track.tolist() == [7, 9]


def test_ops_track_objects_checks_arguments_without_a_device():
    import torch
    from codd_amd import _abi, ops
    h, w, m = 6, 8, 4
    ids, count = torch.zeros(h, w, dtype=torch.uint16), torch.zeros(4, dtype=torch.int32)
    out = (torch.zeros(4, dtype=torch.int32), torch.zeros(m, 8, dtype=torch.int32), torch.zeros(m, 8))
    state = torch.zeros(256, dtype=torch.uint8)
    args = (None, None, KS, (h, w), ids, count, state) + out
    for bad in (dict(max_objects=0), dict(max_objects=1025), dict(min_votes=0, max_objects=m), dict(min_votes=1.5, max_objects=m)):
        with pytest.raises(ValueError):
            ops.track_objects(*args, **bad)
    with pytest.raises(ValueError):
        ops.track_objects(None, None, KS, (0, w), ids, count, state, *out, max_objects=m)
    with pytest.raises(ValueError):  # T without depth_prev
        ops.track_objects(torch.zeros(1, h, w, 7), None, KS, (h, w), ids, count, state, *out, max_objects=m)
    with pytest.raises(_abi.CoddHipError):  # no CPU fallback
        ops.track_objects(*args, max_objects=m)
    for fn in (ops.track_state_bytes, ops.track_scratch):
        for bad in ((0, 5, 4), (5, 0, 4), (5, 5, 0), (5, 5, 1025), (65536, 32768, 4)):
            with pytest.raises(ValueError):
                fn(*bad)


def test_cli_parser_tracks():
    from codd_amd import inference
    base = ["--img-dir", "x", "--r-img-dir", "y"]
    for argv in (["--tracks"], ["--live", "--tracks"], ["--live", "--ground", "--tracks"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)
    assert inference.parse_args(base + ["--live", "--ground", "--objects", "--tracks"]).tracks
    assert not inference.parse_args(base + ["--live", "--ground", "--objects"]).tracks
