"""LiveSession obstacle objects without a GPU: the restatement of tests/live_objects_ref.py against
scipy.sparse.csgraph.connected_components on the same edge list, the key rule, the numbering, truncation and the nearest
pixel's tie on hand-made 6 x 8 maps with the answers written out, what each GPU case is built to show (asserted on the
restatement alone), objects= validation, the ABI binding, the size function and the CODD_EINVAL list of the entry called
with no device, and the host converter."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_objects_ref as lo  # noqa: E402
from codd_amd import live  # noqa: E402

IDS = [lo.case_id(c) for c in lo.CASES]
_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = lo.reference(lo.CASES[lo.NAMES[name]])
    return _REF[name]


@pytest.mark.parametrize("name", IDS)
def test_partition_equals_scipy(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix
    c = lo.CASES[lo.NAMES[name]]
    h, w = c["crop"]
    fg = lo.foreground(c)
    right, down = lo.edges(c, fg)
    idx = np.arange(h * w).reshape(h, w)
    a = np.concatenate([idx[:, :-1][right], idx[:-1, :][down]])
    b = np.concatenate([idx[:, 1:][right], idx[1:, :][down]])
    n, lab = csgraph.connected_components(coo_matrix((np.ones(a.size), (a, b)), shape=(h * w, h * w)), directed=False)
    smallest = np.full(n, h * w)
    np.minimum.at(smallest, lab, idx.ravel())  # scipy's label -> the component's smallest raster index
    want = np.where(fg, smallest[lab].reshape(h, w), -1)
    assert np.array_equal(lo.components(c, fg), want)
    assert _ref(name)["count"][2] == np.unique(want[fg]).size and _ref(name)["count"][3] == int(fg.sum())


MAP = np.array([[1, 1, 0, 0, 0, 1, 0, 0],
                [0, 1, 0, 1, 0, 1, 0, 1],
                [0, 1, 1, 1, 0, 0, 0, 1],
                [0, 0, 0, 0, 0, 1, 1, 1],
                [1, 0, 0, 0, 0, 0, 0, 0],
                [1, 1, 0, 0, 0, 0, 0, 0]], np.uint8)
N = lo.NONE


def _hand(**par):
    d = np.full((6, 8), 8.0, np.float32)
    d[1, 3] = d[2, 3] = 9.0  # two equally near pixels of the first component; |8 - 9| <= gap_px joins them
    return lo.reference(lo.make("hand", MAP, d, padded=(64, 64), min_height=lo.ANY_HEIGHT, **par))


def test_hand_made_map_keys_order_and_nearest():
    r = _hand(min_pixels=1)
    assert r["count"].tolist() == [4, 4, 4, 17]
    # (pixels, x0, y0, x1, y1, near_x, near_y, key): keys 0, 5, 1 * 8 + 7, 4 * 8 + 0, ascending
    assert r["obj_i"][:4].tolist() == [[7, 0, 0, 3, 2, 3, 1, 0],  # nearest: (1, 3) before (2, 3) in the raster
                                       [2, 5, 0, 5, 1, 5, 0, 5],  # all pixels equally near: the first in the raster
                                       [5, 5, 1, 7, 3, 7, 1, 15],
                                       [3, 0, 4, 1, 5, 0, 4, 32]]
    assert not r["obj_i"][4:].any() and not r["obj_f"][4:].any()
    assert r["obj_f"][:4, 6].tolist() == [8.0] * 4 and r["obj_f"][:4, 7].tolist() == [9.0, 8.0, 8.0, 8.0]
    assert r["ids"].tolist() == [[0, 0, N, N, N, 1, N, N],
                                 [N, 0, N, 0, N, 1, N, 2],
                                 [N, 0, 0, 0, N, N, N, 2],
                                 [N, N, N, N, N, 2, 2, 2],
                                 [3, N, N, N, N, N, N, N],
                                 [3, 3, N, N, N, N, N, N]]


def test_hand_made_map_selection_and_truncation():
    r = _hand(min_pixels=3)  # the 2-pixel component is dropped and the numbering closes up
    assert r["count"].tolist() == [3, 3, 4, 17] and r["obj_i"][:3, 7].tolist() == [0, 15, 32] and not r["obj_i"][3:].any()
    assert r["ids"][0, 5] == N and r["ids"][1, 7] == 1 and r["ids"][4, 0] == 2
    r = _hand(min_pixels=3, max_objects=2)  # the first two in key order stay; found says there were three
    assert r["count"].tolist() == [2, 3, 4, 17] and r["obj_i"].shape == (2, 8) and r["obj_i"][:, 7].tolist() == [0, 15]
    assert r["ids"][4, 0] == N and r["ids"][5, 1] == N and r["ids"][3, 6] == 1
    r = _hand(min_pixels=1, gap_px=0.5, gap_rel=0.0)  # the step of 1 now splits (1, 3) and (2, 3) off, joined to each other
    assert r["count"].tolist() == [5, 5, 5, 17] and r["obj_i"][:5, 7].tolist() == [0, 5, 11, 15, 32]
    assert r["obj_i"][0].tolist() == [5, 0, 0, 2, 2, 0, 0, 0] and r["obj_i"][2].tolist() == [2, 3, 1, 3, 2, 3, 1, 11]


def test_cases_show_what_they_are_built_for():
    h, w = lo.CROP
    count = lambda name: _ref(name)["count"].tolist()  # noqa: E731
    path = int((lo.CASES[lo.NAMES["serpentine"]]["labels"] == 1).sum())
    assert count("serpentine") == [1, 1, 1, path] and path == 35 * w + 35
    assert count("comb")[:3] == [1, 1, 1] and count("u")[:3] == [1, 1, 1]
    assert count("checkerboard") == [256, h * w // 2, h * w // 2, h * w // 2]  # truncated: found > n
    assert count("exactly-max") == [37, 37, 37, 37] and count("max-plus-one") == [37, 38, 38, 38]
    assert count("boxes-split")[:3] == [2, 2, 2] and count("boxes-joined")[:3] == [1, 1, 1]
    r = _ref("slant")
    assert r["count"][:3].tolist() == [1, 1, 1] and r["obj_f"][0, 7] - r["obj_f"][0, 6] == 74.5
    assert count("gap-rel")[:3] == [3, 3, 3]  # the near pair is one component, the far pair two
    r = _ref("min-pixels")
    assert r["count"].tolist() == [1, 1, 2, 127] and r["obj_i"][0, 0] == 64
    assert (r["ids"][28:36, 124:132] == N).all() and (r["ids"][12:20, 60:68] == 0).all()
    r = _ref("near-tie")
    assert r["count"][0] == 1 and r["obj_i"][0, 5:7].tolist() == [25, 20] and r["obj_f"][0, 7] == 12.0
    r = _ref("bad-disparity")
    c = lo.CASES[lo.NAMES["bad-disparity"]]
    assert r["count"][3] == int((c["disp"][:h, :w] == 8.0).sum()) and 0 < r["count"][3] < h * w
    r = _ref("two-labels")
    lab = lo.CASES[lo.NAMES["two-labels"]]["labels"]
    assert r["count"][3] == int(((lab == 1) | (lab == 2)).sum()) and r["count"][2] == 3  # 150 columns: 3 obstacle + overhead bands
    assert count("all-foreground") == [1, 1, 1, h * w] and _ref("all-foreground")["obj_i"][0].tolist() == [h * w, 0, 0, w - 1, h - 1, 0, 0, 0]
    for name in ("no-foreground", "no-floor"):
        r = _ref(name)
        assert not r["count"].any() and not r["obj_i"].any() and not r["obj_f"].any() and (r["ids"] == N).all()
    assert count("one-row") == [1, 1, 1, 150] and count("one-column") == [1, 1, 1, 70] and count("five-by-seven") == [18] * 4
    r = _ref("both-signs")
    assert r["count"][0] == 1 and r["obj_f"][0, 0] < 0 < r["obj_f"][0, 1] and r["obj_f"][0, 2] < 0 < r["obj_f"][0, 3]
    assert count("min-height-kept")[:3] == [1, 1, 2] and count("min-height-dropped")[:3] == [0, 0, 2]
    r = _ref("min-height-kept")
    assert r["obj_i"][0, 7] == 10 * w + 20 and (r["ids"][14:34, 90:120] == N).all()


def test_ordered_image():
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    o = lo.ordered(v)
    assert (np.diff(o.astype(np.int64)) > 0).all() and lo.unordered(o).tobytes() == v.tobytes()


BAD = [3, "yes", dict(speed=1), dict(select=()), dict(select=("wall",)), dict(select=1), dict(select=("obstacle", 2)),
       dict(gap_px=0.0), dict(gap_px=-1.0), dict(gap_px=float("nan")), dict(gap_px="x"), dict(gap_rel=-0.1),
       dict(gap_rel=float("inf")), dict(min_pixels=0), dict(min_pixels=2.0), dict(min_pixels=True),
       dict(min_height=float("nan")), dict(min_height=None), dict(max_objects=0), dict(max_objects=4097),
       dict(max_objects=8.0), dict(map=1), dict(map="yes")]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_check_objects_rejects(bad):
    with pytest.raises(ValueError, match="objects"):
        live._check_objects(bad)
    with pytest.raises(ValueError, match="objects"):  # before the estimator is looked at: no device call
        live.LiveSession(None, (8, 8), ground=True, objects=bad)


def test_check_objects_accepts():
    from codd_amd import ops
    assert live._check_objects(False) is None and live._check_objects(None) is None
    assert live._check_objects(True) == live.OBJECT_DEFAULTS and live._check_objects(True) is not live.OBJECT_DEFAULTS
    assert live.OBJECT_DEFAULTS == dict(select=("obstacle",), gap_px=1.0, gap_rel=0.05, min_pixels=64, min_height=0.15,
                                        max_objects=256, map=False)
    p = live._check_objects(dict(select=["obstacle", "overhead"], gap_px=2, max_objects=4096, map=True, min_height=-1))
    assert p == dict(live.OBJECT_DEFAULTS, select=("obstacle", "overhead"), gap_px=2.0, max_objects=4096, map=True, min_height=-1.0)
    assert isinstance(p["gap_px"], float) and live._check_objects(dict(select="floor"))["select"] == ("floor",)
    assert live.select_mask(("obstacle",)) == 2 == ops.OBJECT_PARAMS["select"] and live.select_mask(("floor", "below", "floor")) == 9
    assert set(ops.OBJECT_PARAMS) | {"map"} == set(live.OBJECT_DEFAULTS)
    assert all(ops.OBJECT_PARAMS[k] == live.OBJECT_DEFAULTS[k] for k in ops.OBJECT_PARAMS if k != "select")
    assert live.Objects._fields == ("n", "found", "components", "foreground", "pixels", "box", "near_px", "key", "extent",
                                    "height", "disparity", "ids")


def test_objects_need_ground():
    for objects in (True, dict(map=True)):
        with pytest.raises(ValueError, match="objects: needs ground"):
            live.LiveSession(None, (8, 8), objects=objects)
        with pytest.raises(ValueError, match="objects: needs ground"):
            live.LiveSession(None, (8, 8), ground=False, objects=objects)
    s = live.LiveSession(None, (48, 64), ground=True, objects=dict(select=("obstacle", "overhead"), max_objects=16))
    assert not s._open_done and s._objects_par == dict(select=6, gap_px=1.0, gap_rel=0.05, min_pixels=64, min_height=0.15,
                                                       max_objects=16)
    assert live.LiveSession(None, (48, 64), ground=True).objects is None


def test_entries_are_bound():
    from codd_amd import _abi
    _abi.load()
    assert not _abi.MISSING and _abi.load().codd_abi_version() == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "codd_hip.h")).read()
    for name in ("codd_objects_scratch", "codd_objects"):
        assert name in _abi.SIGNATURES and f" {name}(" in header


def test_entry_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    import ctypes as C
    from codd_amd import _abi
    lib = _abi.load()
    scr = lib.codd_objects_scratch
    assert scr(0, 4, 8) == -1 and scr(4, -1, 8) == -1 and scr(65536, 32768, 8) == -1 and scr(4, 4, 0) == -1 and scr(4, 4, 4097) == -1
    for h, w in ((1, 1), (37, 53), (540, 960), (46340, 46340)):  # 1024 chunk rows, parents (padded to 16), 64 per pixel
        n = h * w
        assert scr(h, w, 1) == scr(h, w, 4096) == 16 + 16 * 1024 + (4 * n + 15) // 16 * 16 + 64 * n
    need = scr(24, 40, 256)
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = buf.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def call(disp=p, H=64, W=64, h=24, w=40, fx=40.0, fy=40.0, cx=20.0, cy=8.0, calib=20.0, labels=p, record=p, select=2,
             gap_px=1.0, gap_rel=0.05, min_pixels=64, min_height=0.15, max_objects=256, scratch=p, nbytes=need, count=p,
             obj_i=p, obj_f=p, ids=None):
        return lib.codd_objects(disp, H, W, h, w, fx, fy, cx, cy, calib, labels, record, select, gap_px, gap_rel, min_pixels,
                                min_height, max_objects, scratch, nbytes, count, obj_i, obj_f, ids, None)

    for name in ("disp", "labels", "record", "scratch", "count", "obj_i", "obj_f"):
        assert call(**{name: None}) == -1, name
    for bad in (dict(h=0), dict(w=0), dict(H=0), dict(W=-3), dict(h=65), dict(w=65), dict(H=65536, W=32768, h=65536, w=32768),
                dict(max_objects=0), dict(max_objects=4097), dict(max_objects=-1), dict(select=0), dict(gap_px=0.0),
                dict(gap_px=-1.0), dict(gap_px=nan), dict(gap_px=inf), dict(gap_rel=-0.01), dict(gap_rel=nan), dict(min_pixels=0),
                dict(min_pixels=-5), dict(min_height=nan), dict(fx=0.0), dict(fy=nan), dict(calib=inf), dict(cx=nan),
                dict(cy=inf), dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**bad) == -1, bad


def test_objects_from_buffers():
    r = _hand(min_pixels=3)
    ob = live.objects_from_buffers(r["count"], r["obj_i"], r["obj_f"], r["ids"])
    assert isinstance(ob, live.Objects) and (ob.n, ob.found, ob.components, ob.foreground) == (3, 3, 4, 17)
    assert ob.pixels.tolist() == [7, 5, 3] and ob.pixels.dtype == np.int32 and ob.key.tolist() == [0, 15, 32]
    assert ob.box.tolist() == [[0, 0, 3, 2], [5, 1, 7, 3], [0, 4, 1, 5]] and ob.near_px.tolist() == [[3, 1], [7, 1], [0, 4]]
    assert ob.extent.shape == (3, 4) and ob.extent.dtype == np.float32 and np.array_equal(ob.extent, r["obj_f"][:3, 0:4])
    assert np.array_equal(ob.height, r["obj_f"][:3, 4:6]) and np.array_equal(ob.disparity, r["obj_f"][:3, 6:8])
    assert ob.ids is r["ids"] and not np.shares_memory(ob.pixels, r["obj_i"]) and not np.shares_memory(ob.extent, r["obj_f"])
    none = live.objects_from_buffers(np.zeros(4, np.int32), np.zeros((8, 8), np.int32), np.zeros((8, 8), np.float32))
    assert none.n == 0 and none.pixels.shape == (0,) and none.box.shape == (0, 4) and none.height.shape == (0, 2) and none.ids is None


class _Done:
    def synchronize(self):
        pass


def test_tuple_order():
    """result[, ground][, objects]: the collection step on host buffers standing in for the downloads."""
    import torch
    r = _hand(min_pixels=3)
    rec = torch.zeros(32, dtype=torch.float64)
    rec[3] = 1.0
    for with_map in (True, False):
        s = live.LiveSession(None, (6, 8), ground=True, objects=dict(map=with_map))
        s._e_down, s._h_out = [_Done(), _Done()], [torch.zeros(6, 8)] * 2
        s._h_ground = [[rec, torch.zeros(6, 8, dtype=torch.uint8)]] * 2
        bufs = [torch.from_numpy(r["count"].copy()), torch.from_numpy(r["obj_i"].copy()), torch.from_numpy(r["obj_f"].copy())]
        s._h_objects = [bufs + ([torch.from_numpy(r["ids"].copy())] if with_map else [])] * 2
        s._inflight.append(0)
        got = s.pop()
        assert isinstance(got, tuple) and len(got) == 3 and isinstance(got[1], live.Ground) and isinstance(got[2], live.Objects)
        ob = got[2]
        assert ob.n == 3 and ob.key.tolist() == [0, 15, 32] and (ob.ids is None) == (not with_map)
        bufs[1].zero_()  # the result is the caller's: the session's slot may be reused
        assert ob.pixels.tolist() == [7, 5, 3]
        if with_map:
            assert ob.ids.dtype == np.uint16 and np.array_equal(ob.ids, r["ids"]) and ob.ids.flags["OWNDATA"]


def test_cli_objects_arguments():
    from codd_amd import inference
    base = ["--img-dir", "x", "--r-img-dir", "y"]
    for argv in (["--objects"], ["--live", "--objects"]):  # needs --ground (which needs --live)
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)
    assert inference.parse_args(base + ["--live", "--ground", "--objects"]).objects
    assert not inference.parse_args(base + ["--live", "--ground"]).objects
