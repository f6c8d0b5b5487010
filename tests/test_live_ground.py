"""LiveSession ground plane on the CPU: the restatement of tests/live_ground_ref.py recovers planted floors (and recognises
the one scene it cannot), its cases leave few undecided pixels, live.ground_seed is the closed form, LiveSession's ground=
validation makes no device call, the tuple order, the entry's argument checks and the command line's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ground_ref as lg  # noqa: E402

from codd_amd import live  # noqa: E402

_CACHE = {}
IDS = [lg.case_id(s) for s in lg.CASES]
# A fit that found the floor errs by the noise averaged over thousands of pixels plus the bias of the asymmetric weight,
# a fraction of the noise's sigma; one that locked onto something else errs by pixels.  The planted plane is recovered
# when the two planes differ by less than one sigma of the disparity noise at every floor pixel of the crop.
RECOVERED_PX = lg.NOISE_PX


def _ref(i):
    if i not in _CACHE:
        c = lg.case(lg.CASES[i])
        _CACHE[i] = (c, lg.reference(c))
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(lg.CASES)), ids=IDS)
def test_restatement_against_reference(i):
    c, ref = _ref(i)
    r64, r32 = ref["r64"], ref["r32"]
    f, m = r64["fit"], r64["plane"]
    h, w = c["crop"]
    nv, und = int(ref["valid"].sum()), int(ref["undecided"].sum())
    yy, xx = np.mgrid[0:h, 0:w]
    err = np.abs(lg.plane_disp(f["coef"], c["K"], xx, yy) - lg.plane_disp(c["plant"], c["K"], xx, yy))
    worst = float(err[c["floor"]].max()) if c["floor"].any() else 0.0
    print(f"{IDS[i]}: valid {nv}, floor {int(c['floor'].sum())}, fit pixels {f['n']}, inliers {f['inliers']}, ok {m['ok']}, coef "
          f"{f['coef'].tolist()} (planted {c['plant'].tolist()}), worst |fitted - planted| on the floor {worst:.4f} px, Hc "
          f"{m['Hc']:.4f}, tilt {m['tilt']:.2f}; undecided {und}; dev e {ref['dev_e']:.3e}, h {ref['dev_h']:.3e}, u "
          f"{ref['dev_u']:.3e}, coef {ref['dev_coef']:.3e}, normal {ref['dev_normal']:.3e}, Hc {ref['dev_Hc']:.3e}")
    rec = lg.record(r64)
    assert np.isfinite(rec).all() and not rec[25:].any()
    assert r32["plane"]["ok"] == m["ok"] and r32["fit"]["steps"] == f["steps"] and r32["fit"]["n"] == f["n"]
    # one fp32 rounding of a disparity below 128 px is at most 7.6e-6 px and a residual takes five of them; the fit averages
    # them and the re-weighting feeds them back: an order of magnitude of margin on the coefficients (c2 is in pixels)
    assert ref["dev_coef"] <= 1e-4 and ref["dev_e"] <= 1e-4
    if c["name"] == "none":  # nothing valid: ok = 0, a finite zero record, labels all 255
        assert nv == 0 and not m["ok"] and not f["alive"] and not rec.any()
        assert (r64["pix"]["labels"] == lg.INVALID).all() and not r64["pix"]["grid_count"].any()
        return
    # the share of undecided pixels; the restatement takes the reference's decisions outside them
    assert und < 0.01 * nv
    same = r32["pix"]["labels"] == r64["pix"]["labels"]
    assert same[~ref["undecided"]].all()
    assert f["alive"] and f["steps"] == c["par"]["iters"]
    if c["fails"] == "inliers":  # the floor is found, but on too few pixels to be believed
        assert not m["ok"] and f["n"] >= c["par"]["min_valid"] > f["inliers"] and m["tilt"] <= c["par"]["max_tilt_deg"]
        assert worst <= RECOVERED_PX and (r64["pix"]["labels"] == lg.INVALID).all() and not r64["pix"]["grid_count"].any()
        return
    if c["fails"]:
        # the one scene whose floor an unseeded fit cannot find: it locks onto the boxes, whose plane faces the camera, and
        # is recognised through the tilt rule (the inliers alone would have passed)
        assert not m["ok"] and m["tilt"] > c["par"]["max_tilt_deg"] and f["inliers"] >= c["par"]["min_valid"]
        assert worst > 1.0 and abs(f["coef"][1]) < 0.25 * c["plant"][1]
        assert (r64["pix"]["labels"] == lg.INVALID).all() and np.isnan(r64["pix"]["height"]).all()
        assert not r64["pix"]["grid_count"].any() and not r64["pix"]["grid_height"].any()
        return
    assert m["ok"] and worst <= RECOVERED_PX
    cam_h = lg.CASES[i]["cam_h"]
    assert abs(m["Hc"] - cam_h) <= 0.01 * cam_h
    u = lg.up_vector(lg.CASES[i]["pitch"], lg.CASES[i]["roll"])
    assert np.degrees(np.arccos(np.clip(m["normal"] @ u, -1, 1))) <= 0.2
    assert abs(np.linalg.norm(m["forward"]) - 1) <= 1e-12 and abs(m["forward"] @ m["normal"]) <= 1e-12
    assert np.abs(np.cross(m["forward"], m["normal"]) - m["right"]).max() <= 1e-15 and m["right"][0] > 0.9
    # the labels say what the scene holds: the floor pixels are floor, the boxes' pixels are not
    lab = r64["pix"]["labels"]
    valid = ref["valid"]
    assert (lab[c["floor"] & valid] == lg.FLOOR).mean() >= 0.99
    assert not (~c["floor"] & valid).any() or (lab[~c["floor"] & valid] != lg.FLOOR).mean() >= 0.9
    if c["grid"] is not None:
        gc = r64["pix"]["grid_count"]
        assert gc.sum() <= int(((lab == lg.FLOOR) | (lab == lg.OBSTACLE)).sum()) and gc[0].sum() > 0
        assert ((r64["pix"]["grid_height"] > 0) == (gc[1] > 0)).all()


def test_scenes_cover_every_label():
    seen = set()
    for i in range(len(lg.CASES)):
        seen |= set(np.unique(_ref(i)[1]["r64"]["pix"]["labels"]).tolist())
    assert seen == {lg.FLOOR, lg.OBSTACLE, lg.OVERHEAD, lg.BELOW, lg.INVALID}


def test_ground_seed_closed_form():
    K, calib = (120.0, 100.0, 80.0, 40.0), 60.0
    c = live.ground_seed(1.2, K, calib)  # a level camera: the horizon at cy, rows below it grow by calib / (height fy)
    assert np.allclose(c, [0.0, 60.0 / 1.2 / 100.0, 0.0], atol=1e-15)
    for pitch, up in ((0.15, (0, -1, 0)), (-0.05, (0.1, -2.0, 0.05))):
        u = lg.up_vector(pitch, 0.0, np.array(up, float) / np.linalg.norm(up))
        want = -(calib / 0.9) * np.array([u[0] / K[0], u[1] / K[1], u[2]])
        got = live.ground_seed(0.9, K, calib, up=up, pitch_deg=np.degrees(pitch))
        assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
        assert np.abs(lg.plane_coef(0.9, K, calib, u) - got).max() <= 1e-14 * np.abs(want).max()
    assert live.ground_seed(1.0, K, calib, pitch_deg=10.0)[2] > 0  # looking down: the floor at the image centre is finite
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            live.ground_seed(bad, K, calib)
    with pytest.raises(ValueError):
        live.ground_seed(1.0, K, calib, up=(0, 0, 0))


BAD = [3, "yes", dict(speed=1), dict(step=0), dict(step=9), dict(step=2.0), dict(step=True), dict(iters=0), dict(iters=33),
       dict(iters=None), dict(min_valid=2.5), dict(delta_px=0.0), dict(delta_px=float("nan")), dict(delta0_px=-1.0),
       dict(delta0_px="x"), dict(asym=0.5), dict(asym=float("inf")), dict(max_tilt_deg=-1.0), dict(tol_px=-0.1),
       dict(ground_tol=-0.1), dict(ground_tol=0.5, clearance=0.4), dict(clearance=float("nan")), dict(height=0.0),
       dict(height=-1.0), dict(height="tall"), dict(pitch_deg=float("nan")), dict(pitch_deg=None), dict(up=(0, 0, 0)),
       dict(up=(0, -1)), dict(up=1), dict(map=1), dict(map="yes"), dict(grid=5), dict(grid=(0, 4)), dict(grid=(4, 4.0)),
       dict(grid=(4, 4, 4)), dict(grid=(65536, 65536)), dict(cell=0.0), dict(cell=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_check_ground_rejects(bad):
    with pytest.raises(ValueError, match="ground"):
        live._check_ground(bad)
    with pytest.raises(ValueError, match="ground"):  # before the estimator is looked at: no device call
        live.LiveSession(None, (8, 8), ground=bad)


def test_check_ground_accepts():
    assert live._check_ground(False) is None and live._check_ground(None) is None
    assert live._check_ground(True) == live.GROUND_DEFAULTS and live._check_ground(True) is not live.GROUND_DEFAULTS
    assert live.GROUND_DEFAULTS == dict(step=2, iters=8, delta_px=0.25, delta0_px=4.0, asym=4.0, min_valid=256,
                                        max_tilt_deg=45.0, tol_px=0.5, ground_tol=0.05, clearance=2.0, height=None,
                                        pitch_deg=0.0, up=(0, -1, 0), map=False, grid=None, cell=0.1)
    p = live._check_ground(dict(step=4, map=True, height=2, grid=[8, 6], asym=1))
    assert p == dict(live.GROUND_DEFAULTS, step=4, map=True, height=2.0, grid=(8, 6), asym=1.0)
    assert isinstance(p["height"], float) and isinstance(p["grid"], tuple)
    assert live.Ground._fields == ("coef", "ok", "normal", "camera_height", "tilt_deg", "forward", "valid", "inliers", "rms_px",
                                   "steps", "labels", "height", "grid_count", "grid_height")
    from codd_amd import ops
    assert set(ops.GROUND_PARAMS) < set(live.GROUND_DEFAULTS)
    assert all(ops.GROUND_PARAMS[k] == live.GROUND_DEFAULTS[k] for k in ops.GROUND_PARAMS)


def test_session_construction_touches_no_device():
    s = live.LiveSession(None, (48, 64), intrinsics=(100.0, 90.0, 32.0, 24.0), calib=50.0,
                         ground=dict(height=1.5, pitch_deg=10.0, grid=(8, 8)))
    assert not s._open_done
    assert np.array_equal(s._ground_seed, live.ground_seed(1.5, (100.0, 90.0, 32.0, 24.0), 50.0, pitch_deg=10.0))
    assert np.allclose(s._ground_up, (0.0, -np.cos(np.radians(10.0)), -np.sin(np.radians(10.0))))
    assert live.LiveSession(None, (48, 64), ground=True)._ground_seed is None
    assert live.LiveSession(None, (48, 64)).ground is None


def test_record_layout():
    rec = np.zeros(32)
    rec[:13] = [0.01, 0.4, 7.5, 1, 2800, 2500, 0.06, 8, 0.0, -0.98, -0.15, 1.2, 8.8]
    rec[13:22] = np.arange(1, 10)
    rec[22:25] = [0.0, -0.15, 0.98]
    lab = np.zeros((2, 2), np.uint8)
    g = live.ground_from_record(rec, lab)
    assert g.coef.tolist() == [0.01, 0.4, 7.5] and g.ok is True and (g.valid, g.inliers, g.steps) == (2800, 2500, 8)
    assert g.normal.tolist() == [0.0, -0.98, -0.15] and (g.camera_height, g.tilt_deg, g.rms_px) == (1.2, 8.8, 0.06)
    assert g.forward.tolist() == [0.0, -0.15, 0.98] and g.labels is lab
    assert g.height is None and g.grid_count is None and g.grid_height is None


class _Done:
    def synchronize(self):
        pass


def test_tuple_order():
    """result[, confidence][, epipolar][, ground]: the collection step on host buffers standing in for the downloads."""
    import torch
    s = live.LiveSession(None, (4, 6), confidence=True, epipolar=True, ground=dict(map=True, grid=(3, 2)))
    s._e_down = [_Done(), _Done()]
    s._h_out = [torch.zeros(4, 6)] * 2
    s._h_conf = [(torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(4, 6))] * 2
    s._h_epi = [(torch.zeros(32, dtype=torch.float64),)] * 2
    rec = torch.zeros(32, dtype=torch.float64)
    rec[3], rec[11] = 1.0, 1.25
    s._h_ground = [[rec, torch.full((4, 6), 255, dtype=torch.uint8), torch.ones(4, 6),
                    torch.ones(2, 3, 2, dtype=torch.int32), torch.zeros(3, 2)]] * 2
    s._inflight.append(0)
    got = s.pop()
    assert isinstance(got, tuple) and len(got) == 4
    assert isinstance(got[0], np.ndarray) and isinstance(got[1], live.Confidence) and isinstance(got[2], live.Epipolar)
    g = got[3]
    assert isinstance(g, live.Ground) and g.ok and g.camera_height == 1.25
    assert g.labels.shape == (4, 6) and g.labels.dtype == np.uint8 and g.height.shape == (4, 6)
    assert g.grid_count.shape == (2, 3, 2) and g.grid_count.dtype == np.int32 and g.grid_height.shape == (3, 2)
    # without map and grid the same buffers' list is shorter: labels only
    s = live.LiveSession(None, (4, 6), ground=True)
    s._e_down, s._h_out = [_Done(), _Done()], [torch.zeros(4, 6)] * 2
    s._h_ground = [[rec, torch.zeros(4, 6, dtype=torch.uint8)]] * 2
    s._inflight.append(1)
    res, g = s.pop()
    assert isinstance(g, live.Ground) and g.height is None and g.grid_count is None and g.grid_height is None


def test_entry_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    import ctypes as C
    from codd_amd import _abi
    lib = _abi.load()
    scr = lib.codd_ground_scratch
    assert not _abi.MISSING and scr(0, 4, 0, 0) == -1 and scr(4, -1, 0, 0) == -1 and scr(65536, 32768, 0, 0) == -1
    assert scr(4, 4, 0, 3) == -1 and scr(4, 4, 3, 0) == -1 and scr(4, 4, -1, -1) == -1 and scr(4, 4, 32768, 32768) == -1
    need = scr(24, 40, 7, 5)
    assert need > 0 and scr(24, 40, 0, 0) == need and scr(46340, 46340, 0, 0) == need  # the sums only: no plane per pixel
    for h, w in ((1, 1), (37, 53), (540, 960)):  # the layout is part of the contract: rows, states, ticket
        assert scr(h, w, 0, 0) == 41120 and scr(h, w, 128, 128) == 41120
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = buf.ctypes.data_as(C.c_void_p)
    up = (C.c_float * 3)(0.0, -1.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def call(disp=p, H=64, W=64, h=24, w=40, fx=40.0, fy=40.0, cx=20.0, cy=8.0, calib=20.0, seed=None, up=up, step=2, iters=8,
             delta_px=0.25, delta0_px=4.0, asym=4.0, min_valid=16, max_tilt_deg=45.0, tol_px=0.5, ground_tol=0.05,
             clearance=2.0, cell=1.0, gh=7, gw=5, scratch=p, nbytes=need, record=p, labels=p, height=None, grid_count=p,
             grid_height=p):
        return lib.codd_ground_plane(disp, H, W, h, w, fx, fy, cx, cy, calib, seed, up, step, iters, delta_px, delta0_px, asym,
                                     min_valid, max_tilt_deg, tol_px, ground_tol, clearance, cell, gh, gw, scratch, nbytes,
                                     record, labels, height, grid_count, grid_height, None)

    for name in ("disp", "up", "scratch", "record", "labels", "grid_count", "grid_height"):
        assert call(**{name: None}) == -1, name
    nogrid = dict(grid_count=None, grid_height=None)
    for bad in (dict(h=0), dict(w=0), dict(H=0), dict(W=-3), dict(h=65), dict(w=65), dict(step=0), dict(step=9), dict(iters=0),
                dict(iters=33), dict(fx=0.0), dict(fx=nan), dict(fy=-1.0), dict(fy=inf), dict(cx=nan), dict(cy=inf),
                dict(calib=0.0), dict(calib=nan), dict(delta_px=0.0), dict(delta_px=nan), dict(delta0_px=0.0),
                dict(delta0_px=nan), dict(asym=0.5), dict(asym=nan), dict(asym=inf), dict(delta_px=1e-30),
                dict(max_tilt_deg=-1.0), dict(max_tilt_deg=nan), dict(tol_px=-0.5), dict(tol_px=nan), dict(ground_tol=-0.1),
                dict(ground_tol=nan), dict(clearance=0.01), dict(clearance=nan), dict(cell=0.0), dict(cell=-1.0), dict(cell=nan),
                dict(cell=inf), dict(gh=0), dict(gw=0), dict(gh=-7), dict(gh=0, gw=0), dict(nogrid, gh=7, gw=5),
                dict(nogrid, gh=0, gw=5), dict(nogrid, gh=0, gw=0, cell=nan), dict(gh=32768, gw=32768),
                dict(up=(C.c_float * 3)(0.0, 0.0, 0.0)), dict(up=(C.c_float * 3)(0.0, nan, 0.0)),
                dict(seed=(C.c_double * 3)(0.0, nan, 1.0)), dict(seed=(C.c_double * 3)(inf, 0.0, 1.0)),
                dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**bad) == -1, bad


def test_cli_ground_arguments():
    from codd_amd import inference
    base = ["--img-dir", "x", "--r-img-dir", "y"]
    for argv in (["--ground"],  # needs --live
                 ["--live", "--ground-height", "1.2"], ["--live", "--ground-grid", "32x32"],  # need --ground
                 ["--live", "--ground", "--ground-cell", "0.2"],  # needs --ground-grid
                 ["--live", "--ground", "--ground-grid", "32"], ["--live", "--ground", "--ground-grid", "0x4"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + argv)
    a = inference.parse_args(base + ["--live", "--ground", "--ground-height", "1.2", "--ground-grid", "32x48", "--ground-cell", "0.2"])
    assert a.ground and a.ground_height == 1.2 and a.ground_grid == (32, 48) and a.ground_cell == 0.2
    assert not inference.parse_args(base + ["--live"]).ground
