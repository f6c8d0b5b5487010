"""Live stereo session, the parts that need no GPU: argument checks of the two C-ABI entries (every call is rejected
before any launch), LiveSession input validation, the numpy restatement of the rectifying remap, and the --live frame
iterator."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_ref  # noqa: E402

from codd_amd import _abi  # noqa: E402

EINVAL = -1  # CODD_EINVAL


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_ingest_pair_rejects_bad_arguments():
    """(no launch: every call below is rejected first)"""
    lib = _abi.load()
    assert "codd_ingest_pair" in _abi.SIGNATURES and lib.codd_ingest_pair is not None
    buf = np.zeros(64, np.uint8)  # host memory standing in for device pointers: never dereferenced
    p = _ptr(buf)
    m, s = (C.c_float * 3)(1, 2, 3), (C.c_float * 3)(1, 1, 1)

    def call(left=p, right=p, h=40, w=50, mean=m, std=s, lx=None, ly=None, rx=None, ry=None, H=64, W=64, ol=p, orr=p):
        return lib.codd_ingest_pair(left, right, h, w, 0, mean, std, lx, ly, rx, ry, H, W, ol, orr, None)

    assert call(left=None) == EINVAL
    assert call(right=None) == EINVAL
    assert call(mean=None) == EINVAL
    assert call(std=None) == EINVAL
    assert call(ol=None) == EINVAL
    assert call(orr=None) == EINVAL
    assert call(H=39) == EINVAL  # H < h
    assert call(W=49) == EINVAL  # W < w
    assert call(w=32, W=64) == EINVAL  # W - w >= w: the reflection would leave the image
    assert call(h=32, H=64) == EINVAL
    assert call(lx=p) == EINVAL  # a map for one axis only
    assert call(ly=p) == EINVAL
    assert call(rx=p) == EINVAL
    assert call(lx=p, ly=p, ry=p) == EINVAL


def test_export_depth_rejects_bad_arguments():
    lib = _abi.load()
    assert "codd_export_depth" in _abi.SIGNATURES and lib.codd_export_depth is not None
    p = _ptr(np.zeros(64, np.uint8))

    def call(disp=p, H=64, W=64, h=40, w=50, mode=0, out=p):
        return lib.codd_export_depth(disp, H, W, h, w, mode, 1.0, out, None)

    assert call(disp=None) == EINVAL
    assert call(out=None) == EINVAL
    assert call(H=39) == EINVAL
    assert call(W=49) == EINVAL
    assert call(mode=3) == EINVAL
    assert call(mode=-1) == EINVAL


def _cpu_session(**kw):
    from codd_amd import configs
    from codd_amd.live import LiveSession
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.stereo_only()).eval()  # on the CPU: any device call would raise CoddHipError
    return LiveSession(est, (40, 50), **kw)


def test_session_validates_frames_before_touching_the_device():
    s = _cpu_session()
    good = np.zeros((40, 50, 3), np.uint8)
    with pytest.raises(ValueError):
        s.push(good.astype(np.float32), good)  # dtype
    with pytest.raises(ValueError):
        s.push(good, np.zeros((40, 51, 3), np.uint8))  # shape
    with pytest.raises(ValueError):
        s.push(good, np.zeros((40, 50), np.uint8))
    with pytest.raises(ValueError):
        s.push(np.zeros((40, 100, 3), np.uint8)[:, ::2], good)  # not contiguous
    with pytest.raises(ValueError):
        s.step(torch.zeros(40, 50, 3, dtype=torch.float32), torch.from_numpy(good))
    with pytest.raises(TypeError):
        s.push(good.tolist(), good)
    with pytest.raises(TypeError):
        s.step(None, good)
    assert s.pending() == 0 and not s._open_done  # nothing was allocated, nothing is in flight
    with pytest.raises(IndexError):
        s.pop()
    # a valid pair gets past validation and is then refused by the device check: there is no CPU fallback
    with pytest.raises(_abi.CoddHipError):
        s.push(good, good)


def test_session_validates_its_configuration():
    with pytest.raises(ValueError):
        _cpu_session(output="metres")
    ident = np.zeros((40, 50), np.float32)
    with pytest.raises(ValueError):
        _cpu_session(rectify=((ident, None), (ident, ident)))  # one axis only
    with pytest.raises(ValueError):
        _cpu_session(rectify=((ident, ident), (ident, np.zeros((40, 51), np.float32))))
    s = _cpu_session(rectify=((ident, ident), None), calib=100.0, intrinsics=(500.0, 500.0, 25.0, 20.0))
    meta = s.metas[0]
    assert meta["img_shape"] == (40, 50, 3) and meta["pad_shape"] == (64, 64, 3)
    assert meta["calib"] == 100.0 and meta["intrinsics"] == [500.0, 500.0, 25.0, 20.0]


def test_remap_restatement():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(9, dtype=np.float32), np.arange(11, dtype=np.float32), indexing="ij")
    assert np.array_equal(live_ref.remap(img, xx, yy), img.astype(np.float64))  # identity
    half = live_ref.remap(img, xx + 0.5, yy)  # two-tap average along x; the last column's right tap is outside
    f = img.astype(np.float64)
    assert np.array_equal(half[:, :-1], 0.5 * (f[:, :-1] + f[:, 1:]))
    assert np.array_equal(half[:, -1], 0.5 * f[:, -1])
    assert np.array_equal(live_ref.remap(img, xx - 1.0, yy)[:, 0], np.zeros((9, 3)))  # outside taps give 0
    assert np.array_equal(live_ref.remap(img, xx, yy + 9.0), np.zeros((9, 11, 3)))
    bad = xx.copy()
    bad[2, 3], bad[4, 5] = np.nan, np.inf
    out = live_ref.remap(img, bad, yy)
    assert np.array_equal(out[2, 3], np.zeros(3)) and np.array_equal(out[4, 5], np.zeros(3))
    # identity ingest = plain normalisation with the reflected border
    a = live_ref.ingest(img, 16, 16, False)
    assert np.array_equal(a, live_ref.ingest(img, 16, 16, False, maps=(xx, yy)))
    assert np.array_equal(a[:, 9, :11], a[:, 7, :11]) and np.array_equal(a[:, :, 12], a[:, :, 8])  # REFLECT_101


def test_export_restatement():
    d = np.array([[0.0, 255.998, 300.0, np.inf, np.nan, -3.0, 0.5 / 256, 1.5 / 256, 2.5 / 256]], np.float32)
    q = live_ref.export(d, 1, 9, "disp_u16")
    assert q.dtype == np.uint16 and q.tolist() == [[0, 65535, 65535, 0, 0, 0, 0, 2, 2]]
    assert np.array_equal(live_ref.export(d, 1, 3, "disp"), d[:, :3])


def test_live_frame_iterator_is_lazy_and_ordered(tmp_path):
    from PIL import Image
    from codd_amd import inference
    for side in ("l", "r"):
        os.makedirs(tmp_path / side)
        for i in (10, 9, 1, 2, 11, 3):  # natural order is not lexicographic order
            Image.fromarray(np.full((8, 12, 3), i + (100 if side == "r" else 0), np.uint8)).save(tmp_path / side / f"f{i}.png")
    (name, lefts, rights), = inference.list_videos(str(tmp_path / "l"), str(tmp_path / "r"), ".png")
    decoded = []

    def counting(frames):
        for f in frames:
            decoded.append(int(f[0][0, 0, 0]))
            yield f

    class Session:  # stands in for LiveSession: same push / pop / pending contract, identity "network"
        def __init__(self):
            self.q, self.most = [], 0

        def pending(self):
            return len(self.q)

        def push(self, left, right):
            assert left.dtype == np.uint8 and left.shape == (8, 12, 3) and left.flags["C_CONTIGUOUS"]
            assert int(right[0, 0, 0]) == int(left[0, 0, 0]) + 100
            self.q.append(int(left[0, 0, 0]))
            self.most = max(self.most, len(self.q))

        def pop(self):
            return self.q.pop(0)

    s = Session()
    got = []
    for res in inference.live_results(s, counting(inference.iter_frames(lefts, rights))):
        assert len(decoded) - len(got) <= 2  # never more frames decoded and unreturned than the pipeline holds
        got.append(res)
    assert got == decoded == [1, 2, 3, 9, 10, 11]
    assert s.most == 2


def test_step_fill_goes_through_step_until_the_graph_is_live():
    """Without a live graph FrameRunner.step_fill fills the caller's scratch pair and is ``step`` on it."""
    from codd_amd.runtime import FrameRunner

    class Est:  # records what the frame was run on
        motion = fusion = None

        def consistent_online_depth_estimation(self, left, right, metas, state):
            return dict(pred_disp=left + right)

    runner = FrameRunner(Est(), [dict()], use_graph=False)
    scratch = (torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))
    seen = []

    def fill(left, right):
        seen.append((left, right))
        left.fill_(1.0)
        right.fill_(2.0)

    out = runner.step_fill(fill, scratch)
    assert seen[0][0] is scratch[0] and seen[0][1] is scratch[1]
    assert runner.frames == 1 and torch.equal(out, torch.full((1, 3, 4, 4), 3.0))


def test_npz_stream_writes_what_savez_compressed_writes(tmp_path):
    from codd_amd.inference import _NpzStream
    a = np.random.default_rng(1).random((5, 7, 9)).astype(np.float32)
    w = _NpzStream(str(tmp_path / "x.npz"), "disp", (1, 5, 7, 9), np.float32)
    for frame in a:
        w.write(frame)
    w.close()
    np.savez_compressed(tmp_path / "y.npz", disp=a[None])
    x, y = np.load(tmp_path / "x.npz"), np.load(tmp_path / "y.npz")
    assert x.files == y.files == ["disp"] and x["disp"].dtype == np.float32 and np.array_equal(x["disp"], y["disp"])
