"""Restatement of codd_track_objects (include/codd_hip.h) shared by the CPU and the GPU tests, in numpy only.

The geometry is fp32 operation by operation: one numpy operation on np.float32 arrays per operation of the header, in the
order of codd_amd/csrc/se3.h (numpy has no fused multiply-add and its division is correctly rounded).  The displacements
are quantised to integers exactly as the header says, summed in int64 (any order gives the same sum) and divided in
fp64, so this restatement equals the kernel bit for bit, with no excluded pixel and no tolerance.

The state is a dict(hdr int32 [8], table int32 [max_objects,2], ids uint16 [h,w]); ``state_bytes`` lays it out as the
header documents it.  ``field`` builds a synthetic SE3 field and depth map whose padding is poisoned (NaN), which a
kernel that reads outside the crop would pick up.
"""
import numpy as np

f32 = np.float32
NONE = 0xFFFF
MIN_DEPTH, PEPS = f32(0.05), f32(1e-5)
QSCALE, QMAX = 262144.0, f32(4096.0)
CROP, PADDED = (70, 150), (128, 192)  # the shape of tests/test_gpu_live_objects.py
K = (100.0, 100.0, 74.5, 20.25)
TRACK_MAX = 1024


# ---- inputs -------------------------------------------------------------------------------------------------------------
def new_state(h, w, m):
    return dict(hdr=np.zeros(8, np.int32), table=np.zeros((m, 2), np.int32), ids=np.full((h, w), NONE, np.uint16))


def state_bytes(st):
    return st["hdr"].astype(np.int32).tobytes() + st["table"].astype(np.int32).tobytes() + st["ids"].astype(np.uint16).tobytes()


def field(crop, padded, shift=(0.0, 0.0), Z=10.0, dz=0.0, K=K, q=(0.0, 0.0, 0.0, 1.0)):
    """T [H,W,7] and depth [H,W]: a fronto-parallel wall at depth Z moved by the translation that shifts its image by
    ``shift`` = (dx, dy) pixels (arrays [h,w] or numbers) and its depth by dz, after the rotation q.  Padding: NaN."""
    h, w = crop
    H, W = padded
    T = np.full((H, W, 7), np.nan, f32)
    depth = np.full((H, W), np.nan, f32)
    dx, dy = (np.broadcast_to(np.asarray(v, np.float64), (h, w)) for v in shift)
    Zc = np.broadcast_to(np.asarray(Z, np.float64), (h, w))
    T[:h, :w, 0] = dx * Zc / K[0]
    T[:h, :w, 1] = dy * Zc / K[1]
    T[:h, :w, 2] = dz
    T[:h, :w, 3:7] = np.asarray(q, f32)
    depth[:h, :w] = Zc
    return T, depth


# ---- the geometry, generic in the dtype (fp32: the contract; fp64: the plain reference of the CPU test) ----------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def qrot(q, v, dt=f32):
    """se3.h qrot: v + w * uv + u x uv with uv = 2 (u x v); q = (x, y, z, w)."""
    u = (q[0], q[1], q[2])
    uv = tuple(dt(2.0) * c for c in _cross(u, v))
    uuv = _cross(u, uv)
    return tuple((v[k] + q[3] * uv[k]) + uuv[k] for k in range(3))


def geometry(T, depth, K, crop, dt=f32):
    """X0, X1 (tuples of [h,w] arrays) and the projection (cx, cy) of X1, in dtype dt from the fp32 inputs."""
    h, w = crop
    fx, fy, cx, cy = (dt(f32(v)) for v in K)
    d = depth[:h, :w].astype(dt)
    Tc = T[:h, :w].astype(dt)
    x = np.arange(w, dtype=dt)[None, :]
    y = np.arange(h, dtype=dt)[:, None]
    with np.errstate(all="ignore"):
        X0 = (d * ((x - cx) / fx), d * ((y - cy) / fy), d * np.ones((h, w), dt))
        r = qrot((Tc[..., 3], Tc[..., 4], Tc[..., 5], Tc[..., 6]), X0, dt)
        X1 = tuple(r[k] + Tc[..., k] for k in range(3))
        Zp = X1[2] + dt(PEPS)
        c = (fx * (X1[0] / Zp) + cx, fy * (X1[1] / Zp) + cy)
    return X0, X1, c


def quantise(v):
    """Q(v) of the header: int64."""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(np.asarray(v, f32), -QMAX), QMAX)
    return np.rint(c.astype(np.float64) * QSCALE).astype(np.int64)


def pixels(state, T, depth, K, crop, ids_cur, n_prev, n_cur, ego=None, scale=1.0):
    """Per pixel of the crop: a, valid, votes, b, D (fp32 [3,h,w]), O (or None)."""
    h, w = crop
    a = state["ids"].astype(np.int64)
    cand = a < n_prev  # (0xFFFF >= n_prev: max_objects <= 1024)
    X0, X1, c = geometry(T, depth, K, crop)
    fin = np.ones((h, w), bool)
    for v in X0 + X1:
        fin &= np.isfinite(v)
    with np.errstate(all="ignore"):
        valid = cand & (X0[2] >= MIN_DEPTH) & (X1[2] >= MIN_DEPTH) & fin
        u, v = np.floor(c[0] + f32(0.5)), np.floor(c[1] + f32(0.5))
        lands = valid & (u >= f32(0)) & (u < f32(w)) & (v >= f32(0)) & (v < f32(h))
    ui, vi = np.where(lands, u, 0).astype(np.int64), np.where(lands, v, 0).astype(np.int64)
    b = np.where(lands, ids_cur[vi, ui].astype(np.int64), NONE)
    votes = lands & (b < n_cur)
    s = f32(scale)
    with np.errstate(all="ignore"):
        D = np.stack([s * (X1[k] - X0[k]) for k in range(3)])
        O = None
        if ego is not None and ego[7] != 0:
            e = np.asarray(ego, f32)
            Y = qrot((e[3], e[4], e[5], e[6]), X0)
            O = np.stack([s * (X1[k] - Y[k]) - e[k] for k in range(3)])
    return a, valid, votes, b, D, O


def track(state, T, depth, K, crop, ids_cur, count, ego=None, moving=None, scale=1.0, min_votes=16, max_objects=256,
          fresh=False):
    """One call of the entry.  Returns dict(count int32 [4], trk_i int32 [m,8], trk_f fp32 [m,8], state: the rolled state,
    and the sums V, n, mv, no, S, So for the tests that look inside).  ``state`` is not modified."""
    h, w = crop
    m = int(max_objects)
    ids_cur = np.asarray(ids_cur, np.uint16).reshape(h, w)
    n_cur = min(max(int(count[0]), 0), m)
    n_prev = 0 if fresh else min(max(int(state["hdr"][0]), 0), m)
    nid = 1 if fresh else int(state["hdr"][1])
    if nid < 1 or nid > 2 ** 31 - 1 - m:
        nid = 1
    frames = 0 if fresh else int(state["hdr"][2])
    V = np.zeros((m, m), np.int64)
    n, mv, no = (np.zeros(m, np.int64) for _ in range(3))
    S, So = np.zeros((m, 3), np.int64), np.zeros((m, 3), np.int64)
    if T is not None and n_prev > 0:
        a, valid, votes, b, D, O = pixels(state, T, depth, K, crop, ids_cur, n_prev, n_cur, ego, scale)
        np.add.at(V, (a[votes], b[votes]), 1)
        np.add.at(n, a[valid], 1)
        for k in range(3):
            np.add.at(S[:, k], a[valid], quantise(D[k])[valid])
        if O is not None:
            np.add.at(no, a[valid], 1)
            for k in range(3):
                np.add.at(So[:, k], a[valid], quantise(O[k])[valid])
        if moving is not None:
            sel = valid & (np.asarray(moving).reshape(h, w) == 1)
            np.add.at(mv, a[sel], 1)
    best_cur = np.full(m, -1, np.int64)
    best_prev = np.full(m, -1, np.int64)
    if T is not None:
        for i in range(n_prev):
            row = V[i, :n_cur]
            if row.size and row.max() > 0:
                best_cur[i] = int(np.argmax(row))  # (the first maximum: ties to the smallest index)
        for j in range(n_cur):
            col = V[:n_prev, j]
            if col.size and col.max() > 0:
                best_prev[j] = int(np.argmax(col))
    trk_i, trk_f = np.zeros((m, 8), np.int32), np.zeros((m, 8), f32)
    table = np.zeros((m, 2), np.int32)
    continued = started = 0
    for j in range(n_cur):
        i = int(best_prev[j])
        if i >= 0 and best_cur[i] == j and V[i, j] >= min_votes:
            continued += 1
            table[j] = (state["table"][i, 0], int(state["table"][i, 1]) + 1)
            trk_i[j] = (table[j, 0], table[j, 1], i, V[i, j], n[i], mv[i], no[i], 0)
            with np.errstate(all="ignore"):
                for k in range(3):
                    trk_f[j, k] = f32(float(S[i, k]) / float(n[i]) / QSCALE) if n[i] else np.nan
                    trk_f[j, 3 + k] = f32(float(So[i, k]) / float(no[i]) / QSCALE) if no[i] else np.nan
        else:
            table[j] = (nid + started, 1)
            started += 1
            trk_i[j] = (table[j, 0], 1, -1, 0, 0, 0, 0, 0)
            trk_f[j, :6] = np.nan
    hdr = np.zeros(8, np.int32)
    hdr[:3] = (n_cur, nid + started, frames + 1)
    return dict(count=np.array([n_cur, continued, started, n_prev - continued], np.int32), trk_i=trk_i, trk_f=trk_f,
                state=dict(hdr=hdr, table=table, ids=ids_cur.copy()), V=V, n=n, mv=mv, no=no, S=S, So=So)


# ---- the cases of tests/test_gpu_live_tracks.py: sequences of frames on synthetic id maps and fields -------------------
def boxes(crop, *bs):
    """uint16 [h,w]: box k = (y0, y1, x0, x1), half-open and clipped to the crop, carries the id k; 0xFFFF elsewhere."""
    m = np.full(crop, NONE, np.uint16)
    for k, (y0, y1, x0, x1) in enumerate(bs):
        m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = k
    return m


def frame(ids, n, T=None, depth=None, ego=None, moving=None, fresh=False):
    return dict(ids=np.ascontiguousarray(ids, np.uint16), count=np.array([n, n, n, int((ids != NONE).sum())], np.int32), T=T,
                depth=depth, ego=None if ego is None else np.asarray(ego, f32),
                moving=None if moving is None else np.ascontiguousarray(moving, np.uint8), fresh=fresh)


def make(name, frames, crop=CROP, padded=PADDED, K=K, scale=1.0, min_votes=16, max_objects=256, seed=None):
    """A case: the frames in order (the first one fresh unless ``seed``, a state to start from, is given)."""
    return dict(name=name, frames=frames, crop=tuple(crop), padded=tuple(padded), K=tuple(K), scale=scale,
                par=dict(min_votes=min_votes, max_objects=max_objects), seed=seed)


def reference(c):
    """The restatement's result of every frame of the case, in order."""
    st = c["seed"] if c["seed"] is not None else new_state(*c["crop"], c["par"]["max_objects"])
    out = []
    for f in c["frames"]:
        r = track(st, f["T"], f["depth"], c["K"], c["crop"], f["ids"], f["count"], ego=f["ego"], moving=f["moving"],
                  scale=c["scale"], fresh=f["fresh"], **c["par"])
        out.append(r)
        st = r["state"]
    return out


EGO = np.array([0.01, -0.004, 0.03, 0.002, 0.001, -0.003, 0.99999297, 1.0, 0, 0, 0, 0, 0, 0, 0, 0], f32)
Q_SMALL = (0.004, -0.003, 0.002, 0.99998546)


BOXES = ((4, 30, 10, 50), (20, 60, 70, 120), (40, 66, 5, 40))


def _shift_case(name, dx, crop=CROP, ego=None, with_moving=False, q=(0.0, 0.0, 0.0, 1.0), third=True, bs=BOXES, **kw):
    """Three boxes (clipped to the crop) that move by dx pixels between frames, and by (1, -2) in a third frame."""
    r = int(np.floor(dx + 0.5))
    rng = np.random.default_rng(11)
    mv = rng.choice(np.array([0, 1, 255], np.uint8), size=crop) if with_moving else None
    f0 = frame(boxes(crop, *bs), 3, fresh=True)
    T, depth = field(crop, PADDED, (dx, 0.0), Z=10.0, q=q)
    fr = [f0, frame(boxes(crop, *((y0, y1, x0 + r, x1 + r) for y0, y1, x0, x1 in bs)), 3, T, depth, ego, mv)]
    if third:
        T2, depth2 = field(crop, PADDED, (1.0, -2.0), Z=8.0, dz=0.25)
        fr.append(frame(boxes(crop, *((y0 - 2, y1 - 2, x0 + r + 1, x1 + r + 1) for y0, y1, x0, x1 in bs)), 3, T2, depth2, ego, mv))
    return make(name, fr, crop=crop, **kw)


def _leaving():
    bs = ((10, 40, 120, 145), (45, 65, 20, 60), (5, 25, 30, 70))
    ids0 = boxes(CROP, *bs)
    dx = np.zeros(CROP)
    dx[ids0 == 0], dx[ids0 == 1], dx[ids0 == 2] = 20.0, 200.0, -35.0  # partly out on the right, wholly out, partly out on the left
    T, depth = field(CROP, PADDED, (dx, 0.0))
    ids1 = boxes(CROP, (5, 25, 0, 35), (10, 40, 140, 150))  # raster order: the left object first
    return make("leaving", [frame(ids0, 3, fresh=True), frame(ids1, 2, T, depth)])


def _invalid():
    bs = ((4, 34, 10, 60), (36, 66, 70, 140))
    ids0 = boxes(CROP, *bs)
    T, depth = field(CROP, PADDED, (2.0, 1.0))
    bad_d = (0.0, -3.0, np.nan, np.inf, 0.04, 0.05, -np.inf, 1e-30)
    for k, v in enumerate(bad_d):
        depth[6 + k, 12:40] = v
    for k, (ch, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (6, np.inf), (2, -9.96), (2, -9.94), (0, 3e38))):
        T[40 + k, 75:130, ch] = v  # (t_z = -9.96: X1.z below MIN_DEPTH; -9.94: just above)
    ids1 = boxes(CROP, *((y0 + 1, y1 + 1, x0 + 2, x1 + 2) for y0, y1, x0, x1 in bs))
    return make("invalid", [frame(ids0, 2, fresh=True), frame(ids1, 2, T, depth, EGO)])


def _whole_crop():
    ids = np.zeros(CROP, np.uint16)
    T, depth = field(CROP, PADDED, (1.0, 0.0), q=Q_SMALL)
    mv = np.ones(CROP, np.uint8)
    return make("whole-crop", [frame(ids, 1, fresh=True), frame(ids, 1, T, depth, EGO, mv), frame(ids, 1, T, depth, EGO, mv)], scale=0.37)


def _checkerboard():
    h, w = CROP
    yy, xx = np.mgrid[:h, :w]
    on = ((yy + xx) % 2 == 0).ravel()
    ids = np.full(h * w, NONE, np.uint16)
    where = np.flatnonzero(on)[:TRACK_MAX]
    ids[where] = np.arange(where.size)
    ids = ids.reshape(CROP)
    T, depth = field(CROP, PADDED, (2.0, 0.0))
    return make("checkerboard", [frame(ids, TRACK_MAX, fresh=True), frame(ids, TRACK_MAX, T, depth, EGO)], min_votes=1,
                max_objects=TRACK_MAX)


def _empty(which):
    ids = boxes(CROP, (4, 30, 10, 50), (20, 60, 70, 120))
    none = np.full(CROP, NONE, np.uint16)
    T, depth = field(CROP, PADDED)
    if which == "n-cur-0":
        return make(which, [frame(ids, 2, fresh=True), frame(none, 0, T, depth), frame(ids, 2, T, depth)])
    return make(which, [frame(none, 0, fresh=True), frame(ids, 2, T, depth), frame(ids, 2, T, depth)])


def _truncated():
    bs = tuple((4 + 10 * k, 12 + 10 * k, 10, 60) for k in range(6))
    ids = boxes(CROP, *bs)  # the ids 4 and 5 are in the map but not among the max_objects = 4 objects
    T, depth = field(CROP, PADDED)
    return make("truncated", [frame(ids, 6, fresh=True), frame(ids, 6, T, depth), frame(ids, 6, T, depth)], max_objects=4)


def _split_merge_tie():
    whole = boxes(CROP, (10, 30, 10, 90), (40, 60, 10, 50), (40, 60, 60, 100), (2, 8, 100, 140))
    # object 0 splits 50 : 29 columns; objects 1 and 2 (40 columns each) merge: an exact tie; object 3 splits into equal halves
    parts = boxes(CROP, (2, 8, 100, 120), (2, 8, 120, 140), (10, 30, 10, 60), (10, 30, 61, 90), (40, 60, 10, 100))
    T, depth = field(CROP, PADDED)
    return make("split-merge-tie", [frame(whole, 4, fresh=True), frame(parts, 5, T, depth), frame(whole, 4, T, depth)])


def _min_votes():
    a = boxes(CROP, (10, 11, 10, 25), (20, 21, 10, 26))  # 15 and 16 pixels
    T, depth = field(CROP, PADDED)
    return make("min-votes", [frame(a, 2, fresh=True), frame(a, 2, T, depth)])


def _wrap():
    m = 256
    st = new_state(*CROP, m)
    st["hdr"][:3] = (2, 2 ** 31 - m, 41)  # next_id one past the last admissible start
    st["table"][:2] = ((2 ** 31 - 1 - m, 7), (5, 3))
    ids = boxes(CROP, (4, 30, 10, 50), (20, 60, 70, 120))
    st["ids"] = ids.copy()
    T, depth = field(CROP, PADDED)
    ids1 = boxes(CROP, (4, 30, 10, 50), (20, 60, 70, 120), (62, 68, 3, 30))
    return make("wrap", [frame(ids1, 3, T, depth)], seed=st)


def cases():
    out = [_shift_case("shift-3.5", -3.5), _shift_case("shift0", 0.0, q=Q_SMALL), _shift_case("shift+7.25", 7.25, scale=0.37),
           _shift_case("ego-moving", 2.0, ego=EGO, with_moving=True, q=Q_SMALL, scale=0.37),
           _shift_case("ego-not-ok", 2.0, ego=np.where(np.arange(16) == 7, 0, EGO), with_moving=True),
           _shift_case("moving-only", 2.0, with_moving=True, third=False),
           _leaving(), _invalid(), _whole_crop(), _checkerboard(), _empty("n-cur-0"), _empty("n-prev-0"), _truncated(),
           _split_merge_tie(), _min_votes(), _wrap()]
    for crop, dx, bs in (((1, 150), 1.0, ((0, 1, 10, 50), (0, 1, 70, 120), (0, 1, 125, 140))),
                         ((70, 1), 0.0, ((4, 30, 0, 1), (35, 60, 0, 1), (62, 68, 0, 1))),  # (the third frame's field leaves the image)
                         ((5, 7), 1.0, ((0, 2, 0, 3), (3, 5, 1, 5), (0, 3, 4, 6)))):
        out.append(_shift_case("crop-%dx%d" % crop, dx, crop=crop, ego=EGO, with_moving=True, bs=bs, min_votes=1, max_objects=8))
    return out


CASES = cases()
NAMES = {c["name"]: i for i, c in enumerate(CASES)}
