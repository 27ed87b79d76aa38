"""The instances of one sample matched to those of the sample before it (pca_voxel_instance_match): a brute-force numpy model
of the contract of include/pca.h and the scene builders the tests of tests/test_voxel_tracks_model.py and
tests/test_gpu_voxel_tracks.py share.  A plain module: no test, no fixture.

The model restates the header.  For a voxel (k, row, col) of `cur` with id b in [0, n_cur): u = col + 0.5, v = row + 0.5,
w = k + 0.5 and q_i = ((M[i][0] u + M[i][1] v) + M[i][2] w) + M[i][3] in f64 -- numpy rounds every ufunc on its own and fuses
nothing, which is what the library (built with -ffp-contract=off) computes.  In view iff 0 <= q_0 < px, 0 <= q_1 < px,
0 <= q_2 < nz on the f64 values; then a = prev[floor q_2, floor q_1, floor q_0] and, if 0 <= a < n_prev, C(a, b) gains one."""
import numpy as np

NONE32 = 0xffffffff
STATS = ('cur_voxels', 'in_view', 'sum_c', 'pairs', 'dropped', 'matched', 'new', 'lost', 'cur_skipped', 'prev_skipped')


def images(shape, M):
    """(q_0, q_1, q_2, in view) of every voxel centre of a volume of `shape` = (nz, px, px) under M (3 x 4)."""
    nz, px, _ = shape
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    k, row, col = np.meshgrid(np.arange(nz), np.arange(px), np.arange(px), indexing='ij')
    u, v, w = col + 0.5, row + 0.5, k + 0.5
    with np.errstate(all='ignore'):
        q = [((M[i, 0] * u + M[i, 1] * v) + M[i, 2] * w) + M[i, 3] for i in range(3)]
        view = (q[0] >= 0) & (q[0] < px) & (q[1] >= 0) & (q[1] < px) & (q[2] >= 0) & (q[2] < nz)
    return q[0], q[1], q[2], view


def model(prev, n_prev, cur, n_cur, M, min_overlap=1, min_iou=0.0, prev_track=None, t0=0, ids=None, cap_pairs=None):
    """Every output of pca_voxel_instance_match as numpy arrays under the header's names ('pairs': the used rows only, sorted by
    (b, a); with cap_pairs, padded to [cap_pairs, 3] with 0xffffffff rows behind them), plus 'counter': track_counter after
    the call.  stats[4] is 0: the model drops nothing."""
    prev, cur = np.asarray(prev, dtype=np.int32), np.asarray(cur, dtype=np.int32)
    assert prev.shape == cur.shape and prev.ndim == 3 and prev.shape[1] == prev.shape[2]
    nz, px, _ = cur.shape
    ok_cur = (cur >= 0) & (cur < n_cur)
    ok_prev = (prev >= 0) & (prev < n_prev)
    q0, q1, q2, view = images(cur.shape, M)
    view &= ok_cur
    vox_cur = np.bincount(cur[ok_cur], minlength=n_cur).astype(np.int64)
    in_view = np.bincount(cur[view], minlength=n_cur).astype(np.int64)
    vox_prev = np.bincount(prev[ok_prev], minlength=n_prev).astype(np.int64)
    a = prev[np.floor(q2[view]).astype(np.int64), np.floor(q1[view]).astype(np.int64), np.floor(q0[view]).astype(np.int64)].astype(np.int64)
    b = cur[view].astype(np.int64)
    hit = (a >= 0) & (a < n_prev)
    key, C = np.unique(b[hit] * 65536 + a[hit], return_counts=True)          # sorted by (b, a)
    pa, pb, C = key % 65536, key // 65536, C.astype(np.int64)

    def best(of, other, n):
        """per row of `of`: (C at its best partner, the partner + 1): the largest C, the smallest partner among equal ones"""
        out_c, out_p = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for j in np.lexsort((other, -C, of))[::-1]:          # the last write per row is its first in (of, -C, other) order
            out_c[of[j]], out_p[of[j]] = C[j], other[j] + 1
        return out_c, out_p
    c_prev, best_prev = best(pb, pa, n_cur)
    c_cur, best_cur = best(pa, pb, n_prev)
    match = np.full(n_cur, -1, dtype=np.int64)
    for bb in range(n_cur):
        aa = best_prev[bb] - 1
        if aa < 0 or best_cur[aa] - 1 != bb:
            continue
        c = c_prev[bb]
        if c >= min_overlap and np.float64(c) >= np.float64(min_iou) * np.float64(vox_prev[aa] + vox_cur[bb] - c):
            match[bb] = aa
    matched_b = np.zeros(n_prev, dtype=np.int64)
    matched_b[match[match >= 0]] = np.flatnonzero(match >= 0) + 1
    new = (match < 0) & (vox_cur > 0)
    track = np.full(n_cur, -1, dtype=np.int64)
    tr_prev = np.arange(n_prev) if prev_track is None else np.asarray(prev_track, dtype=np.int64)
    track[match >= 0] = tr_prev[match[match >= 0]]
    track[new] = t0 + np.arange(int(new.sum()))
    track = track.astype(np.int32)
    pairs = np.stack([pa, pb, C], axis=1).astype(np.uint32).reshape(-1, 3)
    if cap_pairs is not None:
        assert pairs.shape[0] <= cap_pairs
        pairs = np.concatenate([pairs, np.full((cap_pairs - pairs.shape[0], 3), NONE32, dtype=np.uint32)])
    stats = np.array([ok_cur.sum(), view.sum(), C.sum(), C.size, 0, (match >= 0).sum(), new.sum(),
                      ((vox_prev > 0) & (matched_b == 0)).sum(), ((~ok_cur) & (cur != -1)).sum(), ((~ok_prev) & (prev != -1)).sum()],
                     dtype=np.int64)
    out = {'cur_track': track, 'match': match.astype(np.int32),
           'cur_info': np.stack([vox_cur, in_view, c_prev, best_prev], axis=1).astype(np.uint32),
           'prev_info': np.stack([vox_prev, c_cur, best_cur, matched_b], axis=1).astype(np.uint32),
           'track_vol': np.where(ok_cur, track[np.where(ok_cur, cur, 0)], -1).astype(np.int32),
           'pairs': pairs, 'stats': stats, 'counter': np.int32(t0 + int(new.sum()))}
    if ids is not None:
        ids = np.asarray(ids, dtype=np.int32)
        ok = (ids >= 0) & (ids < n_cur)
        out['track_ids'] = np.where(ok, track[np.where(ok, ids, 0)], -1).astype(np.int32)
    return out


def loop_counts(prev, n_prev, cur, n_cur, M):
    """{(a, b): C} by a direct Python loop over the voxels of cur, scalar f64 arithmetic: what the vectorised model must equal."""
    nz, px, _ = cur.shape
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    out = {}
    for k in range(nz):
        for row in range(px):
            for col in range(px):
                b = int(cur[k, row, col])
                if not 0 <= b < n_cur:
                    continue
                u, v, w = np.float64(col + 0.5), np.float64(row + 0.5), np.float64(k + 0.5)
                q = [((M[i, 0] * u + M[i, 1] * v) + M[i, 2] * w) + M[i, 3] for i in range(3)]
                if not (0 <= q[0] < px and 0 <= q[1] < px and 0 <= q[2] < nz):
                    continue
                a = int(prev[int(np.floor(q[2])), int(np.floor(q[1])), int(np.floor(q[0]))])
                if 0 <= a < n_prev:
                    out[a, b] = out.get((a, b), 0) + 1
    return out


def sorted_pairs(pairs):
    """The used rows of a `pairs` output (any order, 0xffffffff rows unused) sorted by (b, a); the unused rows are checked."""
    p = np.asarray(pairs).reshape(-1, 3).astype(np.int64) & NONE32
    unused = p[:, 0] == NONE32
    assert (p[unused] == NONE32).all()
    p = p[~unused]
    return p[np.lexsort((p[:, 0], p[:, 1]))].astype(np.uint32)


# ---------------------------------------------------------------------------------------------- index maps
def shift_map(dcol=0, drow=0, dk=0):
    """M of an integer shift: the centre of cur voxel (k, row, col) lands on that of prev voxel (k + dk, row + drow, col + dcol)."""
    M = np.zeros((3, 4))
    M[:, :3] = np.eye(3)
    M[:, 3] = (dcol, drow, dk)
    return M


def turn_map(deg, centre, shift=(0., 0., 0.), scale=1.0):
    """M of a turn by `deg` degrees about the vertical through `centre` = (col, row) (continuous indices), scaled by `scale`
    about it, then shifted by (dcol, drow, dk)."""
    t = np.deg2rad(deg)
    c, s = np.cos(t) * scale, np.sin(t) * scale
    M = np.zeros((3, 4))
    M[0, :2], M[1, :2], M[2, 2] = (c, -s), (s, c), 1.
    M[0, 3] = centre[0] - (c * centre[0] - s * centre[1]) + shift[0]
    M[1, 3] = centre[1] - (s * centre[0] + c * centre[1]) + shift[1]
    M[2, 3] = shift[2]
    return M


def random_rigid_map(rng, px, nz):
    """A turn of up to +-40 degrees about a point near the middle plus a shift of a few voxels (fractional, also in k)."""
    centre = rng.uniform(0.3 * px, 0.7 * px, 2)
    return turn_map(rng.uniform(-40, 40), centre, (rng.uniform(-0.15, 0.15) * px, rng.uniform(-0.15, 0.15) * px, rng.uniform(-1.5, 1.5)))


def affine_map(rng, px, nz):
    """A general affine map with scale and shear: nothing in the contract asks M to be rigid."""
    M = turn_map(rng.uniform(-25, 25), (0.5 * px, 0.5 * px), (rng.uniform(-2, 2), rng.uniform(-2, 2), 0.25), scale=rng.uniform(0.8, 1.25))
    M[0, 1] += 0.07
    M[2, 2], M[2, 0] = 0.9, 0.01
    return M


# ---------------------------------------------------------------------------------------------- scenes
def blobs(px, nz, n_blobs, radius, seed, n_rows=None, stray=0):
    """(volume int32 [nz, px, px], rows): n_blobs balls of up to `radius` voxels at random places, ball i with id i (a later ball
    overwrites an earlier one; some ids may end without a voxel), -1 elsewhere; rows = n_rows or n_blobs + 3 (rows without a
    voxel); `stray` voxels get ids outside [-1, rows): rows, rows + 7, -2, the int32 extremes."""
    rng = np.random.default_rng(seed)
    vol = np.full((nz, px, px), -1, dtype=np.int32)
    for i in range(n_blobs):
        ck, cr, cc = rng.integers(0, nz), rng.integers(0, px), rng.integers(0, px)
        r = rng.uniform(0.5, radius)
        h = int(np.ceil(r))
        k0, r0, c0 = max(ck - h, 0), max(cr - h, 0), max(cc - h, 0)
        sub = vol[k0:ck + h + 1, r0:cr + h + 1, c0:cc + h + 1]                   # (a view: the ball is written into vol)
        k, row, col = np.meshgrid(np.arange(sub.shape[0]) + k0, np.arange(sub.shape[1]) + r0, np.arange(sub.shape[2]) + c0, indexing='ij')
        sub[((k - ck) * 2.0) ** 2 + (row - cr) ** 2 + (col - cc) ** 2 <= r * r] = i
    rows = n_blobs + 3 if n_rows is None else n_rows
    if stray:
        at = rng.choice(vol.size, size=stray, replace=False)
        vol.reshape(-1)[at] = rng.choice(np.array([rows, rows + 7, -2, -2 ** 31, 2 ** 31 - 1], dtype=np.int64), size=stray).astype(np.int32)
    return vol, rows


def moved(vol, M_inv_shift):
    """`vol` shifted by whole voxels (dcol, drow, dk): out[k, row, col] = vol[k - dk, row - drow, col - dcol], -1 where that
    falls outside -- the cur volume of a scene whose prev is `vol` and whose map is shift_map(-dcol, -drow, -dk)."""
    dcol, drow, dk = M_inv_shift
    nz, px, _ = vol.shape
    out = np.full_like(vol, -1)
    k, row, col = np.meshgrid(np.arange(nz), np.arange(px), np.arange(px), indexing='ij')
    sk, sr, sc = k - dk, row - drow, col - dcol
    ok = (sk >= 0) & (sk < nz) & (sr >= 0) & (sr < px) & (sc >= 0) & (sc < px)
    out[ok] = vol[sk[ok], sr[ok], sc[ok]]
    return out


def whole_lines(px, nz):
    """One instance filling whole lines (every other row of every k): a wave sees ONE run per segment."""
    vol = np.full((nz, px, px), -1, dtype=np.int32)
    vol[:, ::2, :] = 0
    return vol, 1


def checker(px, nz):
    """A checkerboard of the ids 0 and 1: every lane of a wave is its own run."""
    k, row, col = np.meshgrid(np.arange(nz), np.arange(px), np.arange(px), indexing='ij')
    return ((k + row + col) & 1).astype(np.int32), 2


def many_pairs(px, nz):
    """Every voxel its own instance in both volumes (ids along the first line only, so the rows stay few): more than 16 pairs."""
    vol = np.full((nz, px, px), -1, dtype=np.int32)
    n = min(px, 40)
    vol[0, 0, :n] = np.arange(n)
    return vol, n


SHAPES = [(8, 1), (33, 7), (72, 5), (136, 32)]      # a single line; odd sizes; wider than one wave per line; the full height
DENSITIES = ('sparse', 'dense')
_scenes, _models = {}, {}


def random_scene(px, nz, density):
    """Two blob volumes of one shape, made once and never changed: 'sparse' = a few large instances, 'dense' = many small ones
    (most lanes of a wave then see another key than their neighbour).  Returns a dict: prev, n_prev, cur, n_cur, ids (per-point
    ids of cur, some outside the rows), prev_track (numbers with gaps and a -1) and t0."""
    key = (px, nz, density)
    if key not in _scenes:
        cells = px * px * nz
        n, radius = (max(cells // 500, 4), 6.0) if density == 'sparse' else (max(cells // 60, 6), 2.5)
        n = min(n, 60000)
        seed = px * 1000 + nz * 10 + DENSITIES.index(density)
        prev, n_prev = blobs(px, nz, n, radius, seed, stray=min(5, cells // 8))
        cur, n_cur = blobs(px, nz, n + 2, radius, seed + 5, stray=min(7, cells // 8))
        rng = np.random.default_rng(seed + 9)
        ids = rng.integers(-3, n_cur + 4, size=501).astype(np.int32)
        prev_track = (rng.permutation(n_prev) * 3 + 100).astype(np.int32)
        prev_track[n_prev // 2] = -1
        for a in (prev, cur, ids, prev_track):
            a.setflags(write=False)
        _scenes[key] = dict(prev=prev, n_prev=n_prev, cur=cur, n_cur=n_cur, ids=ids, prev_track=prev_track, t0=1000 + n_prev * 3)
    return _scenes[key]


def scene_maps(px, nz):
    """{name: M}: the identity, a shift by whole voxels, a rigid turn with a fractional shift, a general affine map."""
    rng = np.random.default_rng(px * 77 + nz)
    return {'identity': shift_map(), 'shift': shift_map(min(3, px - 1), -min(2, px - 1), 1 if nz > 1 else 0),
            'rigid': random_rigid_map(rng, px, nz), 'affine': affine_map(rng, px, nz)}


def scene_model(px, nz, density, name):
    """model() of random_scene(px, nz, density) under scene_maps(px, nz)[name], computed once."""
    key = (px, nz, density, name)
    if key not in _models:
        s = random_scene(px, nz, density)
        _models[key] = model(s['prev'], s['n_prev'], s['cur'], s['n_cur'], scene_maps(px, nz)[name], prev_track=s['prev_track'],
                             t0=s['t0'], ids=s['ids'])
    return _models[key]


# ---------------------------------------------------------------------------------------------- geometry
def index_to_store(geom):
    """A (4 x 4): continuous index (u, v, w) = (col, row, k) of a grid -> store coordinates, the inverse of the view's cell
    rule (cell i covers [(i - px / 2) view / px, ...), image row = px - 1 - j, bin k covers [z_lo + k z_step, ...), the view
    frame is R (p - origin) + (dx, dy)), written out independently of pca_amd.host_logic.voxel_index_map."""
    origin, R, dx, dy, view, px, z_lo, z_step = geom
    c = view / px
    S = np.array([[c, 0, 0, -0.5 * px * c - dx], [0, -c, 0, 0.5 * px * c - dy], [0, 0, z_step, z_lo], [0, 0, 0, 1.]])
    Rt = np.eye(4)
    Rt[:3, :3] = np.asarray(R, dtype=np.float64).reshape(3, 3).T
    Tr = np.eye(4)
    Tr[:3, 3] = origin
    return Tr @ Rt @ S


def cell_of(p, geom):
    """(k, row, col) as floats (floor applied) of store points p [n, 3] under the cell rule of voxel_labels_common /
    elev_partition_common: a = R (p - origin) + (dx, dy), i = floor(a_x / view px + px / 2), row = px - 1 - j,
    k = floor((z - oz - z_lo) / z_step); plus the fractional distances to the nearest cell edge, in cells."""
    origin, R, dx, dy, view, px, z_lo, z_step = geom
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    d = p - np.asarray(origin, dtype=np.float64)
    ax = R[0, 0] * d[:, 0] + R[0, 1] * d[:, 1] + dx
    ay = R[1, 0] * d[:, 0] + R[1, 1] * d[:, 1] + dy
    t = np.stack([(d[:, 2] - z_lo) / z_step, ay / view * px + 0.5 * px, ax / view * px + 0.5 * px], axis=1)
    edge = np.abs(t - np.rint(t)).min(axis=1)
    f = np.floor(t)
    f[:, 1] = px - 1 - f[:, 1]
    return f, edge
