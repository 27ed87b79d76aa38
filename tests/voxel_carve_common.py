"""Free-space carving by ray hit / miss (pca_bev_voxel_carve): a numpy model of the kernel contract and the synthetic scene of
the tests (a wall, a parked car and a car that leaves).

The model restates include/pca.h.  The rays are those of tests/voxel_rays_common.py (grid_coords, the drop rules, the step
loop of traverse, here with the step index):
    a point TAKES PART iff it lies inside the window cut at max_points and (include_dyn or dyn != 1); its ray runs from the origin
    of its frame to itself and is CAST unless a coordinate is not finite or >= 2^30, or N > MAX_STEPS;
    hits[v] = the cast rays whose end voxel is v, inside the grid;
    a CANDIDATE POINT has a cast ray, an end voxel inside the grid and a class in `classes`; a candidate voxel holds one;
    cross[v] = for a candidate voxel the cast rays with a step it < N - end_margin at v, else 0;
    a candidate point in v is FLAGGED iff cross[v] >= min_cross and float(cross[v]) >= ratio * float(hits[v]);
    flags = 1 flagged, 0 candidate kept, 255 everything else;
    stats = [take part, cast, dropped not finite, dropped too long, candidate points, flagged points]."""
import numpy as np

import voxel_rays_common as rc

MAX_STEPS = rc.MAX_STEPS
DEFAULTS = (1, 2, 1.0)                 # end_margin, min_cross, ratio


def carve(s, e, in_class, px, nz, end_margin, min_cross, ratio, max_steps=MAX_STEPS):
    """Rays from grid coordinates s to e, (M, 3) each, of the points that take part; in_class (M,) bool.  Returns a dict:
    'hits', 'cross' int64 (nz, px, px); 'flags' uint8 (M,); 'stats' int64 [6]; 'place' int64 (M,): the end voxel's place in
    the output, -1 where the ray is dropped or ends outside; 'N' int64 (M,): the steps of a cast ray, -1 for a dropped one."""
    s, e = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(e, dtype=np.float64).reshape(-1, 3)
    in_class = np.asarray(in_class, dtype=bool).reshape(-1)
    M = s.shape[0]
    dims = np.array([px, px, nz], dtype=np.int64)
    stats = np.zeros(6, dtype=np.int64)
    stats[0] = M
    with np.errstate(all='ignore'):
        ok = (np.abs(s) < rc.COORD_LIM).all(axis=1) & (np.abs(e) < rc.COORD_LIM).all(axis=1)     # (False for NaN)
    stats[2] = M - ok.sum()
    c = np.zeros((M, 3), dtype=np.int64)
    g = np.zeros((M, 3), dtype=np.int64)
    c[ok], g[ok] = np.floor(s[ok]).astype(np.int64), np.floor(e[ok]).astype(np.int64)
    n = np.abs(g - c)
    N = n.sum(axis=1)
    too_long = ok & (N > max_steps)
    stats[3] = too_long.sum()
    cast = ok & ~too_long
    stats[1] = cast.sum()
    # the ends
    ends_inside = cast & ((g >= 0) & (g < dims)).all(axis=1)
    place = np.full(M, -1, dtype=np.int64)
    place[ends_inside] = (g[ends_inside, 2] * px + (px - 1 - g[ends_inside, 1])) * px + g[ends_inside, 0]
    hits = np.bincount(place[ends_inside], minlength=nz * px * px).astype(np.int64)
    is_cand = ends_inside & in_class
    cand = np.zeros(nz * px * px, dtype=bool)
    cand[place[is_cand]] = True
    # the traversal: traverse()'s loop, with the step index
    step = np.sign(g - c)
    with np.errstate(all='ignore'):
        d = e - s
        moving = cast[:, None] & (n > 0)
        tmax = np.where(moving, ((c + (step > 0)).astype(np.float64) - s) / d, np.inf)
        tdelta = np.where(moving, 1.0 / np.abs(d), 0.0)
    cross = np.zeros(nz * px * px, dtype=np.int64)
    idx = np.flatnonzero(cast & (N > 0))
    it = 0
    while idx.size:
        ci = c[idx]
        counts = ((ci >= 0) & (ci < dims)).all(axis=1) & (it < N[idx] - end_margin)
        at = ci[counts]
        lin = (at[:, 2] * px + (px - 1 - at[:, 1])) * px + at[:, 0]
        np.add.at(cross, lin[cand[lin]], 1)
        t = tmax[idx]
        a = np.where((t[:, 0] <= t[:, 1]) & (t[:, 0] <= t[:, 2]), 0, np.where(t[:, 1] <= t[:, 2], 1, 2))
        c[idx, a] += step[idx, a]
        n[idx, a] -= 1
        assert (n[idx, a] >= 0).all()
        tmax[idx, a] = np.where(n[idx, a] > 0, t[np.arange(idx.size), a] + tdelta[idx, a], np.inf)
        it += 1
        idx = idx[N[idx] > it]
    assert (c[cast] == g[cast]).all()
    flags = np.full(M, 255, dtype=np.uint8)
    pc = place[is_cand]
    flags[is_cand] = ((cross[pc] >= min_cross) & (cross[pc].astype(np.float64) >= ratio * hits[pc].astype(np.float64))).astype(np.uint8)
    stats[4], stats[5] = is_cand.sum(), (flags == 1).sum()
    return {'hits': hits.reshape(nz, px, px), 'cross': cross.reshape(nz, px, px), 'flags': flags, 'stats': stats,
            'place': place, 'N': np.where(cast, N, -1)}


def model(frames, origins, origin, R, dx, dy, view, px, z_lo, z_step, nz, include_dyn, classes, end_margin=1, min_cross=2,
          ratio=1.0, max_points=None):
    """frames: per-frame (n, 10) stored rows (x, y, z absolute, column 7 = class, column 9 = dyn; owed re-transforms already
    applied); origins: (len(frames), 3).  max_points: the window is cut there.  Returns carve()'s dict with 'flags' and
    'place' over the whole (cut) window, a point that takes no part having 255 and -1, plus 'take' (bool, the cut window)
    and 's', 'e', the grid coordinates of the rays of the points that take part."""
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    assert origins.shape[0] == len(frames)
    rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in frames]) if frames else np.zeros((0, 10))
    start = np.concatenate([np.repeat(origins[k:k + 1], np.asarray(f).reshape(-1, 10).shape[0], axis=0)
                            for k, f in enumerate(frames)]) if frames else np.zeros((0, 3))
    if max_points is not None:
        rows, start = rows[:max_points], start[:max_points]
    take = np.ones(rows.shape[0], dtype=bool) if include_dyn else rows[:, 9] != 1
    s = rc.grid_coords(start[take], origin, R, dx, dy, view, px, z_lo, z_step)
    e = rc.grid_coords(rows[take, 0:3], origin, R, dx, dy, view, px, z_lo, z_step)
    out = carve(s, e, np.isin(rows[take, 7], np.asarray(list(classes), dtype=np.float64)), px, nz, end_margin, min_cross, ratio)
    for key, fill in (('flags', 255), ('place', -1)):
        whole = np.full(rows.shape[0], fill, dtype=out[key].dtype)
        whole[take] = out[key]
        out[key] = whole
    out.update(take=take, s=s, e=e)
    return out


def compare(out, want):
    """A DeviceStore.bev_voxel_carve result against the model's, everything exact."""
    assert sorted(out) == ['cross', 'flags', 'hits', 'stats']
    hits, cross = out['hits'].cpu().numpy(), out['cross'].cpu().numpy()
    flags, stats = out['flags'].cpu().numpy(), out['stats'].cpu().numpy()
    assert stats.dtype == np.int64 and stats.tolist() == want['stats'].tolist(), (stats, want['stats'])
    for name, got in (('hits', hits), ('cross', cross)):
        assert got.dtype == np.int32 and got.shape == want[name].shape, name
        bad = got.view(np.uint32).astype(np.int64) != want[name]
        assert not bad.any(), (name, int(bad.sum()))
    assert flags.dtype == np.uint8 and flags.shape == want['flags'].shape, (flags.shape, want['flags'].shape)
    assert np.array_equal(flags, want['flags']), int((flags != want['flags']).sum())


# ---------------------------------------------------------------------------------------------- the synthetic scene
def _slab(rng, n, x, y_lo, y_hi, z_lo, z_hi, cls):
    rows = np.zeros((n, 10))
    rows[:, 0] = x + rng.uniform(-0.2, 0.2, n)
    rows[:, 1] = rng.uniform(y_lo, y_hi, n)
    rows[:, 2] = rng.uniform(z_lo, z_hi, n)
    rows[:, 7] = cls
    return rows


WALL, CAR = 3, 13


def street_scene(seed=0):
    """Three frames, the sensor moving 1 m per frame along x at z = 1.  A wall (class WALL) of 3 000 points per frame at
    x = 20, y -10..10; a car slab (class CAR, 300 points) at x = 8, y -1..1, present in frame 0 only, with the wall behind
    it left out of frame 0 where the car shadows it; a parked car slab (300 points per frame) at x = 12, y 4..6, in every
    frame, the wall behind it left out likewise.  Returns (frames, origins, kind): kind per point of the window, 0 wall,
    1 the car that leaves, 2 the parked car.  The grid to use: origin 0, identity, view 64, px 64 (1 m cells), z 0..4, nz 4."""
    rng = np.random.default_rng(seed)
    frames, kinds = [], []
    origins = np.array([[0., 0., 1.], [1., 0., 1.], [2., 0., 1.]])
    for k in range(3):
        sensor = origins[k]
        wall = _slab(rng, 3000, 20., -10., 10., 0.2, 2.8, WALL)
        wall[:, 0] = 20.5                                        # a plane in the middle of its cells
        parked = _slab(rng, 300, 12.5, 4., 6., 0.2, 1.8, CAR)
        parts, kind = [parked], [np.full(300, 2)]
        blockers = [(12.5, 4., 6.)]
        if k == 0:
            parts.append(_slab(rng, 300, 8.5, -1., 1., 0.2, 1.8, CAR))
            kind.append(np.full(300, 1))
            blockers.append((8.5, -1., 1.))
        # the wall points whose beam meets a car slab first (y at the slab's x, with some margin) are not seen
        keep = np.ones(wall.shape[0], dtype=bool)
        for bx, y0, y1 in blockers:
            t = (bx - sensor[0]) / (wall[:, 0] - sensor[0])
            y_at = sensor[1] + t * (wall[:, 1] - sensor[1])
            z_at = sensor[2] + t * (wall[:, 2] - sensor[2])
            keep &= ~((y_at > y0 - 0.5) & (y_at < y1 + 0.5) & (z_at < 2.3))
        parts.append(wall[keep])
        kind.append(np.zeros(int(keep.sum()), dtype=np.int64))
        frames.append(np.concatenate(parts))
        kinds.append(np.concatenate(kind))
    return frames, origins, np.concatenate(kinds)


STREET_GRID = dict(origin=(0., 0., 0.), R=np.eye(3), dx=0., dy=0., view=64., px=64, z_lo=0., z_step=1., nz=4)
