"""Lidar rays cast through the voxel grid of the occupancy labels (pca_bev_voxel_rays): a numpy model of the kernel contract
(vectorised over the rays, a loop over the steps) and the builders of the GPU tests' inputs.

The model restates include/pca.h.  Everything is f64, each operation rounded on its own; the product sum is the UNFUSED
one, so numpy repeats the kernel's grid coordinates bit for bit (owed re-transforms aside: the callers hand over rows that
already carry them, as voxel_labels_common's callers do):
    x = X - ox, y = Y - oy;  ax = (r0 x + r1 y) + dx,  ay = (r3 x + r4 y) + dy
    u = ax / view * px + 0.5 px,  v = ay / view * px + 0.5 px,  w = (((Z - oz) + 0.0) - z_lo) / z_step
    voxel (i, j, k) = (floor u, floor v, floor w), unclamped; in the grid iff 0 <= i, j < px and 0 <= k < nz; its place in
    the output is [k][px - 1 - j][i].
One ray per stored point (dyn == 1 only with include_dyn), from the origin of the point's frame to the point.  A ray with a
coordinate that is not finite or >= 2^30 in magnitude is dropped (stats[2]); with start voxel c, end voxel g, n_a = |g_a -
c_a|, a ray with N = n_0 + n_1 + n_2 > MAX_STEPS is dropped (stats[3]).  Traversal: d = e - s, step = sign(g - c); for
n_a > 0: tMax_a = ((c_a + (step_a > 0)) - s_a) / d_a, tDelta_a = 1 / |d_a|, else tMax_a = inf.  N times: mark c if it is in
the grid; a = 0 if t0 <= t1 and t0 <= t2, else 1 if t1 <= t2, else 2; c_a += step_a; n_a -= 1; tMax_a = tMax_a + tDelta_a
if n_a else inf.  The end voxel is never marked by its own ray."""
import numpy as np

import elev_partition_common as ec

random_rows = ec.random_rows
rotation = ec.rotation
MAX_STEPS = 16384
COORD_LIM = 2.0 ** 30


def grid_coords(P, origin, R, dx, dy, view, px, z_lo, z_step):
    """(M, 3) positions -> (M, 3) grid coordinates (u, v, w)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    with np.errstate(all='ignore'):
        x, y = P[:, 0] - origin[0], P[:, 1] - origin[1]
        ax = (R[0, 0] * x + R[0, 1] * y) + dx
        ay = (R[1, 0] * x + R[1, 1] * y) + dy
        u = ax / view * px + 0.5 * px
        v = ay / view * px + 0.5 * px
        w = (((P[:, 2] - origin[2]) + 0.0) - z_lo) / z_step
    return np.stack([u, v, w], 1)


def traverse(s, e, px, nz, max_steps=MAX_STEPS, record=False):
    """Rays from grid coordinates s to e, (M, 3) each.  Returns a dict: 'seen' uint8 (nz, px, px); 'stats' int64 [4] with
    [0] = M; 'N' int64 (M,): the steps of a cast ray, -1 for a dropped one; 'marks' int64 (M,): how many of a ray's steps
    were inside the grid; 'ties' the number of steps at which the two smallest tMax were equal (and finite); with record,
    'visited' int64 (K, 4): (ray, i, j, k) of every mark."""
    s, e = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(e, dtype=np.float64).reshape(-1, 3)
    M = s.shape[0]
    dims = np.array([px, px, nz], dtype=np.int64)
    seen = np.zeros(nz * px * px, dtype=np.uint8)
    stats = np.zeros(4, dtype=np.int64)
    stats[0] = M
    with np.errstate(all='ignore'):
        ok = (np.abs(s) < COORD_LIM).all(axis=1) & (np.abs(e) < COORD_LIM).all(axis=1)     # (False for NaN)
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
    step = np.sign(g - c)
    with np.errstate(all='ignore'):
        d = e - s
        moving = cast[:, None] & (n > 0)
        tmax = np.where(moving, ((c + (step > 0)).astype(np.float64) - s) / d, np.inf)
        tdelta = np.where(moving, 1.0 / np.abs(d), 0.0)
    N_out = np.where(cast, N, -1)
    marks = np.zeros(M, dtype=np.int64)
    ties = 0
    visited = []
    idx = np.flatnonzero(cast & (N > 0))
    it = 0
    while idx.size:
        ci = c[idx]
        inside = ((ci >= 0) & (ci < dims)).all(axis=1)
        at = ci[inside]
        seen[(at[:, 2] * px + (px - 1 - at[:, 1])) * px + at[:, 0]] = 1
        marks[idx[inside]] += 1
        if record:
            visited.append(np.concatenate([idx[inside][:, None], at], axis=1))
        t = tmax[idx]
        a = np.where((t[:, 0] <= t[:, 1]) & (t[:, 0] <= t[:, 2]), 0, np.where(t[:, 1] <= t[:, 2], 1, 2))
        ts = np.sort(t, axis=1)
        ties += int(((ts[:, 0] == ts[:, 1]) & np.isfinite(ts[:, 1])).sum())
        c[idx, a] += step[idx, a]
        n[idx, a] -= 1
        assert (n[idx, a] >= 0).all()
        tmax[idx, a] = np.where(n[idx, a] > 0, t[np.arange(idx.size), a] + tdelta[idx, a], np.inf)
        it += 1
        idx = idx[N[idx] > it]
    assert (c[cast] == g[cast]).all()                            # driven by the step counts: every ray ends in its end voxel
    out = {'seen': seen.reshape(nz, px, px), 'stats': stats, 'N': N_out, 'marks': marks, 'ties': ties}
    if record:
        out['visited'] = np.concatenate(visited) if visited else np.zeros((0, 4), dtype=np.int64)
    return out


def model(frames, origins, origin, R, dx, dy, view, px, z_lo, z_step, nz, include_dyn, max_points=None):
    """frames: per-frame (n, 10) stored rows (x, y, z absolute, column 9 = dyn; owed re-transforms already applied);
    origins: (len(frames), 3), the sensor position of every frame.  max_points: the window is cut there.  Returns
    traverse()'s dict for the rays of the points that take part."""
    origins = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    assert origins.shape[0] == len(frames)
    rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in frames]) if frames else np.zeros((0, 10))
    start = np.concatenate([np.repeat(origins[k:k + 1], np.asarray(f).reshape(-1, 10).shape[0], axis=0)
                            for k, f in enumerate(frames)]) if frames else np.zeros((0, 3))
    if max_points is not None:
        rows, start = rows[:max_points], start[:max_points]
    take = np.ones(rows.shape[0], dtype=bool) if include_dyn else rows[:, 9] != 1
    s = grid_coords(start[take], origin, R, dx, dy, view, px, z_lo, z_step)
    e = grid_coords(rows[take, 0:3], origin, R, dx, dy, view, px, z_lo, z_step)
    return traverse(s, e, px, nz)


def state_of(counts, seen):
    """2 occupied (counts > 0), else 1 free (seen), else 0 unseen."""
    return np.where(np.asarray(counts) > 0, 2, np.where(np.asarray(seen) != 0, 1, 0)).astype(np.uint8)


def compare(out, want):
    """A DeviceStore.bev_voxel_rays result against the model's, everything exact."""
    assert sorted(out) == ['seen', 'stats']
    seen, stats = out['seen'].cpu().numpy(), out['stats'].cpu().numpy()
    assert seen.dtype == np.uint8 and seen.shape == want['seen'].shape
    assert stats.dtype == np.int64 and stats.tolist() == want['stats'].tolist(), (stats, want['stats'])
    assert np.array_equal(seen, want['seen']), int((seen != want['seen']).sum())


# ---------------------------------------------------------------------------------------------- the independent check
def segment_box_length(s, e, lo, hi, interior=False):
    """The part of the segments s -> e inside the closed boxes [lo, hi] -- interior: inside the open boxes, which differs for
    a segment that runs in a face's plane -- by the slab method (f64, arrays (M, 3)): its length in grid units (0 where the
    segment misses the box) and the parameter interval (t_in, t_out), empty where t_in > t_out.  Shares nothing with
    traverse()."""
    d = e - s
    with np.errstate(all='ignore'):
        t1, t2 = (lo - s) / d, (hi - s) / d
        tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
        par = d == 0
        inside_par = ((s > lo) & (s < hi)) if interior else ((s >= lo) & (s <= hi))
        tn = np.where(par, np.where(inside_par, -np.inf, np.inf), tn)
        tf = np.where(par, np.where(inside_par, np.inf, -np.inf), tf)
    t_in, t_out = np.maximum(tn.max(axis=1), 0.0), np.minimum(tf.min(axis=1), 1.0)
    length = np.linalg.norm(d, axis=1)
    return np.maximum(t_out - t_in, 0.0) * length, t_in, t_out
