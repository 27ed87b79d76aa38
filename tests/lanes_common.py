"""Shared by tests/test_lanes_golden.py and tests/test_gpu_lanes.py: the fixture tests/golden/lanes.npz as lists, the host
model of the lane clipping (pca_amd.host_logic.transform_traj, bit-equal to the reference: see test_lanes_golden.py) and the
generated map of the GPU tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def split(xyz, start):
    return [xyz[start[i]:start[i + 1]].copy() for i in range(len(start) - 1)]


def split_len(rows, lens):
    cuts = np.cumsum(lens)[:-1] if len(lens) else []
    return [r.copy() for r in np.split(rows, cuts)] if len(lens) else []


class Fixture:
    def __init__(self):
        g = np.load(os.path.join(GOLDEN, 'lanes.npz'), allow_pickle=False)
        self.g = g
        self.T = g['T']
        self.start = g['start']
        self.lanes_global = split(g['xyz_global'], g['start'])
        self.lanes_world = split(g['xyz_world'], g['start'])
        self.n_views = g['views'].shape[0]
        self.nz_lanes = split(g['nz_xyz'], g['nz_start'])

    def view(self, k):
        """(origin, R, dx, dy, aug_view_size, px) of view k, R the reference's own rotation_matrix_3d."""
        ox, oy, oz, rot, dx, dy, zoom, px, view_size = self.g['views'][k]
        return np.array([ox, oy, oz]), self.g['R'][k], float(dx), float(dy), float(zoom * view_size), int(px)

    def rot_ang(self, k):
        return float(self.g['views'][k][3])

    def expected(self, k, prefix=''):
        return split_len(self.g[f'{prefix}rows_{k}'], self.g[f'{prefix}len_{k}'])


def assert_same_lists(got, want, what=''):
    """Equal length, equal per-lane shapes, every f64 bit for bit (so that the sign of a zero and of a NaN counts)."""
    got = list(got)
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == np.float64 and a.shape == b.shape, (what, i, a.dtype, a.shape, b.shape)
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), (what, i)


def host_model(lanes, view):
    """What generate() leaves under 'gt_lanes' for the lanes (world frame) and one view, on the host."""
    from pca_amd import host_logic as hl
    origin, R, dx, dy, aug, px = view
    out = (hl.transform_traj(lane - origin, R, dx, dy, aug, px, mutate=False) for lane in lanes)
    return [r for r in out if r.shape[0] > 0]


# ---- the generated map of test_gpu_lanes.py -----------------------------------------------------------------------------
VIEW = 40 * 1.07
LENGTHS = [0, 1, 2, 3] + list(range(5, 61))


def generated_map(seed, n_lanes=1500, view=VIEW):
    """Lengths cycle through 0, 1, 2, 3 and 5..60; every 16th lane has edges of 1.6 x view, every 16th edges of 2e-5 m,
    every 500th 3000 vertices winding in and out of the view (so a lane spans several workgroups of 256 edges); starts
    uniform over +-1.5 x view."""
    rng = np.random.default_rng(seed)
    lanes = []
    for i in range(n_lanes):
        n = LENGTHS[i % len(LENGTHS)]
        start = np.r_[rng.uniform(-1.5 * view, 1.5 * view, 2), rng.uniform(-0.5, 0.5)]
        if i % 500 == 250:
            t = np.linspace(0, 6 * np.pi, 3000)
            r = 0.5 * view * (1 + 0.45 * np.sin(37 * t + rng.uniform(0, 6)))
            lane = np.c_[r * np.cos(t), r * np.sin(t), 0.1 * np.sin(5 * t)]
            lanes.append(lane + [rng.uniform(-2, 2), rng.uniform(-2, 2), 0.])
            continue
        step = 1.0
        if i % 16 == 7:
            n, step = max(n, 4), 1.6 * view
        elif i % 16 == 11:
            n, step = max(n, 4), 2e-5
            if i % 32 == 11:                       # half of them on the view's border, where they can cross it
                side = 0.5 * view * rng.choice([-1., 1.])
                start[int(rng.integers(0, 2))] = side
        if n == 0:
            lanes.append(np.zeros((0, 3)))
            continue
        heading = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0, 0.15 if step == 1.0 else 1.5, n))
        d = np.c_[step * np.cos(heading), step * np.sin(heading), rng.normal(0, 0.02, n)]
        d[0] = 0
        lanes.append(start + np.cumsum(d, axis=0))
    return lanes


def generated_views(seed, px=64):
    """Four views; the first is the issue's: 40 x 1.07, rot 0.7, px 64, un-shifted."""
    from pca_amd import host_logic as hl
    rng = np.random.default_rng(1000 + seed)
    views = [(np.zeros(3), hl.rotation_matrix_3d(0.7), 0., 0., VIEW, px)]
    for rot in (0., -2.1, 0.5 * np.pi):
        views.append((np.r_[rng.uniform(-6, 6, 2), rng.uniform(0, 1)], hl.rotation_matrix_3d(rot), float(rng.uniform(-2, 2)),
                      float(rng.uniform(-2, 2)), VIEW, px))
    return views


def census(lanes, view):
    """Of the edges of the map under one view: (crossings in -> out, crossings out -> in, edges with both ends outside that
    pass through the box), counted with plain numpy on the transformed vertices."""
    origin, R, dx, dy, aug, px = view
    h = 0.5 * aug
    n_io = n_oi = n_through = 0
    for lane in lanes:
        if lane.shape[0] < 2:
            continue
        p = (lane - origin) @ R.T
        x, y = p[:, 0] + dx, p[:, 1] + dy
        inside = (-h < x) & (x < h) & (-h < y) & (y < h)
        a, b = inside[:-1], inside[1:]
        n_io += int((a & ~b).sum())
        n_oi += int((~a & b).sum())
        for k in np.flatnonzero(~a & ~b):
            # Liang-Barsky: does the segment meet the open box?
            t0, t1, ok = 0., 1., True
            for p0, d in ((x[k], x[k + 1] - x[k]), (y[k], y[k + 1] - y[k])):
                for q, r in ((-d, p0 + h), (d, h - p0)):
                    if q == 0:
                        ok = ok and r > 0
                    elif q < 0:
                        t0 = max(t0, r / q)
                    else:
                        t1 = min(t1, r / q)
            n_through += int(ok and t0 < t1)
    return n_io, n_oi, n_through
