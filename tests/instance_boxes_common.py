"""Oriented metric boxes around the window's instances (pca_bev_instance_boxes): a numpy model of the kernel contract in
include/pca.h, the scene builders and the comparison.  A plain module: no test, no fixture.

The model restates the contract over (ids, stored rows).  A row takes part iff 0 <= id < n_rows.  x = X - ox, y = Y - oy,
ax = fma(r1, y, r0 x) + dx, ay = fma(r4, y, r3 x) + dy -- numpy has no fma: the two are evaluated EXACTLY, in fractions of
integers (render_camera_common._fma), for every point -- z = (Z - oz) + 0.0.  Everything else is plain numpy f64 with the
operations in the written order: e1 = (c ax + s ay) + 0.0, e2 = (c ay - s ax) + 0.0, the extremes per (id, t) with np.fmin /
np.fmax (a NaN is never an extreme), near_t with np.fmin of the four distances, area_t = (hi1 - lo1) (hi2 - lo2), and the
choice as one pass over t that replaces the best only by a strictly better one (a NaN area ranks as +inf)."""
import numpy as np

from render_camera_common import _fma

PIECE = 2048                                                    # BOX_PIECE of pca_bev_boxes.hip: a row above it has several pieces
_coords = {}


def coords(rows, origin, R, dx, dy):
    """(ax, ay, z) of every stored row; the two fma's exact.  Computed once per (points, frame)."""
    xyz = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 10)[:, :3])
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(3, 3)
    o = np.asarray(origin, dtype=np.float64)
    key = (xyz.tobytes(), R.tobytes(), o.tobytes(), float(dx), float(dy))
    if key not in _coords:
        x, y = xyz[:, 0] - o[0], xyz[:, 1] - o[1]
        px, py = R[0, 0] * x, R[1, 0] * x
        ax = np.array([_fma(R[0, 1], b, c) for b, c in zip(y, px)], dtype=np.float64).reshape(-1) + dx
        ay = np.array([_fma(R[1, 1], b, c) for b, c in zip(y, py)], dtype=np.float64).reshape(-1) + dy
        z = (xyz[:, 2] - o[2]) + 0.0
        for a in (ax, ay, z):
            a.setflags(write=False)
        _coords[key] = (ax, ay, z)
    return _coords[key]


def choose(area, near, criterion):
    """t* per row: one pass over t, the best replaced only by a strictly better direction."""
    n_rows, n_angles = area.shape
    ka = np.where(np.isnan(area), np.inf, area)
    kn = near if criterion == 1 else np.zeros_like(near)
    best = np.zeros(n_rows, dtype=np.int64)
    b_n, b_a = kn[:, 0].copy(), ka[:, 0].copy()
    for t in range(1, n_angles):
        better = (kn[:, t] > b_n) | ((kn[:, t] == b_n) & (ka[:, t] < b_a))
        best[better] = t
        b_n[better], b_a[better] = kn[better, t], ka[better, t]
    return best


def model(ids, rows, origin, R, dx, dy, n_rows, cos_sin, criterion=0, edge_dist=0.2, want_near=False, max_points=None):
    """ids: int (N,), rows: (N, 10) stored rows or a list of frames of them, in window order.  Returns a dict: 'fit' f64
    [n_rows, 8], 'fit_n' int64 [n_rows, 2], 'extents' f64 [n_rows, n_angles, 4], 'near' int64 [n_rows, n_angles] (zeros
    unless criterion == 1 or want_near), 'stats' int64 [4], 't' int64 [n_rows] (-1: a row without a point)."""
    if isinstance(rows, (list, tuple)):
        rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in rows]) if rows else np.zeros((0, 10))
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 10)
    ids = np.asarray(ids, dtype=np.int64)[:rows.shape[0]]
    assert ids.shape[0] == rows.shape[0]
    if max_points is not None:
        rows, ids = rows[:max_points], ids[:max_points]
    cs = np.asarray(cos_sin, dtype=np.float64).reshape(-1, 2)
    n_angles = cs.shape[0]
    ax, ay, z = coords(rows, origin, R, dx, dy)
    part = (ids >= 0) & (ids < n_rows)
    pid, ax, ay, z = ids[part], ax[part], ay[part], z[part]
    c, s = cs[None, :, 0], cs[None, :, 1]
    with np.errstate(all='ignore'):
        e1 = (c * ax[:, None] + s * ay[:, None]) + 0.0
        e2 = (c * ay[:, None] - s * ax[:, None]) + 0.0
        ext = np.empty((n_rows, n_angles, 4))
        ext[:, :, 0::2], ext[:, :, 1::2] = np.inf, -np.inf
        order = np.argsort(pid, kind='stable')
        starts = np.flatnonzero(np.r_[True, np.diff(pid[order]) != 0]) if pid.size else np.zeros(0, dtype=np.int64)
        used = pid[order][starts]
        zlo, zhi = np.full(n_rows, np.inf), np.full(n_rows, -np.inf)
        if pid.size:
            ext[used, :, 0] = np.fmin(np.fmin.reduceat(e1[order], starts, axis=0), np.inf)
            ext[used, :, 1] = np.fmax(np.fmax.reduceat(e1[order], starts, axis=0), -np.inf)
            ext[used, :, 2] = np.fmin(np.fmin.reduceat(e2[order], starts, axis=0), np.inf)
            ext[used, :, 3] = np.fmax(np.fmax.reduceat(e2[order], starts, axis=0), -np.inf)
            zlo[used] = np.fmin(np.fmin.reduceat(z[order], starts), np.inf)
            zhi[used] = np.fmax(np.fmax.reduceat(z[order], starts), -np.inf)
        n = np.bincount(pid, minlength=n_rows).astype(np.int64)
        near = np.zeros((n_rows, n_angles), dtype=np.int64)
        if (criterion == 1 or want_near) and pid.size:
            lo1, hi1, lo2, hi2 = (ext[pid, :, k] for k in range(4))
            d = np.fmin(np.fmin(e1 - lo1, hi1 - e1), np.fmin(e2 - lo2, hi2 - e2))
            hit = (d <= edge_dist).astype(np.int64)
            near[used] = np.add.reduceat(hit[order], starts, axis=0)
        area = (ext[:, :, 1] - ext[:, :, 0]) * (ext[:, :, 3] - ext[:, :, 2])
    t = choose(area, near, criterion)
    r = np.arange(n_rows)
    fit = np.full((n_rows, 8), np.nan)
    fit[:, 0:4] = ext[r, t]
    fit[:, 4], fit[:, 5], fit[:, 6], fit[:, 7] = zlo, zhi, area[r, t], t
    fit_n = np.stack([n, near[r, t]], axis=1)
    empty = n == 0
    fit[empty, :7], fit[empty, 7], fit_n[empty] = np.nan, -1., 0
    over = int((ids >= n_rows).sum())
    stats = np.array([part.sum(), over, (n > 0).sum(), n.max() if n_rows else 0], dtype=np.int64)
    return {'fit': fit, 'fit_n': fit_n, 'extents': ext, 'near': near, 'stats': stats, 't': np.where(empty, -1, t)}


def same_f64(a, b):
    """Equal as the contract means it: the same numbers with the same signs of zero, NaN where NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return (a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a, b, equal_nan=True)
            and np.array_equal(np.signbit(a), np.signbit(b)))


def compare(out, want, near_computed=True):
    """A DeviceStore.bev_instance_boxes result against the model's, everything exact."""
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got['stats'].dtype == np.int64 and got['stats'].tolist() == want['stats'].tolist(), (got['stats'], want['stats'])
    assert same_f64(got['fit'], want['fit']), np.argwhere(~np.isclose(got['fit'], want['fit'], rtol=0, atol=0, equal_nan=True))[:5]
    assert got['fit_n'].dtype == np.int32 and got['fit_n'].shape == want['fit_n'].shape
    wn = want['fit_n'].copy()
    if not near_computed:
        wn[:, 1] = 0
    assert np.array_equal(got['fit_n'].view(np.uint32).astype(np.int64), wn)
    if 'extents' in got:
        assert same_f64(got['extents'], want['extents'])
    if 'near' in got:
        assert got['near'].dtype == np.int32 and np.array_equal(got['near'].view(np.uint32).astype(np.int64), want['near'])


# ---------------------------------------------------------------------------------------------- scenes
# A scene is (rows (N, 10), ids int32 (N,), n_rows): points in the view frame of FRAME, taken back to stored coordinates.
FRAME = ((0.3, -0.2, 0.125), 0.4, 0.5, -0.25)                   # origin, the angle of R about z, dx, dy


def rotation(ang):
    return np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])


def frame():
    """(origin, R, dx, dy) of FRAME, the arguments of model() and of window_pass_common.params()."""
    origin, ang, dx, dy = FRAME
    return origin, rotation(ang), dx, dy


def stored(view_xyz, cls=13):
    """Points given in the view frame as stored rows: a = R (X - origin) + d  =>  X = R^T (a - d) + origin.  The trip back
    rounds, so a scene's coordinates are what coords() makes of the stored rows, not view_xyz to the bit."""
    origin, R, dx, dy = frame()
    p = np.asarray(view_xyz, dtype=np.float64).reshape(-1, 3)
    rows = np.zeros((p.shape[0], 10))
    rows[:, 0:3] = (p - [dx, dy, 0.]) @ R + origin
    rows[:, 7] = cls
    return rows


def turned(uv, theta, centre=(0., 0.)):
    """Points (u, v) given along and across direction theta, as view-frame (x, y)."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([c * uv[:, 0] - s * uv[:, 1] + centre[0], s * uv[:, 0] + c * uv[:, 1] + centre[1]], axis=1)


def with_z(xy, z):
    return np.concatenate([xy, np.broadcast_to(np.asarray(z, dtype=np.float64).reshape(-1, 1), (xy.shape[0], 1))], axis=1)


RECT = (4., 2., 0.25)                                           # length, width and spacing of the filled rectangle


def rectangle_scene(theta, centre=(3., -2.)):
    """A filled rectangle of points, 4 m x 2 m at a spacing of 0.25 m, its long side along theta; z 0.5 .. 1.5.  One row."""
    L, W, step = RECT
    u, v = np.meshgrid(np.arange(0., L + 1e-9, step) - 0.5 * L, np.arange(0., W + 1e-9, step) - 0.5 * W)
    xy = turned(np.stack([u.ravel(), v.ravel()], axis=1), theta, centre)
    rows = stored(with_z(xy, np.linspace(0.5, 1.5, xy.shape[0])))
    return rows, np.zeros(rows.shape[0], dtype=np.int32), 1


L_WALLS = np.deg2rad(30.)
L_ANGLES = 18                                                   # the table the L is searched with: 5 degrees a step


def l_scene(theta=L_WALLS, corner=(-4., 5.)):
    """Two thin walls (two lines of points 0.05 m apart) that would meet at a right angle at `corner`, seen from two sides:
    the long one runs from 1 m to 4 m along theta, the short one from 1 m to 2 m across it -- the corner itself was not
    seen.  The smallest rectangle around them lies along the line from one wall's far end to the other's, not along the
    walls: 6.0 m^2 against 8.0 m^2.  One row."""
    a = np.arange(1., 4. + 1e-9, 0.05)
    b = np.arange(1., 2. + 1e-9, 0.05)
    uv = np.concatenate([np.stack([a, np.zeros_like(a)], 1), np.stack([a, np.full_like(a, 0.05)], 1),
                         np.stack([np.zeros_like(b), b], 1), np.stack([np.full_like(b, 0.05), b], 1)])
    rows = stored(with_z(turned(uv, theta, corner), 0.75))
    return rows, np.zeros(rows.shape[0], dtype=np.int32), 1


def point_scene(copies=1):
    """One point, or `copies` coincident ones: area 0 in every direction.  Row 2 of 4."""
    rows = stored(np.tile([[1.25, -0.75, 0.5]], (copies, 1)))
    return rows, np.full(copies, 2, dtype=np.int32), 4


def big_row_scene(n=5000, seed=3):
    """A row of n > 2 PIECE points (a blob of 6 m x 2.5 m turned by 20 degrees), two small rows and points of no row, shuffled."""
    assert n > 2 * PIECE
    rng = np.random.default_rng(seed)
    big = turned(rng.uniform([-3., -1.25], [3., 1.25], (n, 2)), np.deg2rad(20.), (2., 1.))
    small = [turned(rng.uniform([-1., -0.4], [1., 0.4], (k, 2)), np.deg2rad(a), c) for k, a, c in ((37, 55., (-6., -6.)), (300, 80., (8., -5.)))]
    none = rng.uniform(-10., 10., (100, 2))
    xy = np.concatenate([big] + small + [none])
    ids = np.concatenate([np.full(n, 1), np.full(37, 0), np.full(300, 3), np.full(100, -1)]).astype(np.int32)
    perm = rng.permutation(xy.shape[0])
    return stored(with_z(xy, rng.uniform(-1., 2., xy.shape[0])))[perm], ids[perm], 5


def singles_scene(n=8192, seed=4):
    """n single-point rows, ids 0 .. n - 1 in a shuffled order: against n_rows = n / 2 the upper half is skipped."""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.uniform(-15., 15., (n, 2)), rng.uniform(-1., 2., (n, 1))], axis=1)
    return stored(xyz), rng.permutation(n).astype(np.int32), n // 2


def random_scene(n=6000, n_rows=24, seed=5):
    """Random ids in [-1, n_rows + 3) over random points: rows of a few hundred points that overlap, skipped and unused ids."""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([rng.uniform(-12., 12., (n, 2)), rng.uniform(-1., 2., (n, 1))], axis=1)
    return stored(xyz), rng.integers(-1, n_rows + 3, n).astype(np.int32), n_rows


def inside_corners(xy, corners, tol=1e-9):
    """Whether every (x, y) lies inside the counter-clockwise quadrilateral `corners` [4, 2], within tol metres."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if (corners == corners[0]).all():                            # a box of one point
        return np.hypot(xy[:, 0] - corners[0, 0], xy[:, 1] - corners[0, 1]) <= tol
    ok = np.ones(xy.shape[0], dtype=bool)
    for k in range(4):
        p, q = corners[k], corners[(k + 1) % 4]
        e = q - p
        length = np.hypot(e[0], e[1])
        if length == 0.:                                        # (a box without width: its two long sides hold the points)
            continue
        ok &= (e[0] * (xy[:, 1] - p[1]) - e[1] * (xy[:, 0] - p[0])) / length >= -tol
    return ok
