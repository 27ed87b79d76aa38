"""Camera rays cast through the voxel grid of the occupancy labels (pca_bev_voxel_camera): a numpy model of the kernel
contract (vectorised over the rays, a loop over the steps), an independent check of it by the slab method, and the builders
of the GPU tests' inputs.

The model restates include/pca.h.  Everything is f64, each operation rounded on its own.  The camera is Minv (3x3) and C, as
the host hands them over; nu = W // stride, nv = H // stride; ray r = j nu + i goes through u = i stride + (stride - 1) / 2,
v = j stride + (stride - 1) / 2:
    dir_k = (Minv[k][0] u + Minv[k][1] v) + Minv[k][2],  S = C,  E_k = C_k + max_depth dir_k
    s, e = grid_coords(S), grid_coords(E) (voxel_rays_common: the ray passes' own expressions)
A ray with a coordinate that is not finite or >= 2^30 in magnitude is dropped (stats[2]); with start voxel c, end voxel g,
n_a = |g_a - c_a|, a ray with N = n_0 + n_1 + n_2 > MAX_STEPS is dropped (stats[3]).  tMax, tDelta and the step (ties u, v, w)
are those of voxel_rays_common.traverse, but the ray visits N + 1 voxels: each one inside the grid is marked in `visible` at
[k][px - 1 - j][i], and the first whose label is not 255 is the ray's hit and ends it.  t_enter = 0 for the start voxel, else
the tMax of the axis just stepped before its increment; depth = float32(t_enter max_depth)."""
import numpy as np

import voxel_rays_common as rc
from voxel_rays_common import grid_coords

MAX_STEPS = rc.MAX_STEPS
COORD_LIM = rc.COORD_LIM


def camera_of(P):
    """(Minv, C) of P = [M | p4], as _lib.make_ray_camera computes them."""
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    Minv = np.linalg.inv(P[:, :3])
    return Minv, -(Minv @ P[:, 3])


def look_at(centre, target, f, W, H, up=(0., 0., 1.)):
    """P 3x4 of a pinhole at `centre` looking at `target`, focal length f pixels, principal point in the image's middle."""
    centre, target = np.asarray(centre, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - centre
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, dtype=np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    K = np.array([[f, 0., (W - 1) / 2.], [0., f, (H - 1) / 2.], [0., 0., 1.]])
    return K @ np.concatenate([Rm, -(Rm @ centre)[:, None]], axis=1)


def ray_ends(Minv, C, W, H, stride, max_depth):
    """(S, E), (nv nu, 3) each, in ray order r = j nu + i."""
    Minv, C = np.asarray(Minv, dtype=np.float64).reshape(3, 3), np.asarray(C, dtype=np.float64).reshape(3)
    nu, nv = W // stride, H // stride
    half = (stride - 1) / 2.0
    v, u = np.meshgrid(np.arange(nv) * stride + half, np.arange(nu) * stride + half, indexing='ij')
    u, v = u.ravel(), v.ravel()
    with np.errstate(all='ignore'):
        E = np.stack([C[k] + max_depth * ((Minv[k, 0] * u + Minv[k, 1] * v) + Minv[k, 2]) for k in range(3)], 1)
    return np.repeat(C[None], nu * nv, axis=0), E


def walk(s, e, labels, px, nz, max_depth, visible=None, max_steps=MAX_STEPS, record=False):
    """Rays from grid coordinates s to e, (M, 3) each, through `labels` uint8 (nz, px, px).  visible: marked into a copy of
    it (None: zeros).  Returns a dict: 'visible' uint8 (nz, px, px); 'hit' int32, 'depth' float32, 'label' uint8, (M,) each;
    'stats' int64 [5]; 'N' int64 (M,), -1 for a dropped ray; 't_hit' f64 (M,), the hit's t_enter, inf without a hit; 'ties'
    the number of steps at which the two smallest tMax were equal (and finite); with record, 'visited' int64 (K, 4): (ray, i,
    j, k) of every mark."""
    s, e = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(e, dtype=np.float64).reshape(-1, 3)
    lab_flat = np.asarray(labels, dtype=np.uint8).reshape(nz * px * px)
    M = s.shape[0]
    dims = np.array([px, px, nz], dtype=np.int64)
    vis = np.zeros(nz * px * px, dtype=np.uint8) if visible is None else np.array(visible, dtype=np.uint8).reshape(nz * px * px)
    stats = np.zeros(5, dtype=np.int64)
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
    hit = np.full(M, -1, dtype=np.int32)
    depth = np.zeros(M, dtype=np.float32)
    label = np.full(M, 255, dtype=np.uint8)
    t_enter = np.zeros(M)
    t_hit = np.full(M, np.inf)
    ties = 0
    visited = []
    idx = np.flatnonzero(cast)
    it = 0
    while idx.size:
        ci = c[idx]
        inside = ((ci >= 0) & (ci < dims)).all(axis=1)
        at, rays_in = ci[inside], idx[inside]
        place = (at[:, 2] * px + (px - 1 - at[:, 1])) * px + at[:, 0]
        vis[place] = 1
        if record:
            visited.append(np.concatenate([rays_in[:, None], at], axis=1))
        stopped = lab_flat[place] != 255
        hr = rays_in[stopped]
        hit[hr] = place[stopped]
        label[hr] = lab_flat[place[stopped]]
        t_hit[hr] = t_enter[hr]
        depth[hr] = (t_enter[hr] * max_depth).astype(np.float32)
        go_on = np.ones(idx.size, dtype=bool)
        go_on[inside] = ~stopped
        idx = idx[go_on & (N[idx] > it)]                          # (the end voxel has been visited: N + 1 visits)
        t = tmax[idx]
        a = np.where((t[:, 0] <= t[:, 1]) & (t[:, 0] <= t[:, 2]), 0, np.where(t[:, 1] <= t[:, 2], 1, 2))
        ts = np.sort(t, axis=1)
        ties += int(((ts[:, 0] == ts[:, 1]) & np.isfinite(ts[:, 1])).sum())
        t_enter[idx] = t[np.arange(idx.size), a]
        c[idx, a] += step[idx, a]
        n[idx, a] -= 1
        assert (n[idx, a] >= 0).all()
        tmax[idx, a] = np.where(n[idx, a] > 0, t[np.arange(idx.size), a] + tdelta[idx, a], np.inf)
        it += 1
    stats[4] = (hit >= 0).sum()
    out = {'visible': vis.reshape(nz, px, px), 'hit': hit, 'depth': depth, 'label': label, 'stats': stats,
           'N': np.where(cast, N, -1), 't_hit': t_hit, 'ties': ties}
    if record:
        out['visited'] = np.concatenate(visited) if visited else np.zeros((0, 4), dtype=np.int64)
    return out


def model(labels, Minv, C, W, H, stride, max_depth, origin, R, dx, dy, view, px, z_lo, z_step, nz, visible=None, record=False):
    """One call of pca_bev_voxel_camera: walk()'s dict, 'hit', 'depth' and 'label' shaped (nv, nu), plus the rays' grid
    coordinates 's' and 'e'."""
    S, E = ray_ends(Minv, C, W, H, stride, max_depth)
    s = grid_coords(S, origin, R, dx, dy, view, px, z_lo, z_step)
    e = grid_coords(E, origin, R, dx, dy, view, px, z_lo, z_step)
    out = walk(s, e, labels, px, nz, max_depth, visible=visible, record=record)
    nu, nv = W // stride, H // stride
    for k in ('hit', 'depth', 'label'):
        out[k] = out[k].reshape(nv, nu)
    out['s'], out['e'] = s, e
    return out


def lidar_style_marks(s, e, px, nz):
    """What a walk that never stops would mark: traverse()'s 'seen' of the same rays plus their end voxels."""
    out = rc.traverse(s, e, px, nz)
    seen = out['seen'].copy()
    cast = out['N'] >= 0
    g = np.floor(np.asarray(e, dtype=np.float64)[cast]).astype(np.int64)
    inside = ((g >= 0) & (g < np.array([px, px, nz]))).all(axis=1)
    g = g[inside]
    seen[g[:, 2], px - 1 - g[:, 1], g[:, 0]] = 1
    return seen


# ---------------------------------------------------------------------------------------------- the independent check
def slab_check(s, e, out, px, nz, chunk=200):
    """Shares nothing with walk(): (1) the closed box of every voxel a ray marked is met by its segment within 1e-9 grid
    units; (2) every voxel of the grid whose interior holds more than 1e-6 grid units of the segment BEFORE the parameter
    of the ray's hit (its whole length where the ray hit nothing) was marked by that ray.  `out`: walk(record=True) of cast
    rays only.  Returns the number of (ray, voxel) pairs (2) demanded."""
    s, e = np.asarray(s, dtype=np.float64).reshape(-1, 3), np.asarray(e, dtype=np.float64).reshape(-1, 3)
    M = s.shape[0]
    vis = out['visited']
    r, vox = vis[:, 0], vis[:, 1:].astype(np.float64)
    _, t_in, t_out = rc.segment_box_length(s[r], e[r], vox - 1e-9, vox + 1.0 + 1e-9)
    assert (t_in <= t_out).all()
    assert (t_in <= out['t_hit'][r] + 1e-9).all()                 # nothing is marked behind the hit
    ii, jj, kk = np.meshgrid(np.arange(px), np.arange(px), np.arange(nz), indexing='ij')
    boxes = np.stack([ii.ravel(), jj.ravel(), kk.ravel()], 1).astype(np.float64)
    V = boxes.shape[0]
    was = np.zeros((M, V), dtype=bool)
    was[r, (vis[:, 1] * px + vis[:, 2]) * nz + vis[:, 3]] = True
    length = np.linalg.norm(e - s, axis=1)
    demanded = 0
    for lo in range(0, M, chunk):
        sl = slice(lo, lo + chunk)
        m = s[sl].shape[0]
        ss, ee = np.repeat(s[sl], V, axis=0), np.repeat(e[sl], V, axis=0)
        _, t_in, t_out = rc.segment_box_length(ss, ee, np.tile(boxes, (m, 1)), np.tile(boxes, (m, 1)) + 1.0, interior=True)
        t_stop = np.repeat(np.minimum(out['t_hit'][sl], 1.0), V)
        before = np.maximum(np.minimum(t_out, t_stop) - t_in, 0.0) * np.repeat(length[sl], V)
        must = before > 1e-6
        demanded += int(must.sum())
        assert was[sl].ravel()[must].all()
    return demanded


def compare(got, want, cam=0):
    """Camera `cam` of a DeviceStore.bev_voxel_camera result against the model's, everything exact ('visible' is compared by
    the caller where several cameras share it)."""
    for k, dt in (('hit', np.int32), ('depth', np.float32), ('label', np.uint8)):
        a = got[k][cam].cpu().numpy()
        assert a.dtype == dt and a.shape == want[k].shape, k
        assert np.array_equal(a.view(np.uint32) if k == 'depth' else a, want[k].view(np.uint32) if k == 'depth' else want[k]), \
            (k, int((a != want[k]).sum()))
    stats = got['stats'][cam].cpu().numpy()
    assert stats.dtype == np.int64 and stats.tolist() == want['stats'].tolist(), (stats, want['stats'])


# ---------------------------------------------------------------------------------------------- the cases the tests share
ROT_GRID = dict(origin=(0.3, -0.2, 0.125), R=rc.rotation(0.4), dx=0.5, dy=-0.25, view=40.)


def unit_grid(px, nz):
    """Cells of 1 m, R the identity, z from 0: the grid coordinates of (x, y, z) are (x + px / 2, y + px / 2, z), exactly."""
    return dict(origin=(0., 0., 0.), R=np.eye(3), dx=0., dy=0., view=float(px), px=px, z_lo=0., z_step=1., nz=nz)


def axis_camera(at, W, H, f=16., sign=1.):
    """(Minv, C) of a pinhole at `at` looking along sign * x: dir = (sign, (cu - u) / f, (cv - v) / f) with the principal
    point (cu, cv) in the image's middle -- exact for a power of two f; odd W and H put it on a pixel, whose row and column
    of rays then run parallel to a coordinate plane and whose own ray runs parallel to the x axis."""
    cu, cv = (W - 1) / 2., (H - 1) / 2.
    return np.array([[0., 0., sign], [-1. / f, 0., cu / f], [0., -1. / f, cv / f]]), np.asarray(at, dtype=np.float64)


def diagonal_camera(at, W, H, f=16.):
    """(Minv, C) of a pinhole at `at` looking along (1, 1, 0): dir = (1, 1, 0) + (cu - u) / f (1, -1, 0) + (cv - v) / f (0, 0, 1)."""
    cu, cv = (W - 1) / 2., (H - 1) / 2.
    return np.array([[-1. / f, 0., 1. + cu / f], [1. / f, 0., 1. - cu / f], [0., -1. / f, cv / f]]), np.asarray(at, dtype=np.float64)


def scene(name, px=16, nz=4, W=24, H=16, stride=1):
    """One named case: a dict with 'grid' (the keyword arguments of model() that describe the grid), 'labels', 'Minv', 'C',
    'W', 'H', 'stride', 'max_depth'.  Made afresh on every call, from fixed seeds."""
    rng = np.random.default_rng([px, nz, W, H, stride])
    g = unit_grid(px, nz)
    lab = random_labels(rng, px, nz, 0.06)
    h = px / 2.
    if name == 'random':                         # a rotated and shifted grid, a camera inside it looking slightly down
        g = dict(ROT_GRID, px=px, z_lo=-1., z_step=4. / nz, nz=nz)
        Minv, C = camera_of(look_at((-9., 2., 1.5), (8., -3., 0.5), 0.6 * W, W, H))
        depth = 40.
    elif name == 'inside_occupied':              # the camera's own voxel is occupied
        Minv, C = axis_camera((2.5 - h, 8.25 - h, 1.5), W, H)
        lab[1, px - 1 - 8, 2] = 3
        depth = float(px)
    elif name == 'outside_in':
        Minv, C = axis_camera((-5.5 - h, 8.25 - h, 1.5), W, H)
        depth = 2. * px
    elif name == 'outside_away':
        Minv, C = axis_camera((-5.5 - h, 8.25 - h, 1.5), W, H, sign=-1.)
        depth = 2. * px
    elif name == 'axis_parallel':                # (odd W and H: the middle row, column and pixel)
        Minv, C = axis_camera((1.5 - h, 8.5 - h, 1.5), W, H)
        lab[:, px - 1 - 8, :6] = 255             # (the middle ray runs a few voxels before anything can stop it)
        depth = float(px)
    elif name == 'diagonal_ties':                # the camera at integer grid coordinates: tMax_u == tMax_v on the middle ray
        Minv, C = diagonal_camera((2. - h, 2. - h, 1.), W, H)
        depth = float(px)
    elif name == 'ends_inside':                  # max_depth ends the rays inside the grid; the middle ray's end voxel is occupied
        Minv, C = axis_camera((2.5 - h, 8.5 - h, 1.5), W, H)
        lab[:] = 255
        lab[1, px - 1 - 8, 8] = 7
        depth = 6.
    elif name == 'too_long':                     # N > MAX_STEPS for every ray
        Minv, C = axis_camera((2.5 - h, 8.5 - h, 1.5), W, H)
        depth = 1e5
    elif name == 'not_finite':                   # the end's grid coordinates lie beyond 2^30
        Minv, C = axis_camera((2.5 - h, 8.5 - h, 1.5), W, H)
        depth = 1e12
    else:
        raise KeyError(name)
    return dict(grid=g, labels=lab, Minv=Minv, C=C, W=W, H=H, stride=stride, max_depth=depth)


def model_of(sc, visible=None, record=False):
    return model(sc['labels'], sc['Minv'], sc['C'], sc['W'], sc['H'], sc['stride'], sc['max_depth'], visible=visible,
                 record=record, **sc['grid'])


def random_labels(rng, px, nz, fill):
    """uint8 (nz, px, px): a fraction `fill` of the voxels occupied with labels 0 .. 9, the rest 255."""
    lab = np.full((nz, px, px), 255, dtype=np.uint8)
    occ = rng.random((nz, px, px)) < fill
    lab[occ] = rng.integers(0, 10, int(occ.sum()), dtype=np.uint8)
    return lab
