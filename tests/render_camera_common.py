"""The window of the store rendered into a pinhole camera (pca_render_camera): a numpy model of the kernel contract, the
camera of the GPU tests and the comparison.  A plain module: no test, no fixture.

The model restates include/pca.h.  A stored row (X, Y, Z, ..., r, g, b, class, inst, dyn) of the window takes part unless
include_dyn is off and dyn == 1, or a class set is given and does not hold its class.  fx, fy, d = the rows of P applied to
(X, Y, Z, 1) as fma chains in k order -- numpy has no fma: every chain is evaluated EXACTLY, in fractions, for every point --
d == 0 -> -1e-6, u = round(fx / |d|), v = round(fy / |d|); kept iff 0 <= u < W, 0 <= v < H, min_depth < d < max_depth.
key = (bits of float32(d), index in the window); a pixel takes the lexicographic minimum over the kept points whose
(2 radius + 1)^2 footprint, clipped to the image, holds it."""
import numpy as np

EMPTY = np.uint64(0xffffffffffffffff)


def _fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all='ignore'):
            return a * b + c                                  # (nothing finite to round: IEEE gives the same either way)
    # a b + c as one fraction of integers (what elev_partition_common._fma builds from Fraction objects, without their gcds:
    # every point goes through here nine times); int / int is correctly rounded
    (na, da), (nb, db), (nc, dc) = float(a).as_integer_ratio(), float(b).as_integer_ratio(), float(c).as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def row4(r, x, y, z):
    """r . [x y z 1]: the product, then three fused steps, as the kernels' row4."""
    with np.errstate(all='ignore'):
        a = np.float64(r[0]) * x
    return _fma(r[3], 1.0, _fma(r[2], z, _fma(r[1], y, a)))


_proj = {}


def project(rows, P):
    """(fx, fy, d) of every row, each an exact fma chain; computed once per (points, P)."""
    xyz = np.ascontiguousarray(np.asarray(rows, dtype=np.float64)[:, :3])
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(3, 4)
    key = (xyz.tobytes(), P.tobytes())
    if key not in _proj:
        out = np.empty((3, xyz.shape[0]))
        for k in range(3):
            out[k] = [row4(P[k], x, y, z) for x, y, z in xyz]
        out.setflags(write=False)
        _proj[key] = out
    return _proj[key]


def pixels(rows, P, W, H, depth_range=(0., np.inf)):
    """(kept [N] bool, u, v int64 [N] (0 where not kept), d f64 [N]): the reference's velo2img mask with the depth range."""
    fx, fy, d = project(rows, P)
    with np.errstate(all='ignore'):
        d = np.where(d == 0, -1e-6, d)
        u, v = np.round(fx / np.abs(d)), np.round(fy / np.abs(d))
        kept = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (d > depth_range[0]) & (d < depth_range[1])
    return kept, np.where(kept, u, 0).astype(np.int64), np.where(kept, v, 0).astype(np.int64), d


def model(frames, P, W, H, radius=0, include_dyn=True, depth_range=(0., np.inf), classes=None, max_points=None):
    """frames: list of (M, 10) stored rows in window order (or one array).  Returns a dict: 'depth' f32 [H, W], 'index' int64
    [H, W], 'rgb' u8 [H, W, 3], 'sem' u8 [H, W], 'stats' int64 [3], and for the tests' floors 'ties' (pixels whose two best
    candidates share their depth bits) and 'most' (the most candidates any pixel has)."""
    rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in frames]) if isinstance(frames, (list, tuple)) \
        else np.asarray(frames, dtype=np.float64)
    if max_points is not None:
        rows = rows[:max_points]
    n = rows.shape[0]
    part = np.ones(n, dtype=bool)
    if not include_dyn:
        part &= rows[:, 9] != 1
    if classes is not None:
        part &= np.isin(rows[:, 7], list(classes))
    if n:
        kept, u, v, d = pixels(rows, P, W, H, depth_range)
    else:
        kept, u, v, d = np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    kept = kept & part
    idx = np.flatnonzero(kept)
    with np.errstate(all='ignore'):
        bits = d[idx].astype(np.float32).view(np.uint32).astype(np.uint64)
    key = (bits << np.uint64(32)) | idx.astype(np.uint64)
    keys = np.full(H * W, EMPTY, dtype=np.uint64)
    cand = []                                                     # (pixel, key) of every candidate
    for dv in range(-radius, radius + 1):
        for du in range(-radius, radius + 1):
            uu, vv = u[idx] + du, v[idx] + dv
            ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)       # clipped to the image, not wrapped
            pix = vv[ok] * W + uu[ok]
            np.minimum.at(keys, pix, key[ok])
            cand.append((pix, key[ok]))
    pix = np.concatenate([c[0] for c in cand]) if cand else np.zeros(0, np.int64)
    ckey = np.concatenate([c[1] for c in cand]) if cand else np.zeros(0, np.uint64)
    best = (ckey >> np.uint64(32)) == (keys[pix] >> np.uint64(32))
    n_best = np.bincount(pix[best], minlength=H * W)
    covered = keys != EMPTY
    win = (keys & np.uint64(0xffffffff)).astype(np.int64)
    index = np.where(covered, win, -1)
    depth = np.where(covered, (keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    src = rows[np.where(covered, win, 0)] if n else np.zeros((H * W, 10))
    rgb = np.where(covered[:, None], src[:, 4:7], 0).astype(np.uint8)
    sem = np.where(covered, src[:, 7], 255).astype(np.uint8)
    return {'depth': depth.reshape(H, W), 'index': index.reshape(H, W), 'rgb': rgb.reshape(H, W, 3), 'sem': sem.reshape(H, W),
            'stats': np.array([int(part.sum()), idx.size, int(covered.sum())], dtype=np.int64),
            'ties': int((n_best >= 2).sum()), 'most': int(np.bincount(pix, minlength=1).max()) if pix.size else 0}


def empty(W, H):
    """What a window without a kept point renders to."""
    return {'depth': np.zeros((H, W), np.float32), 'index': np.full((H, W), -1, np.int64), 'rgb': np.zeros((H, W, 3), np.uint8),
            'sem': np.full((H, W), 255, np.uint8), 'stats': np.zeros(3, np.int64)}


# ---------------------------------------------------------------------------------------------- the GPU tests' camera
POSITION, YAW = (0.25, -0.5, 1.5), 0.3
# W, H, f and the floors of the model's own counts (points kept with include_dyn, pixels covered at radius 0)
SHAPES = [(1, 1, 0.5), (2, 1, 1.0), (5, 7, 3.0), (65, 33, 32.), (1408, 376, 552.)]


def camera(W, H, f, position=POSITION, yaw=YAW):
    """P (3x4) of a pinhole camera at `position`, looking along the x axis turned by `yaw` about z: camera axes z forward,
    x right, y down; K = [[f, 0, (W-1)/2], [0, f, (H-1)/2], [0, 0, 1]]."""
    c, s = np.cos(yaw), np.sin(yaw)
    fwd, left, up = np.array([c, s, 0.]), np.array([-s, c, 0.]), np.array([0., 0., 1.])
    R = np.stack([-left, -up, fwd])                               # world -> camera rows: x right, y down, z forward
    K = np.array([[f, 0., (W - 1) / 2.], [0., f, (H - 1) / 2.], [0., 0., 1.]])
    return K @ np.concatenate([R, (-R @ np.asarray(position, dtype=np.float64))[:, None]], axis=1)


def compare(out, want):
    """A DeviceStore.render_camera result against the model's, everything exact."""
    for k, dt in (('depth', np.float32), ('index', np.int64), ('rgb', np.uint8), ('sem', np.uint8), ('stats', np.int64)):
        got = out[k].cpu().numpy()
        assert got.dtype == dt and got.shape == want[k].shape, k
        a, b = (got.view(np.uint32), want[k].view(np.uint32)) if k == 'depth' else (got, want[k])
        assert np.array_equal(a, b), (k, int((a != b).sum()))
