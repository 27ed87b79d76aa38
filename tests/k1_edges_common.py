"""K1's frustum edges (tests/golden/k1_edges_<camera>.npz, made by tools/make_golden.py --only k1_edges): one frame per
camera whose points sit where K1's cheap f32 test and the reference's f64 projection could part.  CPU only, numpy only,
deterministic: the fixtures hold these very points and what the reference makes of them.

Families of a frame (Frame.fam holds one code per point, FAMILIES names them):
  planes   u/d = -1/2, u/d = W - 1/2, v/d = -1/2, v/d = H - 1/2, d = 0: random points in front of the camera at distances
           1, 1e3, 1e6 from it, the coordinate with the largest coefficient in the plane's form solved so that the point lies
           on the plane, rounded to f32 and stepped by -3 .. +3 f32 neighbours.  A point next to d = 0 is inside the image
           only next to the camera centre: d0 also holds the f32 lattice around the centre, column by column.
  ladder   directions inside the image scaled to a largest coordinate of 10^e (e = 30, 33 .. 38, capped at FLT_MAX), and
           ovf_*: directions and scales at which only d, only fx or only fy leaves the f32 range (where the camera has such).
  specials +-inf, NaN, -0.0, denormals and +-FLT_MAX in each coordinate in turn of a point inside the image, the all-zero point.
Placement: copies of edge points lie at lane 0 and 63, at the first and last thread of a workgroup in both rows of a packed
pair, at the first and last point of a tile, for every tile shape K1 runs (256 x 4, 512 x 4, 1024 x 4); the frame's length is
no multiple of any tile and its very last point is a ladder point of e = 36: the idle lanes of the last tile re-read it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KITTI_FILTERS = [10, 11, 12, 16, 18, 255]
FLT_MAX = float(np.finfo(np.float32).max)
STEPS = (-3, -2, -1, 0, 1, 2, 3)
PLANES = ('u_lo', 'u_hi', 'v_lo', 'v_hi', 'd0')
RUNGS = (30, 33, 34, 35, 36, 37, 38)
OVERFLOWS = ('ovf_d', 'ovf_fx', 'ovf_fy')
FAMILIES = PLANES + tuple(f'ladder_e{e}' for e in RUNGS) + OVERFLOWS + ('specials', )
FILLER = -1
N_POINTS = 3 * 4096 + 1531           # 14 tiles of 1024 (the last: 507 points), 7 of 2048, 4 of 4096
TILE_SHAPES = ((256, 4), (512, 4), (1024, 4))      # FUSED, SPLIT, the deferred frame riding in the raster

CAM_TO_VELO = np.array([[0.04307104361, -0.08829286498, 0.995162929, 0.8043914418],
                        [-0.999004371, 0.007784614041, 0.04392796942, 0.2993489574],
                        [-0.01162548558, -0.9960641394, -0.08786966659, -0.1770225824], [0, 0, 0, 1]])
P_RECT = np.array([[552.554261, 0, 682.049453, 0], [0, 552.554261, 238.769549, 0], [0, 0, 1, 0]])
ALONG_X = np.array([[0., -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]])        # camera looking along +x, y left, z up


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    T = np.eye(4)
    T[:3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                 @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T[:3, 3] = t
    return T


# camera -> (P, H, W, image seed)
CAMERAS = {
    'kitti': (P_RECT @ np.linalg.inv(CAM_TO_VELO), 376, 1408, 9001),
    'axis': (np.array([[8., 0, 48, 0], [0, 8, 32, 0], [0, 0, 1, 0]]), 64, 96, 9002),          # P2 of k1.npz
    # rotated about all three axes, 1e4 m from the origin: P[3], P[7], P[11] are large and every form cancels
    'rot': (np.array([[300., 0, 160, 0], [0, 300, 120, 0], [0, 0, 1, 0]]) @ ALONG_X
            @ np.linalg.inv(_rigid(0.3, -0.4, 1.1, [-3.1e2, 1e4, 1.7e1])), 240, 320, 9003),
    # H > W (the bound's wh = max(W, H) + 1 is H + 1); the matrix carries a factor 3, so d is three times the depth
    'portrait': (3. * np.array([[30., 0, 20, 0], [0, 30, 48, 0], [0, 0, 1, 0]]) @ ALONG_X
                 @ np.linalg.inv(_rigid(0., 0., 0., [300., 0.02, 0.01])), 96, 40, 9004),
    'tiny': (np.array([[0.8, 0, 1.0, 0], [0, 0.8, 0.5, 0], [0, 0, 1, 0]]) @ ALONG_X
             @ np.linalg.inv(_rigid(0., 0., 0.2, [0.75, -0.3, 0.1])), 1, 2, 9005),
}
CASES = tuple(CAMERAS)


def image_of(seed, H, W):
    """The image and the class map of a case: drawn at test time, never stored."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    sem = rng.integers(0, 19, (H, W)).astype(np.uint8)
    sem[rng.random((H, W)) < 0.01] = 255
    return img, sem


def stepped(x, k):
    """The k-th f32 neighbour of x (f32 array)."""
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def plane_forms(P, H, W):
    """The five forms whose sign is the frustum test, as rows [cx, cy, cz, c1]: inside means every form >= 0 (d > 0)."""
    return {'u_lo': P[0] + 0.5 * P[2], 'u_hi': (W - 0.5) * P[2] - P[0], 'v_lo': P[1] + 0.5 * P[2],
            'v_hi': (H - 0.5) * P[2] - P[1], 'd0': P[2].copy()}


def project(P, pts, H, W):
    """The generator's own f64 projection (to steer the choice of points only; the fixtures come from the reference)."""
    X = np.asarray(pts, np.float64)[:, :3]
    with np.errstate(all='ignore'):
        f = X @ P[:, :3].T + P[:, 3]
        d = np.where(f[:, 2] == 0, -1e-6, f[:, 2])
        u, v = np.round(f[:, 0] / np.abs(d)), np.round(f[:, 1] / np.abs(d))
        return (u >= 0) & (u < W) & (v >= 0) & (v < H) & (d > 0) & (d < np.inf)


def _solve_on_plane(form, X32):
    """X32 (f32 [m,3]) with the coordinate of the largest coefficient solved in f64 so that form . [X, 1] = 0, rounded to f32."""
    j = int(np.argmax(np.abs(form[:3])))
    X = X32.astype(np.float64)
    rest = form[3] + sum(form[i] * X[:, i] for i in range(3) if i != j)
    out = X32.copy()
    out[:, j] = (-rest / form[j]).astype(np.float32)
    return out, j


def _with_steps(X32, j):
    """Every point of X32 seven times: coordinate j stepped by -3 .. +3 neighbours (consecutive rows)."""
    out = np.repeat(X32, len(STEPS), axis=0)
    for s, k in enumerate(STEPS):
        out[s::len(STEPS), j] = stepped(X32[:, j], k)
    return out


def _back_project(P, uv, lam):
    """The points that project to pixel uv (f64 [m,2]) with third form lam."""
    A, p4 = P[:, :3], P[:, 3]
    rhs = lam[:, None] * np.concatenate([uv, np.ones((len(uv), 1))], 1) - p4
    return np.linalg.solve(A, rhs.T).T


def _interior_uv(rng, m, H, W):
    """Pixel coordinates well inside the image (a 1 x 2 image has little room)."""
    lo_u, hi_u = (0.5, W - 1.5) if W > 2 else (-0.3, W - 0.7)
    lo_v, hi_v = (0.5, H - 1.5) if H > 2 else (-0.3, H - 0.7)
    return np.stack([rng.uniform(lo_u, hi_u, m), rng.uniform(lo_v, hi_v, m)], 1)


def _plane_family(rng, P, H, W, name, per_scale):
    form = plane_forms(P, H, W)[name]
    dnorm = np.linalg.norm(P[2, :3])
    out = []
    for scale in (1., 1e3, 1e6):
        uv = _interior_uv(rng, per_scale, H, W)
        if name[0] == 'u':
            uv[:, 0] = -0.5 if name == 'u_lo' else W - 0.5
        elif name[0] == 'v':
            uv[:, 1] = -0.5 if name == 'v_lo' else H - 0.5
        else:                                               # d = 0: anywhere at that distance, then onto the plane
            uv = rng.uniform(-2., 2., (per_scale, 2)) * [W, H]
        X = _back_project(P, uv, dnorm * scale * rng.uniform(0.7, 40., per_scale)).astype(np.float32)
        X, j = _solve_on_plane(form, X)
        out.append(_with_steps(X, j))
    return np.concatenate(out)


def _centre_lattice(P, H, W, max_columns):
    """The f32 lattice around the camera centre: columns along the coordinate with d's largest coefficient, each solved onto
    d = 0 and stepped -3 .. +3.  Columns that hold a point inside the image first, nearest the centre first."""
    form = P[2]
    C = -np.linalg.solve(P[:, :3], P[:, 3])
    j = int(np.argmax(np.abs(form[:3])))
    i1, i2 = [i for i in range(3) if i != j]
    c32 = C.astype(np.float32)
    L = 24
    ab = np.array([(a, b) for a in range(-L, L + 1) for b in range(-L, L + 1)])
    ab = ab[np.argsort(np.abs(ab).sum(1), kind='stable')]
    base = np.repeat(c32[None], len(ab), 0)
    for row, (a, b) in enumerate(ab):
        base[row, i1], base[row, i2] = stepped(c32[i1:i1 + 1], a)[0], stepped(c32[i2:i2 + 1], b)[0]
    base, _ = _solve_on_plane(form, base)
    pts = _with_steps(base, j)
    inside = project(P, pts, H, W).reshape(len(ab), len(STEPS)).any(1)
    cols = np.concatenate([np.flatnonzero(inside)[:max_columns], np.flatnonzero(~inside)[:max_columns // 6]])
    return pts.reshape(len(ab), len(STEPS), 3)[np.sort(cols)].reshape(-1, 3)


def _directions(P, uv):
    """Unit (largest coordinate 1) directions through the pixels uv, pointing away from the camera."""
    r = np.linalg.solve(P[:, :3], np.concatenate([uv, np.ones((len(uv), 1))], 1).T).T
    return r / np.abs(r).max(1, keepdims=True)


def _ladder(rng, P, H, W, e, m):
    r = _directions(P, _interior_uv(rng, m, H, W))
    mag = np.minimum(10.0**e * rng.uniform(1., 4., m), FLT_MAX)
    return (r * mag[:, None]).astype(np.float32)


def _only_overflows(rng, P, H, W, which, m):
    """Directions inside the image and a scale at which form `which` (0 fx, 1 fy, 2 d) exceeds FLT_MAX while the other two and
    every coordinate stay below it; none where the camera has no such direction."""
    uv = np.concatenate([_interior_uv(rng, 4000, H, W), rng.uniform(-0.4, 1.4, (4000, 2))])
    uv = uv[(uv[:, 0] < W - 0.6) & (uv[:, 1] < H - 0.6)]
    r = _directions(P, uv)
    f = np.abs(r @ P[:, :3].T)
    others = np.delete(f, which, axis=1).max(1)
    lo, hi = FLT_MAX / f[:, which] * 1.02, np.minimum(FLT_MAX, FLT_MAX / others * 0.98)
    ok = np.flatnonzero(lo < hi)[:m]
    pts = (r[ok] * (0.5 * (lo[ok] + hi[ok]))[:, None]).astype(np.float32)
    g = np.abs(pts.astype(np.float64) @ P[:, :3].T)
    assert (g[:, which] > FLT_MAX).all() and (np.delete(g, which, axis=1) < FLT_MAX).all()
    return pts[project(P, pts, H, W)]


def _specials(rng, P, H, W):
    base = _back_project(P, _interior_uv(rng, 3, H, W), np.linalg.norm(P[2, :3]) * rng.uniform(4., 20., 3)).astype(np.float32)
    vals = np.array([np.inf, -np.inf, np.nan, -0.0, 1e-45, -1e-45, 1e-39, FLT_MAX, -FLT_MAX], np.float32)
    out = [base]
    for b in base:
        for j in range(3):
            p = np.repeat(b[None], len(vals), 0)
            p[:, j] = vals
            out.append(p)
    z, n0, d = np.float32(0), np.float32(-0.0), np.float32(1e-45)
    out.append(np.array([[z, z, z], [n0, n0, n0], [np.nan] * 3, [np.inf] * 3, [z, z, d], [d, z, z], [z, d, z], [-d, d, -d]], np.float32))
    return np.concatenate(out)


def hot_slots(n):
    """Where a fault of one lane, one half of a packed pair or one tile edge would show: for every tile shape (BLK threads x 4
    rows) and every tile of the frame, rows k = 0 and 1 (a packed pair; the second tile: rows 2 and 3) at lanes 0 and 63 and
    the workgroup's last thread, and the tile's last point."""
    slots = set()
    for blk, ppt in TILE_SHAPES:
        tile = blk * ppt
        for t0 in range(0, n, tile):
            pair = 2 * ((t0 // tile) % 2)
            for k in (pair, pair + 1):
                slots.update(t0 + k * blk + t for t in (0, 63, blk - 1))
            slots.update((t0, t0 + tile - 1))
    return np.array(sorted(s for s in slots if s < n - 1))


class Frame:
    def __init__(self, name):
        self.name = name
        self.P, self.H, self.W, self.seed = CAMERAS[name]
        self.filters = KITTI_FILTERS
        P, H, W = self.P, self.H, self.W
        rng = np.random.default_rng(self.seed + 50)
        fams = {}
        for pl in PLANES[:4]:
            fams[pl] = _plane_family(rng, P, H, W, pl, 40)                   # 3 x 40 x 7 = 840 points per plane
        fams['d0'] = np.concatenate([_plane_family(rng, P, H, W, 'd0', 12), _centre_lattice(P, H, W, 300)])
        for e in RUNGS:
            fams[f'ladder_e{e}'] = _ladder(rng, P, H, W, e, 330)
        for which, key in enumerate(('ovf_fx', 'ovf_fy', 'ovf_d')):
            fams[key] = _only_overflows(rng, P, H, W, which, 24)
        fams['specials'] = _specials(rng, P, H, W)
        n = N_POINTS
        # ordinary points everywhere first: around the camera, as a KITTI sweep lies around the sensor
        C = -np.linalg.solve(P[:, :3], P[:, 3])
        xyz = (C + np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-2, 3, n)], 1)).astype(np.float32)
        fam = np.full(n, FILLER, np.int32)
        # the hot slots take copies of edge points in turn: wrongly-cullable ladder points, on-plane points, specials
        hot = hot_slots(n)
        turn = [k for k in ('ladder_e36', 'u_hi', 'ladder_e38', 'v_hi', 'ladder_e34', 'u_lo', 'specials', 'v_lo', 'ladder_e35', 'd0')]
        for i, s in enumerate(hot):
            key = turn[i % len(turn)]
            src = fams[key]
            xyz[s], fam[s] = src[(3 + 7 * (i // len(turn))) % len(src)], FAMILIES.index(key)
        # the families themselves, one after the other from point 700 on, around the hot slots
        free = np.setdiff1d(np.arange(700, n - 1), hot)
        body = np.concatenate([fams[k] for k in FAMILIES])
        code = np.concatenate([np.full(len(fams[k]), i, np.int32) for i, k in enumerate(FAMILIES)])
        assert len(body) <= len(free), (name, len(body), len(free))
        xyz[free[:len(body)]], fam[free[:len(body)]] = body, code
        xyz[n - 1], fam[n - 1] = fams['ladder_e36'][0], FAMILIES.index('ladder_e36')
        self.pts = np.concatenate([xyz, ((np.arange(n) % 251) / np.float32(256.))[:, None].astype(np.float32)], 1)
        self.fam = fam
        self.pts.setflags(write=False)

    def case(self):
        """(pts float32 [n,4], P, H, W, filters, image seed)"""
        return self.pts, self.P, self.H, self.W, self.filters, self.seed

    def of(self, family):
        return np.flatnonzero(self.fam == FAMILIES.index(family))

    def images(self):
        return image_of(self.seed, self.H, self.W)


_frames = {}


def frame(name):
    if name not in _frames:
        _frames[name] = Frame(name)
    return _frames[name]


def case_kitti():
    return frame('kitti').case()


def case_axis():
    return frame('axis').case()


def case_rot():
    return frame('rot').case()


def case_portrait():
    return frame('portrait').case()


def case_tiny():
    return frame('tiny').case()


_fixtures = {}


def fixture(name):
    """What the reference made of a case: pts, mask [n], u / v of the masked points, kept (indices after the class filter)."""
    if name not in _fixtures:
        with np.load(os.path.join(GOLDEN, f'k1_edges_{name}.npz'), allow_pickle=False) as f:
            _fixtures[name] = {k: f[k] for k in f.files}
    return _fixtures[name]
