"""Scenes and plain f64 numpy models for the NuScenes front end of csrc/pca_accum.hip: K0n (k0n_project: which camera a lidar
point belongs to and where it lands), K1n (k1n_nusc and the batch form: which pixel gives a point its colour and class), the
strict bilinear sampler (sample_bilinear) and the image normaliser (image_to_nchw_f32).
tests/test_nusc_front_edges_golden.py holds the models and the C oracle to the reference's recorded outputs
(tests/golden/nusc_front_edges.npz, written by tools/make_golden.py --only nusc_front_edges) and checks the conditions the
scenes must meet; tests/test_gpu_nusc_front_edges.py runs the scenes on the device.  Nothing here needs a tolerance.

  k0n_model       ego = T @ [p; 1] (numpy's matmul, as the reference takes it), global, every camera in order; intrinsics
                  padded to 4x4, division by the third row, cz > 1e-3, 1 < u < w - 1, 1 < v < h - 1; later cameras overwrite
                  earlier ones; uv starts at 0, cam_idx at -1
  k1n_model       nearest pixel by np.round (half to even); cam_idx outside [0, ncam) dropped silently; class filter; order
                  kept; T @ [p; 1]; plus the flag "the reference would assert" (an assigned point with uv outside)
  bilinear_model  the reference's bilinear branch for a 2-D map, 0 / 0 at integer coordinates included
  nchw_model      ((x.astype(f32) / f32(255)) - mean) / std, all f32

Every image encodes position: r = column & 255, g = row & 255, b and the class depend on camera, row and column, so that the
four neighbours of a pixel differ from it in r or g (and in the class), and another camera's pixel differs in b.

A K0n scene's points near a bound are chosen by a search (select(), run by tools/make_golden.py only): 2^20 candidates per
camera and bound -- a point ON the bound in the camera frame, carried back to the lidar frame in f64 -- of which the 200 nearest
on either side stay.  A candidate is a pure function of its index (a Weyl sequence per coordinate), so the fixture stores the
chosen indices and the rig's matrices, and k0n_scene() rebuilds the very points from them without a matrix product or inverse."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTH = 1e-3                                     # project_pts3d's depth_thres
N_CAND = 1 << 20
N_SIDE = 200
N_OVERLAP = 220
BOUNDS = ('u_lo', 'u_hi', 'v_lo', 'v_hi', 'cz')
RIGS = ('nusc', 'mixed', 'axis')
K0N_TRIP = 2048 * 256                            # points one trip of k0n_project's grid-stride loop covers
NCHW_TRIP = 4096 * 256                           # pixels one trip of image_to_nchw_f32's loop covers
K1N_TILE = 512
K1N_MAX_BATCH_TILES = 16384


def same_bits(a, b):
    """Equal shape, type and bit patterns (-0.0 is not 0.0; a NaN equals only itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(u), b.view(u))


def same_bits_or_nan(a, b):
    """same_bits, but a NaN equals any NaN: the sign (and payload) of a NaN the arithmetic itself produced (0 x inf, 0 / 0,
    inf - inf) is not held -- gfx950 clears the sign, x86 sets it, and such rows never reach the store."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and same_bits(np.where(na, 0, a), np.where(nb, 0, b))


def rigid(rx, ry, rz, tx, ty, tz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    T = np.eye(4)
    T[:3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                 @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T[:3, 3] = [tx, ty, tz]
    return T


def homo(T, pts):
    """T @ [p; 1] for (n,3) points, as numpy's matmul takes it."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all='ignore'):
        return (T @ np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1).T)[:3, :].T


# ---- K0n: rigs ----------------------------------------------------------------------------------
def intrinsics(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def rig(name):
    """dict: ego_from_lidar, glob_from_ego (4,4), glob_from_cam (ncam,4,4), cam_from_glob (their inverses, as the reference
    takes them: np.linalg.inv), K (ncam,3,3), wh (ncam,2)."""
    if name == 'nusc':                           # the six cameras, K and 1600 x 900 of the utils fixture: global coordinates near 1000 m
        g = np.load(os.path.join(HERE, 'golden', 'utils.npz'))
        r = dict(ego_from_lidar=g['c6_ego_from_lidar'], glob_from_ego=g['c6_glob_from_ego'], glob_from_cam=g['c6_glob_from_cam'],
                 K=np.tile(g['pp_K'], (6, 1, 1)), wh=np.tile(g['pp_wh'], (6, 1)))
    elif name == 'mixed':
        # camera 0 (800 x 900, f = 200) contains camera 1 (a 360 x 640 portrait, f = 300); camera 2 (640 x 480, f = 400) is
        # turned by 0.766 rad, so that a third of its frame lies over camera 1 (and over camera 0)
        gfe = rigid(0.004, -0.007, 2.1, 1203.4, -987.6, 1.3)
        efc = [rigid(-1.57, 0.0, -1.57, 1.5, 0.0, 1.5), rigid(-1.57, 0.0, -1.52, 1.6, 0.1, 1.4), rigid(-1.57, 0.0, -1.57 - 0.766, 1.4, -0.2, 1.6)]
        r = dict(ego_from_lidar=rigid(0.002, -0.004, 0.01, 0.9, 0.02, 1.8), glob_from_ego=gfe,
                 glob_from_cam=np.stack([rigid(0.004, -0.007, 2.1 + 0.002 * j, 1203.4 + 0.03 * j, -987.6, 1.3) @ e for j, e in enumerate(efc)]),
                 K=np.stack([intrinsics(200.0, 401.3, 447.9), intrinsics(300.0, 178.6, 322.2), intrinsics(400.0, 321.7, 238.4)]),
                 wh=np.array([[800.0, 900.0], [360.0, 640.0], [640.0, 480.0]]))
    elif name == 'axis':                         # every bound can be hit exactly
        r = dict(ego_from_lidar=np.eye(4), glob_from_ego=np.eye(4), glob_from_cam=np.eye(4)[None].copy(),
                 K=intrinsics(256.0, 128.0, 64.0)[None].copy(), wh=np.array([[256.0, 128.0]]))
    elif name == 'eight':                        # the limit of pca_nusc_project_cams: the six of 'nusc' and two more over cameras 0 and 3
        b = rig('nusc')
        r = dict(ego_from_lidar=b['ego_from_lidar'], glob_from_ego=b['glob_from_ego'],
                 glob_from_cam=np.concatenate([b['glob_from_cam'], b['glob_from_cam'][[0, 3]] @ rigid(0.01, 0.2, 0.02, 0.1, 0.0, 0.0)]),
                 K=np.concatenate([b['K'], np.stack([intrinsics(500.0, 399.2, 301.1), intrinsics(350.0, 240.4, 319.7)])]),
                 wh=np.concatenate([b['wh'], [[800.0, 600.0], [480.0, 640.0]]]))
    else:
        raise KeyError(name)
    r['cam_from_glob'] = np.stack([np.linalg.inv(T) for T in r['glob_from_cam']])
    r['lidar_from_cam'] = np.stack([np.linalg.inv(r['ego_from_lidar']) @ np.linalg.inv(r['glob_from_ego']) @ T for T in r['glob_from_cam']])
    r['name'] = name
    return r


RIG_KEYS = ('ego_from_lidar', 'glob_from_ego', 'glob_from_cam', 'cam_from_glob', 'lidar_from_cam', 'K', 'wh')


def sel_from(fx, name):
    """What the fixture keeps of a K0n scene: the rig's matrices as the recorded run had them (rig() goes through cos, sin,
    inverses and 4x4 products, whose last bit another numpy build need not share) and the candidate indices the searches chose."""
    return {k: fx['k0n_%s_%s' % (name, k)] for k in ('fam_idx', 'ovl_idx') + RIG_KEYS}


def rig_of(name, sel):
    return dict({k: sel[k] for k in RIG_KEYS}, name=name)


def sub_rig(r, ncam):
    """The first ncam cameras of a rig."""
    out = dict(r)
    for k in ('glob_from_cam', 'cam_from_glob', 'K', 'wh'):
        out[k] = r[k][:ncam]
    return out


# ---- K0n: model ---------------------------------------------------------------------------------
def project_one(pc_glob, cam_from_glob, K, ge_cz=False):
    """One camera's part of the chain for points in the global frame: (uv (n,2) with -10 where the depth test fails, cz (n,))."""
    pcam = homo(cam_from_glob, pc_glob)
    cz = pcam[:, 2]
    with np.errstate(all='ignore'):
        valid = cz >= DEPTH if ge_cz else cz > DEPTH
        viewpad = np.eye(4)
        viewpad[:3, :3] = K
        q = viewpad @ np.concatenate([pcam[valid].T, np.ones((1, int(valid.sum())))])
        q = q[:3, :] / q[2:3, :]
    uv = np.full((pc_glob.shape[0], 2), -10.0)
    uv[valid] = q[:2, :].T
    return uv, cz


def k0n_model(pc, ego_from_lidar, glob_from_ego, glob_from_cam, K, wh, variant=None, cam_from_glob=None):
    """(pc_in_ego (n,3), uv (n,2), cam_idx (n,) int64).  variant names one wrong reading of the rule (the CPU suite shows that
    the scenes tell each of them from the right one): 'ge_' + a bound, 'first_wins', 'wh0', 'w_not_w1'.  cam_from_glob: the
    inverses of glob_from_cam where the caller holds them already (else np.linalg.inv, as the reference takes them)."""
    pc = np.asarray(pc, dtype=np.float64).reshape(-1, 3)
    ego = homo(ego_from_lidar, pc)
    glob = homo(glob_from_ego, ego)
    n, ncam = pc.shape[0], len(glob_from_cam)
    uv, cam = np.zeros((n, 2)), -np.ones(n, dtype=np.int64)
    for j in (range(ncam - 1, -1, -1) if variant == 'first_wins' else range(ncam)):
        uvj, cz = project_one(glob, np.linalg.inv(glob_from_cam[j]) if cam_from_glob is None else cam_from_glob[j], K[j], ge_cz=variant == 'ge_cz')
        w, h = wh[0] if variant == 'wh0' else wh[j]
        u, v = uvj[:, 0], uvj[:, 1]
        hi_u, hi_v = (w, h) if variant == 'w_not_w1' else (w - 1, h - 1)
        with np.errstate(all='ignore'):
            m = (u >= 1 if variant == 'ge_u_lo' else u > 1) & (u <= hi_u if variant == 'ge_u_hi' else u < hi_u) \
                & (v >= 1 if variant == 'ge_v_lo' else v > 1) & (v <= hi_v if variant == 'ge_v_hi' else v < hi_v) \
                & (cz >= DEPTH if variant == 'ge_cz' else cz > DEPTH)
        uv[m] = uvj[m]
        cam[m] = j
    return ego, uv, cam


def k0n_model_rig(pc, r, variant=None):
    return k0n_model(pc, r['ego_from_lidar'], r['glob_from_ego'], r['glob_from_cam'], r['K'], r['wh'], variant, r['cam_from_glob'])


# ---- K0n: candidates, search, scenes -------------------------------------------------------------
WEYL = (0.8191725133961645, 0.6710436067037893, 0.5497004779019703, 0.41421356237309515)     # 1/g, 1/g^2, 1/g^3 (g^4 = g + 1); sqrt(2) - 1
JITTER_PX, JITTER_M = 1e-8, 1e-10                # half-widths of the candidates' offsets from their bound


def hash_name(name):
    return int.from_bytes(name.encode(), 'little') % (1 << 31)


def weyl(idx, k, salt):
    """Coordinate k of candidate idx in [0, 1): frac(idx * a_k + offset(salt)), plain f64 arithmetic."""
    off = ((salt * 2654435761 + k * 40503) % 1000003) / 1000003.0
    return np.modf(np.asarray(idx, dtype=np.float64) * WEYL[k] + off)[0]


def apply_elementwise(M, p):
    """M @ [p; 1] with one numpy operation per product and sum (no BLAS: the same bits wherever it runs)."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([x * M[i, 0] + y * M[i, 1] + z * M[i, 2] + M[i, 3] for i in range(3)], axis=1)


def cam_points(r, j, u, v, z):
    """Camera-frame points of depth z that project to (u, v) in camera j, carried to the lidar frame."""
    K = r['K'][j]
    p = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], axis=1)
    return apply_elementwise(r['lidar_from_cam'][j], p)


def candidates(r, j, bound, idx):
    """Lidar-frame points for candidates idx of camera j's bound: on the bound in the camera frame (u = 1, u = w - 1, v = 1,
    v = h - 1 at a depth of 2 .. 60 m, or cz = 1e-3), elsewhere inside the image.  "On" is up to a seeded offset of at most
    1e-8 px (1e-10 m for cz): the rounding of the carry-back alone moves every point of a camera to the same side of a bound
    (its matrix is off by a few 1e-13 m at global coordinates near 1000 m), and a family needs both sides."""
    salt = hash_name(r['name']) + 97 * j + 7 * BOUNDS.index(bound)
    w, h = r['wh'][j]
    u = 1.5 + (w - 3.0) * weyl(idx, 0, salt)
    v = 1.5 + (h - 3.0) * weyl(idx, 1, salt)
    z = 2.0 + 58.0 * weyl(idx, 2, salt)
    jit = 2.0 * weyl(idx, 3, salt) - 1.0
    if bound == 'cz':
        z = DEPTH + JITTER_M * jit
    else:
        fixed = {'u_lo': 1.0, 'u_hi': w - 1.0, 'v_lo': 1.0, 'v_hi': h - 1.0}[bound] + JITTER_PX * jit
        u, v = (fixed, v) if bound[0] == 'u' else (u, fixed)
    return cam_points(r, j, u, v, z)


def bound_value(r, j, bound):
    w, h = r['wh'][j]
    return {'u_lo': 1.0, 'u_hi': w - 1.0, 'v_lo': 1.0, 'v_hi': h - 1.0, 'cz': DEPTH}[bound]


def bound_side(r, j, bound, uvj, cz):
    """(value the bound is about, True where it is on the kept side) from one camera's uv and cz."""
    val = cz if bound == 'cz' else uvj[:, 0] if bound[0] == 'u' else uvj[:, 1]
    b = bound_value(r, j, bound)
    return val, (val < b if bound.endswith('hi') else val > b)


def search(r, j, bound):
    """Indices of the N_SIDE candidates nearest the bound on the kept side, then the N_SIDE nearest on the other, by the model."""
    idx = np.arange(N_CAND)
    pc = candidates(r, j, bound, idx)
    glob = homo(r['glob_from_ego'], homo(r['ego_from_lidar'], pc))
    uvj, cz = project_one(glob, r['cam_from_glob'][j], r['K'][j])
    val, inside = bound_side(r, j, bound, uvj, cz)
    d = np.abs(val - bound_value(r, j, bound))
    out = []
    for side in (inside, ~inside):
        cand = np.flatnonzero(side)
        out.append(cand[np.argsort(d[cand], kind='stable')[:N_SIDE]])
    assert len(out[0]) == N_SIDE and len(out[1]) == N_SIDE, (r['name'], j, bound, len(out[0]), len(out[1]))
    return np.concatenate(out).astype(np.int32)


def overlap_candidates(r, cams, idx):
    """Points inside the LAST camera of `cams` (anywhere in its image, 2 .. 40 m deep); search_overlap keeps those that lie
    in every camera of `cams` and in no other."""
    j = cams[-1]
    salt = hash_name(r['name']) + 1009 * sum((c + 1) * 8 ** k for k, c in enumerate(cams))
    w, h = r['wh'][j]
    return cam_points(r, j, 2.0 + (w - 4.0) * weyl(idx, 0, salt), 2.0 + (h - 4.0) * weyl(idx, 1, salt), 2.0 + 38.0 * weyl(idx, 2, salt))


def overlap_sets(r):
    """Camera pairs (and on 'mixed' the triple) whose frusta share points."""
    n = len(r['wh'])
    if r['name'] == 'mixed':
        return [(0, 1), (0, 2), (0, 1, 2)]          # (camera 0 contains camera 1: what 1 and 2 share, all three share)
    return [(a, b) for a in range(n) for b in range(a + 1, n) if r['name'] == 'nusc' and (b - a) in (1, 5)]


def search_overlap(r, cams):
    idx = np.arange(1 << 16)
    pc = overlap_candidates(r, cams, idx)
    glob = homo(r['glob_from_ego'], homo(r['ego_from_lidar'], pc))
    ok = np.ones(len(idx), bool)
    for j in cams:
        uvj, cz = project_one(glob, r['cam_from_glob'][j], r['K'][j])
        w, h = r['wh'][j]
        ok &= (uvj[:, 0] > 2) & (uvj[:, 0] < w - 2) & (uvj[:, 1] > 2) & (uvj[:, 1] < h - 2) & (cz > 1)
    for j in set(range(len(r['wh']))) - set(cams):           # ... and in no other camera: the last of `cams` must win
        uvj, cz = project_one(glob, r['cam_from_glob'][j], r['K'][j])
        w, h = r['wh'][j]
        ok &= ~((uvj[:, 0] > 0) & (uvj[:, 0] < w) & (uvj[:, 1] > 0) & (uvj[:, 1] < h) & (cz > 0))
    got = np.flatnonzero(ok)[:N_OVERLAP]
    assert len(got) == N_OVERLAP, (r['name'], cams, len(got))
    return got.astype(np.int32)


def select(name):
    """The searches of a rig (slow: tools/make_golden.py runs them, the fixture keeps the result): dict fam_idx
    (ncam * 5, 2 * N_SIDE), ovl_idx (len(overlap_sets), N_OVERLAP) and the rig's own matrices (RIG_KEYS)."""
    r = rig(name)
    fam = np.stack([search(r, j, b) for j in range(len(r['wh'])) for b in BOUNDS])
    sets = overlap_sets(r)
    ovl = np.stack([search_overlap(r, c) for c in sets]) if sets else np.zeros((0, N_OVERLAP), np.int32)
    return dict({k: r[k] for k in RIG_KEYS}, fam_idx=fam, ovl_idx=ovl)


SPECIALS = (np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e300, -1e300)
AXIS_DEPTHS = (1.0, 2.0, 0.5, 4.0)


def axis_exact_points():
    """On 'axis' (K = [[256, 0, 128], [0, 256, 64], [0, 0, 1]], 256 x 128, identity poses) every product and quotient below is
    exact.  (points, kept): u == 1, u == w - 1, v == 1, v == h - 1 at four depths, the four corners, cz == the double 1e-3
    are refused; the points one lattice step inside each of them and nextafter(1e-3) are kept."""
    pts, kept = [], []
    for z in AXIS_DEPTHS:
        for x, y in ((-127.0, 0.0), (127.0, 0.0), (0.0, -63.0), (0.0, 63.0), (-127.0, -63.0), (127.0, 63.0), (-127.0, 63.0), (127.0, -63.0)):
            pts.append([x / 256.0 * z, y / 256.0 * z, z])                     # on the bound(s): refused
            kept.append(False)
            pts.append([(x - np.sign(x)) / 256.0 * z, (y - np.sign(y)) / 256.0 * z, z])      # u = 2 / 254, v = 2 / 126: kept
            kept.append(True)
    pts += [[0.0, 0.0, DEPTH], [0.0, 0.0, np.nextafter(DEPTH, 1.0)], [0.0, 0.0, np.nextafter(DEPTH, 0.0)]]
    kept += [False, True, False]
    return np.array(pts), np.array(kept)


def k0n_scene(name, sel):
    """dict: pc (n,3) and `sections`, name -> slice.  The families come first (family f = camera f // 5, bound f % 5: N_SIDE
    points on the kept side, nearest first, then N_SIDE on the other), so that family points sit at lanes 0, 63, 64 and 255 of
    the first workgroups; then the overlaps, points behind each camera whose quotient lies inside the image, the specials,
    seeded fillers, on 'axis' the exact hits, and as the frame's last point the nearest kept-side point of the last family
    of u = w - 1."""
    r = rig_of(name, sel)
    ncam = len(r['wh'])
    parts, sections, at = [], {}, 0

    def add(key, pts):
        nonlocal at
        parts.append(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
        sections[key] = slice(at, at + len(parts[-1]))
        at += len(parts[-1])

    for f in range(ncam * len(BOUNDS)):
        add('fam_%d_%s' % (f // 5, BOUNDS[f % 5]), candidates(r, f // 5, BOUNDS[f % 5], sel['fam_idx'][f]))
    for cams, idx in zip(overlap_sets(r), sel['ovl_idx']):
        add('ovl_' + '_'.join(map(str, cams)), overlap_candidates(r, cams, idx))
    k = np.arange(40)
    for j in range(ncam):                        # cz < 0, quotient inside the image: the mirror image of a visible point
        salt = 5 + j
        w, h = r['wh'][j]
        K = r['K'][j]
        u, v, z = 2.0 + (w - 4.0) * weyl(k, 0, salt), 2.0 + (h - 4.0) * weyl(k, 1, salt), -(2.0 + 30.0 * weyl(k, 2, salt))
        add('behind_%d' % j, apply_elementwise(r['lidar_from_cam'][j], np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], 1)))
    base = overlap_candidates(r, (0, ), np.arange(3 * len(SPECIALS)) + 77)
    for c in range(3):
        for i, s in enumerate(SPECIALS):
            base[c * len(SPECIALS) + i, c] = s
    add('specials', base)
    rng = np.random.default_rng(hash_name(name))
    add('fillers', np.stack([rng.uniform(-40, 40, 300), rng.uniform(-40, 40, 300), rng.uniform(-3, 5, 300)], 1))
    if name == 'axis':
        add('exact', axis_exact_points()[0])
    add('last', parts[5 * (ncam - 1) + 1][:1])
    return dict(pc=np.concatenate(parts), sections=sections, rig=r)


def k0n_second_trip_scene(sel):
    """K0N_TRIP + 1 points on 'mixed': the scene (families first), fillers, the families again, and the scene's last point
    (kept side of u = w - 1) as the one point of the second trip."""
    sc = k0n_scene('mixed', sel)
    fam = sc['pc'][:sc['sections']['ovl_0_1'].start]
    rng = np.random.default_rng(11)
    n_fill = K0N_TRIP + 1 - len(sc['pc']) - len(fam) - 1
    fill = np.stack([rng.uniform(-60, 60, n_fill), rng.uniform(-60, 60, n_fill), rng.uniform(-4, 8, n_fill)], 1)
    pc = np.concatenate([sc['pc'], fill, fam, sc['pc'][-1:]])
    assert len(pc) == K0N_TRIP + 1
    return dict(pc=pc, rig=sc['rig'])


# ---- images that encode position -----------------------------------------------------------------
K1N_STACKS = {'s3': (1, 3, 3), 's8': (2, 8, 12), 'nusc': (6, 900, 1600)}


@functools.lru_cache(maxsize=None)
def stack(name, rgb='position'):
    """(imgs (ncam,H,W,3) u8, sems (ncam,H,W) u8): r = x & 255, g = y & 255, b = (37 c + 5 (x >> 8) + 11 (y >> 8)) & 255,
    class = 37 (3 x + 5 y + 7 c) % 200.  A step of one column changes r and the class (by 111), of one row g and the class
    (by 185); another camera changes b.  rgb = 'random': seeded colours under the same classes, for the bilinear mode -- the
    bilinear mix of a colour that is linear in the position rounds to the nearest pixel's."""
    ncam, H, W = K1N_STACKS[name]
    c, y, x = np.meshgrid(np.arange(ncam), np.arange(H), np.arange(W), indexing='ij')
    imgs = np.stack([x & 255, y & 255, (37 * c + 5 * (x >> 8) + 11 * (y >> 8)) & 255], axis=-1).astype(np.uint8)
    if rgb == 'random':
        imgs = np.random.default_rng(hash_name('rgb' + name)).integers(0, 256, imgs.shape, dtype=np.uint8)
    sems = (37 * (3 * x + 5 * y + 7 * c) % 200).astype(np.uint8)
    for a in (imgs, sems):
        a.setflags(write=False)
    return imgs, sems


# ---- K1n: model ---------------------------------------------------------------------------------
def k1n_model(pc7, cam_idx, imgs, sems, T, filters, variant=None):
    """(rows (M,10): x y z intensity r g b class inst 0 in the order of the input, asserts: the reference would raise).
    variant: 'half_up', 'trunc', 'swap_uv', 'bilinear_class' (the class of the upper neighbour), 'keep_ge_ncam'."""
    pc7 = np.asarray(pc7, dtype=np.float64).reshape(-1, 7)
    cam = np.asarray(cam_idx, dtype=np.int64)
    ncam, H, W = sems.shape
    if variant == 'keep_ge_ncam':
        cam = np.where(cam >= ncam, ncam - 1, cam)
    assigned = (cam >= 0) & (cam < ncam)
    u, v = (pc7[:, 5], pc7[:, 4]) if variant == 'swap_uv' else (pc7[:, 4], pc7[:, 5])
    with np.errstate(all='ignore'):
        inside = (u > 1) & (u < W - 1) & (v > 1) & (v < H - 1)
    ok = assigned & inside
    rnd = {'half_up': lambda a: np.floor(a + 0.5), 'trunc': np.trunc}.get(variant, np.round)
    ui, vi = rnd(u[ok]).astype(np.int64), rnd(v[ok]).astype(np.int64)
    feat = -np.ones((pc7.shape[0], 4))
    feat[ok, :3] = imgs[cam[ok], vi, ui]
    feat[ok, 3] = sems[cam[ok], np.ceil(v[ok]).astype(np.int64), np.ceil(u[ok]).astype(np.int64)] if variant == 'bilinear_class' \
        else sems[cam[ok], vi, ui]
    keep = ~(np.any(feat < 0, axis=1) | np.isin(feat[:, 3], np.asarray(filters, dtype=np.float64)))
    rows = np.zeros((int(keep.sum()), 10))
    rows[:, :3] = homo(T, pc7[keep, :3])
    rows[:, 3] = pc7[keep, 3]
    rows[:, 4:8] = feat[keep]
    rows[:, 8] = pc7[keep, 6]
    return rows, bool(np.any(assigned & ~inside))


def soa(rows):
    """The store's seven arrays for (M,10) rows (intensity raw f32, colours and class packed)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 10)
    c = rows[:, 4:8].astype(np.uint32)
    return dict(x=rows[:, 0].copy(), y=rows[:, 1].copy(), z=rows[:, 2].copy(), intensity=rows[:, 3].astype(np.float32),
                rgbs=(c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)).astype(np.uint32),
                inst=rows[:, 8].astype(np.int32), dyn=(rows[:, 9] == 1).astype(np.uint8))


# ---- K1n: scenes --------------------------------------------------------------------------------
K1N_T = rigid(0.01, -0.02, 0.7, 1012.3, -633.1, 2.4)
BIG = 1 << 40


def steps(a, toward, k):
    for _ in range(k):
        a = np.nextafter(a, toward)
    return float(a)


@functools.lru_cache(maxsize=None)
def k1n_scene(name):
    """dict: pc (n,7) x y z intensity u v inst, cam (n,) int64, filters, T, `tags` (what each point is there for) and
    `stored` (indices of the edge points the scene wants stored).  Point 0 is the victim of the offending frames: camera 0,
    the middle of the image."""
    ncam, H, W = K1N_STACKS[name]
    imgs, sems = stack(name)
    rng = np.random.default_rng(hash_name('k1n' + name))
    um, vm = 1.0 + (W - 2.0) * 0.37, 1.0 + (H - 2.0) * 0.31
    uvc, tags = [(um, vm, 0)], ['victim']

    def add(u, v, c, tag):
        uvc.append((u, v, c))
        tags.append(tag)

    for c in range(ncam):                        # nextafter steps inside each bound: pixel column 1 / W - 1, row 1 / H - 1
        for k in (1, 2, 3):
            add(steps(1.0, 2.0, k), vm, c, 'edge_u_lo')
            add(steps(W - 1.0, 0.0, k), vm, c, 'edge_u_hi')
            add(um, steps(1.0, 2.0, k), c, 'edge_v_lo')
            add(um, steps(H - 1.0, 0.0, k), c, 'edge_v_hi')
    for size, axis in ((W, 0), (H, 1)):          # exact ties k + 0.5, odd and even k: lowest, highest, middle
        lo, hi, mid = 1, size - 2, (size - 1) // 2
        for k in sorted({lo, hi, mid, mid + 1, lo + 1, hi - 1} & set(range(lo, hi + 1))):
            add(*((k + 0.5, vm) if axis == 0 else (um, k + 0.5)), (k + axis) % ncam, 'tie')
    add(1.25, 1.25, 0, 'first_pixel')
    for c in range(ncam):
        add(W - 1.25, H - 1.25, c, 'last_pixel')
    for c in (-BIG, -1, 0, ncam - 1, ncam, 7, BIG):
        add(um + 0.11, vm + 0.07, c, 'cam_%d' % c)
    n_rand = 150
    for _ in range(n_rand):
        add(rng.uniform(1.001, W - 1.001), rng.uniform(1.001, H - 1.001), int(rng.integers(-1, ncam)), 'random')
    uvc_a = np.array([(u, v) for u, v, _ in uvc])
    cam = np.array([c for _, _, c in uvc], dtype=np.int64)
    okc = (cam >= 0) & (cam < ncam)
    used = set(sems[cam[okc], np.round(uvc_a[okc, 1]).astype(int), np.round(uvc_a[okc, 0]).astype(int)].tolist())
    # one class per 64-bit word of the mask: where it can be, one that an interior pixel holds and no point above lands on
    filters = []
    for wd in range(4):
        inner = sems[:, 2:H - 2, 2:W - 2][:, :40, :40]
        here = [int(c) for c in np.unique(inner) if wd * 64 <= c < wd * 64 + 64 and int(c) not in used]
        f = here[0] if here else next(c for c in range(wd * 64 + 5, wd * 64 + 64) if c not in used)
        filters.append(f)
        hit = np.argwhere(inner == f)
        for cc, yy, xx in hit[:2]:
            add(xx + 2 + 0.2, yy + 2 - 0.3, int(cc), 'filtered')
    n = len(uvc)
    pc = np.zeros((n, 7))
    pc[:, :3] = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-2, 4, n)], 1)
    pc[:, 3] = rng.integers(0, 256, n)
    pc[:, 4:6] = [(u, v) for u, v, _ in uvc]
    pc[:, 6] = rng.integers(-1, 6, n)
    cam = np.array([c for _, _, c in uvc], dtype=np.int64)
    for a in (pc, cam):
        a.setflags(write=False)
    return dict(pc=pc, cam=cam, filters=filters, T=K1N_T, tags=tags, name=name,
                stored=[i for i, t in enumerate(tags) if t.startswith(('edge', 'tie', 'first', 'last'))])


OFFENDERS = ('u_lo_bound', 'u_lo_step', 'u_hi_bound', 'u_hi_step', 'v_lo_bound', 'v_lo_step', 'v_hi_bound', 'v_hi_step',
             'nan', 'pinf', 'ninf', 'negzero')


def k1n_offender(name, kind, twin=False):
    """The scene with its victim (point 0, camera 0) moved outside: (pc, cam).  twin: the same with the victim's cam_idx set
    to -1 or to ncam, which the reference drops before it looks at uv."""
    sc = k1n_scene(name)
    ncam, H, W = K1N_STACKS[name]
    pc, cam = sc['pc'].copy(), sc['cam'].copy()
    col = 5 if kind.startswith('v') or kind == 'pinf' else 4
    size = H if col == 5 else W
    pc[0, col] = {'lo_bound': 1.0, 'lo_step': np.nextafter(1.0, 0.0), 'hi_bound': size - 1.0, 'hi_step': np.nextafter(size - 1.0, 1e9),
                  'nan': np.nan, 'pinf': np.inf, 'ninf': -np.inf, 'negzero': -0.0}[kind.split('_', 1)[-1]]
    if twin:
        cam[0] = -1 if OFFENDERS.index(kind) % 2 == 0 else ncam
    return pc, cam


def k1n_random_frame(name, n, seed):
    """n points with legal uv on the stack `name`, cameras -1 .. ncam - 1."""
    ncam, H, W = K1N_STACKS[name]
    rng = np.random.default_rng(seed)
    pc = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-2, 4, n), rng.integers(0, 256, n).astype(float),
                   rng.uniform(1.001, W - 1.001, n), rng.uniform(1.001, H - 1.001, n), rng.integers(-1, 6, n).astype(float)], 1).reshape(n, 7)
    return pc, rng.integers(-1, ncam, n)


# ---- strict bilinear sampler ---------------------------------------------------------------------
def bilinear_model(fmap, uv):
    """pts_feat_from_img(uv, fmap, 'bilinear') for a 2-D map with every coordinate inside: the weights as that branch writes
    them, 0 / 0 at an integer coordinate included."""
    u, v = uv[:, 0], uv[:, 1]
    uf, uc, vf, vc = np.floor(u), np.ceil(u), np.floor(v), np.ceil(v)
    with np.errstate(all='ignore'):
        total = (uc - uf) * (vc - vf)
        w_ff = (uc - u) * (vc - v) / total
        w_cc = (u - uf) * (v - vf) / total
        w_fc = (u - uf) * (vc - v) / total
        w_cf = 1. - (w_ff + w_cc + w_fc)
        uf, uc, vf, vc = uf.astype(int), uc.astype(int), vf.astype(int), vc.astype(int)
        return w_ff * fmap[vf, uf] + w_cc * fmap[vc, uc] + w_cf * fmap[vc, uf] + w_fc * fmap[vf, uc]


BIL_HW = (9, 13)


@functools.lru_cache(maxsize=None)
def bilinear_scene():
    """(map (9,13) f64, uv (n,2)): the four points one step inside a bound (then two, three), integer u, integer v, both,
    halves, and seeded coordinates; every one inside (1, W - 1) x (1, H - 1)."""
    H, W = BIL_HW
    rng = np.random.default_rng(2718)
    fmap = rng.uniform(-5, 260, (H, W))
    uv = []
    for k in (1, 2, 3):
        uv += [(steps(1.0, 2.0, k), 4.3), (steps(W - 1.0, 0.0, k), 4.3), (6.7, steps(1.0, 2.0, k)), (6.7, steps(H - 1.0, 0.0, k)),
               (steps(1.0, 2.0, k), steps(H - 1.0, 0.0, k)), (steps(W - 1.0, 0.0, k), steps(1.0, 2.0, k))]
    uv += [(3.0, 2.5), (11.0, 6.25), (2.0, 7.75), (5.5, 4.0), (1.5, 7.0), (11.5, 2.0), (4.0, 4.0), (2.0, 7.0), (11.0, 2.0),
           (1.5, 1.5), (11.5, 7.5), (6.5, 4.5), (steps(3.0, 0.0, 1), 2.5), (steps(3.0, 9.0, 1), 2.5)]
    uv += list(zip(rng.uniform(1.01, W - 1.01, 257 - len(uv)), rng.uniform(1.01, H - 1.01, 257 - len(uv))))
    uv = np.array(uv, dtype=np.float64)
    assert len(uv) == 257
    for a in (fmap, uv):
        a.setflags(write=False)
    return fmap, uv


# ---- image normaliser ----------------------------------------------------------------------------
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # the semseg wrapper's (utils/onnx_utils.py)


def nchw_model(img, mean, std):
    """(H,W,3) u8 -> (3,H,W) f32: ToTensor + Normalize in f32, one rounding per operation."""
    x = img.astype(np.float32) / np.float32(255)
    m, s = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    return np.ascontiguousarray(((x - m) / s).transpose(2, 0, 1))


def nchw_image(H, W, seed=0):
    """Every byte value in every channel (where the image has 256 pixels or more), shifted per channel, then seeded."""
    n = H * W
    p = np.arange(n, dtype=np.int64)
    img = np.stack([p, p * 7 + 85, 255 - p], axis=-1) & 255
    if n > 256:
        rng = np.random.default_rng(seed + n)
        img[256:] = rng.integers(0, 256, (n - 256, 3))
    return img.astype(np.uint8).reshape(H, W, 3)
