"""CPU models of the stages of csrc/pca_icp.hip (numpy + scipy's cKDTree; no GPU needed) and the scenes the stage tests
share.  Where a stage's result is discrete -- a cell, a neighbour set, a partner -- the model restates the kernel's own
expression in the kernel's own number format, so that the results compare exactly:

  cells         floor((double(x_f32) - origin) / cell) per axis; inside iff all three indices are in range
  normals       candidates: the targets inside the coarse grid within ICP_NORMAL_RINGS cells of the target's own cell on every
                axis; distances in float32 as (dx*dx + dy*dy) + dz*dz (the library is built with -ffp-contract=off: numpy's
                float32 gives the same bits); kth = the 30th smallest (the point itself counts), or the largest of fewer;
                the set = every candidate with d2 <= kth; covariance in float64, eigenvector of the smallest eigenvalue
  partners      q = T[0]*x + T[1]*y + T[2]*z + T[3] in float64, d2 = dx*dx + dy*dy + dz*dz in float64 over the targets inside the
                coarse grid; the smallest d2 strictly below max_corr_dist^2, lowest original index among equals
  accumulators  the 30 sums of a pass from partners and normals: J = [q x n, n], r = (q - t).n
"""
import math

import numpy as np

NX, NY, NZ = 512, 512, 64
LEVELS = ((0.5, (-128.0, -128.0, -16.0)), (0.25, (-64.0, -64.0, -8.0)))     # (cell, origin) of the coarse and the fine grid
SLAB = NX * NY
K = 30
NORMAL_RINGS = 6
MATCH_REACH = 4.0            # ICP_MATCH_RINGS x 0.5 m: the nearest target is found whatever the threshold if it is closer


def cells(xyz, lv):
    """xyz (N,3) float32 (or float64 queries) -> inside (N,) bool, cell coordinates (N,3) int64 (0 outside), cell index (N,)
    int64 (-1 outside).  NaN and +-inf are outside."""
    cell, o = LEVELS[lv]
    f = np.floor((np.asarray(xyz, dtype=np.float64) - np.array(o)) / cell)
    inside = np.all((f >= 0) & (f < np.array([NX, NY, NZ], dtype=np.float64)), axis=1)
    c = np.where(inside[:, None], f, 0.0).astype(np.int64)
    idx = np.where(inside, (c[:, 2] * NY + c[:, 1]) * NX + c[:, 0], -1)
    return inside, c, idx


def grid_model(tgt, lv):
    """The counting sort of one level: n_in, the slab words (min slab, max slab + 1; (0xffffffff, 0) if the grid is empty) and
    the (cell, original index) pairs in ascending order."""
    inside, c, idx = cells(tgt[:, :3], lv)
    members = np.flatnonzero(inside)
    members = members[np.argsort(idx[members], kind='stable')]
    slab = (int(c[inside, 2].min()), int(c[inside, 2].max()) + 1) if members.size else (0xffffffff, 0)
    return dict(n_in=int(members.size), slab=slab, cell=idx[members], index=members)


def f32_dist2(w, v):
    """(dx*dx + dy*dy) + dz*dz in float32 with dx = w.x - v.x: w (...,3), v broadcastable, both float32."""
    d = np.asarray(w, dtype=np.float32) - np.asarray(v, dtype=np.float32)
    assert d.dtype == np.float32
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbour_sets(tgt, use_tree=True):
    """Per target: the original indices of its neighbour set (None outside the coarse grid), kth (float32, nan outside) and
    whether the set came from the brute-force box (else from a 64-nearest k-d-tree query that provably contains it)."""
    from scipy.spatial import cKDTree
    xyz = np.ascontiguousarray(tgt[:, :3], dtype=np.float32)
    n = len(xyz)
    inside, c_all, _ = cells(xyz, 0)
    ins = np.flatnonzero(inside)
    P, C = xyz[ins], c_all[ins]
    sets, kth, brute = [None] * n, np.full(n, np.nan, np.float32), np.zeros(n, bool)
    done = np.zeros(len(ins), bool)
    if use_tree and len(ins) > 64:
        _, nb = cKDTree(P.astype(np.float64)).query(P.astype(np.float64), k=64)
        d2 = f32_dist2(P[nb], P[:, None, :])
        srt = np.sort(d2, axis=1)
        k30 = srt[:, K - 1]
        member = d2 <= k30[:, None]
        # every point outside the 64 is farther than their farthest: beyond kth by more than any rounding of the distances
        complete = srt[:, 63].astype(np.float64) > k30.astype(np.float64) * (1.0 + 1e-5)
        in_box = np.all(np.abs(C[nb] - C[:, None, :]) <= NORMAL_RINGS, axis=2)
        done = complete & np.all(in_box | ~member, axis=1)
        for m in np.flatnonzero(done):
            sets[ins[m]] = np.sort(ins[nb[m][member[m]]])
            kth[ins[m]] = k30[m]
    for m in np.flatnonzero(~done):
        cand = np.flatnonzero(np.all(np.abs(C - C[m]) <= NORMAL_RINGS, axis=1))
        d2 = f32_dist2(P[cand], P[m])
        kk = np.partition(d2, K - 1)[K - 1] if len(cand) >= K else d2.max()
        sets[ins[m]] = ins[cand[d2 <= kk]]
        kth[ins[m]] = kk
        brute[ins[m]] = True
    return sets, kth, brute


def normal_of(diffs, order=None, dtype=np.float64):
    """Covariance (two-pass, /n) of the float32 differences to the query and its eigen decomposition: (normal, eigenvalues
    ascending).  order / dtype: another summation order or precision, for the error estimate of the bound."""
    P = np.asarray(diffs, dtype=np.float32).astype(dtype)
    if order is not None:
        P = P[order]
    m = P.sum(0) / len(P)
    Q = P - m
    cov = np.zeros((3, 3), dtype)
    for row in Q:                                            # (in the order given: a plain loop, no pairwise summation)
        cov += np.outer(row, row)
    cov = (cov / len(P)).astype(np.float64)
    lam, vec = np.linalg.eigh(cov)
    return vec[:, 0], lam


def normals_model(tgt, use_tree=True, sets=None):
    """valid (N,) bool, normal (N,3) float64 ((0,0,1) where invalid), kth (N,) float32, lam (N,3), brute (N,) bool, sets."""
    xyz = np.ascontiguousarray(tgt[:, :3], dtype=np.float32)
    if sets is None:
        sets, kth, brute = neighbour_sets(tgt, use_tree)
    else:
        sets, kth, brute = sets
    n = len(xyz)
    valid, normal, lam = np.zeros(n, bool), np.tile([0.0, 0.0, 1.0], (n, 1)), np.zeros((n, 3))
    for i in range(n):
        s = sets[i]
        if s is None or len(s) < 3:
            continue
        D = (xyz[s] - xyz[i]).astype(np.float64)
        Q = D - D.mean(0)
        w, v = np.linalg.eigh(Q.T @ Q / len(s))
        valid[i], normal[i], lam[i] = True, v[:, 0], w
    return dict(valid=valid, normal=normal, kth=kth, lam=lam, brute=brute, sets=sets)


def small_gap(lam):
    """The eigen-gap rule: the normal of a (nearly) rotation-symmetric neighbourhood is not defined -- (l1 - l0) < 1e-3 l2."""
    return ~((lam[:, 1] - lam[:, 0]) >= 1e-3 * lam[:, 2]) | ~(lam[:, 1] - lam[:, 0] > 0)


def angle_bound(kth, lam):
    """2^-22 (two float32 roundings of a unit vector) + 2^-44 r_K^2 / (l1 - l0) (the eigenvector's sensitivity to the order
    of the sums) [rad]."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return 2.0 ** -22 + 2.0 ** -44 * kth.astype(np.float64) / (lam[:, 1] - lam[:, 0])


def sine_between(a, b):
    """|a x b| of unit vectors: the angle between two normals, sign-free."""
    return np.linalg.norm(np.cross(a, b), axis=-1)


def transform(T, src):
    """q = T[0]*x + T[1]*y + T[2]*z + T[3] in float64, left to right (N,3)."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z = (src[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([T[i, 0] * x + T[i, 1] * y + T[i, 2] * z + T[i, 3] for i in range(3)], 1)


def f64_dist2(w, q):
    """dx*dx + dy*dy + dz*dz in float64 with dx = w.x - q.x (the kernel's order)."""
    d = np.asarray(w, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def partners_model(q, tgt):
    """Per query: in_grid (q inside the coarse grid), nearest (original index of the nearest target inside the coarse grid,
    lowest index among equal d2; -1 for a non-finite query or no target), d2 (its distance^2, inf if none), ties (targets at
    exactly that distance)."""
    from scipy.spatial import cKDTree
    in_grid = cells(q, 0)[0]
    cand = np.flatnonzero(cells(tgt[:, :3], 0)[0])
    W = tgt[cand, :3].astype(np.float64)
    n = len(q)
    nearest, d2, ties = np.full(n, -1, np.int64), np.full(n, np.inf), np.zeros(n, np.int64)
    fin = np.flatnonzero(np.all(np.isfinite(q), axis=1))
    if len(cand) == 0 or len(fin) == 0:
        return dict(in_grid=in_grid, nearest=nearest, d2=d2, ties=ties)
    tree = cKDTree(W)
    r, _ = tree.query(q[fin])
    balls = tree.query_ball_point(q[fin], r * (1.0 + 1e-9) + 1e-12)
    for i, b in zip(fin, balls):
        b = np.sort(np.asarray(b, dtype=np.int64))           # ascending original index (cand is ascending)
        dd = f64_dist2(W[b], q[i])
        j = int(np.argmin(dd))                               # the first of equals: the lowest index
        nearest[i], d2[i], ties[i] = cand[b[j]], dd[j], int((dd == dd[j]).sum())
    return dict(in_grid=in_grid, nearest=nearest, d2=d2, ties=ties)


PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]      # the 21 products of J^T J, row-wise


def accumulators_model(q, tgt, partner, normal4):
    """The 30 sums of a pass and, per sum, the sum of the absolute terms.  partner (N,) original index or -1; normal4 (n_tgt,4)
    nx, ny, nz, valid.  A pair whose partner has no valid normal counts in [27] (sum d2) and [28] (pairs) only."""
    has = np.flatnonzero(partner >= 0)
    qq, t = q[has], tgt[partner[has], :3].astype(np.float64)
    nn = normal4[partner[has]].astype(np.float64)
    val = (nn[:, 3] != 0).astype(np.float64)
    nx, ny, nz = nn[:, 0], nn[:, 1], nn[:, 2]
    r = (qq[:, 0] - t[:, 0]) * nx + (qq[:, 1] - t[:, 1]) * ny + (qq[:, 2] - t[:, 2]) * nz
    J = np.stack([qq[:, 1] * nz - qq[:, 2] * ny, qq[:, 2] * nx - qq[:, 0] * nz, qq[:, 0] * ny - qq[:, 1] * nx, nx, ny, nz], 1)
    terms = np.zeros((len(has), 30))
    for k, (i, j) in enumerate(PAIRS):
        terms[:, k] = J[:, i] * J[:, j] * val
    for i in range(6):
        terms[:, 21 + i] = J[:, i] * r * val
    terms[:, 27] = f64_dist2(t, qq)
    terms[:, 28] = 1.0
    terms[:, 29] = r * r * val
    sums = np.array([math.fsum(terms[:, k]) for k in range(30)])
    return sums, np.abs(terms).sum(0)


def system_of(sums):
    """J^T J (6,6) and J^T r (6,) from the 30 sums."""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(PAIRS):
        A[i, j] = A[j, i] = sums[k]
    return A, sums[21:27].copy()


def exp_step(x):
    """The update of x = (alpha, beta, gamma, tx, ty, tz): R = Rz(gamma) Ry(beta) Rx(alpha), then the translation."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4)
    U[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                 [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa], [-sb, cb * sa, cb * ca]]
    U[:3, 3] = x[3:]
    return U


# ---- the scenes ----
_CACHE = {}


def _sweeps(name):
    """'sparse': ~9 300 points, 5 % of the 30-neighbourhoods reach past 3 m; 'dense': ~10 700 points, all inside.  (a, b): two
    sweeps 0.9 m apart, cast once, read-only."""
    from test_gpu_icp import sweep
    if name not in _CACHE:
        kw = dict(n_beams=32, n_az=300) if name == 'sparse' else dict(n_beams=48, n_az=256, max_range=14.0)
        pair = []
        for args in ((0.0, 0.0, 0.0, 31), (0.9, 0.03, 0.008, 32)):
            pts = sweep(*args, **kw)
            pts.setflags(write=False)
            pair.append(pts)
        _CACHE[name] = tuple(pair)
    return _CACHE[name]


def rows(xyz):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], 1)


PLANT_Z = 6.0                # the sweeps end below 2.5 m: everything planted from here up is alone in its search boxes


def lattice_patch(centre, seed):
    """A patch of a 0.125 m lattice between two oblique faces i + j + 2k in [0, 2]: a thin sheet whose 30th distance is shared
    by several non-coplanar points (lattice coordinates are exact in float32: the ties are exact)."""
    g = np.arange(-7, 8)
    i, j, k = (a.ravel() for a in np.meshgrid(g, g, np.arange(-8, 9), indexing='ij'))
    keep = (i + j + 2 * k >= 0) & (i + j + 2 * k <= 2)
    pts = np.stack([i, j, k], 1)[keep] * 0.125 + np.asarray(centre)
    return rows(np.random.default_rng(seed).permutation(pts))


def normal_plants():
    """Clusters for the normals: two lattice patches (one inside the fine grid's box, one beyond the fine grid), an isolated
    cluster of 10 (flat: a clear normal), clusters of 2 and of 1 (no normal), a lone point."""
    rng = np.random.default_rng(77)
    ten = rng.normal(size=(10, 3)) * [0.3, 0.2, 0.02] + [30.0, -40.0, PLANT_Z + 1.0]
    two = np.array([[-30.0, 40.0, PLANT_Z], [-30.1, 40.05, PLANT_Z + 0.1]])
    one = np.array([[-50.0, -50.0, PLANT_Z + 2.0]])
    lone = np.array([[100.0, -100.0, 12.0]])
    return np.concatenate([lattice_patch([10.0, -20.0, PLANT_Z + 0.5], 1), lattice_patch([80.0, 30.0, PLANT_Z + 3.0], 2),
                           rows(ten), rows(two), rows(one), rows(lone)])


def normals_scene(name):
    """The second sweep of the pair with the planted clusters mixed in at scattered indices."""
    key = 'normals_' + name
    if key not in _CACHE:
        b = _sweeps(name)[1]
        plants = normal_plants()
        tgt = np.concatenate([b, plants])
        tgt = tgt[np.random.default_rng(5).permutation(len(tgt))]
        tgt.setflags(write=False)
        _CACHE[key] = tgt
    return _CACHE[key]


def grid_plants():
    """Rows 0..: coordinates on cell borders and on the grids' faces, NaN and +-inf rows; rows 60..70 one cell (a run across
    a 64-lane boundary); rows 71..110 two cells in alternation; 300 consecutive copies of one point from row 260 on."""
    f32 = np.float32
    up = lambda v: np.nextafter(f32(v), f32(0))             # noqa: E731  (the float32 next to v, towards 0)
    p = []
    p += [(-128.0, -128.0, -16.0), (128.0, 0.0, 0.0), (up(128), up(128), up(16)), (0.0, 128.0, 0.0), (0.0, 0.0, 16.0),
          (-128.0, 5.0, 1.0), (up(-128), 5.0, 1.0), (5.0, -128.0, -16.0), (5.0, 5.0, up(-16)), (np.nextafter(f32(-128), f32(-200)), 0.0, 0.0),
          (-64.0, -64.0, -8.0), (64.0, 0.0, 0.0), (up(64), up(64), up(8)), (0.0, 64.0, 0.0), (0.0, 0.0, 8.0), (0.0, 0.0, -8.0),
          (up(-64), 1.0, 1.0), (1.0, 1.0, up(-8)), (np.nan, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.nan), (np.inf, 0.0, 0.0),
          (-np.inf, 0.0, 0.0), (0.0, 0.0, np.inf), (0.0, -np.inf, 0.0), (np.nan, np.nan, np.nan),
          (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0)]
    assert len(p) <= 60
    rng = np.random.default_rng(3)
    p += [tuple(v) for v in rng.uniform(-20, 20, (60 - len(p), 3)) * [1, 1, 0.1]]
    p += [tuple(v) for v in rng.uniform(0.0, 0.24, (11, 3)) + [7.0, 7.0, 0.5]]      # rows 60..70: one fine (and coarse) cell
    for k in range(40):                                                            # rows 71..110: A, B, A, B
        p.append(tuple(rng.uniform(0.0, 0.24, 3) + ([9.0, 2.0, 0.5] if k % 2 == 0 else [9.0, 2.5, 0.5])))
    for m in (0.25, 0.5, 0.75, 1.0, -0.25, -0.5, -0.75, 17.25, -33.5):             # exact multiples of the cell sizes
        p += [(m, 3.1, 0.3), (3.1, m, 0.3), (3.1, 3.1, m if abs(m) < 8 else 0.25), (m, m, m if abs(m) < 8 else 0.5),
              (up(m), 3.1, 0.3), (3.1, np.nextafter(f32(m), f32(1e3)), 0.3)]
    assert len(p) <= 260
    p += [tuple(v) for v in rng.uniform(-30, 30, (260 - len(p), 3)) * [1, 1, 0.05]]
    p += [(4.3, -2.2, 0.4)] * 300
    out = rows(np.array(p, dtype=np.float32))
    assert len(out) == 560 and len(np.unique(cells(out[60:71, :3], 1)[2])) == 1 and cells(out[60, :3][None], 1)[2][0] >= 0
    return out


def grid_scene():
    if 'grid' not in _CACHE:
        tgt = np.concatenate([grid_plants(), _sweeps('sparse')[1]])
        tgt.setflags(write=False)
        _CACHE['grid'] = tgt
    return _CACHE['grid']


def two_slab_scene():
    """Two occupied slabs with empty slabs between them, in both grids."""
    rng = np.random.default_rng(9)
    lo = rng.uniform([-30, -30, -5.2], [30, 30, -5.05], (300, 3))
    hi = rng.uniform([-30, -30, 5.05], [30, 30, 5.2], (300, 3))
    return rows(np.concatenate([lo, hi])[rng.permutation(600)])


N_HIGH = 8                   # sources whose query falls outside the grid (above 16 m), at the head of both clouds
N_FAR = 200                  # sources 2.2 .. 4.6 m from any target
DUP_PAIRS = 40
DUP_GROUPS, DUP_COPIES = 6, 24


def partner_scene():
    """(src, tgt, info) of the partner / accumulator tests: the sparse pair with
      - rows 0..N_HIGH-1 of the source above the grid (z 16.3; T keeps them there) and of the target just inside it, same index
        -- what the first pass's warm start looks at;
      - N_FAR sources on rings of 55 m (inside the fine grid) and 70 m radius whose only target within reach lies 2.2-4.6 m away;
      - targets duplicated at far-apart indices: DUP_PAIRS pairs and DUP_GROUPS groups of DUP_COPIES, a source next to each;
      - a NaN and an inf source row."""
    if 'partner' in _CACHE:
        return _CACHE['partner']
    from test_gpu_icp import pose_T
    a, b = _sweeps('sparse')
    rng = np.random.default_rng(11)
    motion = np.float32([0.9, 0.03, 0.0])
    high_s = rows([(5.0 + 3.0 * k, 2.0, 16.3) for k in range(N_HIGH)])
    high_t = rows([(5.0 + 3.0 * k - 0.9, 2.0, 15.7 if k % 2 == 0 else 11.0) for k in range(N_HIGH)])
    ang = rng.uniform(-np.pi, np.pi, N_FAR)
    rad = np.where(np.arange(N_FAR) % 2 == 0, 55.0, 70.0)
    far = rows(np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1.5, 3.0, N_FAR)], 1))
    step = rng.normal(size=(N_FAR, 3))
    step *= (rng.uniform(2.2, 4.6, N_FAR) / np.linalg.norm(step, axis=1))[:, None]
    twin = far.copy()
    twin[:, :3] += step.astype(np.float32) - motion            # (the target frame lies 0.9 m ahead)
    pick = rng.choice(len(b), DUP_PAIRS + DUP_GROUPS, replace=False)
    dup = np.concatenate([b[pick[:DUP_PAIRS]], np.repeat(b[pick[DUP_PAIRS:]], DUP_COPIES - 1, 0)])
    dup = dup[rng.permutation(len(dup))]
    T_true = np.linalg.inv(pose_T(0.9, 0.03, 0.008))
    near = b[pick, :3].astype(np.float64) + rng.normal(0, 0.004, (len(pick), 3))
    near_s = rows((near - T_true[:3, 3]) @ T_true[:3, :3])      # T_true^-1: lands next to the duplicated target
    bad = rows([(np.nan, 1.0, 1.0), (np.inf, 1.0, 1.0)])
    src = np.concatenate([high_s, a, far, near_s, bad]).astype(np.float32)
    tgt = np.concatenate([high_t, b, twin, dup]).astype(np.float32)
    info = dict(high=np.arange(N_HIGH), nan_row=len(src) - 2, inf_row=len(src) - 1)
    src.setflags(write=False)
    tgt.setflags(write=False)
    _CACHE['partner'] = (src, tgt, info)
    return _CACHE['partner']


def step_scene():
    """(src, tgt, init) of the one-step test: the dense pair (every query inside the grid) and an init 8 cm / 0.3 degrees off."""
    from test_gpu_icp import pose_T
    a, b = _sweeps('dense')
    init = np.linalg.inv(pose_T(0.82, 0.06, 0.003))
    init[2, 3] = 0.02
    return a, b, init


def plane_scene():
    """A target of lattice points on one horizontal plane (every normal is (0, 0, 1): J^T J has three zero columns) and a
    source hovering over a part of it; a non-trivial init."""
    from test_gpu_icp import pose_T
    g = np.arange(-40, 41) * 0.125
    x, y = (v.ravel() for v in np.meshgrid(g, g, indexing='ij'))
    tgt = rows(np.stack([x, y, np.full(x.shape, -1.5)], 1))
    rng = np.random.default_rng(21)
    src = rows(rng.uniform([-6.0, -6.0, -1.6], [6.0, 6.0, -1.2], (3000, 3)))      # a part of it lies beyond the plane's edge
    return src, tgt, pose_T(0.3, -0.2, 0.05)
