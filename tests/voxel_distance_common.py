"""The numpy model of pca_voxel_distance (include/pca.h) and the scenes the tests of tests/test_voxel_distance_model.py and
tests/test_gpu_voxel_distance.py share.  The transform is brute force over (voxel, site) pairs, in chunks: the key D 2^32 + q
in int64 is exact under the call's limit (D <= 2^31 - 2, q < 2^25) and its minimum IS the contract's lexicographic minimum of
(D, q); nothing here knows about axes, passes or envelopes.  max_dist2 needs no second transform: the minimum pair has the
smallest D, so it either survives the bound or no site does.  fill and tsdf are worded as the contract words them.
A plain module: no test, no fixture."""
import numpy as np

MAX_LABELS = 32
SUBSET = (0, 1, 2, 3, 4, 5)                # the site subset of the random scenes; they hold the labels 0 .. 9
MAX_DIST2 = (0, 1, 2, 3, 9)                # at unit weights; times the weight otherwise
SLAB = 7                                   # columns of the empty slab: a voxel in its middle is 4 columns from any site, 16 > 9
# (px, nz) of the GPU test.  (1, 1); px < nz and nz < px; (16, 4); (33, 7): px no multiple of 4, nz odd; (72, 16): the row
# kernel's tiles are 64 columns wide, so 72 = 64 + 8 has a whole tile and a narrow one; (136, 32): 45-column tiles, three of
# them the last one narrow, 32 k in rounds of 32; (200, 8): 6144 // 200 = 30 columns a tile, seven tiles.
SHAPES = [(1, 1), (3, 5), (5, 3), (16, 4), (33, 7), (72, 16), (136, 32), (200, 8)]
PAIR_BUDGET = 5e7                          # (voxel, site) pairs the model may cost for one scene: about a second of numpy


def densities(px, nz):
    """(sparse, dense) fractions of random sites for a shape: dense is 0.3 where the model can afford it (small volumes, where
    nearly every voxel ties) and PAIR_BUDGET / voxels^2 above that; sparse is an eighth of it."""
    n = nz * px * px
    dense = min(0.3, PAIR_BUDGET / (float(n) * n))
    return dense / 8, dense


def site_mask(labels, site_labels=None):
    ok = labels < MAX_LABELS
    if site_labels is not None:
        ok &= np.isin(labels, np.asarray(sorted(site_labels), dtype=np.uint8))
    return ok


def transform(labels, site_labels=None, weights=(1, 1), chunk=None):
    """(D, q) int64 [nz, px, px] of the unbounded transform; -1, -1 without a site in the volume."""
    nz, px, _ = labels.shape
    w_xy, w_z = int(weights[0]), int(weights[1])
    assert w_xy * 2 * (px - 1) ** 2 + w_z * (nz - 1) ** 2 <= 2 ** 31 - 2
    q = np.flatnonzero(site_mask(labels, site_labels)).astype(np.int64)
    n = nz * px * px
    if q.size == 0:
        return np.full(labels.shape, -1, np.int64), np.full(labels.shape, -1, np.int64)
    sk, sr, sc = q // (px * px), (q // px) % px, q % px
    best = np.empty(n, dtype=np.int64)
    chunk = chunk or max(1, int(4e6) // q.size)
    for lo in range(0, n, chunk):
        p = np.arange(lo, min(lo + chunk, n), dtype=np.int64)
        k, r, c = (p // (px * px))[:, None], ((p // px) % px)[:, None], (p % px)[:, None]
        d = w_xy * ((r - sr) ** 2 + (c - sc) ** 2) + w_z * (k - sk) ** 2
        best[lo:lo + p.size] = ((d << 32) + q).min(axis=1)
    return (best >> 32).reshape(labels.shape), (best & 0xffffffff).reshape(labels.shape)


def model(labels, seen=None, sites=None, weights=(1, 1), max_dist2=None, fill_dist2=None, fill_free=False, tsdf=None,
          base=None):
    """The call's outputs as numpy arrays: 'dist2', 'nearest' int32, 'nearest_label' uint8, 'filled' with fill_dist2, 'tsdf'
    with tsdf = (unit, trunc, flip).  base: transform(labels, sites, weights), where the caller keeps it."""
    D, q = transform(labels, sites, weights) if base is None else base
    has = D >= 0
    if max_dist2 is not None and max_dist2 >= 0:
        has = has & (D <= int(max_dist2))
    D, q = np.where(has, D, -1), np.where(has, q, -1)
    nl = np.where(has, labels.reshape(-1)[np.maximum(q, 0)], 255).astype(np.uint8)
    out = {'dist2': D.astype(np.int32), 'nearest': q.astype(np.int32), 'nearest_label': nl}
    empty = labels >= MAX_LABELS
    if fill_dist2 is not None:
        eligible = np.ones(labels.shape, bool) if (fill_free or seen is None) else seen == 0
        out['filled'] = np.where(~empty, labels, np.where(has & (D <= int(fill_dist2)) & eligible, nl, 255)).astype(np.uint8)
    if tsdf is not None:
        unit, trunc, flip = np.float64(tsdf[0]), np.float64(tsdf[1]), bool(tsdf[2])
        m = np.minimum(np.sqrt(np.where(has, D, 0).astype(np.float64)) * unit, trunc) / trunc
        m = np.where(has, m, np.float64(1.0))
        v = np.float64(1.0) - m if flip else m
        sign = np.where((empty & (seen == 0)) if seen is not None else np.zeros(labels.shape, bool), np.float64(-1.0), np.float64(1.0))
        out['tsdf'] = (sign * v).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
PAIR_KINDS = (('col', (0, 0, 1)), ('row', (0, 1, 0)), ('k', (1, 0, 0)), ('diag', (0, 1, 1)))


def planted_pairs(px, nz):
    """[(kind, mid, lower site, upper site)] as (k, row, col) triples: two sites two apart with nothing else within Chebyshev
    distance 2 of the voxel between them, which therefore ties and must go to the lower site, the smaller place.  All four
    kinds where px >= 32 and nz >= 3; a grid of 16 has no room for the diagonal one beside its slab, one below 5 holds one pair."""
    out = []
    if px < 3:
        return out
    km = 1 if nz >= 3 else 0
    for i, (kind, d) in enumerate(PAIR_KINDS):
        row, col = (1, 1) if px < 5 else (2 + 5 * (i % 3), 2 + 6 * (i // 3))
        slab = slab_columns(px)
        if (px < 5 and i > 0) or row + 1 >= px or col + 1 >= px or (kind == 'k' and nz < 3) or (slab and col + 2 >= slab[0]):
            continue
        mid = (km, row, col)
        out.append((kind, mid, tuple(m - e for m, e in zip(mid, d)), tuple(m + e for m, e in zip(mid, d))))
    return out


def corners(px, nz):
    return sorted({(k, r, c) for k in (0, nz - 1) for r in (0, px - 1) for c in (0, px - 1)})


def slab_columns(px):
    """The columns of the planted empty slab (every k, every row), or None where the grid is too small for one."""
    return (px - 3 - SLAB, px - 3) if px >= 16 else None


_scenes = {}


def random_scene(px, nz, density, planted=True):
    """(labels, seen, subset): labels uint8 [nz, px, px] with about `density` of the voxels holding a label 0 .. 9 -- those
    outside `subset` are occupied voxels that are no sites under it -- and 2 % of the rest a byte >= 32 that must count as
    empty; seen uint8, about half ones.  planted: the empty slab (slab_columns), the pairs of planted_pairs with their
    neighbourhoods cleared, a site in every corner and the byte 200 beside the first corner.  Made once, read-only."""
    key = (px, nz, float(density), planted)
    if key not in _scenes:
        rng = np.random.default_rng([px, nz, int(density * 1e9), int(planted)])
        shape = (nz, px, px)
        labels = np.full(shape, 255, dtype=np.uint8)
        occ = rng.random(shape) < density
        labels[occ] = rng.integers(0, 10, size=int(occ.sum()), dtype=np.uint8)
        junk = ~occ & (rng.random(shape) < 0.02)
        labels[junk] = rng.choice(np.array([32, 100, 200, 254], dtype=np.uint8), size=int(junk.sum()))
        seen = (rng.random(shape) < 0.5).astype(np.uint8)
        if planted:
            slab = slab_columns(px)
            if slab:
                labels[:, :, slab[0]:slab[1]] = 255
            for n, (_, mid, lo, hi) in enumerate(planted_pairs(px, nz)):
                box = tuple(slice(max(m - 2, 0), m + 3) for m in mid)
                labels[box] = 255
                labels[lo], labels[hi] = 1 + n % 2, 2 - n % 2
            for c in corners(px, nz):
                labels[c] = 3
            if px >= 2:
                labels[0, 0, 1] = 200
        labels.setflags(write=False)
        seen.setflags(write=False)
        _scenes[key] = (labels, seen, SUBSET)
    return _scenes[key]


_bases = {}


def scene_base(px, nz, density, subset=None, weights=(1, 1)):
    """transform() of random_scene(px, nz, density), kept: every test of a scene shares one brute-force run."""
    key = (px, nz, float(density), None if subset is None else tuple(subset), tuple(weights))
    if key not in _bases:
        labels, _, _ = random_scene(px, nz, density)
        D, q = transform(labels, subset, weights)
        D.setflags(write=False)
        q.setflags(write=False)
        _bases[key] = (D, q)
    return _bases[key]


def long_line_scene():
    """px = 1024, nz = 1: 32 sites, the four corners among them -- the longest line and the largest D."""
    rng = np.random.default_rng(1024)
    labels = np.full((1, 1024, 1024), 255, dtype=np.uint8)
    for r, c in [(0, 0), (0, 1023), (1023, 0), (1023, 1023)] + [tuple(v) for v in rng.integers(0, 1024, size=(28, 2))]:
        labels[0, r, c] = (r + c) % 7
    seen = (rng.random(labels.shape) < 0.5).astype(np.uint8)
    return labels, seen


def tied(labels, site_labels=None, weights=(1, 1), base=None):
    """bool [nz, px, px]: voxels whose smallest D is reached by more than one site (brute force again, counting)."""
    nz, px, _ = labels.shape
    D, _ = transform(labels, site_labels, weights) if base is None else base
    q = np.flatnonzero(site_mask(labels, site_labels)).astype(np.int64)
    sk, sr, sc = q // (px * px), (q // px) % px, q % px
    n = nz * px * px
    out = np.zeros(n, bool)
    chunk = max(1, int(4e6) // max(q.size, 1))
    flat = D.reshape(-1)
    for lo in range(0, n, chunk):
        p = np.arange(lo, min(lo + chunk, n), dtype=np.int64)
        k, r, c = (p // (px * px))[:, None], ((p // px) % px)[:, None], (p % px)[:, None]
        d = int(weights[0]) * ((r - sr) ** 2 + (c - sc) ** 2) + int(weights[1]) * (k - sk) ** 2
        out[lo:lo + p.size] = (d == flat[lo:lo + p.size, None]).sum(axis=1) > 1
    return out.reshape(labels.shape)
