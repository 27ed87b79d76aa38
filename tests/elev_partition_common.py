"""Partition of a BEV window by height above the cell minimum (pca_bev_elev_partition): a numpy model of the kernel
contract, the names of the fixture's cases (tests/golden/elev_partition.npz, made by tools/make_golden.py from the
reference's static_obj_partitioning_by_elev) and the builders of the GPU tests' inputs.

The model restates include/pca.h: owed re-transforms aside, a stored point (X, Y, Z, dyn) is IN VIEW if
    ax = fma(R01, Y - oy, R00 (X - ox)) + dx,  ay = fma(R11, Y - oy, R10 (X - ox)) + dy   lie strictly inside +-view / 2,
    Z is finite, Z - oz < height_filter (if one is set) and -- include_dyn == 0 -- dyn != 1;
its cell is (row px - 1 - j, column i) with i, j = clamp(floor(a / view * px + px / 2), 0, px - 1); its height is
z = (Z - oz) + 0.0; elev = the minimum z per cell (0.0 where none), flags = 255 not in view, else z > elev + thresh.
numpy has no fma: the model evaluates the product-sum unfused and repeats it exactly (fractions) for the few points whose
grid coordinate or crop test could depend on the last bit."""
from fractions import Fraction

import numpy as np

FATE_STATIC, FATE_DYNAMIC, FATE_NEITHER, FATE_OUT = 0, 1, 2, 3
THRESHOLDS = (0.2, 0.0, -0.1)
# the fixture's cases: (name, variant of the origin, height filter on, static partition only, index into THRESHOLDS)
CASES = [(f'a_hf{h}_dyn{1 - s}_t{k}', 'a', bool(h), bool(s), k) for h in (0, 1) for s in (0, 1) for k in range(3)] + \
        [(f'z0_hf0_dyn1_t{k}', 'z0', False, False, k) for k in (0, 1)]


def grid_name(case):
    """The key of the gridded rows a case hands to the reference's method (shared by the case's thresholds)."""
    return 'grid_' + case.rsplit('_', 1)[0]


def rotation(ang):
    return np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])


def _fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def view_coord(x, y, ra, rb, d, view, px):
    """fma(rb, y, ra x) + d for arrays: unfused, then exactly wherever the cell or the crop test is within reach of the
    difference (unfused and fused differ by at most half an ulp of rb y: far below the 1e-6 margin used here)."""
    with np.errstate(all='ignore'):
        p = ra * x
        a = (rb * y + p) + d
        t = a / view * px + 0.5 * px
        near = (np.abs(t - np.rint(t)) < 1e-6) | (np.abs(np.abs(a) - 0.5 * view) < 1e-6)
    for k in np.flatnonzero(near & np.isfinite(a)):
        a[k] = _fma(rb, y[k], p[k]) + d
    return a


def model(rows, origin, R, dx, dy, view, px, hf, thresh, include_dyn):
    """rows: (N, 10) stored rows (x, y, z absolute, column 9 = dyn) in window order.  Returns a dict: 'elev' f64 (px, px),
    'observed' bool (px, px), 'flags' uint8 (N,), 'counts' int64 [3], 'cell' int64 (N,) (row * px + column, -1 not in view)."""
    rows = np.asarray(rows, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    X, Y, Z, D = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 9]
    x, y = X - origin[0], Y - origin[1]
    ax = view_coord(x, y, R[0, 0], R[0, 1], dx, view, px)
    ay = view_coord(x, y, R[1, 0], R[1, 1], dy, view, px)
    half = 0.5 * view
    with np.errstate(all='ignore'):
        keep = (ax > -half) & (ax < half) & (ay > -half) & (ay < half) & np.isfinite(Z)
        if not include_dyn:
            keep &= D != 1
        if hf is not None:
            keep &= (Z - origin[2]) < hf
        z = (Z - origin[2]) + 0.0
        i = np.clip(np.floor(ax[keep] / view * px + 0.5 * px), 0, px - 1).astype(np.int64)
        j = np.clip(np.floor(ay[keep] / view * px + 0.5 * px), 0, px - 1).astype(np.int64)
    cell = np.full(rows.shape[0], -1, dtype=np.int64)
    cell[keep] = (px - 1 - j) * px + i
    mn = np.full(px * px, np.inf)
    np.minimum.at(mn, cell[keep], z[keep])
    observed = np.zeros(px * px, dtype=bool)
    observed[cell[keep]] = True
    flags = np.full(rows.shape[0], 255, dtype=np.uint8)
    flags[keep] = (z[keep] > (mn[cell[keep]] + thresh)).astype(np.uint8)
    n_in, n_el = int(keep.sum()), int((flags == 1).sum())
    return {'elev': np.where(observed, mn, 0.0).reshape(px, px), 'observed': observed.reshape(px, px), 'flags': flags,
            'counts': np.array([n_in, n_el, n_in - n_el], dtype=np.int64), 'cell': cell}


def fates(flags, col8):
    """Where the reference's bookkeeping puts every row: elevated -> pc_dynamic; else by column 8 (0 static, 1 dynamic,
    anything else neither); a row that is not in view was never handed to the method."""
    col8 = np.asarray(col8)
    f = np.where(col8 == 0, FATE_STATIC, np.where(col8 == 1, FATE_DYNAMIC, FATE_NEITHER))
    f = np.where(flags == 1, FATE_DYNAMIC, f)
    return np.where(flags == 255, FATE_OUT, f).astype(np.int8)


def fixture_case(g, case):
    """(frames, origin, hf, thresh, include_dyn) of one case of the fixture."""
    name, variant, use_hf, static_only, k = next(c for c in CASES if c[0] == case)
    view, px, hf, rot, dx, dy = g['cfg']
    frames = [g[f'frame{f}'] for f in range(3)]
    return frames, g[f'origin_{variant}'], (float(hf) if use_hf else None), THRESHOLDS[k], not static_only


# ---------------------------------------------------------------------------------------------- inputs of the GPU tests
def random_rows(rng, n, lim, dyn_frac=0.15):
    rows = np.zeros((n, 10))
    rows[:, 0:2] = rng.uniform(-lim, lim, (n, 2))
    rows[:, 2] = rng.integers(-2048, 4096, n) / 1024.        # (ties for a cell's minimum and at the threshold do occur)
    rows[:, 3] = rng.integers(0, 256, n)
    rows[:, 4:7] = rng.integers(0, 256, (n, 3))
    rows[:, 7] = rng.integers(0, 19, n)
    rows[:, 8] = rng.integers(-1, 4, n)
    rows[:, 9] = (rng.random(n) < dyn_frac).astype(float)
    return rows


def heavy_window(rng, view, px, dx, dy):
    """35 frames x 8 000 rows, 70 000 rows more in ONE cell and 40 000 more spread over that cell's tile: 390 000 points."""
    frames = [random_rows(rng, 8000, 0.6 * view) for _ in range(35)]
    cell_lo = np.array([(140 - px // 2) * view / px - dx, (90 - px // 2) * view / px - dy])
    pile = random_rows(rng, 70000, 1.)
    pile[:, 0:2] = cell_lo + rng.uniform(0.05, 0.3, (70000, 2))
    tile_lo = np.array([(136 - px // 2) * view / px - dx, (88 - px // 2) * view / px - dy])
    heap = random_rows(rng, 40000, 1.)
    heap[:, 0:2] = tile_lo + rng.uniform(0.01, 8 * view / px - 0.01, (40000, 2))
    frames[25] = np.concatenate([frames[25], pile])
    frames[3] = np.concatenate([heap, frames[3]])
    return frames


def compare(out, want):
    """A DeviceStore.bev_elev_partition result against the model's, everything exact."""
    elev, obs = out['elev'].cpu().numpy(), out['observed'].cpu().numpy()
    flags, counts = out['flags'].cpu().numpy(), out['counts'].cpu().numpy()
    assert obs.dtype == np.bool_ and np.array_equal(obs, want['observed'])
    assert elev.dtype == np.float64 and np.array_equal(elev.view(np.uint64), want['elev'].view(np.uint64))
    assert flags.dtype == np.uint8 and flags.shape == want['flags'].shape and np.array_equal(flags, want['flags'])
    assert counts.dtype == np.int64 and np.array_equal(counts, want['counts'])
