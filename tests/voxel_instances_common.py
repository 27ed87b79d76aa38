"""The object voxels of the BEV window clustered into instances (pca_bev_voxel_instances): a numpy model of the kernel contract
in include/pca.h, the scene builders and the masks of the tests.  A plain module: no test, no fixture.

The kept points, their voxels and the counts are those of the occupancy labels' model (voxel_labels_common.model, pinned by
tests/test_voxel_labels_model.py).  On top of that:
    dyn_mode 0 / 1: include_dyn of that model; 2: the rows with dyn == 1 only, every one of them taking part
    foreground = counts >= min_points
    components by repeated np.minimum over the 6 or 26 shifted copies of the foreground voxels' labels until nothing changes
    (the shifts are per axis with explicit edges: nothing wraps); between two rounds every voxel also takes the label of the
    voxel its label names (a label is a voxel of the same component, so this only speeds the rounds up)
    root = the smallest place; survive = voxels >= min_voxels; ids 0 .. n - 1 by ascending root
    inst, ids, table (root, voxels, kept points, col_min, col_max, row_min, row_max, k_min, k_max), label_counts, stats."""
import numpy as np

import voxel_labels_common as vl

COLS = 9
CAR, TRUCK, BUS, MOTO, ROAD = 13, 14, 15, 17, 0
DYN_LABELS = vl.table_of([[CAR], [TRUCK], [BUS], [MOTO]])       # (label_of, n_labels) of the four movable classes


def offsets(connectivity):
    assert connectivity in (6, 26)
    all26 = [(dk, dr, dc) for dk in (-1, 0, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dk, dr, dc) != (0, 0, 0)]
    return [d for d in all26 if connectivity == 26 or abs(d[0]) + abs(d[1]) + abs(d[2]) == 1]


def components(fg, connectivity):
    """fg: bool [nz, px, px].  Returns int64 [nz, px, px]: the smallest place of the voxel's component, fg.size for background.
    Works on the list of foreground voxels in place order (a smaller index is a smaller place): per offset, the index of the
    shifted voxel, -1 where the shift leaves the grid or meets background."""
    big = fg.size
    nz, px, _ = fg.shape
    k, r, c = np.nonzero(fg)
    place = (k * px + r) * px + c
    index = np.full(big, -1, dtype=np.int64)
    index[place] = np.arange(place.shape[0])
    pairs = []
    for d in offsets(connectivity):
        kk, rr, cc = k + d[0], r + d[1], c + d[2]
        ok = (kk >= 0) & (kk < nz) & (rr >= 0) & (rr < px) & (cc >= 0) & (cc < px)      # the edges, per axis: nothing wraps
        nb = np.full(place.shape[0], -1, dtype=np.int64)
        nb[ok] = index[(kk[ok] * px + rr[ok]) * px + cc[ok]]
        pairs.append((np.flatnonzero(nb >= 0), nb[nb >= 0]))
    lab = np.arange(place.shape[0])
    while True:
        new = lab.copy()
        for at, nb in pairs:
            new[at] = np.minimum(new[at], lab[nb])
        if np.array_equal(new, lab):
            break
        while True:                                             # a label names a voxel of the same component: take its label
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        lab = new
    root = np.full(fg.shape, big, dtype=np.int64)
    root[fg] = place[lab]
    return root


def model(rows, origin, R, dx, dy, view, px, hf, z_lo, z_step, nz, label_of, n_labels, dyn_mode=0, min_points=1, connectivity=26,
          min_voxels=1, max_instances=4096, max_points=None, mask=None):
    """rows: (N, 10) stored rows or a list of frames of them, in window order.  mask: the foreground the caller expects
    (asserted).  Returns a dict: 'counts' uint32 and 'inst' int32 [nz, px, px]; 'ids' int32 (N,); 'table' int64
    [max_instances, 9]; 'label_counts' int64 [max_instances, n_labels]; 'top_label' uint8 [max_instances]; 'stats' int64 [6];
    'n' = stats[3]."""
    if isinstance(rows, (list, tuple)):
        rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in rows]) if rows else np.zeros((0, 10))
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 10)
    if max_points is not None:
        rows = rows[:max_points]
    assert dyn_mode in (0, 1, 2)
    grid = (origin, R, dx, dy, view, px, hf, z_lo, z_step, nz, label_of, n_labels)
    if dyn_mode == 2:
        sel = rows[:, 9] == 1
        part = vl.model(rows[sel], *grid, True)
        counts = part['counts']
        voxel = np.full(rows.shape[0], -1, dtype=np.int64)
        voxel[sel] = part['voxel']
    else:
        part = vl.model(rows, *grid, bool(dyn_mode))
        counts, voxel = part['counts'], part['voxel']
    kept = voxel >= 0
    label = np.asarray(label_of, dtype=np.uint8)[rows[:, 7].astype(np.int64)].astype(np.int64)
    fg = counts >= min_points
    if mask is not None:
        assert np.array_equal(fg, mask)
    root = components(fg, connectivity)
    roots, sizes = np.unique(root[fg], return_counts=True)      # ascending roots
    survive = sizes >= min_voxels
    n = int(survive.sum())
    rid = np.full(fg.size + 1, -1, dtype=np.int64)
    rid[roots[survive]] = np.arange(n)
    inst = rid[root]
    ids = np.where(kept, inst.ravel()[np.where(kept, voxel, 0)], -1)
    table = np.zeros((max_instances, COLS), dtype=np.int64)
    label_counts = np.zeros((max_instances, n_labels), dtype=np.int64)
    k, r, c = np.nonzero(inst >= 0)
    of = inst[k, r, c]
    for i in range(min(n, max_instances)):
        m = of == i
        table[i] = [roots[survive][i], sizes[survive][i], (ids == i).sum(), c[m].min(), c[m].max(), r[m].min(), r[m].max(),
                    k[m].min(), k[m].max()]
    inside = kept & (ids >= 0) & (ids < max_instances)
    np.add.at(label_counts, (ids[inside], label[inside]), 1)
    top_label = np.where(label_counts.sum(axis=1) > 0, label_counts.argmax(axis=1), 255).astype(np.uint8)
    stats = np.array([kept.sum(), fg.sum(), roots.shape[0], n, (ids >= 0).sum(), sizes[survive].max() if n else 0], dtype=np.int64)
    return {'counts': counts, 'inst': inst.astype(np.int32), 'ids': ids.astype(np.int32), 'table': table,
            'label_counts': label_counts, 'top_label': top_label, 'stats': stats, 'n': n}


def compare(out, want, ids=True):
    """A DeviceStore.bev_voxel_instances result against the model's, everything exact."""
    assert sorted(out) == ['ids', 'inst', 'label_counts', 'stats', 'table', 'top_label']
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got['stats'].dtype == np.int64 and got['stats'].tolist() == want['stats'].tolist(), (got['stats'], want['stats'])
    assert got['inst'].dtype == np.int32 and got['inst'].shape == want['inst'].shape
    assert np.array_equal(got['inst'], want['inst']), int((got['inst'] != want['inst']).sum())
    if ids:
        assert got['ids'].dtype == np.int32 and got['ids'].shape == want['ids'].shape, (got['ids'].shape, want['ids'].shape)
        assert np.array_equal(got['ids'], want['ids']), int((got['ids'] != want['ids']).sum())
    for name in ('table', 'label_counts'):
        assert got[name].dtype == np.int32 and got[name].shape == want[name].shape, name
        bad = got[name].view(np.uint32).astype(np.int64) != want[name]
        assert not bad.any(), (name, np.argwhere(bad)[:5].tolist())
    assert got['top_label'].dtype == np.uint8 and np.array_equal(got['top_label'], want['top_label'])


# ---------------------------------------------------------------------------------------------- scenes from masks
def grid_of(px, nz):
    """The frame in which rows_for_mask's points sit at voxel centres: identity, no shift, cells and bins of 1 m from z = 0
    (every centre is exact in f64 and strictly inside the crop).  The arguments of model() up to nz."""
    return ((0., 0., 0.), np.eye(3), 0., 0., float(px), px, None, 0., 1., nz)


def rows_for_mask(mask, n=1, cls=CAR, dyn=0., rng=None):
    """n points of class cls at the centre of every voxel of the bool [nz, px, px] mask, in the frame of grid_of; n, cls and
    dyn may be [nz, px, px] arrays (per voxel).  In place order, or shuffled by rng."""
    mask = np.asarray(mask, dtype=bool)
    nz, px, _ = mask.shape
    k, r, c = np.nonzero(mask)
    per = np.broadcast_to(np.asarray(n), mask.shape)[k, r, c].astype(np.int64)
    rows = np.zeros((int(per.sum()), 10))
    rep = np.repeat(np.arange(k.shape[0]), per)
    rows[:, 0] = c[rep] + 0.5 - 0.5 * px                         # column i = floor(x + px / 2)
    rows[:, 1] = (px - 1 - r[rep]) + 0.5 - 0.5 * px              # row = px - 1 - j
    rows[:, 2] = k[rep] + 0.5
    rows[:, 7] = np.broadcast_to(np.asarray(cls, dtype=np.float64), mask.shape)[k, r, c][rep]
    rows[:, 9] = np.broadcast_to(np.asarray(dyn, dtype=np.float64), mask.shape)[k, r, c][rep]
    if rng is not None:
        rows = rows[rng.permutation(rows.shape[0])]
    return rows


# ---------------------------------------------------------------------------------------------- the masks
def serpentine(px, nz):
    """Every second plane holds a path that runs along every second row and steps to the next one at alternating ends; a
    single voxel in the plane between joins the end of one plane's path to the start of the next plane's, which runs the
    other way.  One component at both connectivities whose far end is (nearly) all of its voxels away from its root."""
    if px < 3:
        return None
    m = np.zeros((nz, px, px), dtype=bool)
    last = ((px - 1) // 2) * 2                                   # the last path row
    for k in range(0, nz, 2):
        m[k, 0:last + 1:2, :] = True
        for j, r in enumerate(range(1, last, 2)):
            m[k, r, px - 1 if j % 2 == 0 else 0] = True
        # the path of plane k starts at (0, 0) and ends in row `last`; that of plane k + 2 is the same path run backwards
        if k + 2 < nz:
            end_col = px - 1 if (last // 2) % 2 == 0 else 0
            where = (last, end_col) if (k // 2) % 2 == 0 else (0, 0)
            m[k + 1, where[0], where[1]] = True
    return m


def spiral(px, nz, pitch=2):
    """A rectangular spiral arm in plane 0, `pitch` - 1 empty cells between its turns (pitch >= 2: the turns do not touch)."""
    if px < 5:
        return None
    m = np.zeros((nz, px, px), dtype=bool)
    r = c = 0
    m[0, 0, 0] = True
    length, turn = px - 1, 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while length > 0:
        dr, dc = dirs[turn % 4]
        for _ in range(length):
            r, c = r + dr, c + dc
            m[0, r, c] = True
        turn += 1
        if turn >= 3 and turn % 2 == 1:
            length -= pitch
    return m


def u_shape(px, nz):
    """Two arms along columns 0 and 2 that meet only in the last row: the second arm's top is far from the root at (0, 0, 0)."""
    if px < 3:
        return None
    m = np.zeros((nz, px, px), dtype=bool)
    m[0, :, 0] = m[0, :, 2] = True
    m[0, px - 1, 1] = True
    return m


def checkerboard(px, nz):
    k, r, c = np.indices((nz, px, px))
    return (k + r + c) % 2 == 0


def diagonals(px, nz):
    """Three cubes (side 2 where the grid allows, else 1): the second touches the first along an edge only, the third touches
    the second at a corner only.  One component at 26, three at 6."""
    s = 2 if px >= 8 and nz >= 4 else 1
    if px < 3 * s or nz < 2 * s:
        return None
    m = np.zeros((nz, px, px), dtype=bool)
    m[0:s, 0:s, 0:s] = True
    m[0:s, s:2 * s, s:2 * s] = True
    m[s:2 * s, 2 * s:3 * s, 2 * s:3 * s] = True
    return m


def column_wrap(px, nz):
    """The last column and the first column of plane 0: (0, row, px - 1) and (0, row + 1, 0) are adjacent PLACES, not
    neighbours.  Two components at both connectivities."""
    if px < 3:
        return None
    m = np.zeros((nz, px, px), dtype=bool)
    m[0, :, px - 1] = m[0, :, 0] = True
    return m


def plane_wrap(px, nz):
    """The last row of plane 0 and the first row of plane 1: adjacent places across the plane border, not neighbours."""
    if px < 3 or nz < 2:
        return None
    m = np.zeros((nz, px, px), dtype=bool)
    m[0, px - 1, :] = m[1, 0, :] = True
    return m


MASKS = {'serpentine': serpentine, 'spiral': spiral, 'u_shape': u_shape, 'checkerboard': checkerboard, 'diagonals': diagonals,
         'column_wrap': column_wrap, 'plane_wrap': plane_wrap}
