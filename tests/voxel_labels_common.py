"""The BEV window voxelised into semantic occupancy labels (pca_bev_voxel_labels): a numpy model of the kernel contract and
the builders of the GPU tests' inputs.

The model restates include/pca.h.  The cell and the keep test of a stored point are those of the elevation partition
(elev_partition_common.view_coord / model, pinned to the reference by tests/test_elev_partition_golden.py): owed
re-transforms aside, a stored point (X, Y, Z, class, dyn) is in view if its view coordinates lie strictly inside +-view / 2,
Z is finite, Z - oz < height_filter (if one is set) and -- include_dyn == 0 -- dyn != 1; its cell is (row px - 1 - j,
column i).  On top of that:
    label = label_of[class]; 255: the point takes no part
    z = (Z - oz) + 0.0,  t = (z - z_lo) / z_step,  k = floor(t)   (f64, numpy's division is the IEEE one)
    kept iff 0 <= k < nz -- nothing is clamped in z
    per voxel (k, row, col) with n_l kept points of label l: counts = sum n_l, top = max n_l, labels = the smallest l with
    n_l == top (np.argmax returns the first maximum), 255 where counts == 0."""
import numpy as np

import elev_partition_common as ec

random_rows = ec.random_rows
heavy_window = ec.heavy_window
rotation = ec.rotation
EMPTY = 255


def identity_table(n_labels):
    """label = class for the classes below n_labels, every other class ignored."""
    t = np.full(256, EMPTY, dtype=np.uint8)
    t[:n_labels] = np.arange(n_labels)
    return t


def table_of(classes):
    """class lists -> (label_of, n_labels): list i becomes label i."""
    t = np.full(256, EMPTY, dtype=np.uint8)
    for label, group in enumerate(classes):
        for c in group:
            assert t[c] == EMPTY
            t[c] = label
    return t, len(classes)


def height_bin(Z, oz, z_lo, z_step):
    """k = floor(((Z - oz) + 0.0 - z_lo) / z_step) as f64 (NaN / +-inf where the input has them)."""
    with np.errstate(all='ignore'):
        z = (np.asarray(Z, dtype=np.float64) - oz) + 0.0
        return np.floor((z - z_lo) / z_step)


def model(rows, origin, R, dx, dy, view, px, hf, z_lo, z_step, nz, label_of, n_labels, include_dyn):
    """rows: (N, 10) stored rows (x, y, z absolute, column 7 = class, column 9 = dyn).  Returns a dict: 'labels' uint8,
    'counts' and 'top' uint32, each (nz, px, px), and 'voxel' int64 (N,): (k * px + row) * px + column, -1 for a point that
    takes no part."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 10)
    label_of = np.asarray(label_of, dtype=np.uint8)
    cell = ec.model(rows, origin, R, dx, dy, view, px, hf, 0.0, include_dyn)['cell']
    k = height_bin(rows[:, 2], origin[2], z_lo, z_step)
    label = label_of[rows[:, 7].astype(np.int64)]
    with np.errstate(all='ignore'):
        keep = (cell >= 0) & (label != EMPTY) & (k >= 0) & (k < nz)
    assert (label[keep] < n_labels).all()
    voxel = np.full(rows.shape[0], -1, dtype=np.int64)
    voxel[keep] = k[keep].astype(np.int64) * (px * px) + cell[keep]
    n = np.zeros((nz * px * px, n_labels), dtype=np.uint32)   # (32 bits, as the contract's counters)
    np.add.at(n, (voxel[keep], label[keep].astype(np.int64)), 1)
    counts, top = n.sum(axis=1), n.max(axis=1)
    labels = np.where(counts > 0, n.argmax(axis=1), EMPTY)
    shape = (nz, px, px)
    return {'labels': labels.astype(np.uint8).reshape(shape), 'counts': counts.astype(np.uint32).reshape(shape),
            'top': top.astype(np.uint32).reshape(shape), 'voxel': voxel}


# ---------------------------------------------------------------------------------------------- inputs of the GPU tests
def edge_rows(rng, n_each, lim, oz, z_lo, z_step, nz, classes):
    """Rows whose height is z_lo + k z_step for k = 0 .. nz and its two f64 neighbours (as stored z: + oz), n_each of
    every height at random places within +-lim, their classes drawn from `classes`: the quotient (z - z_lo) / z_step is
    then within an ulp or two of an integer, mostly inexact."""
    edges = z_lo + np.arange(nz + 1) * z_step
    z = np.concatenate([np.nextafter(edges, -np.inf), edges, np.nextafter(edges, np.inf)])
    z = np.repeat(z, n_each)
    rows = random_rows(rng, z.shape[0], lim, dyn_frac=0.)
    rows[:, 2] = z + oz
    rows[:, 7] = rng.choice(np.asarray(classes), z.shape[0])
    return rows


def pile(cell_xy, z, cls, n, dyn=0.):
    """n rows of class `cls` at one place and height."""
    rows = np.zeros((n, 10))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 7], rows[:, 9] = cell_xy[0], cell_xy[1], z, cls, dyn
    return rows


def compare(out, want):
    """A DeviceStore.bev_voxel_labels result against the model's, everything exact."""
    labels, counts, top = (out[k].cpu().numpy() for k in ('labels', 'counts', 'top'))
    assert sorted(out) == ['counts', 'labels', 'top']
    assert labels.dtype == np.uint8 and counts.dtype == np.int32 and top.dtype == np.int32
    assert labels.shape == counts.shape == top.shape == want['labels'].shape
    assert np.array_equal(counts.view(np.uint32), want['counts'])
    assert np.array_equal(top.view(np.uint32), want['top'])
    assert np.array_equal(labels, want['labels'])
