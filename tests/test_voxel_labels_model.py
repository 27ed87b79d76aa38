"""The numpy model of pca_bev_voxel_labels (tests/voxel_labels_common.py) on hand-made rows whose voxel contents are written
out by hand: the yardstick the GPU tests of tests/test_gpu_voxel_labels.py compare with.  No GPU needed."""
import numpy as np

import voxel_labels_common as vc

# a 4 x 4 grid over 8 m, identity rotation, no shift: the cell of (x, y) is column floor(x / 2 + 2), row 3 - floor(y / 2 + 2)
ORIGIN, R, VIEW, PX = (0., 0., 0.), np.eye(3), 8., 4


def row(x, y, z, cls, dyn=0.):
    r = np.zeros(10)
    r[0], r[1], r[2], r[7], r[9] = x, y, z, cls, dyn
    return r


def run(rows, z_lo, z_step, nz, label_of=None, n_labels=8, include_dyn=False, hf=None, origin=ORIGIN):
    label_of = vc.identity_table(n_labels) if label_of is None else label_of
    return vc.model(np.array(rows), origin, R, 0., 0., VIEW, PX, hf, z_lo, z_step, nz, label_of, n_labels, include_dyn)


def expect(out, nz, voxels):
    """voxels: {(k, row, col): (label, counts, top)}; every other voxel is empty."""
    labels = np.full((nz, PX, PX), 255, dtype=np.uint8)
    counts, top = np.zeros((nz, PX, PX), dtype=np.uint32), np.zeros((nz, PX, PX), dtype=np.uint32)
    for at, (lab, n, t) in voxels.items():
        labels[at], counts[at], top[at] = lab, n, t
    assert np.array_equal(out['labels'], labels) and out['labels'].dtype == np.uint8
    assert np.array_equal(out['counts'], counts) and out['counts'].dtype == np.uint32
    assert np.array_equal(out['top'], top) and out['top'].dtype == np.uint32


def test_cells_are_image_rows_and_bins_are_half_open():
    # bins of 0.5 m from -1: [-1, -0.5), [-0.5, 0), [0, 0.5), [0.5, 1)
    rows = [row(1., 1., -1.0, 2),          # the lowest edge belongs to bin 0; cell: column 2, row 3 - 2 = 1
            row(1., 1., -0.5, 2),          # an inner edge belongs to the bin above it
            row(1., 1., -0.5000001, 3),
            row(-3.5, -3.5, 0.999, 1),     # column 0, row 3
            row(-3.5, -3.5, 1.0, 1),       # the top edge: dropped, not clamped into bin 3
            row(-3.5, -3.5, -1.0000001, 1),  # below z_lo: dropped, not clamped into bin 0
            row(3.9, 3.9, 0.25, 0)]        # column 3, row 0
    out = run(rows, -1., 0.5, 4)
    expect(out, 4, {(0, 1, 2): (2, 2, 1), (1, 1, 2): (2, 1, 1), (3, 3, 0): (1, 1, 1), (2, 0, 3): (0, 1, 1)})
    assert out['voxel'].tolist() == [0 * 16 + 6, 1 * 16 + 6, 0 * 16 + 6, 3 * 16 + 12, -1, -1, 2 * 16 + 3]


def test_ties_go_to_the_smallest_label():
    rows = [row(1., 1., 0.1, c) for c in (3, 1, 3, 5, 1)] + [row(-1., 1., 0.1, c) for c in (7, 7, 0)]
    out = run(rows, 0., 1., 1)
    expect(out, 1, {(0, 1, 2): (1, 5, 2), (0, 1, 1): (7, 3, 2)})


def test_label_table_ignores_and_merges_classes():
    table, n_labels = vc.table_of([[4, 9], [2]])                 # classes 4 and 9 share label 0, class 2 is label 1
    rows = [row(1., 1., 0.1, 4), row(1., 1., 0.1, 9), row(1., 1., 0.1, 2), row(1., 1., 0.1, 0), row(1., 1., 0.1, 200),
            row(-1., -1., 0.1, 7)]                               # a voxel that holds ignored classes only stays empty
    out = run(rows, 0., 1., 1, label_of=table, n_labels=n_labels)
    expect(out, 1, {(0, 1, 2): (0, 3, 2)})
    assert out['voxel'].tolist() == [6, 6, 6, -1, -1, -1]


def test_dyn_points_are_dropped_unless_included():
    rows = [row(1., 1., 0.1, 1, dyn=1.), row(1., 1., 0.1, 1, dyn=1.), row(1., 1., 0.1, 2), row(1., 1., 0.1, 3, dyn=2.)]
    expect(run(rows, 0., 1., 1), 1, {(0, 1, 2): (2, 2, 1)})      # (dyn == 1 alone is dynamic)
    expect(run(rows, 0., 1., 1, include_dyn=True), 1, {(0, 1, 2): (1, 4, 2)})


def test_minus_zero_non_finite_z_origin_and_height_filter():
    rows = [row(1., 1., -0.0, 1),          # (Z - oz) + 0.0 turns -0.0 into +0.0: t = +0, bin 0
            row(1., 1., -1e-300, 2),       # a hair below z_lo = 0: floor(t) = -1, dropped
            row(1., 1., np.nan, 3), row(1., 1., np.inf, 3), row(1., 1., -np.inf, 3),
            row(1., 1., 1.75, 4),          # bin 1 ...
            row(1., 1., 1.5, 5)]
    out = run(rows, 0., 1., 2)
    expect(out, 2, {(0, 1, 2): (1, 1, 1), (1, 1, 2): (4, 2, 1)})
    out = run(rows, 0., 1., 2, hf=1.75)                          # ... unless the height filter (strict) takes the point out
    expect(out, 2, {(0, 1, 2): (1, 1, 1), (1, 1, 2): (5, 1, 1)})
    # the height counts from the origin's z
    out = run([row(1., 1., 2.25, 1), row(1., 1., 1.9, 2)], 0., 1., 2, origin=(0., 0., 2.))
    expect(out, 2, {(0, 1, 2): (1, 1, 1)})


def test_inexact_quotients_follow_the_f64_division():
    # z_lo = -2, z_step = 0.2: neither the edges -2 + 0.2 k nor the quotients are exact; the bin is whatever the f64
    # expression gives, and the two neighbours of an edge land on either side of it or not -- written out with Python floats
    z_lo, z_step, nz = -2.0, 0.2, 32
    edges = z_lo + np.arange(nz + 1) * z_step
    zs = np.concatenate([np.nextafter(edges, -np.inf), edges, np.nextafter(edges, np.inf)])
    out = run([row(1., 1., z, 1) for z in zs], z_lo, z_step, nz)
    want = np.zeros(nz, dtype=np.int64)
    for z in zs.tolist():
        k = int(np.floor((z - z_lo) / z_step)) if (z - z_lo) / z_step >= 0 else -1
        if 0 <= k < nz:
            want[k] += 1
    assert out['counts'][:, 1, 2].tolist() == want.tolist() and want.sum() >= 3 * nz - 2
    assert (out['counts'].sum(axis=(1, 2)) == out['counts'][:, 1, 2]).all()
    # an exactly representable case: 0.125 steps from -1, the point ON every edge opens the bin above
    out = run([row(1., 1., -1. + 0.125 * k, 1) for k in range(9)], -1., 0.125, 8)
    assert out['counts'][:, 1, 2].tolist() == [1] * 8
