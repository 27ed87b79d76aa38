"""The numpy model of the instance clustering (tests/voxel_instances_common.py, the contract of pca_bev_voxel_instances in
include/pca.h): hand-written expectations on 4 x 4 x 2 and 5 x 5 x 3 grids, scipy.ndimage.label as an independent
implementation of the components, pca_amd.host_logic.instance_boxes and the tie rule of top_label.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import voxel_instances_common as ic
from voxel_instances_common import BUS, CAR, ROAD, TRUCK

LABELS = ic.DYN_LABELS


def run(voxels, n=1, cls=CAR, dyn=0., **kw):
    """The model on n points of class cls in every voxel of the bool array `voxels`."""
    nz, px, _ = np.asarray(voxels).shape
    return ic.model(ic.rows_for_mask(voxels, n, cls, dyn), *ic.grid_of(px, nz), *LABELS, **kw)


def mask_of(shape, voxels):
    m = np.zeros(shape, dtype=bool)
    for v in voxels:
        m[v] = True
    return m


def test_the_entry_points_and_their_bindings_exist():
    """(missing before this feature)"""
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from pca_amd import host_logic as hl
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    for name in ('pca_bev_instances_workspace_bytes', 'pca_bev_voxel_instances'):
        assert name in _lib.EXPORTS and isinstance(getattr(lib, name), C._CFuncPtr)
    assert len(_lib.KERNEL_IDS_INST) == 8 and _lib.BEV_INST_COLS == ic.COLS
    # the workspace: the voxel pass's, then counts, parent, size and inst
    assert lib.pca_bev_instances_workspace_bytes(1000, 16, 4, 4096) >= lib.pca_bev_voxel_workspace_bytes(1000, 16) + 4 * 16 * 16 * 4 * 4
    p = inspect.signature(DeviceStore.bev_voxel_instances).parameters
    assert list(p)[:7] == ['self', 'prm', 'z_lo', 'z_step', 'nz', 'label_of', 'n_labels']
    for fn in (DeviceStore.bev_voxel_instances, SemBEVGenerator.voxel_instances_device, SemanticPointCloudAccumulator.voxel_instances):
        p = inspect.signature(fn).parameters
        assert (p['min_points'].default, p['connectivity'].default, p['min_voxels'].default, p['max_instances'].default,
                p['dyn'].default) == (1, 26, 1, 4096, 'static')
    assert inspect.signature(SemanticPointCloudAccumulator.voxel_instances).parameters['classes'].default is None
    assert callable(hl.instance_boxes)


# ---------------------------------------------------------------------------------------------- hand-written expectations
def test_diagonal_contacts_are_one_component_at_26_and_separate_at_6():
    # 5 x 5 x 3: (0, 0, 0) - edge - (0, 1, 1) - corner - (1, 2, 2)
    m = ic.diagonals(5, 3)
    assert np.argwhere(m).tolist() == [[0, 0, 0], [0, 1, 1], [1, 2, 2]]
    a, b = run(m, connectivity=26), run(m, connectivity=6)
    assert a['stats'].tolist() == [3, 3, 1, 1, 3, 3] and a['inst'][m].tolist() == [0, 0, 0]
    assert a['table'][0].tolist() == [0, 3, 3, 0, 2, 0, 2, 0, 1] and not a['table'][1:].any()
    assert b['stats'].tolist() == [3, 3, 3, 3, 3, 1] and b['inst'][m].tolist() == [0, 1, 2]
    assert b['table'][:3].tolist() == [[0, 1, 1, 0, 0, 0, 0, 0, 0], [6, 1, 1, 1, 1, 1, 1, 0, 0], [37, 1, 1, 2, 2, 2, 2, 1, 1]]
    assert (a['inst'][~m] == -1).all() and a['ids'].tolist() == [0, 0, 0] and b['ids'].tolist() == [0, 1, 2]


@pytest.mark.parametrize('connectivity', [6, 26])
def test_adjacent_places_across_a_row_or_a_plane_border_are_not_neighbours(connectivity):
    # 4 x 4 x 2: place 7 = (0, 1, 3) and place 8 = (0, 2, 0); place 15 = (0, 3, 3) and place 16 = (1, 0, 0)
    m = mask_of((2, 4, 4), [(0, 1, 3), (0, 2, 0), (0, 3, 3), (1, 0, 0)])
    out = run(m, connectivity=connectivity)
    assert out['table'][:4, 0].tolist() == [7, 8, 15, 16] and out['stats'].tolist() == [4, 4, 4, 4, 4, 1]
    # the two line masks: two components each
    for name in ('column_wrap', 'plane_wrap'):
        lines = ic.MASKS[name](5, 3)
        out = run(lines, connectivity=connectivity)
        assert out['n'] == 2 and out['table'][:2, 1].tolist() == [5, 5], name
    assert run(ic.column_wrap(5, 3), connectivity=connectivity)['table'][:2, 0].tolist() == [0, 4]
    assert run(ic.plane_wrap(5, 3), connectivity=connectivity)['table'][:2, 0].tolist() == [20, 25]


def test_a_bridge_voxel_below_min_points_splits_a_component():
    # 4 x 4 x 2, a bar along row 1 of plane 0 with 3 points per voxel, but min_points - 1 = 2 in its second-to-last voxel
    m = mask_of((2, 4, 4), [(0, 1, c) for c in range(4)])
    n = np.where(m, 3, 0)
    whole = run(m, n, min_points=3)
    assert whole['n'] == 1 and whole['table'][0].tolist() == [4, 4, 12, 0, 3, 1, 1, 0, 0]
    n[0, 1, 2] = 2
    rows = ic.rows_for_mask(m, n)
    split = ic.model(rows, *ic.grid_of(4, 2), *LABELS, min_points=3)
    assert split['stats'].tolist() == [11, 3, 2, 2, 9, 2]
    assert split['table'][:2].tolist() == [[4, 2, 6, 0, 1, 1, 1, 0, 0], [7, 1, 3, 3, 3, 1, 1, 0, 0]]
    assert split['ids'].tolist() == [0] * 6 + [-1] * 2 + [1] * 3      # the bridge's points are kept, and belong to nothing
    assert ic.model(rows, *ic.grid_of(4, 2), *LABELS, min_points=2)['n'] == 1


def test_min_voxels_drops_a_singleton_and_renumbers_the_rest():
    # 5 x 5 x 3: a pair, a singleton between them in place order, a triple
    m = mask_of((3, 5, 5), [(0, 0, 0), (0, 0, 1), (0, 2, 2), (1, 4, 2), (1, 4, 3), (2, 4, 3)])
    a = run(m, connectivity=6)
    assert a['table'][:3, :2].tolist() == [[0, 2], [12, 1], [47, 3]] and a['inst'][m].tolist() == [0, 0, 1, 2, 2, 2]
    b = run(m, connectivity=6, min_voxels=2)
    assert b['stats'].tolist() == [6, 6, 3, 2, 5, 3]
    assert b['table'][:2, :2].tolist() == [[0, 2], [47, 3]] and not b['table'][2:].any()
    assert b['inst'][m].tolist() == [0, 0, -1, 1, 1, 1] and b['ids'].tolist() == [0, 0, -1, 1, 1, 1]
    assert b['table'][1].tolist() == [47, 3, 3, 2, 3, 4, 4, 1, 2]
    c = run(m, connectivity=6, min_voxels=4)
    assert c['stats'].tolist() == [6, 6, 3, 0, 0, 0] and (c['inst'] == -1).all() and not c['table'].any()
    # max_instances caps the tables, not inst, ids or the counts of stats
    d = run(m, connectivity=6, max_instances=2)
    assert d['table'].shape == (2, 9) and d['table'][:, 0].tolist() == [0, 12] and d['ids'].tolist() == [0, 0, 1, 2, 2, 2]
    assert d['stats'].tolist() == a['stats'].tolist() and d['label_counts'][:, 0].tolist() == [2, 1]


def test_dyn_modes_on_a_scene_with_a_marked_mover():
    # 5 x 5 x 3: a parked pair (dyn 0), a mover pair (dyn 1) touching it, a road voxel (no label) and a truck voxel
    m = mask_of((3, 5, 5), [(0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 1, 3), (1, 3, 3), (2, 0, 4)])
    dyn = np.zeros(m.shape)
    dyn[0, 1, 2] = dyn[0, 1, 3] = 1
    cls = np.full(m.shape, CAR)
    cls[1, 3, 3], cls[2, 0, 4] = ROAD, TRUCK
    static, every, movers = (run(m, 2, cls, dyn, dyn_mode=k) for k in (0, 1, 2))
    assert static['stats'].tolist() == [6, 3, 2, 2, 6, 2] and static['table'][:2, 0].tolist() == [5, 54]
    assert static['ids'].tolist() == [0, 0, 0, 0, -1, -1, -1, -1, -1, -1, 1, 1]
    assert static['label_counts'][:2].tolist() == [[4, 0, 0, 0], [0, 2, 0, 0]] and static['top_label'][:3].tolist() == [0, 1, 255]
    assert every['stats'].tolist() == [10, 5, 2, 2, 10, 4] and every['table'][0].tolist() == [5, 4, 8, 0, 3, 1, 1, 0, 0]
    assert movers['stats'].tolist() == [4, 2, 1, 1, 4, 2] and movers['table'][0].tolist() == [7, 2, 4, 2, 3, 1, 1, 0, 0]
    assert movers['ids'].tolist() == [-1] * 4 + [0] * 4 + [-1] * 4


# ---------------------------------------------------------------------------------------------- an independent implementation
def scipy_labels(mask, connectivity):
    ndi = pytest.importorskip('scipy.ndimage')
    lab, n = ndi.label(mask, ndi.generate_binary_structure(3, 1 if connectivity == 6 else 3))
    return lab.astype(np.int64) - 1, n


@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('name', sorted(ic.MASKS))
def test_every_mask_against_scipy(name, connectivity):
    """scipy numbers components in C order of their first voxel: the ascending-root order, so inst == label - 1."""
    for px, nz in ((5, 3), (8, 5), (20, 32), (64, 7)):
        m = ic.MASKS[name](px, nz)
        if m is None:
            continue
        lab, n = scipy_labels(m, connectivity)
        root = ic.components(m, connectivity)
        big = m.size
        assert (root[~m] == big).all() and np.unique(root[m]).shape[0] == n, (name, px, nz)
        # every voxel of scipy's component i carries that component's smallest place
        first = np.full(n, big)
        np.minimum.at(first, lab[m], np.flatnonzero(m.ravel()))
        assert np.array_equal(root[m], first[lab[m]]), (name, px, nz)
    # ... and the whole model on one shape
    m = ic.MASKS[name](8, 5)
    lab, n = scipy_labels(m, connectivity)
    out = run(m, connectivity=connectivity, mask=m)
    assert out['n'] == n and np.array_equal(out['inst'], lab)
    assert out['table'][:n, 1].tolist() == np.bincount(lab[m], minlength=n).tolist()


def test_mask_shapes_are_what_they_claim():
    s = ic.serpentine(64, 7)
    assert [run(s, connectivity=c)['n'] for c in (6, 26)] == [1, 1] and s.sum() == 4 * (32 * 64 + 31) + 3
    assert [run(ic.spiral(20, 3), connectivity=c)['n'] for c in (6, 26)] == [1, 1]
    assert [run(ic.u_shape(8, 5), connectivity=c)['n'] for c in (6, 26)] == [1, 1]
    assert run(ic.checkerboard(8, 4), connectivity=6)['n'] == 128 and run(ic.checkerboard(8, 4), connectivity=26)['n'] == 1
    assert [run(ic.diagonals(8, 5), connectivity=c)['n'] for c in (6, 26)] == [3, 1] and ic.diagonals(8, 5).sum() == 24


@pytest.mark.parametrize('connectivity', [6, 26])
def test_random_masks_against_scipy(connectivity):
    rng = np.random.default_rng(3)
    for density in np.linspace(0.05, 0.6, 20):
        px, nz = int(rng.integers(3, 24)), int(rng.integers(1, 9))
        m = rng.random((nz, px, px)) < density
        lab, n = scipy_labels(m, connectivity)
        out = run(m, connectivity=connectivity, mask=m)
        assert out['n'] == n and np.array_equal(out['inst'], lab), (px, nz, density)
        assert out['stats'].tolist() == [m.sum(), m.sum(), n, n, m.sum(), np.bincount(lab[m]).max() if n else 0]


# ---------------------------------------------------------------------------------------------- small checks
def test_instance_boxes_in_metres():
    from pca_amd import host_logic as hl
    # px 8, view 16 m (cells of 2 m), bins of 0.5 m from z = -1: columns 1..2, rows 0..3 (the TOP rows: the largest y), bins 2..2
    table = np.zeros((4, 9), dtype=np.int32)
    table[0] = [17, 5, 9, 1, 2, 0, 3, 2, 2]
    table[1] = [63, 1, 1, 7, 7, 7, 7, 0, 3]
    boxes = hl.instance_boxes(table, 2, 16., 8, -1., 0.5)
    assert boxes.dtype == np.float64 and boxes.tolist() == [[-6., -2., 0., 8., 0., 0.5], [6., 8., -8., -6., -1., 1.]]
    assert hl.instance_boxes(table, 0, 16., 8, -1., 0.5).shape == (0, 6)
    # a model's table: every kept point of an instance lies inside its box
    m = ic.diagonals(8, 5)
    rows = ic.rows_for_mask(m)
    out = ic.model(rows, *ic.grid_of(8, 5), *LABELS, connectivity=6)
    boxes = hl.instance_boxes(out['table'], out['n'], 8., 8, 0., 1.)
    for i in range(out['n']):
        p = rows[out['ids'] == i, 0:3]
        assert (p[:, 0] > boxes[i, 0]).all() and (p[:, 0] < boxes[i, 1]).all() and (p[:, 1] > boxes[i, 2]).all()
        assert (p[:, 1] < boxes[i, 3]).all() and (p[:, 2] > boxes[i, 4]).all() and (p[:, 2] < boxes[i, 5]).all()
        assert np.array_equal(boxes[i, 1::2] - boxes[i, 0::2], [2., 2., 2.])


def test_top_label_takes_the_smallest_label_of_a_tie():
    # one voxel with two cars and two buses (and one truck): a tie between labels 0 and 2
    m = mask_of((2, 4, 4), [(0, 0, 0)])
    rows = np.concatenate([ic.rows_for_mask(m, 2, BUS), ic.rows_for_mask(m, 1, TRUCK), ic.rows_for_mask(m, 2, CAR)])
    out = ic.model(rows, *ic.grid_of(4, 2), *LABELS)
    assert out['label_counts'][0].tolist() == [2, 1, 2, 0] and out['top_label'][:2].tolist() == [0, 255]
