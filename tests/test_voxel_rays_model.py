"""The numpy model of the rays through the voxel grid (tests/voxel_rays_common.py, the contract of pca_bev_voxel_rays in
include/pca.h) on hand-written rays whose marked sets are written out here, and an independent geometric check of the
traversal on random rays (slab method: it shares nothing with the model), so that the model is not pinned to itself alone.
No GPU."""
import ctypes as C
import os

import numpy as np

import voxel_rays_common as rc


def marked(out):
    """The marked voxels as a sorted list of (i, j, k)."""
    k, row, i = np.nonzero(out['seen'])
    px = out['seen'].shape[1]
    return sorted(zip(i.tolist(), (px - 1 - row).tolist(), k.tolist()))


def cast(s, e, px=4, nz=4):
    return rc.traverse(np.array(s, dtype=np.float64).reshape(-1, 3), np.array(e, dtype=np.float64).reshape(-1, 3), px, nz)


def test_the_entry_point_and_its_bindings_exist():
    """(missing before this feature)"""
    import inspect

    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    assert 'pca_bev_voxel_rays' in _lib.EXPORTS and hasattr(lib, 'pca_bev_voxel_rays')
    assert _lib.KERNEL_IDS_RAYS == ('bev_voxel_rays', ) and _lib.KERNEL_IDS_VOXEL == ('bev_voxel_bin', 'bev_voxel_cells')
    assert list(inspect.signature(DeviceStore.bev_voxel_rays).parameters)[:6] == ['self', 'prm', 'z_lo', 'z_step', 'nz', 'origins']
    assert 'origins' in inspect.signature(SemBEVGenerator.voxel_rays_device).parameters
    assert inspect.signature(SemanticPointCloudAccumulator.voxel_occupancy).parameters['origins'].default is None
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pca.h')) as f:
        text = f.read()
    assert '#define PCA_BEV_RAYS_MAX_STEPS 16384' in text and rc.MAX_STEPS == 16384
    assert isinstance(lib.pca_bev_voxel_rays, C._CFuncPtr)


def test_axis_parallel_ray():
    out = cast([0.5, 1.5, 2.5], [3.5, 1.5, 2.5])
    assert marked(out) == [(0, 1, 2), (1, 1, 2), (2, 1, 2)]          # the end voxel (3, 1, 2) is not marked by its own ray
    assert out['stats'].tolist() == [1, 1, 0, 0] and out['N'].tolist() == [3]
    assert out['seen'][2, 4 - 1 - 1].tolist() == [1, 1, 1, 0]         # place [k][px - 1 - j][i]
    # and along w, downwards
    out = cast([1.5, 2.5, 3.25], [1.5, 2.5, 0.75])
    assert marked(out) == [(1, 2, 1), (1, 2, 2), (1, 2, 3)]


def test_exact_diagonal_every_step_a_three_way_tie_in_the_order_u_v_w():
    out = rc.traverse(np.array([[0.5, 0.5, 0.5]]), np.array([[3.5, 3.5, 3.5]]), 4, 4, record=True)
    assert out['visited'][:, 1:].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 1, 1], [2, 2, 1], [2, 2, 2],
                                              [3, 2, 2], [3, 3, 2]]
    assert out['N'].tolist() == [9] and out['ties'] == 6 and not out['seen'][3, 0, 3]
    # the same backwards: the order of the axes stays u, v, w
    out = rc.traverse(np.array([[3.5, 3.5, 3.5]]), np.array([[0.5, 0.5, 0.5]]), 4, 4, record=True)
    assert out['visited'][:, 1:].tolist() == [[3, 3, 3], [2, 3, 3], [2, 2, 3], [2, 2, 2], [1, 2, 2], [1, 1, 2], [1, 1, 1],
                                              [0, 1, 1], [0, 0, 1]]


def test_start_on_an_integer_coordinate_moving_down_steps_at_once():
    """c = floor(2.0) = 2, step -1: tMax = (2 - 2.0) / -1.5 = -0.0, the smallest: voxel 2 is marked, then left at once."""
    out = rc.traverse(np.array([[2.0, 0.5, 0.5]]), np.array([[0.5, 0.75, 0.5]]), 4, 4, record=True)
    assert out['visited'][:, 1:].tolist() == [[2, 0, 0], [1, 0, 0]] and out['N'].tolist() == [2]
    # in v as well, with u moving too: v steps first (tMax 0), then u
    out = rc.traverse(np.array([[0.75, 3.0, 0.5]]), np.array([[1.25, 2.5, 0.5]]), 4, 4, record=True)
    assert out['visited'][:, 1:].tolist() == [[0, 3, 0], [0, 2, 0]]


def test_origin_outside_end_inside_and_both_ends_outside():
    out = cast([-2.5, 1.5, 0.5], [2.5, 1.5, 0.5])
    assert marked(out) == [(0, 1, 0), (1, 1, 0)] and out['N'].tolist() == [5] and out['marks'].tolist() == [2]
    out = cast([-1.5, 0.5, 0.5], [5.5, 0.5, 0.5])
    assert marked(out) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)] and out['N'].tolist() == [7]
    # through a corner region: enters at the top (w = 4), leaves through the side
    out = cast([1.5, 1.25, 5.5], [1.5, 5.25, 1.5])
    assert marked(out) == [(1, 2, 3), (1, 3, 2), (1, 3, 3)]
    # through the grid's edge itself (v = 3 at w = 4, v = 4 at w = 3: exact ties, v steps first): one voxel
    out = cast([1.5, 1.5, 5.5], [1.5, 5.5, 1.5])
    assert marked(out) == [(1, 3, 3)] and out['ties'] == 4
    # outside all the way: nothing
    out = cast([-1.5, -0.5, 0.5], [-0.5, 5.5, 0.5])
    assert marked(out) == [] and out['stats'].tolist() == [1, 1, 0, 0] and out['N'].tolist() == [7]


def test_no_step_marks_nothing():
    out = cast([1.2, 1.2, 1.2], [1.8, 1.7, 1.3])
    assert marked(out) == [] and out['stats'].tolist() == [1, 1, 0, 0] and out['N'].tolist() == [0]


def test_an_end_voxel_is_marked_by_another_rays_passage():
    a_s, a_e = [-2.5, 1.5, 0.5], [2.5, 1.5, 0.5]                      # ends in (2, 1, 0)
    b_s, b_e = [2.5, 0.5, 0.5], [2.5, 3.5, 0.5]                       # passes through it
    assert (2, 1, 0) not in marked(cast(a_s, a_e))
    out = cast([a_s, b_s], [a_e, b_e])
    assert marked(out) == [(0, 1, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0), (2, 2, 0)]
    assert out['stats'].tolist() == [2, 2, 0, 0]


def test_non_finite_and_huge_coordinates_drop_the_ray():
    s = [[0.5, 0.5, 0.5]] * 6 + [[np.nan, 0.5, 0.5], [0.5, 0.5, 0.5]]
    e = [[np.nan, 1.5, 0.5], [1.5, np.inf, 0.5], [1.5, 1.5, -np.inf], [2.0 ** 30, 0.5, 0.5], [0.5, -2.0 ** 30, 0.5],
         [3.5, 0.5, 0.5], [3.5, 0.5, 0.5], [np.nextafter(2.0 ** 30, 0), 0.5, 0.5]]
    out = cast(s, e)
    assert out['stats'].tolist() == [8, 1, 6, 1]                       # the last one is finite and below 2^30: too long
    assert out['N'].tolist() == [-1, -1, -1, -1, -1, 3, -1, -1]
    assert marked(out) == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]


def test_the_step_cap_is_exact():
    out = cast([[0.5, 0.5, 0.5]], [[0.5 + rc.MAX_STEPS, 0.5, 0.5]])
    assert out['stats'].tolist() == [1, 1, 0, 0] and out['N'].tolist() == [rc.MAX_STEPS]
    assert marked(out) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)]
    out = cast([[0.5, 0.5, 0.5]], [[1.5 + rc.MAX_STEPS, 0.5, 0.5]])
    assert out['stats'].tolist() == [1, 0, 0, 1] and out['N'].tolist() == [-1] and marked(out) == []
    # the cap counts all three axes
    out = cast([[0.5, 0.5, 0.5]], [[0.5 + rc.MAX_STEPS - 1, 1.5, 1.5]])
    assert out['stats'].tolist() == [1, 0, 0, 1]


def test_view_transform_frames_dyn_and_the_cut():
    """model(): x to the right, y up (image rows count down), z through z_lo / z_step; a quarter turn; one origin per frame;
    dyn == 1 casts no ray unless asked; the window cut at max_points."""
    def row(x, y, z, dyn=0.):
        r = np.zeros(10)
        r[0], r[1], r[2], r[9] = x, y, z, dyn
        return r
    view, px, nz = 8., 4, 2                                           # cells of 2 m, bins of 1 m from z = 0
    frames = [np.array([row(3., -3., 0.5), row(-1., 3., 1.5, dyn=1.)]), np.zeros((0, 10)), np.array([row(3., 3., 0.5)])]
    origins = np.array([[-3., -3., 0.5], [0., 0., 0.], [3., -3., 1.5]])
    args = (frames, origins, (0., 0., 0.), np.eye(3), 0., 0., view, px, 0., 1., nz)
    out = rc.model(*args, False)
    # frame 0: (0, 0, 0) -> (3, 0, 0) along u; frame 2: from (3, 0, 1) to (3, 3, 0): v at 1 / 6, v and w at 1 / 2 (v first,
    # whether the sum 1 / 6 + 1 / 3 rounds to 1 / 2 or just below it), v at 5 / 6 into the end voxel
    assert marked(out) == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 1), (3, 1, 1), (3, 2, 0), (3, 2, 1)]
    assert out['stats'].tolist() == [2, 2, 0, 0]
    out = rc.model(*args, True)
    assert out['stats'].tolist() == [3, 3, 0, 0] and (1, 3, 1) not in marked(out) and (0, 1, 0) in marked(out)
    assert rc.model(*args, True, max_points=2)['stats'].tolist() == [2, 2, 0, 0]
    # a quarter turn and a shift: ax = -y + 1, ay = x
    R = np.array([[0., -1., 0.], [1., 0., 0.], [0., 0., 1.]])
    g = rc.grid_coords([[1., 2., 0.25]], (0.5, 0.5, 0.25), R, 1., 0., view, px, -1., 0.5)
    assert g.tolist() == [[(-1.5 + 1.) / 8. * 4 + 2., 0.5 / 8. * 4 + 2., 2.0]]
    assert rc.state_of([[0, 3], [0, 1]], [[0, 0], [1, 1]]).tolist() == [[0, 2], [1, 2]]


def test_traversal_against_the_slab_method_on_random_rays():
    """Independent of the model: (1) the closed box of every marked voxel is met by the segment within 1e-9 grid units;
    (2) every voxel of the grid whose interior holds more than 1e-6 grid units of the segment, and which is not the ray's end
    voxel, is marked.  Half of the rays have coordinates on a 1 / 4 lattice (edges, corners, faces: ties)."""
    rng = np.random.default_rng(5)
    px, nz, M = 6, 5, 4000
    s = rng.uniform(-3., 9., (M, 3))
    e = rng.uniform(-3., 9., (M, 3))
    s[M // 2:], e[M // 2:] = np.rint(s[M // 2:] * 4) / 4, np.rint(e[M // 2:] * 4) / 4
    e[::7, 0] = s[::7, 0]                                              # some rays parallel to an axis plane
    out = rc.traverse(s, e, px, nz, record=True)
    vis = out['visited']
    assert vis.shape[0] > 10000 and out['ties'] > 300 and (out['N'] >= 0).all()
    r, vox = vis[:, 0], vis[:, 1:].astype(np.float64)
    _, t_in, t_out = rc.segment_box_length(s[r], e[r], vox - 1e-9, vox + 1.0 + 1e-9)
    assert (t_in <= t_out).all()
    # (2): every ray against every voxel of the grid
    ii, jj, kk = np.meshgrid(np.arange(px), np.arange(px), np.arange(nz), indexing='ij')
    boxes = np.stack([ii.ravel(), jj.ravel(), kk.ravel()], 1)
    V = boxes.shape[0]
    was = np.zeros((M, V), dtype=bool)
    was[r, (vis[:, 1] * px + vis[:, 2]) * nz + vis[:, 3]] = True
    end = np.floor(e).astype(np.int64)
    n_long = 0
    for lo in range(0, M, 500):
        sl = slice(lo, lo + 500)
        m = s[sl].shape[0]
        ss, ee = np.repeat(s[sl], V, axis=0), np.repeat(e[sl], V, axis=0)
        bb = np.tile(boxes, (m, 1)).astype(np.float64)
        length, _, _ = rc.segment_box_length(ss, ee, bb, bb + 1.0, interior=True)
        is_end = (np.tile(boxes, (m, 1)) == np.repeat(end[sl], V, axis=0)).all(axis=1)
        must = (length > 1e-6) & ~is_end
        n_long += int(must.sum())
        assert was[sl].ravel()[must].all()
    assert n_long > 10000
