"""CPU: the bindings of pca_bev_instance_boxes exist, the numpy model of tests/instance_boxes_common.py -- which the GPU tests of
tests/test_gpu_instance_boxes.py hold the kernels to -- agrees with a brute-force loop, and the scenes of the GPU test hold the
situations they are meant to hold: a rectangle whose own direction and extents come back, an L on which the two criteria
choose different directions (a test that cannot see the difference proves nothing), a tie of areas and a tie of near counts.
pca_amd.host_logic.fit_angles and oriented_boxes."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import instance_boxes_common as bc
from conftest import ROOT


def test_bindings_and_signatures():
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    for name, n_args in (('pca_bev_instance_boxes_workspace_bytes', 3), ('pca_bev_instance_boxes', 24)):
        assert name in _lib.EXPORTS and isinstance(getattr(lib, name), C._CFuncPtr) and len(getattr(lib, name).argtypes) == n_args
    assert _lib.KERNEL_IDS_BOX == ('bev_box_table', 'bev_box_count', 'bev_box_offsets', 'bev_box_scatter', 'bev_box_extents',
                                   'bev_box_near', 'bev_box_choose')
    assert _lib.BOX_CRITERIA == {'area': 0, 'edge': 1}
    # the fifth enum block begins where the fourth ends, and the profiler's tables reach its end
    text = open(os.path.join(ROOT, 'include', 'pca.h')).read()
    fifth = text[text.index('PCA_K_BEV_BOX_TABLE = PCA_K_LAST'):]
    fifth = fifth[:fifth.index('}')].replace('= PCA_K_LAST', '').replace(',', ' ').split()
    assert fifth == ['PCA_K_' + n.upper() for n in _lib.KERNEL_IDS_BOX] + ['PCA_K_ALL']
    common = open(os.path.join(ROOT, 'pc-accumulation-lib_amd', 'csrc', 'pca_common.h')).read()
    assert 'prof_ms[PCA_K_ALL]' in common and 'prof_n[PCA_K_ALL]' in common
    # the workspace at its limits; -1 outside them; no device needed
    ws = lib.pca_bev_instance_boxes_workspace_bytes
    pts, ext = 3 * 8 * ((1 << 31) - 1), 2 * 8 * (65536 * 256 * 2 + 65536)
    assert pts + ext < ws((1 << 31) - 1, 65536, 256) < pts + ext + 4 * 65536 * 256 + (1 << 24)
    assert 0 < ws(1, 1, 1) < 1 << 14 and ws(0, 1, 1) == ws(1, 1, 1)
    assert ws(5000, 4096, 90) > ws(5000, 4096, 89) > ws(5000, 4095, 89) and ws(1 << 20, 8, 8) > ws(1 << 19, 8, 8)
    assert [ws(*a) for a in ((1 << 31, 1, 1), (1, 0, 1), (1, 65537, 1), (1, 1, 0), (1, 1, 257))] == [-1] * 5
    p = inspect.signature(DeviceStore.bev_instance_boxes).parameters
    assert list(p)[1:] == ['prm', 'ids', 'n_rows', 'cos_sin', 'criterion', 'edge_dist', 'extents', 'near', 'first_frame',
                           'last_frame', 'max_points']
    assert p['criterion'].default == 'area' and p['edge_dist'].default == 0.2 and p['extents'].default is False
    p = inspect.signature(SemBEVGenerator.instance_boxes_device).parameters
    assert list(p)[1:] == ['pc', 'ids', 'n_rows', 'rot_mat', 'dx', 'dy', 'aug_view_size', 'n_angles', 'criterion', 'edge_dist',
                           'cos_sin', 'extents', 'near']
    p = inspect.signature(SemanticPointCloudAccumulator.instance_boxes).parameters
    assert list(p)[1:] == ['present_idx', 'part', 'z_range', 'nz', 'classes', 'min_points', 'connectivity', 'min_voxels',
                           'max_instances', 'dyn', 'n_angles', 'criterion', 'edge_dist', 'instances']
    assert (p['n_angles'].default, p['criterion'].default, p['edge_dist'].default, p['instances'].default) == (90, 'area', 0.2, None)
    v = inspect.signature(SemanticPointCloudAccumulator.voxel_instances).parameters      # the arguments it passes on
    assert all(p[k].default == v[k].default for k in list(v)[2:])
    doc = SemanticPointCloudAccumulator.instance_boxes.__doc__
    assert "this project's" in doc and 'no real-data number exists' in doc and 'integrate() never calls' in doc


def test_fit_angles():
    from pca_amd.host_logic import fit_angles
    t = fit_angles(90)
    assert t.shape == (90, 2) and t.dtype == np.float64 and t[0].tolist() == [1., 0.]
    assert np.array_equal(t[:, 0], np.cos(np.arange(90) * (0.5 * np.pi) / 90)) and t[30, 1] == np.sin(30 * (0.5 * np.pi) / 90)
    assert (t > 0).all() or t[0, 1] == 0. and (t[1:] > 0).all()
    assert fit_angles(1).tolist() == [[1., 0.]] and fit_angles(256).shape == (256, 2)
    with pytest.raises(ValueError):
        fit_angles(0)


# ---------------------------------------------------------------------------------------------- the model against a loop
def brute(ids, rows, origin, R, dx, dy, n_rows, cs, criterion, edge_dist):
    """The contract, point by point and direction by direction, in Python floats (which are IEEE f64)."""
    from fractions import Fraction
    fma = lambda a, b, c: float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))      # noqa: E731
    R = np.asarray(R, dtype=np.float64)
    pts = [[] for _ in range(n_rows)]
    for i, (X, Y, Z) in zip(ids, np.asarray(rows)[:, :3].tolist()):
        if 0 <= i < n_rows:
            x, y = X - origin[0], Y - origin[1]
            pts[i].append((fma(R[0, 1], y, float(R[0, 0]) * x) + dx, fma(R[1, 1], y, float(R[1, 0]) * x) + dy, (Z - origin[2]) + 0.0))
    fit, fit_n = np.full((n_rows, 8), np.nan), np.zeros((n_rows, 2), dtype=np.int64)
    fit[:, 7] = -1
    for r, p in enumerate(pts):
        if not p:
            continue
        best = None
        for t, (c, s) in enumerate(np.asarray(cs).tolist()):
            e = [((c * ax + s * ay) + 0.0, (c * ay - s * ax) + 0.0) for ax, ay, _ in p]
            lo1, hi1 = min(a for a, _ in e), max(a for a, _ in e)
            lo2, hi2 = min(b for _, b in e), max(b for _, b in e)
            area = (hi1 - lo1) * (hi2 - lo2)
            near = sum(min(min(a - lo1, hi1 - a), min(b - lo2, hi2 - b)) <= edge_dist for a, b in e)
            key = (-near if criterion == 1 else 0, area, t)
            if best is None or key < best[0]:
                best = (key, [lo1, hi1, lo2, hi2, min(q[2] for q in p), max(q[2] for q in p), area, t], near)
        fit[r], fit_n[r] = best[1], (len(p), best[2])
    return fit, fit_n


@pytest.mark.parametrize('criterion', [0, 1])
def test_model_equals_the_brute_force_loop(criterion):
    from pca_amd.host_logic import fit_angles
    rng = np.random.default_rng(21 + criterion)
    origin, R, dx, dy = bc.frame()
    for n, n_rows, n_angles in ((1, 1, 1), (40, 3, 7), (150, 6, 12)):
        rows = bc.stored(np.concatenate([rng.uniform(-3., 3., (n, 2)), rng.uniform(-1., 1., (n, 1))], axis=1))
        ids = rng.integers(-1, n_rows + 2, n)
        cs = fit_angles(n_angles)
        want = bc.model(ids, rows, origin, R, dx, dy, n_rows, cs, criterion, 0.3)
        fit, fit_n = brute(ids.tolist(), rows, origin, R, dx, dy, n_rows, cs, criterion, 0.3)
        assert bc.same_f64(want['fit'], fit)
        if criterion == 1:
            assert np.array_equal(want['fit_n'], fit_n)
        else:
            assert np.array_equal(want['fit_n'][:, 0], fit_n[:, 0]) and not want['fit_n'][:, 1].any()
        assert want['stats'].tolist() == [((ids >= 0) & (ids < n_rows)).sum(), (ids >= n_rows).sum(), (fit_n[:, 0] > 0).sum(), fit_n[:, 0].max()]


# ---------------------------------------------------------------------------------------------- what the scenes hold
@pytest.mark.parametrize('t_own', [0, 17, 30, 89])
def test_the_rectangle_gives_its_own_direction_and_extents_under_both_criteria(t_own):
    from pca_amd.host_logic import fit_angles, oriented_boxes
    cs = fit_angles(90)
    theta = t_own * (0.5 * np.pi) / 90
    rows, ids, n_rows = bc.rectangle_scene(theta)
    L, W, _ = bc.RECT
    for criterion in (0, 1):
        m = bc.model(ids, rows, *bc.frame(), n_rows, cs, criterion, 0.2, want_near=True)
        lo1, hi1, lo2, hi2, zlo, zhi, area, t = m['fit'][0]
        assert t == t_own and m['fit_n'][0, 0] == 17 * 9
        # (the scene's coordinates went to the store and back: the identity holds to rounding, the bits are the model's)
        assert abs(hi1 - lo1 - L) < 1e-12 and abs(hi2 - lo2 - W) < 1e-12 and abs(area - L * W) < 1e-11 and (zlo, zhi) == (0.5, 1.5)
        boxes, corners = oriented_boxes(m['fit'], cs)
        assert np.allclose(boxes[0], [3., -2., 1., L, W, 1., theta], rtol=0, atol=1e-12)
    # the near tie: the outer ring of the grid lies within edge_dist of the sides in the neighbouring directions too, so
    # criterion 1 meets equal counts there and the smaller area decides
    near = m['near'][0]
    ring = 2 * 17 + 2 * 9 - 4
    assert near[t_own] == ring and m['fit_n'][0, 1] == ring
    tied = np.flatnonzero(near == ring)
    assert tied.size >= 2 and (t_own + 1) % 90 in tied and near.max() == ring
    area = (m['extents'][0, :, 1] - m['extents'][0, :, 0]) * (m['extents'][0, :, 3] - m['extents'][0, :, 2])
    assert (area[tied[tied != t_own]] > area[t_own] + 0.1).all()


def test_the_l_separates_the_two_criteria():
    """At the default edge_dist of 0.2 m a wall of 3 m still lies within reach of its side when the box is turned by 3 degrees,
    so the table is one of 18 directions, 5 degrees apart: there the count of near points peaks at the walls' own entry alone."""
    from pca_amd.host_logic import fit_angles, oriented_boxes
    cs = fit_angles(bc.L_ANGLES)
    step = 90. / bc.L_ANGLES
    walls = int(round(np.rad2deg(bc.L_WALLS) / step))
    rows, ids, n_rows = bc.l_scene()
    by_area = bc.model(ids, rows, *bc.frame(), n_rows, cs, 0, 0.2, want_near=True)
    by_edge = bc.model(ids, rows, *bc.frame(), n_rows, cs, 1, 0.2)
    n = rows.shape[0]
    # the walls stand at 30 degrees, table entry 6: criterion 1 finds them, with EVERY point near a side and no other entry tied
    assert walls == 6 and by_edge['t'][0] == walls and by_edge['fit_n'][0].tolist() == [n, n]
    assert (np.delete(by_edge['near'][0], walls) < n - 20).all() and abs(by_edge['fit'][0, 6] - 4.0 * 2.0) < 1e-9
    # criterion 0 boxes the L diagonally, along the line between the far ends of the walls (atan(2 / 4) from the long one):
    # 6.0 m^2 in that very direction, a little more in the table's nearest one, against 8.0 m^2 along the walls
    diag = (np.rad2deg(bc.L_WALLS) + 180. - np.rad2deg(np.arctan2(2., 4.))) % 90.
    assert by_area['t'][0] != walls and abs(by_area['t'][0] * step - diag) <= step and by_area['fit'][0, 6] < 6.5
    # and in that direction few points are near a side
    assert by_area['fit_n'][0, 1] < n // 3
    for m in (by_area, by_edge):
        boxes, corners = oriented_boxes(m['fit'], cs)
        ax, ay, _ = bc.coords(rows, *bc.frame())
        assert bc.inside_corners(np.stack([ax, ay], 1), corners[0]).all()
    # the swap: turned by a quarter, the same table entry has the long wall ACROSS it
    rows90, ids90, _ = bc.l_scene(theta=bc.L_WALLS + 0.5 * np.pi)
    m90 = bc.model(ids90, rows90, *bc.frame(), 1, cs, 1, 0.2)
    lo1, hi1, lo2, hi2 = m90['fit'][0, :4]
    assert m90['t'][0] == walls and hi2 - lo2 > hi1 - lo1
    boxes, corners = oriented_boxes(m90['fit'], cs)
    assert abs(boxes[0, 3] - 4.) < 1e-9 and abs(boxes[0, 4] - 2.) < 1e-9 and abs(boxes[0, 6] - (bc.L_WALLS + 0.5 * np.pi)) < 1e-12
    ax, ay, _ = bc.coords(rows90, *bc.frame())
    assert bc.inside_corners(np.stack([ax, ay], 1), corners[0]).all()


@pytest.mark.parametrize('copies', [1, 2])
def test_a_single_point_ties_every_direction_and_takes_the_first(copies):
    from pca_amd.host_logic import fit_angles, oriented_boxes
    cs = fit_angles(90)
    rows, ids, n_rows = bc.point_scene(copies)
    for criterion in (0, 1):
        m = bc.model(ids, rows, *bc.frame(), n_rows, cs, criterion, 0.2, want_near=True)
        assert m['t'].tolist() == [-1, -1, 0, -1] and (m['fit'][2, [6, 7]] == 0).all() and m['fit_n'][2].tolist() == [copies, copies]
        ext = m['extents'][2]
        assert ((ext[:, 1] - ext[:, 0]) * (ext[:, 3] - ext[:, 2]) == 0).all() and (m['near'][2] == copies).all()     # the tie
        assert np.isnan(m['fit'][[0, 1, 3], :7]).all() and np.isinf(m['extents'][0]).all() and not m['fit_n'][[0, 1, 3]].any()
        assert m['stats'].tolist() == [copies, 0, 1, copies]
        boxes, corners = oriented_boxes(m['fit'], cs)
        assert np.isnan(boxes[[0, 1, 3]]).all() and np.isnan(corners[0]).all()
        assert np.allclose(boxes[2], [1.25, -0.75, 0.5, 0., 0., 0., 0.], rtol=0, atol=1e-12)


def test_oriented_boxes_on_the_random_rows():
    """length >= width, yaw in [0, pi), and the four corners hold every point of their row."""
    from pca_amd.host_logic import fit_angles, oriented_boxes
    cs = fit_angles(45)
    swaps = 0
    for scene in (bc.random_scene(n=1500, n_rows=12), bc.big_row_scene()):
        rows, ids, n_rows = scene
        m = bc.model(ids, rows, *bc.frame(), n_rows, cs, 0, 0.2)
        boxes, corners = oriented_boxes(m['fit'], cs)
        ax, ay, z = bc.coords(rows, *bc.frame())
        used = np.flatnonzero(m['t'] >= 0)
        assert used.size >= 3 and np.isnan(boxes[m['t'] < 0]).all()
        for r in used:
            mine = ids == r
            assert bc.inside_corners(np.stack([ax[mine], ay[mine]], 1), corners[r]).all(), r
            assert boxes[r, 3] >= boxes[r, 4] >= 0 and 0 <= boxes[r, 6] < math.pi
            assert abs(boxes[r, 2] - 0.5 * (z[mine].min() + z[mine].max())) < 1e-12 and abs(boxes[r, 5] - (z[mine].max() - z[mine].min())) < 1e-12
            assert abs(boxes[r, 3] * boxes[r, 4] - m['fit'][r, 6]) < 1e-9
            swapped = m['fit'][r, 3] - m['fit'][r, 2] > m['fit'][r, 1] - m['fit'][r, 0]
            swaps += swapped
            theta = m['t'][r] * (0.5 * np.pi) / 45
            assert abs(boxes[r, 6] - (theta + (0.5 * np.pi if swapped else 0.))) < 1e-12
    assert swaps >= 2                                               # the swap case is covered
    # the big row's blob stands at 20 degrees, table entry 10 of 45, and is found to about its size
    assert m['t'][1] == 10 and abs(boxes[1, 3] - 6.) < 0.05 and abs(boxes[1, 4] - 2.5) < 0.05


def test_the_scenes_of_the_gpu_test():
    rows, ids, n_rows = bc.big_row_scene()
    assert (ids == 1).sum() > 2 * bc.PIECE and rows.shape[0] < 6000 and set(ids.tolist()) == {-1, 0, 1, 3}
    rows, ids, n_rows = bc.singles_scene()
    assert n_rows == 4096 and sorted(ids.tolist()) == list(range(8192))
    rows, ids, n_rows = bc.random_scene()
    assert ids.min() == -1 and ids.max() == n_rows + 2 and np.bincount(ids[ids >= 0]).min() > 100
