"""GT lane centrelines, CPU side: the host path reproduces what the reference itself returned (tests/golden/lanes.npz, made by
tools/make_golden.py --only lanes), bit for bit -- which pins the model the device path is compared against on the GPU -- and
the device path's names exist."""
import ctypes
import os

import numpy as np
import pytest

import lanes_common as lc
from conftest import PKG


@pytest.fixture(scope='module')
def fx():
    return lc.Fixture()


def test_fixture_holds_the_cases_it_was_built_for(fx):
    g = fx.g
    lens = np.diff(fx.start)
    assert len(fx.lanes_global) <= 400 and fx.n_views >= 12 and {0, 1, 2, 3} <= set(lens.tolist())
    rots = {round(float(r), 6) for r in g['views'][:, 3]}
    assert {0., 0.7, round(0.5 * np.pi, 6), -2.1} <= rots
    assert {0.9, 1., 1.07} <= set(g['views'][:, 6].tolist()) and {7., 64., 256.} <= set(g['views'][:, 7].tolist())
    assert any(g[f'len_{k}'].size == 0 for k in range(fx.n_views))                          # no lane survives
    assert any(g[f'len_{k}'].size == int((lens >= 2).sum()) for k in range(fx.n_views))     # every lane with an edge does
    assert np.isnan(g['xyz_global']).sum() == 1 and np.isinf(g['xyz_global']).sum() == 1
    assert np.signbit(g['nz_xyz'][0, 2]) and g['nz_xyz'][0, 2] == 0


def test_transform_traj_reproduces_the_reference_lists(fx):
    for k in range(fx.n_views):
        with np.errstate(invalid='ignore'):
            got = lc.host_model(fx.lanes_world, fx.view(k))
        lc.assert_same_lists(got, fx.expected(k), f'view {k}')
    for k in (0, 3):
        lc.assert_same_lists(lc.host_model(fx.nz_lanes, fx.view(k)), fx.expected(k, 'nz_'), f'-0.0 lanes, view {k}')


def test_homo_transform_reproduces_the_world_lanes(fx):
    from datasets.nuscenes_utils import homo_transform
    with np.errstate(invalid='ignore'):
        got = [homo_transform(fx.T, lane) for lane in fx.lanes_global]
    lc.assert_same_lists(got, fx.lanes_world, 'world')


def test_generate_with_a_plain_list_reproduces_the_reference_lists(fx):
    """BEVGenerator.generate's own host path (a list under trajs['gt_lanes']), without a device: the raster is stubbed."""
    from bev_generator.bev_generator import BEVGenerator
    from pca_amd import host_logic as hl

    class Probe(BEVGenerator):
        def generate_bev(self, pc_present, pc_future, pc_full, trajs_present, trajs_future, trajs_full, gt_lane_trajs=None):
            return gt_lane_trajs

        def viz_bev(self):
            pass

    for k in range(fx.n_views):
        ox, oy, oz, rot, dx, dy, zoom, px, view_size = fx.g['views'][k]
        origin = np.array([ox, oy, oz])
        assert np.array_equal(hl.rotation_matrix_3d(rot), fx.g['R'][k])
        gen = Probe(view_size, int(px))
        ego = np.array([[0., 0., 0.], [1., 0., 0.], [2., 0.5, 0.]])
        trajs = dict(ego_traj_present=ego[:2], ego_traj_future=ego[1:], ego_traj_full=ego, other_trajs_present=[],
                     other_trajs_future=[], other_trajs_full=[], gt_lanes=[lane - origin for lane in fx.lanes_world])
        pcs = dict(pc_present=np.zeros((1, 10)), pc_future=np.zeros((1, 10)), pc_full=np.zeros((1, 10)))
        with np.errstate(invalid='ignore'):
            got = gen.generate(pcs, trajs, rot, dx, dy, zoom, do_warping=True)
        lc.assert_same_lists(got, fx.expected(k), f'view {k}')


def test_device_lane_surface_exists():
    """Fails on a tree without the device lanes: the class, the accumulator's entry and the three C names."""
    from nuscenes_oracle_sem_pc_accum import NuScenesOracleSemanticPointCloudAccumulator
    from pca_amd import _lib
    from pca_amd.lanes import DeviceLanes, LaneHandle, PendingLanes
    assert callable(getattr(NuScenesOracleSemanticPointCloudAccumulator, 'set_gt_lanes'))
    for name in ('transform', 'to_grid', 'as_list'):
        assert callable(getattr(DeviceLanes, name))
    assert LaneHandle and PendingLanes
    import torch  # noqa: F401  (first, as _lib.load() does)
    lib = ctypes.CDLL(os.path.join(PKG, 'pca_amd', 'libpca_hip.so'))
    for name in ('pca_lanes_workspace_bytes', 'pca_lanes_transform', 'pca_lanes_to_grid'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    lib.pca_lanes_workspace_bytes.restype = ctypes.c_int64
    lib.pca_lanes_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int64]
    assert lib.pca_lanes_workspace_bytes(1000, 4, 64) >= 4 * 128 + 4 * 4 * 4
    assert lib.pca_lanes_workspace_bytes(-1, 4, 64) == -1 and lib.pca_lanes_workspace_bytes(10, 4, -1) == -1
