"""GT lane centrelines on the device (csrc/pca_lanes.hip, pca_amd/lanes.py) against the reference's recorded lists
(tests/golden/lanes.npz) and against the host model that test_lanes_golden.py holds to the reference.  Every comparison is
bit for bit on the f64 rows; lists have equal length and equal per-lane shapes."""
import gzip
import os
import random

import numpy as np
import pytest

import lanes_common as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return lc.Fixture()


def lane_views(views):
    from pca_amd.lanes import LaneView
    return [LaneView(*v) for v in views]


def test_fixture_transform_then_to_grid_singly_and_as_one_call(fx):
    from pca_amd.lanes import DeviceLanes
    lanes = DeviceLanes(fx.lanes_global)
    lanes.transform(fx.T)
    lc.assert_same_lists(lanes.as_list(), fx.lanes_world, 'as_list after transform')
    views = lane_views([fx.view(k) for k in range(fx.n_views)])
    for k, v in enumerate(views):
        lc.assert_same_lists(lanes.to_grid([v])[0].resolve(), fx.expected(k), f'view {k} alone')
    before = lanes.launches
    many = lanes.to_grid(views)
    assert lanes.launches == before + 1
    for k, p in enumerate(many):
        lc.assert_same_lists(p.resolve(), fx.expected(k), f'view {k} of one call')
    # the lanes that hold a z of -0.0 (it cannot come out of homo_transform: a set of their own, in world coordinates)
    nz = DeviceLanes(fx.nz_lanes)
    for k, p in zip((0, 3), nz.to_grid(lane_views([fx.view(0), fx.view(3)]))):
        lc.assert_same_lists(p.resolve(), fx.expected(k, 'nz_'), f'-0.0 lanes, view {k}')
    lanes.ctx.check_status()


@pytest.fixture(scope='module')
def generated():
    """(lanes, views, host model lists per view) for three seeds, computed once."""
    out = []
    for seed in (11, 12, 13):
        lanes, views = lc.generated_map(seed), lc.generated_views(seed)
        out.append((lanes, views, [lc.host_model(lanes, v) for v in views]))
    return out


def test_generated_map_against_the_host_model(generated):
    from pca_amd.lanes import DeviceLanes
    for lanes, views, want in generated:
        # what the map has to offer, asserted on the host model before anything is compared
        n_io, n_oi, n_through = lc.census(lanes, views[0])
        print('survivors', len(want[0]), 'crossings', n_io, n_oi, 'through', n_through)
        assert len(want[0]) >= 100 and n_io >= 50 and n_oi >= 50 and n_through >= 4
        assert any(lane.shape[0] >= 3000 and lc.host_model([lane], views[0]) for lane in lanes)
        dev = DeviceLanes(lanes)
        got = dev.to_grid(lane_views(views))
        assert dev.launches == 1
        for k in range(4):
            lc.assert_same_lists(got[k].resolve(), want[k], f'view {k}')
        dev.ctx.check_status()


def test_overflow_reruns_the_sample_once_and_an_exact_cap_does_not(generated):
    from pca_amd.lanes import DeviceLanes
    lanes, views, want = generated[0]
    dev = DeviceLanes(lanes)
    got = dev.to_grid(lane_views(views), cap_rows=64)
    for k in range(4):
        lc.assert_same_lists(got[k].resolve(), want[k], f'view {k}, cap 64')
        assert got[k].reruns == 1
    n = sum(w.shape[0] for w in want[0])
    one = dev.to_grid(lane_views(views[:1]), cap_rows=n)[0]
    lc.assert_same_lists(one.resolve(), want[0], 'cap equal to the row count')
    assert one.reruns == 0
    one = dev.to_grid(lane_views(views[:1]), cap_rows=n - 1)[0]
    lc.assert_same_lists(one.resolve(), want[0], 'cap one short of the row count')
    assert one.reruns == 1
    # asynchronous delivery, decoded later: the same lists, and the overflow is found at decode time
    got = dev.to_grid(lane_views(views), cap_rows=64, asynchronous=True)
    assert not any(p.resolved for p in got)
    for k in range(4):
        lc.assert_same_lists(got[k].resolve(), want[k], f'view {k}, cap 64, asynchronous')


def test_empty_inputs_return_empty_lists_without_a_launch(fx):
    from pca_amd.lanes import DeviceLanes
    v = lane_views([fx.view(0), fx.view(1)])
    for lanes in ([], [np.zeros((0, 3)), np.array([[1., 2., 3.]]), np.zeros((0, 3))]):
        dev = DeviceLanes(lanes)
        dev.transform(fx.T)
        assert [p.resolve() for p in dev.to_grid(v)] == [[], []] and dev.launches == 0
        assert len(dev.as_list()) == len(lanes)
    dev = DeviceLanes(fx.lanes_world)
    assert dev.to_grid([]) == [] and dev.launches == 0


def test_bad_arguments_are_refused(fx):
    import torch

    from pca_amd.lanes import DeviceLanes, PcaLaneView
    dev = DeviceLanes(fx.lanes_world)
    ctx, lib = dev.ctx, dev.ctx.lib
    P, L = dev.n_vertices, dev.n_lanes
    views = (PcaLaneView * 1)()
    views[0].R[:] = np.eye(3).ravel().tolist()
    views[0].view, views[0].px = 40., 64
    cap = 256
    out = torch.zeros(8 + 4 * cap + 24 * cap + 64, dtype=torch.uint8, device=dev.device)
    ws = torch.zeros(lib.pca_lanes_workspace_bytes(P, 1, cap), dtype=torch.uint8, device=dev.device)
    p = out.data_ptr()

    def call(xyz=dev.xyz.data_ptr(), cap_rows=cap, px=64, n_p=P):
        views[0].px = px
        return lib.pca_lanes_to_grid(ctx.h, xyz, dev.vertex_lane.data_ptr(), dev.start.data_ptr(), n_p, L, views, 1, cap_rows,
                                     p + 64 + 4 * cap, p + 64, p, ws.data_ptr(), ctx.stream())

    assert call() == 0
    assert call(xyz=None) == -1 and b'bad arguments' in lib.pca_last_error(ctx.h)
    assert call(cap_rows=-1) == -1
    assert call(px=0) == -1 and b'px' in lib.pca_last_error(ctx.h)
    assert call(n_p=-1) == -1
    assert lib.pca_lanes_transform(ctx.h, None, P, np.eye(4).ctypes.data, ctx.stream()) == -1
    assert lib.pca_lanes_workspace_bytes(-1, 1, 0) == -1
    ctx.check_status()                                   # nothing faulted, nothing was raised
    with pytest.raises(ValueError):
        dev.to_grid(lane_views([fx.view(0)]), cap_rows=-1)


# ---- drop-in: the accumulator and the generator, device lanes against PCA_GT_LANES=host ----------------------------------
NUSC_FILTERS = [10, 11, 12, 16, 18]
SEM_IDXS = {'road': 0, 'car': 13, 'truck': 14, 'bus': 15, 'motorcycle': 17}


class FakeSemSeg:
    def pred(self, rgb):
        a = np.asarray(rgb).astype(np.int64)
        return ((a[..., 0] + 2 * a[..., 1] + 3 * a[..., 2]) % 19)[None, None]


def scene_lanes(g):
    """A few hundred lanes in 'global' coordinates around the scene's ego poses."""
    rng = np.random.default_rng(7)
    centre = np.r_[g['T_0'][:2, 3], 0.]
    lanes = [np.zeros((0, 3)), centre[None] + 1.]
    for i in range(300):
        n = int(rng.integers(2, 40))
        heading = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0, 0.1, n))
        d = np.c_[np.cos(heading), np.sin(heading), rng.normal(0, 0.02, n)]
        lanes.append(centre + np.r_[rng.uniform(-45, 45, 2), 0.] + np.cumsum(d, axis=0))
    return lanes


def scene_lanes_without_crossings(g, idx):
    """Lanes wholly inside every augmented view of sample idx (within 6 m of its pose: the smallest view reaches 9.5 m from
    it in every direction) or far outside all of them.  For the warp: the reference's warp_point raises on the grid
    coordinate -1 that a bisected crossing on the left or lower border can have, on the host path as well."""
    rng = np.random.default_rng(8)
    centre = np.r_[g[f'T_{idx}'][:2, 3], 0.]
    lanes = []
    for i in range(120):
        n = int(rng.integers(2, 9))
        pts = np.c_[rng.uniform(-6, 6, (n, 2)) / np.sqrt(2), rng.normal(0, 0.1, n)]
        if i % 3 == 0:
            pts[:, :2] += rng.choice([-1., 1.], 2) * rng.uniform(80, 200, 2)
        lanes.append(centre + pts)
    return lanes


def make_accumulator(g, bev_params, lanes):
    from PIL import Image

    from nuscenes_oracle_sem_pc_accum import NuScenesOracleSemanticPointCloudAccumulator
    acc = NuScenesOracleSemanticPointCloudAccumulator('fake.onnx', NUSC_FILTERS, SEM_IDXS, False, dict(bev_params), 'boston',
                                                      False, None)
    acc.set_gt_lanes(lanes)
    batch = []
    for k in range(int(g['F'])):
        T = g[f'T_{k}']
        batch.append([dict(images=[Image.fromarray(im) for im in g[f'imgs_{k}']], pc=g[f'pc_{k}'], pc_cam_idx=g[f'cam_idx_{k}'],
                           ego_at_lidar_ts=T, ego_global_x=T[0, 3], ego_global_y=T[1, 3],
                           inst_tokens=str(g['inst_tokens'][k]).split(','), inst_cls=list(g[f'inst_cls_{k}']),
                           inst_center=list(g[f'inst_center_{k}']))])
    acc.integrate(batch[0])                     # both integrate paths move the lanes to the world frame on the first frame
    acc.integrate_many(batch[1:])
    return acc


def same_bev(b, s):
    assert set(b.keys()) == set(s.keys()) and 'gt_lanes' in s
    for key in s:
        if key.startswith('trajs') or key == 'gt_lanes':
            lc.assert_same_lists(b[key], s[key], key)
        else:
            assert np.array_equal(np.asarray(b[key]).view(np.uint16), np.asarray(s[key]).view(np.uint16)), key


def test_dropin_device_lanes_equal_the_host_path(golden, monkeypatch, tmp_path):
    import bev_generator.bev_generator as bg
    import sem_pc_accum
    from bev_generator.sem_bev import LazyBev
    from pca_amd import writer
    from pca_amd.lanes import DeviceLanes, PendingLanes
    monkeypatch.setattr(sem_pc_accum, 'SemSegONNX', lambda path: FakeSemSeg())
    # the augmentation reseeds from pid * time: one fixed second, so that both accumulators draw the same samples

    class FixedTime:
        @staticmethod
        def time():
            return 1700000000.0
    monkeypatch.setattr(bg, 'time', FixedTime)
    g = golden('nusc_oracle')
    F = int(g['F'])
    lanes = scene_lanes(g)
    prm = dict(type='sem', view_size=30, pixel_size=32, max_trans_radius=0., zoom_thresh=0., do_warp=False, int_scaler=1.,
               int_sep_scaler=30., int_mid_threshold=0.12, height_filter=3.)
    aug = dict(prm, max_trans_radius=4., zoom_thresh=0.1)
    warp = dict(aug, do_warp=True)
    idx = int(g['present_idx'])

    def build(p, lanes=lanes):
        monkeypatch.delenv('PCA_GT_LANES', raising=False)
        dev = make_accumulator(g, p, lanes)
        monkeypatch.setenv('PCA_GT_LANES', 'host')
        host = make_accumulator(g, p, lanes)
        monkeypatch.delenv('PCA_GT_LANES')
        assert isinstance(dev._lanes, DeviceLanes) and isinstance(host._lanes, list)
        return dev, host

    dev, host = build(prm)
    lc.assert_same_lists(dev.gt_lane_poses, host.gt_lane_poses, 'gt_lane_poses after the first frame')

    def pending_of(b):
        return b._pending[4]

    # generate_bev(idx, 1, True): asynchronous, the lanes undecoded until somebody looks
    n0 = PendingLanes.n_resolved
    b = dev.generate_bev(idx, 1, True)[0]
    assert isinstance(b, LazyBev) and isinstance(pending_of(b), PendingLanes) and not pending_of(b).resolved
    assert PendingLanes.n_resolved == n0
    s = host.generate_bev(idx, 1, True)[0]
    same_bev(b, s)
    assert len(s['gt_lanes']) > 0 and isinstance(b['gt_lanes'], list) and PendingLanes.n_resolved == n0 + 1
    # generate_bev_many: ONE lane call for all the samples
    idxs = list(range(1, F))
    launches = dev._lanes.launches
    many = dev.generate_bev_many(idxs, True)
    assert dev._lanes.launches == launches + 1 and not any(pending_of(m).resolved for m in many)
    for m, s in zip(many, host.generate_bev_many(idxs, True)):
        same_bev(m, s)
    # the background writer's pickle
    for acc, name in ((dev, 'dev'), (host, 'host')):
        acc.write_compressed_pickle(acc.generate_bev(idx, 1, True)[0], name, str(tmp_path))
    writer.flush_shared()
    blobs = [gzip.open(os.path.join(str(tmp_path), f'{name}.gz'), 'rb').read() for name in ('dev', 'host')]
    assert blobs[0] == blobs[1]
    # PCA_SYNC_BEV=1: plain dicts, decoded at once
    monkeypatch.setenv('PCA_SYNC_BEV', '1')
    b = dev.generate_bev(idx, 1, True)[0]
    assert type(b) is dict and isinstance(b['gt_lanes'], list)
    same_bev(b, host.generate_bev(idx, 1, True)[0])
    monkeypatch.delenv('PCA_SYNC_BEV')
    # bev_num = 3 with augmentation, then with the warp on top (its parameters come from numpy's and random's state)
    for p, lane_set in ((aug, lanes), (warp, scene_lanes_without_crossings(g, idx))):
        dev, host = build(p, lane_set)
        launches = dev._lanes.launches
        random.seed(3)
        got = dev.generate_bev(idx, 3, True)
        assert dev._lanes.launches == launches + 1 and not any(pending_of(x).resolved for x in got)
        random.seed(3)
        want = host.generate_bev(idx, 3, True)
        for x, y in zip(got, want):
            same_bev(x, y)
            assert len(y['gt_lanes']) > 0
    dev.store.check_status()
