"""The device form of the NuScenes sweep merger (kernel K0s, pca_nusc_merge_sweeps) against the reference's RECORDED
results -- tests/golden/nusc_sweeps.npz and nusc_sweeps_edges.npz -- and, for a larger seeded case, against the host form
with its matrix product replaced by the oracle's FMA chain (machine-independent).  Everything is compared bit for bit."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import fake_nuscenes as fk
import nusc_sweeps_edges_common as ec
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def check_result(out, want):
    assert isinstance(out['points'], np.ndarray) and out['points'].dtype == np.float32
    assert out['points'].shape == want['points'].shape
    assert np.array_equal(out['points'], want['points'])
    assert list(out['instances_token']) == [str(t) for t in want['instances_token']]
    assert np.array_equal(np.stack(out['instances_center']), want['instances_center'])
    assert np.array_equal(out['instances_last_box'], want['instances_last_box'])
    assert np.array_equal(out['instances_name'], want['instances_name'])


def plain_quaternion(q):
    return np.asarray(q)


def test_device_merger_matches_reference(tmp_path):
    from datasets.nuscenes_sweeps import inst_centric_get_sweeps_device
    g = np.load(os.path.join(GOLDEN, 'nusc_sweeps.npz'))
    tables = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    nusc = fk.FakeNuScenes(tables, tmp_path, quaternion=plain_quaternion)
    out = inst_centric_get_sweeps_device(nusc, 'sample0', **fk.SWEEP_CFG)
    check_result(out, g)
    assert (out['points'][:, 6] >= 0).sum() > 50


@pytest.mark.parametrize('pretest', ['1', '0'])
@pytest.mark.parametrize('scenario', sorted(ec.SCENARIOS))
def test_device_merger_at_the_edges(scenario, pretest, tmp_path, monkeypatch):
    """box faces and the radius circle with their f32 neighbours, tile-sized sweeps, an empty file, ...; once with the
    certified pre-test of the box loop and once with every point-box pair going through the divisions"""
    from datasets.nuscenes_sweeps import inst_centric_get_sweeps_device
    monkeypatch.setenv('PCA_NUSC_SWEEPS_PRETEST', pretest)
    g = np.load(os.path.join(GOLDEN, 'nusc_sweeps_edges.npz'), allow_pickle=False)
    nusc = fk.FakeNuScenes(ec.load_tables(g, scenario), tmp_path, quaternion=plain_quaternion)
    out = inst_centric_get_sweeps_device(nusc, 'sample0', **ec.cfg(scenario))
    check_result(out, ec.expected(g, scenario))


def test_device_merger_larger_case(tmp_path, monkeypatch):
    """synth_tables(11, 5, 20000): ~99 k rows, more than 190 tiles, against the host form over the oracle's FMA chain"""
    import torch

    from datasets import nuscenes_sweeps as ns
    from oracle import oracle as orc
    nusc = fk.FakeNuScenes(fk.synth_tables(11, 5, 20000), tmp_path, quaternion=plain_quaternion)
    monkeypatch.setattr(ns, '_apply', lambda T, xyz: orc.homo_transform(T, xyz))
    want = ns.inst_centric_get_sweeps(nusc, 'sample0', **fk.SWEEP_CFG)
    assert want['points'].shape[0] > 190 * 512 and (want['points'][:, 6] >= 0).sum() > 500
    out = ns.inst_centric_get_sweeps_device(nusc, 'sample0', **fk.SWEEP_CFG)
    check_result(out, {k: (np.stack(v) if k == 'instances_center' else v) for k, v in want.items()})
    inputs = ns.collect_sweep_inputs(nusc, 'sample0', fk.SWEEP_CFG['n_sweeps'], fk.SWEEP_CFG['detection_classes'])
    dev = ns.merge_sweeps_device(inputs, fk.SWEEP_CFG['center_radius'], fk.SWEEP_CFG['in_box_tolerance'], device_points=True)
    assert isinstance(dev['points'], torch.Tensor) and dev['points'].is_cuda and dev['points'].dtype == torch.float32
    assert np.array_equal(dev['points'].cpu().numpy(), out['points'])
    assert int(dev['sweep_off'][-1]) == out['points'].shape[0] and dev['instances_token'] == out['instances_token']


def synthetic_inputs(n_sweeps, boxes_per_sweep, n_pts):
    box = {'target_from_box': np.eye(4), 'size': np.array([40.0, 20.0, 15.0]), 'center': np.zeros(3), 'cls': 0,
           'instance_token': 'i', 'anno_token': 'a'}
    return {'target_from_glob': np.eye(4),
            'sweeps': [{'raw': np.full((n_pts, 5), 5.0, np.float32), 'lag': 0.05 * k, 'sweep': k, 'target_from_sweep': np.eye(4),
                        'boxes': [dict(box) for _ in range(boxes_per_sweep)]} for k in range(n_sweeps)]}


def test_device_merger_limits():
    import torch

    from datasets import nuscenes_sweeps as ns
    from pca_amd import _lib
    ctx = _lib.Context.get()
    with pytest.raises(RuntimeError, match='at most 4096 boxes'):
        ns.merge_sweeps_device(synthetic_inputs(1, 4097, 8), 2.0, 0.05)
    with pytest.raises(RuntimeError, match='at most 32 sweeps'):
        ns.merge_sweeps_device(synthetic_inputs(33, 1, 8), 2.0, 0.05)
    # tiles: the library counts them from the table alone, before it looks at a buffer
    sweeps = np.zeros(32, ns._SWEEP_DTYPE)
    sweeps['n_rows'], sweeps['row0'] = 513 * 512, np.arange(32) * 513 * 512
    tally = torch.zeros(64, dtype=torch.int32, device='cuda')
    rc = ctx.lib.pca_nusc_merge_sweeps(ctx.h, tally.data_ptr(), 32 * 513 * 512, sweeps.ctypes.data, 32, None, 0, 2.0, 0.55,
                                       tally.data_ptr(), 256, tally.data_ptr(), tally.data_ptr(), ctx.stream())
    assert rc != 0 and b'at most 16384 tiles' in ctx.lib.pca_last_error(ctx.h)
    torch.cuda.synchronize()
    assert not tally.any() and ctx.status() == 0             # nothing ran
    # the limits themselves are fine, and so are a call without points, a sweep without points and a call without boxes
    res = ns.merge_sweeps_device(synthetic_inputs(32, 128, 3), 2.0, 0.05)
    assert res['points'].shape == (96, 8) and (res['points'][:, 6] == 0).all() and len(res['instances_token']) == 4096
    assert np.array_equal(res['points'][:, 5], np.repeat(np.arange(32, dtype=np.float32), 3))
    empty = ns.merge_sweeps_device(synthetic_inputs(3, 2, 0), 2.0, 0.05)
    assert empty['points'].shape == (0, 8) and empty['points'].dtype == np.float32 and empty['instances_token'] == []
    assert ns.merge_sweeps_device(synthetic_inputs(2, 2, 0), 2.0, 0.05, device_points=True)['points'].shape == (0, 8)
    mixed = synthetic_inputs(3, 0, 5)
    mixed['sweeps'][1]['raw'] = np.zeros((0, 5), np.float32)
    res = ns.merge_sweeps_device(mixed, 2.0, 0.05)
    assert res['points'].shape == (10, 8) and (res['points'][:, 6:] == -1).all() and list(res['sweep_off']) == [0, 5, 5, 10]


# ---- loaders ---------------------------------------------------------------------------------------------------------
def make_loader(tmp_path):
    from obs_dataloaders.nuscenes_obs_dataloader import NuScenesDataloader
    g = np.load(os.path.join(GOLDEN, 'utils.npz'), allow_pickle=False)
    nusc = fk.FakeNuScenes(fk.synth_tables(), tmp_path, quaternion=plain_quaternion)
    rng = np.random.default_rng(3)
    W, H = int(g['pp_wh'][0]), int(g['pp_wh'][1])
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(6)]

    class Loader(NuScenesDataloader):
        def __init__(self):
            self.nusc, self.num_sweeps, self.batch_size = nusc, 5, 1
            self.cam_channels = ['CAM%d' % j for j in range(6)]
            self.sample_tokens = ['sample0', 'sample0']
            self.int_idx, self.sweep_idx, self.inst_idx, self.cls_idx = 3, 5, 6, 7
            self.pc_range = [-1000, -1000, -1000, 1000, 1000, 1000]
            self.idx = 0

        def _lidar(self, sample):
            return SimpleNamespace(ego_from_self=g['c6_ego_from_lidar'], glob_from_ego=g['c6_glob_from_ego'])

        def _cameras(self, sample):
            return [SimpleNamespace(img=images[j], glob_from_self=g['c6_glob_from_cam'][j], cam_K=g['pp_K'], img_wh=g['pp_wh'])
                    for j in range(6)]

    return Loader()


def same_value(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


def test_loader_device_mode_equals_default(tmp_path, monkeypatch):
    loader = make_loader(tmp_path)
    monkeypatch.delenv('PCA_NUSC_SWEEPS', raising=False)
    host = loader.read_obs(0)
    monkeypatch.setenv('PCA_NUSC_SWEEPS', 'device')
    assert loader.device_sweeps()
    dev = loader.read_obs(0)
    assert list(host) == list(dev) and host['pc'].shape[0] > 10000 and len(host['inst_tokens']) > 5
    for key in host:
        assert same_value(host[key], dev[key]), key
    loader.sweep_provider = lambda nusc, token, **cfg: 1 / 0          # a provider always wins over the variable
    assert not loader.device_sweeps()


def test_prefetching_loader_device_mode_equals_host_mode(tmp_path, monkeypatch):
    import torch

    from pca_amd.ingest import NuScenesPrefetchingLoader
    loader = make_loader(tmp_path)
    monkeypatch.delenv('PCA_NUSC_SWEEPS', raising=False)
    host = [b[0] for b in NuScenesPrefetchingLoader(loader, depth=2)]
    monkeypatch.setenv('PCA_NUSC_SWEEPS', 'device')
    import datasets.nuscenes_sweeps as ns
    monkeypatch.setattr(ns, 'inst_centric_get_sweeps_device', None)   # the pipeline merges from the collected inputs itself
    dev = [b[0] for b in NuScenesPrefetchingLoader(loader, depth=2)]
    assert len(host) == len(dev) == 2
    for h, d in zip(host, dev):
        assert isinstance(d['pc'], torch.Tensor) and d['pc'].is_cuda and d['pc'].dtype == torch.float64
        assert d['pc'].shape == h['pc'].shape and d['pc'].shape[0] > 10000
        assert np.array_equal(d['pc'].cpu().numpy(), h['pc'].cpu().numpy())
        assert np.array_equal(d['pc_cam_idx'].cpu().numpy(), h['pc_cam_idx'].cpu().numpy())
        assert np.array_equal(d['images'].dev.cpu().numpy(), h['images'].dev.cpu().numpy())
        for key in ('meta', 'inst_tokens', 'inst_cls', 'ego_global_x', 'ego_global_y'):
            assert h[key] == d[key], key
        assert same_value(h['inst_center'], d['inst_center']) and np.array_equal(h['ego_at_lidar_ts'], d['ego_at_lidar_ts'])
