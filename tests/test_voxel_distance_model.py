"""CPU: the bindings of pca_voxel_distance exist, the numpy model of tests/voxel_distance_common.py -- which the GPU tests of
tests/test_gpu_voxel_distance.py hold the kernels to -- agrees with scipy's exact Euclidean transform, resolves ties to the
smaller place, and the scenes of the GPU test hold the situations they are meant to hold: tied voxels (a test that cannot see a
tie-rule bug proves nothing) and voxels without a site within every tested max_dist2.  pca_amd.host_logic.voxel_metric on the
default grid, above the bound and on an irrational ratio."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import voxel_distance_common as vd
from conftest import ROOT


def test_bindings_and_signatures():
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    for name, n_args in (('pca_voxel_distance_workspace_bytes', 2), ('pca_voxel_distance', 22)):
        assert name in _lib.EXPORTS and isinstance(getattr(lib, name), C._CFuncPtr) and len(getattr(lib, name).argtypes) == n_args
    assert _lib.KERNEL_IDS_DIST == ('voxel_dist_lines', 'voxel_dist_rows')
    text = open(os.path.join(ROOT, 'include', 'pca.h')).read()
    fourth = text[text.index('PCA_K_VOXEL_DIST_LINES = PCA_K_END'):]
    fourth = fourth[:fourth.index('}')].replace('= PCA_K_END', '').replace(',', ' ').split()
    assert fourth == ['PCA_K_VOXEL_DIST_LINES', 'PCA_K_VOXEL_DIST_ROWS', 'PCA_K_LAST']
    # two arrays of int32 per voxel, each on a 256-byte boundary; -1 outside the limits; no device needed
    assert lib.pca_voxel_distance_workspace_bytes(256, 32) == 2 * 4 * 256 * 256 * 32
    assert lib.pca_voxel_distance_workspace_bytes(3, 5) == 2 * 256
    assert [lib.pca_voxel_distance_workspace_bytes(*s) for s in ((0, 1), (1025, 1), (1, 0), (1, 33))] == [-1] * 4
    p = inspect.signature(DeviceStore.voxel_distance).parameters
    assert list(p)[1:] == ['labels', 'seen', 'site_labels', 'weights', 'max_dist2', 'fill_dist2', 'fill_free', 'tsdf']
    assert p['weights'].default == (1, 1) and p['fill_free'].default is False and p['tsdf'].default is None
    p = inspect.signature(SemBEVGenerator.voxel_distance_device).parameters
    assert list(p)[1:] == ['labels', 'seen', 'view', 'z_range', 'nz', 'sites', 'metric', 'max_dist', 'fill_dist', 'fill_free',
                           'tsdf_trunc', 'flip']
    assert p['metric'].default == 'metres' and p['flip'].default is True
    p = inspect.signature(SemanticPointCloudAccumulator.voxel_distance).parameters
    assert list(p)[1:10] == ['present_idx', 'part', 'z_range', 'nz', 'classes', 'include_dyn', 'origins', 'sites', 'site_classes']
    assert p['sites'].default == 'labels' and p['input_frames'].default == 1
    assert list(inspect.signature(SemanticPointCloudAccumulator.voxel_ssc_sample_filled).parameters)[1:3] == ['present_idx', 'fill_dist']


# ---------------------------------------------------------------------------------------------- voxel_metric
def test_voxel_metric():
    from pca_amd.host_logic import voxel_metric
    assert voxel_metric(0.3125, 0.2) == (625, 256, 0.0125)
    assert voxel_metric(80. / 256, (4.4 - -2.0) / 32, px=256, nz=32) == (625, 256, 0.0125)     # as the generator computes them
    assert voxel_metric(0.5, 0.5) == (1, 1, 0.5) and voxel_metric(0.2, 0.4) == (1, 4, 0.2)
    # 625 * 2 * 1023^2 is 1.3e9: inside; one more factor of two is not
    assert voxel_metric(0.3125, 0.2, px=1024, nz=32)[:2] == (625, 256)
    with pytest.raises(ValueError, match=r'2\^31 - 2'):
        voxel_metric(0.3125, 0.2 / 1.5, px=1024, nz=32)           # 75 / 32: w_xy = 5625
    with pytest.raises(ValueError, match='finite'):
        voxel_metric(0., 0.2)
    # an irrational ratio is served by the nearest fraction, and `unit` says what the numbers mean
    w_xy, w_z, unit = voxel_metric(math.sqrt(2.) * 0.2, 0.2)
    a, b = math.isqrt(w_xy), math.isqrt(w_z)
    assert a * a == w_xy and b * b == w_z and b <= 64 and math.gcd(a, b) == 1
    assert abs(a / b - math.sqrt(2.)) < 1. / (b * 64) and unit == math.sqrt(2.) * 0.2 / a
    assert abs(b * unit - 0.2) < 0.2 * 1e-3                         # along z a bin counts as b units: nearly z_step
    assert voxel_metric(math.sqrt(2.) * 0.2, 0.2, max_den=1)[:2] == (1, 1)


# ---------------------------------------------------------------------------------------------- the model against scipy
@pytest.mark.parametrize('weights', [(1, 1), (625, 256), (3, 7)])
@pytest.mark.parametrize('px,nz', [(3, 5), (16, 4), (33, 7)])
def test_model_equals_scipy(px, nz, weights):
    ndimage = pytest.importorskip('scipy.ndimage')
    for density in vd.densities(px, nz):
        labels, _, subset = vd.random_scene(px, nz, density)
        for sites in (None, subset):
            D, q = vd.transform(labels, sites, weights)
            mask = vd.site_mask(labels, sites)
            edt, idx = ndimage.distance_transform_edt(~mask, sampling=(math.sqrt(weights[1]), math.sqrt(weights[0]), math.sqrt(weights[0])),
                                                      return_indices=True)
            assert np.array_equal(np.rint(edt * edt).astype(np.int64), D)
            # the model's site is a site, at the distance it states; scipy's own is equally near (its tie rule is its own)
            k, r, c = q // (px * px), (q // px) % px, q % px
            assert mask[k, r, c].all()
            kk, rr, cc = np.indices(labels.shape)
            assert np.array_equal(weights[0] * ((rr - r) ** 2 + (cc - c) ** 2) + weights[1] * (kk - k) ** 2, D)
            assert np.array_equal(weights[0] * ((rr - idx[1]) ** 2 + (cc - idx[2]) ** 2) + weights[1] * (kk - idx[0]) ** 2, D)
            assert (q <= (idx[0] * px + idx[1]) * px + idx[2]).all()


def test_model_without_sites_and_bounds():
    labels = np.full((2, 3, 3), 255, dtype=np.uint8)
    labels[1, 1, 1] = 40                                            # a byte >= 32 is no site
    seen = np.zeros_like(labels)
    seen[0] = 1
    out = vd.model(labels, seen, fill_dist2=4, tsdf=(1., 2., True))
    assert (out['dist2'] == -1).all() and (out['nearest'] == -1).all() and (out['nearest_label'] == 255).all()
    assert (out['filled'] == 255).all()                             # (the byte 40 is empty and is not copied)
    assert (out['tsdf'][0] == 0).all() and (out['tsdf'][1] == 0).all() and np.signbit(out['tsdf'][1]).all()
    assert (vd.model(labels, seen, tsdf=(1., 2., False))['tsdf'][1] == -1).all()
    labels[0, 0, 0] = 4
    out = vd.model(labels, seen, max_dist2=1, fill_dist2=1, fill_free=True, tsdf=(0.5, 2., False))
    assert out['dist2'][0].tolist() == [[0, 1, -1], [1, -1, -1], [-1, -1, -1]] and out['dist2'][1, 0, 0] == 1
    assert out['filled'][0, 0, 1] == 4 and out['filled'][1, 1, 1] == 255 and out['tsdf'][0, 0, 1] == np.float32(0.25)
    assert vd.model(labels, seen, max_dist2=1, fill_dist2=1)['filled'][0, 0, 1] == 255       # seen: a beam crossed it, it stays free
    assert vd.model(labels, seen, max_dist2=1, fill_dist2=1)['filled'][1, 0, 0] == 4


# ---------------------------------------------------------------------------------------------- what the scenes hold
@pytest.mark.parametrize('px,nz', vd.SHAPES)
def test_scenes_hold_ties_and_far_voxels(px, nz):
    pairs = vd.planted_pairs(px, nz)
    assert len(pairs) == (4 if px >= 32 and nz >= 3 else 3 if px >= 16 and nz >= 3 else 1 if px >= 3 else 0)
    for density in vd.densities(px, nz):
        labels, seen, subset = vd.random_scene(px, nz, density)
        assert (labels[labels != 255] >= 32).any() or px == 1       # bytes that must count as empty
        for sites in (None, subset):
            base = vd.scene_base(px, nz, density, sites)
            D, q = base
            assert all(labels[c] == 3 and D[c] == 0 for c in vd.corners(px, nz))
            for kind, mid, lo, hi in pairs:
                dm = 2 if kind == 'diag' else 1
                assert D[mid] == dm and q[mid] == (lo[0] * px + lo[1]) * px + lo[2], (kind, mid)
                assert labels[lo] != labels[hi] and vd.model(labels, base=base)['nearest_label'][mid] == labels[lo]
            if px >= 3 and sites is None:
                assert vd.tied(labels, sites, base=base).sum() >= len(pairs)
            # some voxels have no site within every tested bound, and some have; a grid below 16 has no room for the slab
            # that guarantees it -- with a site in every corner all of (5, 3) lies within 9 -- and is held to bound 0 only
            for m in (vd.MAX_DIST2 if px >= 16 else vd.MAX_DIST2[:1] if px > 1 else ()):
                assert 0 < (D > m).sum() < D.size, m
            if sites is not None and px >= 16:
                assert (~vd.site_mask(labels, sites) & (labels < 32)).any()          # occupied voxels that are no sites
        slab = vd.slab_columns(px)
        if slab:
            assert (labels[:, :, slab[0]:slab[1]] == 255).all()
            assert (vd.scene_base(px, nz, density)[0][:, px // 2, (slab[0] + slab[1]) // 2] > max(vd.MAX_DIST2)).all()


def test_anisotropic_and_long_line_scenes_hold_ties():
    px, nz = 72, 16
    dense = vd.densities(px, nz)[1]
    labels, _, _ = vd.random_scene(px, nz, dense)
    base = vd.scene_base(px, nz, dense, None, (625, 256))
    for kind, mid, lo, hi in vd.planted_pairs(px, nz):
        assert base[0][mid] == {'col': 625, 'row': 625, 'k': 256, 'diag': 1250}[kind] and base[1][mid] == (lo[0] * px + lo[1]) * px + lo[2]
    for m in vd.MAX_DIST2:
        assert 0 < (base[0] > 625 * m).sum() < base[0].size
    labels, _ = vd.long_line_scene()
    assert (labels < 32).sum() == 32 and all(labels[0, r, c] < 32 for r in (0, 1023) for c in (0, 1023))
