"""CPU: the bindings of pca_bev_voxel_camera exist, and the numpy model of tests/voxel_camera_common.py -- which the GPU tests
of tests/test_gpu_voxel_camera.py hold the kernel to -- is right: against the slab method, on a hand-built scene, against the
lidar walk of voxel_rays_common, and non-vacuous on every case the GPU tests share with it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import voxel_camera_common as cc
import voxel_rays_common as rc
from conftest import ROOT

SHAPES = [(16, 4, 24, 16), (32, 8, 65, 33)]


def test_bindings_and_signatures():
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    assert 'pca_bev_voxel_camera' in _lib.EXPORTS and isinstance(lib.pca_bev_voxel_camera, C._CFuncPtr)
    assert len(lib.pca_bev_voxel_camera.argtypes) == 13
    assert _lib.KERNEL_IDS_CAMERA == ('bev_camera_rays', )
    # the id sits in pca.h's second enum block, ahead of PCA_K_TOTAL, and the struct is laid out as the header's
    text = open(os.path.join(ROOT, 'include', 'pca.h')).read()
    second = text[text.index('PCA_K_BEV_INST_INIT = PCA_K_COUNT'):text.index('PCA_K_TOTAL')].replace('= PCA_K_COUNT', '')
    ids = second.replace(',', ' ').split()
    assert len(ids) == len(_lib.KERNEL_IDS_INST) + len(_lib.KERNEL_IDS_CAMERA) and ids[-1] == 'PCA_K_BEV_CAMERA_RAYS'
    assert re.search(r'double Minv\[9\], C\[3\];[^}]*int32_t width, height, stride, clear;\s*double max_depth;\s*} pca_ray_camera;', text)
    assert [f[0] for f in _lib.PcaRayCamera._fields_] == ['Minv', 'C', 'width', 'height', 'stride', 'clear', 'max_depth']
    assert C.sizeof(_lib.PcaRayCamera) == 12 * 8 + 4 * 4 + 8
    P = cc.look_at((1., 2., 3.), (4., 4., 2.), 20., 24, 16)
    cam = _lib.make_ray_camera(P, 24, 16, stride=3, max_depth=7.5, clear=False)
    Minv, Cc = cc.camera_of(P)
    assert list(cam.Minv) == Minv.reshape(9).tolist() and list(cam.C) == Cc.tolist()
    assert (cam.width, cam.height, cam.stride, cam.clear, cam.max_depth) == (24, 16, 3, 0, 7.5)
    assert np.allclose(Cc, (1., 2., 3.), atol=1e-12)              # the camera centre
    p = inspect.signature(DeviceStore.bev_voxel_camera).parameters
    assert list(p)[1:] == ['prm', 'z_lo', 'z_step', 'nz', 'labels', 'cams', 'stride', 'max_depth'] and p['stride'].default == 1
    p = inspect.signature(SemBEVGenerator.voxel_camera_device).parameters
    assert list(p)[1:] == ['pc', 'labels', 'cams', 'rot_mat', 'dx', 'dy', 'aug_view_size', 'z_range', 'nz', 'stride', 'max_depth']
    p = inspect.signature(SemanticPointCloudAccumulator.voxel_visibility).parameters
    assert list(p)[1:] == ['present_idx', 'part', 'z_range', 'nz', 'classes', 'include_dyn', 'origins', 'cameras', 'stride',
                           'max_depth']
    assert p['cameras'].default is None and p['max_depth'].default is None and p['nz'].default == 32


@pytest.mark.parametrize('px,nz,W,H', SHAPES)
@pytest.mark.parametrize('stride', [1, 3])
def test_random_case_against_the_slab_method_and_not_vacuous(px, nz, W, H, stride):
    """The case the GPU tests run at every shape: the model's marks and hits against the slab method, which shares nothing
    with the walk; between 10 % and 90 % of the rays hit, and the hits hide something a walk that never stops would mark."""
    sc = cc.scene('random', px, nz, W, H, stride)
    out = cc.model_of(sc, record=True)
    rays = (W // stride) * (H // stride)
    assert out['stats'][0] == out['stats'][1] == rays and out['hit'].shape == (H // stride, W // stride)
    assert 0.1 * rays <= out['stats'][4] <= 0.9 * rays, out['stats']
    assert cc.slab_check(out['s'], out['e'], out, px, nz) > 3 * rays
    full = cc.lidar_style_marks(out['s'], out['e'], px, nz)
    assert not (out['visible'] & ~full).any() and (full & ~out['visible']).sum() >= 1
    hit = out['hit'].ravel() >= 0
    assert (out['label'].ravel()[hit] == sc['labels'].ravel()[out['hit'].ravel()[hit]]).all()
    assert (out['label'].ravel()[~hit] == 255).all() and (out['depth'].ravel()[~hit] == 0).all()
    assert out['visible'].ravel()[out['hit'].ravel()[hit]].all()  # the voxel that stops a ray is visible
    # the depth of a hit is the camera depth at which the ray enters the hit voxel: between 0 and max_depth, and the point at
    # that depth lies on the voxel's closed box
    t = out['t_hit'][hit]
    at = out['s'][hit] + t[:, None] * (out['e'][hit] - out['s'][hit])
    place = out['hit'].ravel()[hit].astype(np.int64)
    vox = np.stack([place % px, px - 1 - (place // px) % px, place // (px * px)], 1)
    assert (at >= vox - 1e-9).all() and (at <= vox + 1 + 1e-9).all()
    assert np.array_equal(out['depth'].ravel()[hit], (t * sc['max_depth']).astype(np.float32))


def test_a_wall_occludes_what_lies_behind_it():
    """Cells of 1 m, px 16, nz 4; the camera at grid (2.5, 8.25, 1.5) looks along +u at a wall that fills the plane i = 9:
    every free voxel in front of it that a ray crosses is visible, the wall's voxels are visible and hit, and nothing with
    i > 9 is marked."""
    px, nz, W, H = 16, 4, 24, 16
    lab = np.full((nz, px, px), 255, dtype=np.uint8)
    lab[:, :, 9] = 5
    Minv, Cc = cc.axis_camera((2.5 - px / 2., 8.25 - px / 2., 1.5), W, H)
    out = cc.model(lab, Minv, Cc, W, H, 1, 16., **cc.unit_grid(px, nz))
    vis = out['visible']
    assert not vis[:, :, 10:].any()                               # nothing behind the wall
    assert not vis[:, :, :2].any()                                # nor behind the camera
    hit = out['hit'][out['hit'] >= 0].astype(np.int64)
    assert hit.size > 0.5 * W * H and (hit % px == 9).all() and (out['label'][out['hit'] >= 0] == 5).all()
    assert vis[:, :, 9].any() and np.array_equal(np.flatnonzero(vis[:, :, 9].ravel()), np.unique((hit // px // px) * px + (hit // px) % px))
    assert vis[1, px - 1 - 8, 2:10].all()                         # the free voxels straight ahead, and the wall's
    # the depth of a hit is the distance along the optical axis to the wall's near face, 9 - 2.5, for every ray that was
    # not stopped by the floor or ceiling of the grid first (it enters the wall through that face)
    d = out['depth'][out['hit'] >= 0]
    assert np.allclose(d, 6.5, atol=1e-6)
    # free space in front: exactly the voxels some ray's segment crosses before its hit
    assert cc.slab_check(out['s'], out['e'], cc.model(lab, Minv, Cc, W, H, 1, 16., record=True, **cc.unit_grid(px, nz)), px, nz) > 1000
    # rays that leave through the top or the bottom before the wall hit nothing
    assert (out['hit'] < 0).any()


@pytest.mark.parametrize('name', ['random', 'diagonal_ties', 'ends_inside'])
def test_empty_labels_give_the_lidar_walk_plus_the_end_voxels(name):
    sc = cc.scene(name, 16, 4, 65, 33)
    sc['labels'][:] = 255
    out = cc.model_of(sc)
    assert out['stats'][4] == 0 and (out['hit'] == -1).all() and out['visible'].any()
    assert np.array_equal(out['visible'], cc.lidar_style_marks(out['s'], out['e'], 16, 4))
    if name == 'ends_inside':                                     # (the rays end inside the grid: the end voxels count)
        assert not np.array_equal(out['visible'], rc.traverse(out['s'], out['e'], 16, 4)['seen'])


def test_the_shared_cases_are_what_their_names_say():
    """Non-vacuity of the cases of tests/test_gpu_voxel_camera.py, on the model alone."""
    px, nz, W, H = 16, 4, 65, 33
    out = cc.model_of(cc.scene('inside_occupied', px, nz, W, H))
    assert (out['hit'] == out['hit'][0, 0]).all() and out['hit'][0, 0] >= 0 and (out['depth'] == 0).all() and (out['label'] == 3).all()
    assert out['visible'].sum() == 1
    out = cc.model_of(cc.scene('outside_in', px, nz, W, H))
    assert (out['s'][:, 0] < 0).all() and out['visible'].any() and 0 < out['stats'][4] < out['stats'][1] == W * H
    out = cc.model_of(cc.scene('outside_away', px, nz, W, H))
    assert out['stats'].tolist() == [W * H, W * H, 0, 0, 0] and not out['visible'].any()
    out = cc.model_of(cc.scene('axis_parallel', px, nz, W, H))
    c, g = np.floor(out['s']).astype(int), np.floor(out['e']).astype(int)
    mid = (H // 2) * W + W // 2
    assert (c[mid, 1:] == g[mid, 1:]).all() and out['e'][mid, 1] == out['s'][mid, 1] and out['e'][mid, 2] == out['s'][mid, 2]
    assert (out['e'][(H // 2) * W:(H // 2 + 1) * W, 2] == out['s'][0, 2]).all()      # the middle row: parallel to the floor
    assert (out['e'][W // 2::W, 1] == out['s'][0, 1]).all()                          # the middle column
    assert out['visible'][1, px - 1 - 8, 1:6].all()
    out = cc.model_of(cc.scene('diagonal_ties', px, nz, W, H))
    assert out['ties'] > 0 and (out['s'] == np.floor(out['s'])).all()
    sc = cc.scene('ends_inside', px, nz, W, H)
    out = cc.model_of(sc)
    g = np.floor(out['e'][mid]).astype(int)
    assert out['N'][mid] == 6 and out['hit'].ravel()[mid] == (g[2] * px + (px - 1 - g[1])) * px + g[0] == (1 * px + (px - 1 - 8)) * px + 8
    assert out['depth'].ravel()[mid] == np.float32(5.5) and (out['e'][:, 0] == 8.5).all()
    out = cc.model_of(cc.scene('too_long', px, nz, W, H))
    assert out['stats'].tolist() == [W * H, 0, 0, W * H, 0] and not out['visible'].any() and (out['hit'] == -1).all()
    out = cc.model_of(cc.scene('not_finite', px, nz, W, H))
    assert out['stats'].tolist() == [W * H, 0, W * H, 0, 0] and not out['visible'].any()


def test_marking_into_what_is_there_is_the_union():
    a, b = cc.scene('random', 16, 4, 24, 16), cc.scene('outside_in', 16, 4, 24, 16)
    b['grid'], b['labels'] = a['grid'], a['labels']
    b['C'] = np.array([-14., -6., 0.5])
    va, vb = cc.model_of(a)['visible'], cc.model_of(b)['visible']
    both = cc.model_of(b, visible=va)
    assert np.array_equal(both['visible'], va | vb) and (va & ~vb).any() and (vb & ~va).any()
    assert np.array_equal(both['hit'], cc.model_of(b)['hit'])
