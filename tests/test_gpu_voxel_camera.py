"""GPU: camera rays cast through the voxel grid (pca_bev_voxel_camera, DeviceStore.bev_voxel_camera,
SemBEVGenerator.voxel_camera_device, SemanticPointCloudAccumulator.voxel_visibility) against the numpy model of
tests/voxel_camera_common.py (pinned by tests/test_voxel_camera_model.py, which also shows that every case here is what its
name says).  Every comparison is exact; every input is a valid call or a refused one."""
import ctypes as C
import re

import numpy as np
import pytest

import voxel_camera_common as cc
from test_gpu_kernels import T, dev_store  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, kitti_accumulator, params

pytestmark = pytest.mark.gpu

SHAPES = [(16, 4, 24, 16), (32, 8, 65, 33)]
CASES = ['inside_occupied', 'outside_in', 'outside_away', 'axis_parallel', 'diagonal_ties', 'ends_inside', 'too_long', 'not_finite']

_wants = {}


def want_of(name, *shape):
    """(scene, model's result) of a case that several tests share, computed once and never changed."""
    if (name, ) + shape not in _wants:
        sc = cc.scene(name, *shape)
        _wants[(name, ) + shape] = (sc, cc.model_of(sc))
    return _wants[(name, ) + shape]


def prm_of(grid):
    return params(grid['origin'], grid['R'], grid['dx'], grid['dy'], grid['view'], grid['px'])


def raw_call(T, sc, clear=1, into=None, outputs=(True, True, True), **bad):
    """pca_bev_voxel_camera itself on scene `sc`; bad: arguments replaced (prm, nz, z_lo, z_step, width, height, stride,
    max_depth, Minv, C, and labels / cam / visible / stats = None for a null pointer).  The outputs start out filled with 7 (a
    refused call writes nothing; `into`: the marks the call finds in `visible`).  Returns (rc, message, visible, hit, depth, label,
    stats) as numpy arrays."""
    from pca_amd import _lib
    ctx = _lib.Context.get()
    g = sc['grid']
    px, nz = g['px'], g['nz']
    nu, nv = sc['W'] // sc['stride'], sc['H'] // sc['stride']
    labels = T.from_numpy(sc['labels']).cuda()
    vis = T.full((nz, px, px), 7, dtype=T.uint8, device='cuda') if into is None else T.from_numpy(into.copy()).cuda()
    hit = T.full((nv, nu), 7, dtype=T.int32, device='cuda')
    depth = T.full((nv, nu), 7, dtype=T.float32, device='cuda')
    label = T.full((nv, nu), 7, dtype=T.uint8, device='cuda')
    stats = T.full((5, ), 7, dtype=T.int64, device='cuda')
    cam = _lib.PcaRayCamera()
    cam.Minv[:] = np.asarray(bad.get('Minv', sc['Minv']), dtype=np.float64).reshape(9).tolist()
    cam.C[:] = np.asarray(bad.get('C', sc['C']), dtype=np.float64).reshape(3).tolist()
    cam.width, cam.height, cam.stride = bad.get('width', sc['W']), bad.get('height', sc['H']), bad.get('stride', sc['stride'])
    cam.clear, cam.max_depth = clear, bad.get('max_depth', sc['max_depth'])
    prm = bad.get('prm', prm_of(g))
    ptr = {k: (None if k in bad else t.data_ptr()) for k, t in (('labels', labels), ('visible', vis), ('stats', stats))}
    r = ctx.lib.pca_bev_voxel_camera(ctx.h, None if prm is None else C.byref(prm), bad.get('z_lo', g['z_lo']),
                                     bad.get('z_step', g['z_step']), bad.get('nz', nz), ptr['labels'],
                                     None if 'cam' in bad else C.byref(cam), ptr['visible'],
                                     hit.data_ptr() if outputs[0] else None, depth.data_ptr() if outputs[1] else None,
                                     label.data_ptr() if outputs[2] else None, ptr['stats'], ctx.stream())
    T.cuda.synchronize()
    return (r, ctx.lib.pca_last_error(ctx.h).decode()) + tuple(t.cpu().numpy() for t in (vis, hit, depth, label, stats))


def same(got, want):
    """raw_call's result against the model's, everything exact."""
    r, err, vis, hit, depth, label, stats = got
    assert r == 0, err
    assert stats.tolist() == want['stats'].tolist(), (stats, want['stats'])
    assert np.array_equal(vis, want['visible']), int((vis != want['visible']).sum())
    assert np.array_equal(hit, want['hit']), int((hit != want['hit']).sum())
    assert np.array_equal(depth.view(np.uint32), want['depth'].view(np.uint32)) and np.array_equal(label, want['label'])


# ---------------------------------------------------------------------------------------------- 1: the model, small shapes
@pytest.mark.parametrize('px,nz,W,H', SHAPES)
@pytest.mark.parametrize('stride', [1, 3])
def test_marks_hits_and_stats_equal_the_model(T, monkeypatch, px, nz, W, H, stride):
    """A rotated and shifted grid, a camera inside it; by default, with ONE workgroup going round its loop for all the rays
    (PCA_BEV_CAMERA_G=1), and in the plain form and the other depths of the look-ahead (PCA_BEV_CAMERA_DEPTH)."""
    sc, want = want_of('random', px, nz, W, H, stride)
    same(raw_call(T, sc), want)
    monkeypatch.setenv('PCA_BEV_CAMERA_G', '1')
    same(raw_call(T, sc), want)
    monkeypatch.delenv('PCA_BEV_CAMERA_G')
    for depth in ('1', '2', '8'):
        monkeypatch.setenv('PCA_BEV_CAMERA_DEPTH', depth)
        same(raw_call(T, sc), want)


@pytest.mark.parametrize('name', CASES)
def test_camera_cases(T, monkeypatch, name):
    """The camera in an occupied voxel, outside the grid looking in and looking away, rays parallel to the axes, exact ties
    of tMax on a diagonal, rays that end inside the grid with a hit in the end voxel, and the two drop rules."""
    sc, want = want_of(name, 16, 4, 65, 33)
    same(raw_call(T, sc), want)
    monkeypatch.setenv('PCA_BEV_CAMERA_DEPTH', '1')
    same(raw_call(T, sc), want)


# ---------------------------------------------------------------------------------------------- 2: several cameras, absent outputs
def test_clear_0_marks_into_what_is_there(T):
    a, wa = want_of('random', 16, 4, 24, 16)
    b = dict(cc.scene('outside_in', 16, 4, 24, 16), grid=a['grid'], labels=a['labels'], C=np.array([-14., -6., 0.5]))
    wb = cc.model_of(b)
    assert (wa['visible'] & ~wb['visible']).any() and (wb['visible'] & ~wa['visible']).any()
    got = raw_call(T, b, clear=0, into=wa['visible'])
    same(got, dict(wb, visible=wa['visible'] | wb['visible']))


def test_two_cameras_through_the_store_give_the_union(T):
    """DeviceStore.bev_voxel_camera: two cameras (P, size) into one 'visible', per-camera rays; labels as a numpy array and
    as a cuda tensor."""
    sc, _ = want_of('random', 16, 4, 24, 16)
    g = sc['grid']
    cams = [(cc.look_at((-9., 2., 1.5), (8., -3., 0.5), 14., 24, 16), (24, 16)),
            (cc.look_at((12., 9., 0.5), (-5., -8., 1.), 30., 65, 33), (65, 33))]
    st = dev_store(capacity=1024, max_frames=2)
    wants, union = [], np.zeros_like(sc['labels'])
    for P, (W, H) in cams:
        Minv, Cc = cc.camera_of(P)
        wants.append(cc.model(sc['labels'], Minv, Cc, W, H, 3, 25., **g))
        union |= wants[-1]['visible']
    assert all((w['visible'] != union).any() for w in wants)
    for labels in (sc['labels'], T.from_numpy(sc['labels']).cuda()):
        out = st.bev_voxel_camera(prm_of(g), g['z_lo'], g['z_step'], g['nz'], labels, cams, stride=3, max_depth=25.)
        assert sorted(out) == ['depth', 'hit', 'label', 'stats', 'visible'] and tuple(out['stats'].shape) == (2, 5)
        assert out['visible'].dtype == T.uint8 and np.array_equal(out['visible'].cpu().numpy(), union)
        for n, want in enumerate(wants):
            cc.compare(out, want, n)
    one = st.bev_voxel_camera(prm_of(g), g['z_lo'], g['z_step'], g['nz'], sc['labels'], cams[1:], stride=3, max_depth=25.)
    assert np.array_equal(one['visible'].cpu().numpy(), wants[1]['visible'])
    with pytest.raises(ValueError, match='labels'):
        st.bev_voxel_camera(prm_of(g), g['z_lo'], g['z_step'], g['nz'], sc['labels'][:2], cams)
    with pytest.raises(RuntimeError, match='bev voxel camera: stride'):
        st.bev_voxel_camera(prm_of(g), g['z_lo'], g['z_step'], g['nz'], sc['labels'], cams, stride=17)
    st.check_status()


@pytest.mark.parametrize('outputs', [(False, False, False), (True, False, False), (False, True, False), (False, False, True)])
def test_absent_per_ray_outputs(T, outputs):
    sc, want = want_of('random', 16, 4, 24, 16)
    r, err, vis, hit, depth, label, stats = raw_call(T, sc, outputs=outputs)
    assert r == 0, err
    assert np.array_equal(vis, want['visible']) and stats.tolist() == want['stats'].tolist()
    for on, a, k in zip(outputs, (hit, depth, label), ('hit', 'depth', 'label')):
        assert np.array_equal(a, want[k]) if on else (a == 7).all(), k


# ---------------------------------------------------------------------------------------------- 3: the C ABI's checks
def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    from pca_amd import _lib
    sc, want = want_of('random', 16, 4, 24, 16)
    g = sc['grid']
    ctx = _lib.Context.get()
    ctx.profile(1)
    nan, inf = float('nan'), float('inf')
    bad_R = np.array([[1., 0., 0.], [0., np.cos(0.1), -np.sin(0.1)], [0., np.sin(0.1), np.cos(0.1)]])

    def with_entry(key, at, v):
        a = np.array(sc[key], dtype=np.float64)
        a.flat[at] = v
        return {key: a}

    cases = [(dict(prm=None), 'bev voxel camera: prm must not be NULL'),
             (dict(labels=None), 'bev voxel camera: labels must not be NULL'),
             (dict(cam=None), 'bev voxel camera: cam must not be NULL'),
             (dict(visible=None), 'bev voxel camera: visible must not be NULL'),
             (dict(stats=None), 'bev voxel camera: stats must not be NULL'),
             (dict(width=0), 'bev voxel camera: width and height must be >= 1'),
             (dict(height=-3), 'bev voxel camera: width and height must be >= 1'),
             (dict(stride=0), r'bev voxel camera: stride must be in 1\.\.min\(width, height\)'),
             (dict(stride=17), r'bev voxel camera: stride must be in 1\.\.min\(width, height\)'),
             (dict(prm=params(g['origin'], g['R'], 0., 0., g['view'], 1025)), r'bev voxel camera: px must be in 1\.\.1024'),
             (dict(prm=params(g['origin'], g['R'], 0., 0., g['view'], 0)), r'bev voxel camera: px must be in 1\.\.1024'),
             (dict(prm=params(g['origin'], bad_R, 0., 0., g['view'], 16)), 'bev voxel camera: R must be a rotation about the z axis')]
    cases += [(dict(max_depth=v), 'bev voxel camera: max_depth must be finite and > 0') for v in (0., -1., nan, inf)]
    cases += [(with_entry('Minv', at, v), 'bev voxel camera: every entry of Minv must be finite') for at, v in ((0, nan), (8, inf), (4, -inf))]
    cases += [(with_entry('C', at, v), 'bev voxel camera: every entry of C must be finite') for at, v in ((0, nan), (2, inf))]
    cases += [(dict(nz=v), r'bev voxel camera: nz must be in 1\.\.32') for v in (0, -1, 33)]
    cases += [(dict(z_lo=v), 'bev voxel camera: z_lo must be finite') for v in (nan, inf, -inf)]
    cases += [(dict(z_step=v), 'bev voxel camera: z_step must be finite and > 0') for v in (0., -0.5, nan, inf)]
    for bad, msg in cases:
        r, err, vis, hit, depth, label, stats = raw_call(T, sc, **bad)
        assert r == -1 and re.match(msg, err), (err, msg)
        assert all((a == 7).all() for a in (vis, hit, depth, label, stats)), msg
    prof = ctx.profile_read()
    assert prof['bev_camera_rays'][1] == 0
    same(raw_call(T, sc), want)                                   # the call as such is fine, and its launch is counted
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['bev_camera_rays'][1] == 1 and prof['bev_voxel_rays'][1] == 0


# ---------------------------------------------------------------------------------------------- 4: the top level
def test_voxel_visibility_on_a_kitti_sequence(T, tmp_path, monkeypatch):
    from pca_amd import host_logic as hl
    acc, idx = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14), 9
    gen = acc.sem_bev_generator
    z_range, nz, classes = (-2.0, 4.4), 32, [[0, 1, 2], [13, 14, 15, 17], [5], [8, 9]]
    poses = np.array(acc.poses)
    origin = poses[idx]
    R = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:idx] - origin))
    view, px = 1. * gen.view_size, gen.pixel_size
    grid = dict(origin=origin, R=R, dx=0., dy=0., view=view, px=px, z_lo=z_range[0], z_step=(z_range[1] - z_range[0]) / nz, nz=nz)
    P, (W, H) = acc._render_defaults()
    assert (W, H) == (96, 64)
    Minv, Cc = cc.camera_of(np.asarray(P, dtype=np.float64)[:3])
    occ = acc.voxel_occupancy(idx, z_range=z_range, nz=nz, classes=classes)
    before = [t.clone() for t in acc.store._arrays()]
    # the default camera, every pixel
    out = acc.voxel_visibility(idx, z_range=z_range, nz=nz, classes=classes)
    assert sorted(out) == sorted(list(occ) + ['visible', 'hit', 'depth', 'label', 'camera_stats'])
    assert all(T.equal(out[k], occ[k]) for k in occ)
    # nothing was written to the store (bytes: rows behind the stored points hold whatever the allocation held, NaN included)
    assert all(T.equal(a.view(T.uint8), b.view(T.uint8)) for a, b in zip(before, acc.store._arrays()))
    labels = out['labels'].cpu().numpy()
    want = cc.model(labels, Minv, Cc, W, H, 1, view, **grid)
    assert want['stats'][4] > 0.1 * W * H and want['stats'][1] == W * H and 0 < want['visible'].sum() < want['visible'].size
    assert np.array_equal(out['visible'].cpu().numpy(), want['visible'])
    cc.compare(dict(out, stats=out['camera_stats']), want)
    # two cameras, every second pixel, a shorter reach: the default one and one that looks the other way
    back = cc.look_at(origin + np.array([0., 0., 1.]), origin + np.array([-10., 2., 0.]), 40., 65, 33)
    out = acc.voxel_visibility(idx, part='present', z_range=z_range, nz=nz, classes=classes, cameras=[(P, (W, H)), (back, (65, 33))],
                               stride=2, max_depth=12.5)
    labels = out['labels'].cpu().numpy()
    wants = [cc.model(labels, Minv, Cc, W, H, 2, 12.5, **grid), cc.model(labels, *cc.camera_of(back), 65, 33, 2, 12.5, **grid)]
    assert np.array_equal(out['visible'].cpu().numpy(), wants[0]['visible'] | wants[1]['visible'])
    assert wants[1]['visible'].any() and (wants[1]['visible'] & ~wants[0]['visible']).any()
    for n, want in enumerate(wants):
        cc.compare(dict(out, stats=out['camera_stats']), want, n)
    # the generator's form with the cameras in BEV-frame metres equals the window's
    Pm = np.asarray(P, dtype=np.float64)[:3].copy()
    Pm[:, 3] += Pm[:, :3] @ origin
    host = gen.voxel_camera_device(None, labels, [(Pm, (W, H))], R, 0., 0., view, z_range, nz, stride=2, max_depth=12.5)
    want = cc.model(labels, *cc.camera_of(Pm), W, H, 2, 12.5, **dict(grid, origin=np.zeros(3)))
    assert np.array_equal(host['visible'].cpu().numpy(), want['visible']) and want['stats'][4] > 0
    cc.compare(host, want)
    # a dataset without a camera of its own needs `cameras`
    monkeypatch.setattr(acc, '_render_defaults', lambda: (None, None))
    with pytest.raises(ValueError, match='cameras'):
        acc.voxel_visibility(idx, z_range=z_range, nz=nz)
    acc.store.check_status()
