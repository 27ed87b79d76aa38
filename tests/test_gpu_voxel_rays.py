"""GPU: lidar rays cast through the voxel grid (pca_bev_voxel_rays, DeviceStore.bev_voxel_rays,
SemBEVGenerator.voxel_rays_device, SemanticPointCloudAccumulator.voxel_occupancy) against the numpy model of
tests/voxel_rays_common.py (pinned by tests/test_voxel_rays_model.py).  Every comparison is exact; every input is a valid
call or a refused one."""
import ctypes as C
import re

import numpy as np
import pytest

import voxel_labels_common as vc
import voxel_rays_common as rc
from test_gpu_kernels import T  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, frames_of, kitti_accumulator, loaded, owe, params

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1), (8, 5), (20, 32), (64, 32), (64, 7)]
ORIGIN, VIEW = (0.3, -0.2, 0.125), 40.
SENSORS = np.array([[1.0, 2.0, 0.5], [-8.0, 5.0, 1.0], [30.0, -3.0, 0.75]])      # the third one lies outside the view


_wants = {}


def want_of(key, *args):
    """The model's result for a case that several tests share, computed once."""
    if key not in _wants:
        _wants[key] = rc.model(*args)
    return _wants[key]


# ---------------------------------------------------------------------------------------------- 1: the model, small shapes
@pytest.mark.parametrize('px,nz', SHAPES)
def test_seen_and_stats_equal_the_model(T, px, nz):
    """A rotated and shifted view, three sensors (one outside the view), include_dyn both ways."""
    frames = frames_of(1)
    R, dx, dy = rc.rotation(0.4), 0.5, -0.25
    st = loaded(frames)
    for include_dyn in (False, True):
        out = st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.125, nz, SENSORS, include_dyn=include_dyn)
        want = want_of(('rot', px, nz, include_dyn), frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, include_dyn)
        rc.compare(out, want)
        assert want['stats'][1] == want['stats'][0] > 9500 and want['N'].max() < 300
        assert want['seen'].any() and (px < 64 or not want['seen'].all())
    st.check_status()


@pytest.mark.parametrize('store', ['0', '1'])
def test_few_workgroups_walk_the_window_in_rounds(T, monkeypatch, store):
    """PCA_BEV_RAYS_G=3: three workgroups take the 47 chunks of the window in 16 rounds, across the frame borders (by default a
    window below 524 288 points is one round).  PCA_BEV_RAYS_STORE=1, the A/B form whose marks store without the load in
    front, gives the same result."""
    monkeypatch.setenv('PCA_BEV_RAYS_G', '3')
    monkeypatch.setenv('PCA_BEV_RAYS_STORE', store)
    frames, px, nz = frames_of(1), 64, 32
    R, dx, dy = rc.rotation(0.4), 0.5, -0.25
    st = loaded(frames)
    out = st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.125, nz, SENSORS)
    rc.compare(out, want_of(('rot', px, nz, False), frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, False))
    st.check_status()


@pytest.mark.parametrize('turn', [0, 1])
def test_exact_ties_on_a_lattice(T, turn):
    """x, y, z, the sensors and the origin on a 1/1024 lattice, view 40, px 20 (cells of 2 m), z_step 1/8, R the identity and
    the exact quarter turn: rays through cell edges and corners, where two or three tMax are EQUAL and the order of the axes
    decides which voxels are marked."""
    rng = np.random.default_rng(7)
    frames = []
    for _ in range(3):
        f = rc.random_rows(rng, 4000, 25.)
        f[:, 0:2] = np.rint(f[:, 0:2] * 2) / 2                    # (points of the 1/1024 lattice; coarse, so that ties are
        f[:, 2] = np.rint(f[:, 2] * 32) / 32                      #  frequent: quarters of a cell and of a height bin)
        frames.append(f)
    sensors = np.array([[1.0, 2.0, 0.5], [-8.0, 5.0, 1.0], [30.0, -3.0, 0.75]])
    R = np.eye(3) if turn == 0 else np.array([[0., -1., 0.], [1., 0., 0.], [0., 0., 1.]])
    origin, dx, dy, px, nz = (0.5, -0.5, 0.125), 0.5, -0.5, 20, 32
    st = loaded(frames)
    out = st.bev_voxel_rays(params(origin, R, dx, dy, VIEW, px), -1., 0.125, nz, sensors)
    want = rc.model(frames, sensors, origin, R, dx, dy, VIEW, px, -1., 0.125, nz, False)
    rc.compare(out, want)
    assert want['ties'] > 3000                                    # (the case cannot silently go soft)
    st.check_status()


# ---------------------------------------------------------------------------------------------- 2: owed transforms
@pytest.mark.parametrize('ends', [(2, ), (1, 2, 2, 3)])
def test_owed_chain_over_part_of_the_window(T, ends):
    from test_gpu_kernels import _tilting_transform
    frames = frames_of(2)
    R, dx, dy, px, nz = rc.rotation(-0.7), -0.5, 0.25, 64, 32
    prm = params(ORIGIN, R, dx, dy, VIEW, px, 2.5)
    lazy, plain, twin = loaded(frames), loaded(frames), loaded(frames)
    for st in (lazy, plain, twin):
        st.CHAIN_K = 4
        for step, e in enumerate(ends):
            owe(st, _tilting_transform(step), e)
    eager = twin.frame_rows()                                    # K2 writes the transforms into the twin's store
    assert not twin._pending
    n_rows = sum(f.shape[0] for f in frames)
    before = [t[:n_rows].clone() for t in lazy._arrays()]
    pending = [(np.array(Tm).copy(), e) for Tm, e in lazy._pending]
    got = lazy.bev_voxel_rays(prm, -1., 0.125, nz, SENSORS)
    want = rc.model(eager, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, False)
    rc.compare(got, want)
    rc.compare(twin.bev_voxel_rays(prm, -1., 0.125, nz, SENSORS), want)
    assert not np.array_equal(want['seen'], rc.model(frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, False)['seen'])
    assert len(lazy._pending) == len(ends)                       # still owed, and the same list
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(pending, lazy._pending))
    assert all(T.equal(a, b[:n_rows]) for a, b in zip(before, lazy._arrays()))       # no store column was written
    assert not T.equal(lazy.z[:n_rows], twin.z[:n_rows])
    # a main raster after the call is the one made without it, bit for bit
    a16, a64 = lazy.bev(2, prm, want_f64=True)
    b16, b64 = plain.bev(2, prm, want_f64=True)
    assert T.equal(a16.view(T.int16), b16.view(T.int16)) and T.equal(a64.view(T.int64), b64.view(T.int64))
    assert all(T.equal(a[:n_rows], b[:n_rows]) for a, b in zip(lazy._arrays(), plain._arrays()))
    for st in (lazy, plain, twin):
        st.check_status()


# ---------------------------------------------------------------------------------------------- 3: frames and points
def test_empty_frame_nan_origin_and_non_finite_heights(T):
    rng = np.random.default_rng(11)
    a, b, c = rc.random_rows(rng, 3000, 25.), rc.random_rows(rng, 2000, 25.), rc.random_rows(rng, 1500, 25.)
    b[::50, 2], b[1::50, 2], b[2::50, 2] = np.nan, np.inf, -np.inf
    frames = [a, np.zeros((0, 10)), b, np.zeros((0, 10)), np.zeros((0, 10)), c]
    sensors = np.array([[1., 2., 0.5], [0., 0., 0.], [-8., 5., 1.], [3., 3., 3.], [4., 4., 4.], [2., np.nan, 0.75]])
    R, dx, dy, px, nz = rc.rotation(1.3), 0.25, 0.5, 20, 32
    st = loaded(frames)
    out = st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.125, nz, sensors, include_dyn=True)
    want = rc.model(frames, sensors, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, True)
    rc.compare(out, want)
    assert want['stats'].tolist() == [6500, 6500 - 1500 - 120, 1500 + 120, 0]
    # the window of the empty frames alone, and of no frame at all: all zeros
    for f0, f1 in ((3, 5), (2, 2)):
        out = st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.125, nz, sensors[f0:f1], first_frame=f0, last_frame=f1)
        assert not out['seen'].any().item() and out['stats'].tolist() == [0, 0, 0, 0]
    # frames 2 .. 5 with their own sensors
    out = st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.125, nz, sensors[2:], first_frame=2, include_dyn=True)
    rc.compare(out, rc.model(frames[2:], sensors[2:], ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, True))
    with pytest.raises(ValueError, match='origins'):
        st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.125, nz, sensors[:3])
    st.check_status()


def test_the_step_cap_on_the_device(T):
    """Cells of 1 m (view 64, px 64, identity): a sensor 16 384 cells from its point casts a ray of exactly
    PCA_BEV_RAYS_MAX_STEPS steps, one 16 385 cells away is one over: counted in stats[3], nothing marked by it."""
    def row(x, y, z):
        r = np.zeros(10)
        r[0:3] = x, y, z
        return r
    frames = [np.array([row(0.5, 3.5, 0.5)]), np.array([row(0.5, -7.5, 1.5)]), np.array([row(-2.5, 9.5, 2.5)])]
    sensors = np.array([[0.5 + rc.MAX_STEPS, 3.5, 0.5], [1.5 + rc.MAX_STEPS, -7.5, 1.5], [-2.5, 9.5 - (rc.MAX_STEPS - 2), 0.5]])
    px, nz = 64, 4
    st = loaded(frames, capacity=1024)
    out = st.bev_voxel_rays(params((0., 0., 0.), np.eye(3), 0., 0., 64., px), 0., 1., nz, sensors)
    want = rc.model(frames, sensors, (0., 0., 0.), np.eye(3), 0., 0., 64., px, 0., 1., nz, False)
    assert want['N'].tolist() == [rc.MAX_STEPS, -1, rc.MAX_STEPS] and want['stats'].tolist() == [3, 2, 0, 1]   # (the third: v and w)
    rc.compare(out, want)
    seen = out['seen'].cpu().numpy()
    assert seen[0, px - 1 - 35, 33:].all() and not seen[0, px - 1 - 35, :33].any()      # the first ray, up to its end voxel
    assert not seen[1].any()                                      # the second one marked nothing
    st.check_status()


def test_window_above_max_points_is_cut_and_says_so(T):
    from pca_amd import _lib
    frames = frames_of(1)
    R, dx, dy, px, nz = rc.rotation(0.3), 0., 0., 20, 5
    st = loaded(frames)
    cut = 6700                                                    # inside the second frame
    out = st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.5, nz, SENSORS, max_points=cut)
    want = rc.model(frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.5, nz, False, max_points=cut)
    rc.compare(out, want)
    assert st.ctx.status() == _lib.STATUS_STORE_OVERFLOW         # (read and cleared here)
    whole = st.bev_voxel_rays(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.5, nz, SENSORS)
    assert whole['stats'][0].item() > out['stats'][0].item() > 5000
    st.check_status()


# ---------------------------------------------------------------------------------------------- 4: the C ABI's checks
def raw_call(st, prm, max_points=20000, z_lo=-1., z_step=0.5, nz=4, origins=True, outputs=(True, True), pending=None,
             slots=None):
    """pca_bev_voxel_rays itself; returns (rc, message, seen, stats)."""
    import torch
    ctx, lib = st.ctx, st.ctx.lib
    px = min(max(int(prm.px), 1), 64)
    seen = torch.full((32, px, px), 7, dtype=torch.uint8, device=st.device)   # (a refused call writes nothing)
    stats = torch.full((4, ), 7, dtype=torch.int64, device=st.device)
    org = torch.from_numpy(SENSORS[:st.n_frames].copy()).to(st.device)
    store = st.c_store()
    b, e = (st.head, st.head + st.n_frames) if slots is None else slots
    if pending is None:
        pT, pE, nP = None, None, 0
    else:
        Ts, ends, nP = pending
        pT = None if Ts is None else (C.c_double * len(Ts))(*Ts)
        pE = None if ends is None else (C.c_int * len(ends))(*ends)
    r = lib.pca_bev_voxel_rays(ctx.h, C.byref(store), st.frame_off.data_ptr(), b, e, max_points, C.byref(prm), z_lo, z_step, nz, 0,
                               org.data_ptr() if origins else None, pT, pE, nP, seen.data_ptr() if outputs[0] else None,
                               stats.data_ptr() if outputs[1] else None, ctx.stream())
    torch.cuda.synchronize()
    return r, lib.pca_last_error(ctx.h).decode(), seen, stats


def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    frames = frames_of(1)
    R, px = rc.rotation(0.3), 32
    st = loaded(frames)
    prm = params(ORIGIN, R, 0., 0., VIEW, px)
    ctx = st.ctx
    r, _, seen, stats = raw_call(st, prm)                         # the call as such is fine
    assert r == 0 and (seen[:4] <= 1).all().item() and seen[:4].any().item() and (seen[4:] == 7).all().item()
    assert stats.tolist()[1:] == [stats[0].item(), 0, 0] and stats[0].item() > 9000
    r, _, seen, stats = raw_call(st, prm, outputs=(True, False))  # either output alone
    assert r == 0 and seen[:4].any().item() and (stats == 7).all().item()
    r, _, seen, stats = raw_call(st, prm, outputs=(False, True))
    assert r == 0 and (seen == 7).all().item() and stats[0].item() > 9000
    ctx.profile(1)
    bad_R = np.array([[1., 0., 0.], [0., np.cos(0.1), -np.sin(0.1)], [0., np.sin(0.1), np.cos(0.1)]])
    eye = [float(v) for v in np.eye(4).reshape(-1)]
    nan, inf = float('nan'), float('inf')
    h = st.head
    cases = [(dict(prm=params(ORIGIN, R, 0., 0., VIEW, 1025)), r'bev voxel rays: px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, R, 0., 0., VIEW, 0)), r'bev voxel rays: px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, bad_R, 0., 0., VIEW, px)), 'bev voxel rays: R must be a rotation about the z axis'),
             (dict(outputs=(False, False)), 'bev voxel rays: bad arguments'),
             (dict(origins=False), 'bev voxel rays: bad arguments'),
             (dict(slots=(h + 2, h + 1)), 'bev voxel rays: need slot_begin <= slot_end'),
             (dict(pending=(eye * 5, [h + 1] * 5, 5)), 'bev voxel rays: bad chain of owed transforms'),
             (dict(pending=(None, None, 1)), 'bev voxel rays: bad chain of owed transforms'),
             (dict(pending=(eye, [h + 4], 1)), 'bev voxel rays: a pending slot end lies beyond the window'),
             (dict(pending=(eye * 2, [h + 2, h + 1], 2)), 'bev voxel rays: pending slot ends must ascend')]
    cases += [(dict(nz=v), r'bev voxel rays: nz must be in 1\.\.32') for v in (0, -1, 33)]
    cases += [(dict(z_lo=v), 'bev voxel rays: z_lo must be finite') for v in (nan, inf, -inf)]
    cases += [(dict(z_step=v), 'bev voxel rays: z_step must be finite and > 0') for v in (0., -0.5, nan, inf)]
    for bad, msg in cases:
        args = dict(prm=prm)
        args.update(bad)
        r, err, seen, stats = raw_call(st, **args)
        assert r == -1 and re.match(msg, err), (err, msg)
        assert (seen == 7).all().item() and (stats == 7).all().item(), msg
    with pytest.raises(RuntimeError, match=r'bev voxel rays: nz must be in 1\.\.32'):
        st.bev_voxel_rays(prm, -1., 0.5, 33, SENSORS)
    with pytest.raises(RuntimeError, match='z_step must be finite and > 0'):
        st.bev_voxel_rays(prm, -1., 0., 4, SENSORS)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['bev_voxel_rays'][1] == 0
    st.check_status()


# ---------------------------------------------------------------------------------------------- 5: the top level
def test_generator_forms_and_voxel_occupancy_on_a_kitti_sequence(T, tmp_path):
    from pca_amd import host_logic as hl
    acc, idx = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14), 9
    gen = acc.sem_bev_generator
    z_range, nz, classes = (-2.0, 4.4), 32, [[0, 1, 2], [13, 14, 15, 17], [5], [8, 9]]
    frames = acc.sem_pcs
    poses = np.array(acc.poses)
    origin = poses[idx]
    R = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:idx] - origin))
    view, px, hf = 1. * gen.view_size, gen.pixel_size, gen.height_filter
    table, n_labels = vc.table_of(classes)
    z_step = (z_range[1] - z_range[0]) / nz
    lifted = poses + np.array([0., 0., 1.5])                      # a sensor that does not sit at the pose
    for part, sl, sensors in (('full', slice(0, None), None), ('present', slice(0, idx), None), ('future', slice(idx, None), lifted)):
        rows, org = frames[sl], (poses if sensors is None else sensors)[sl]
        out = acc.voxel_occupancy(idx, part=part, z_range=z_range, nz=nz, classes=classes,
                                  origins=None if sensors is None else sensors[sl])
        assert sorted(out) == ['counts', 'labels', 'seen', 'state', 'stats', 'top']
        labels = acc.voxel_labels(idx, part=part, z_range=z_range, nz=nz, classes=classes)
        assert all(T.equal(out[k], labels[k]) for k in ('labels', 'counts', 'top')), part
        want_l = vc.model(np.concatenate(rows), origin, R, 0., 0., view, px, hf, z_range[0], z_step, nz, table, n_labels, False)
        want_r = rc.model(rows, org, origin, R, 0., 0., view, px, z_range[0], z_step, nz, False)
        rc.compare({k: out[k] for k in ('seen', 'stats')}, want_r)
        state = out['state'].cpu().numpy()
        assert state.dtype == np.uint8 and np.array_equal(state, rc.state_of(want_l['counts'], want_r['seen'])), part
        assert all((state == v).sum() > 50 for v in (0, 1, 2)), part
        # the generator: host rows per frame in BEV-frame metres, one origin each, equal the window form
        rel = [f.copy() for f in rows]
        for f in rel:
            f[:, 0:3] -= origin
        host = gen.voxel_rays_device(rel, org - origin, R, 0., 0., view, z_range, nz)
        assert T.equal(host['seen'], out['seen']) and T.equal(host['stats'], out['stats']), part
    with pytest.raises(ValueError):
        acc.voxel_occupancy(idx, part='past')
    with pytest.raises(ValueError, match='origins'):
        acc.voxel_occupancy(idx, part='present', origins=poses)   # one origin per frame of the part
    with pytest.raises(ValueError, match='per-frame'):
        gen.voxel_rays_device(np.concatenate(frames), poses, R, 0., 0., view, z_range, nz)
    acc.store.check_status()
