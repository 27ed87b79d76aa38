"""GPU: free-space carving by ray hit / miss (pca_bev_voxel_carve, DeviceStore.bev_voxel_carve,
SemBEVGenerator.voxel_carve_device, SemanticPointCloudAccumulator.carve_dynamic) against the numpy model of
tests/voxel_carve_common.py (pinned by tests/test_voxel_carve_model.py).  Every comparison is exact; every input is a valid call
or a refused one."""
import ctypes as C
import re

import numpy as np
import pytest

import voxel_carve_common as cc
import voxel_rays_common as rc
from test_gpu_kernels import DYNOBJ, T  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, frames_of, kitti_accumulator, loaded, owe, params

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1), (8, 5), (20, 32), (64, 32), (64, 7)]
RULES = [(1, 2, 1.0), (2, 3, 2.0)]                               # (end_margin, min_cross, ratio)
ORIGIN, VIEW = (0.3, -0.2, 0.125), 40.
SENSORS = np.array([[1.0, 2.0, 0.5], [-8.0, 5.0, 1.0], [30.0, -3.0, 0.75]])      # the third one lies outside the view
ROT = (rc.rotation(0.4), 0.5, -0.25)                             # the rotated and shifted view of the rays tests


def z_step_of(nz):
    """Bins of 1/8 m as in the rays tests; the thin grids of one and of five bins get bins of 1/2 m, or too few points end
    inside them for the floors below (23 candidates at (5, 1) with 1/8 m)."""
    return 0.125 if nz >= 7 else 0.5


_wants = {}


def want_of(key, *args, **kw):
    """The model's result for a case that several tests share, computed once."""
    if key not in _wants:
        _wants[key] = cc.model(*args, **kw)
    return _wants[key]


def counts_of(want):
    """(flagged, kept) candidates and (cross, hits) of every candidate point's voxel."""
    f = want['flags']
    place = want['place'][f != 255]
    return int((f == 1).sum()), int((f == 0).sum()), want['cross'].ravel()[place], want['hits'].ravel()[place]


# ---------------------------------------------------------------------------------------------- 1: the model, small shapes
@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('px,nz', SHAPES)
def test_counts_flags_and_stats_equal_the_model(T, px, nz, rule):
    frames = frames_of(1)
    R, dx, dy = ROT
    st = loaded(frames)
    for include_dyn in (False, True):
        out = st.bev_voxel_carve(params(ORIGIN, R, dx, dy, VIEW, px), -1., z_step_of(nz), nz, SENSORS, DYNOBJ, *rule,
                                 include_dyn=include_dyn)
        want = want_of(('rot', px, nz, include_dyn, rule), frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., z_step_of(nz), nz,
                       include_dyn, DYNOBJ, *rule)
        flagged, kept, cross, hits = counts_of(want)
        print(f'px {px} nz {nz} rule {rule} include_dyn {include_dyn}: flagged {flagged}, kept {kept}, '
              f'cross == min_cross {(cross == rule[1]).sum()}, cross == ratio hits {(cross == rule[2] * hits).sum()}')
        assert flagged >= 50 and kept >= 10                       # (the case cannot go soft)
        if (px, nz) == (20, 32):                                  # both thresholds are met with equality, too
            assert (cross == rule[1]).sum() >= 10 and (cross == rule[2] * hits).sum() >= 10
        cc.compare(out, want)
        assert want['stats'][1] == want['stats'][0] == (12000 if include_dyn else (want['take']).sum())
    st.check_status()


def test_few_workgroups_walk_the_window_in_rounds(T, monkeypatch):
    """PCA_BEV_CARVE_G=3: three workgroups take the 47 chunks of the window in 16 rounds, across the frame borders (by default a
    window below 524 288 points is one round)."""
    monkeypatch.setenv('PCA_BEV_CARVE_G', '3')
    frames, px, nz, rule = frames_of(1), 64, 32, RULES[0]
    R, dx, dy = ROT
    st = loaded(frames)
    out = st.bev_voxel_carve(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.125, nz, SENSORS, DYNOBJ, *rule)
    cc.compare(out, want_of(('rot', px, nz, False, rule), frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, False,
                            DYNOBJ, *rule))
    st.check_status()


@pytest.mark.parametrize('turn', [0, 1])
def test_exact_ties_on_a_lattice(T, turn):
    """The lattice of the rays test: x, y, z, the sensors and the origin on a 1/1024 lattice, cells of 2 m, z_step 1/8, R the
    identity and the exact quarter turn: two or three tMax are EQUAL and the order of the axes decides which voxels count."""
    rng = np.random.default_rng(7)
    frames = []
    for _ in range(3):
        f = rc.random_rows(rng, 4000, 25.)
        f[:, 0:2] = np.rint(f[:, 0:2] * 2) / 2
        f[:, 2] = np.rint(f[:, 2] * 32) / 32
        frames.append(f)
    R = np.eye(3) if turn == 0 else np.array([[0., -1., 0.], [1., 0., 0.], [0., 0., 1.]])
    origin, dx, dy, px, nz = (0.5, -0.5, 0.125), 0.5, -0.5, 20, 32
    st = loaded(frames)
    out = st.bev_voxel_carve(params(origin, R, dx, dy, VIEW, px), -1., 0.125, nz, SENSORS, DYNOBJ)
    want = cc.model(frames, SENSORS, origin, R, dx, dy, VIEW, px, -1., 0.125, nz, False, DYNOBJ)
    cc.compare(out, want)
    assert rc.traverse(want['s'], want['e'], px, nz)['ties'] > 3000 and counts_of(want)[0] >= 50
    st.check_status()


# ---------------------------------------------------------------------------------------------- 2: owed transforms
def test_owed_chain_over_part_of_the_window(T):
    from test_gpu_kernels import _tilting_transform
    frames, ends = frames_of(2), (1, 2, 2, 3)
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
    got = lazy.bev_voxel_carve(prm, -1., 0.125, nz, SENSORS, DYNOBJ)
    want = cc.model(eager, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, False, DYNOBJ)
    cc.compare(got, want)
    cc.compare(twin.bev_voxel_carve(prm, -1., 0.125, nz, SENSORS, DYNOBJ), want)
    assert not np.array_equal(want['cross'], cc.model(frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, False,
                                                      DYNOBJ)['cross'])
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
def test_empty_frames_nan_origin_non_finite_heights_and_empty_windows(T):
    rng = np.random.default_rng(11)
    a, b, c = rc.random_rows(rng, 3000, 25.), rc.random_rows(rng, 2000, 25.), rc.random_rows(rng, 1500, 25.)
    b[::50, 2], b[1::50, 2], b[2::50, 2] = np.nan, np.inf, -np.inf
    frames = [a, np.zeros((0, 10)), b, np.zeros((0, 10)), np.zeros((0, 10)), c]
    sensors = np.array([[1., 2., 0.5], [0., 0., 0.], [-8., 5., 1.], [3., 3., 3.], [4., 4., 4.], [2., np.nan, 0.75]])
    R, dx, dy, px, nz = rc.rotation(1.3), 0.25, 0.5, 20, 32
    prm = params(ORIGIN, R, dx, dy, VIEW, px)
    st = loaded(frames)
    out = st.bev_voxel_carve(prm, -1., 0.125, nz, sensors, DYNOBJ, include_dyn=True)
    want = cc.model(frames, sensors, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, True, DYNOBJ)
    cc.compare(out, want)
    assert want['stats'][:4].tolist() == [6500, 6500 - 1500 - 120, 1500 + 120, 0] and want['stats'][5] > 50
    assert (want['flags'][5000:] == 255).all()                   # the frame with the NaN origin: no ray, no candidate
    # the window of the empty frames alone, and of no frame at all: zeros, no flags
    for f0, f1 in ((3, 5), (2, 2)):
        out = st.bev_voxel_carve(prm, -1., 0.125, nz, sensors[f0:f1], DYNOBJ, first_frame=f0, last_frame=f1)
        assert not out['hits'].any().item() and not out['cross'].any().item() and out['stats'].tolist() == [0] * 6
        assert out['flags'].shape == (0, )
    # frames 2 .. 5 with their own sensors
    out = st.bev_voxel_carve(prm, -1., 0.125, nz, sensors[2:], DYNOBJ, first_frame=2, include_dyn=True)
    cc.compare(out, cc.model(frames[2:], sensors[2:], ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, True, DYNOBJ))
    with pytest.raises(ValueError, match='origins'):
        st.bev_voxel_carve(prm, -1., 0.125, nz, sensors[:3], DYNOBJ)
    st.check_status()


def row(x, y, z, cls=13.):
    r = np.zeros(10)
    r[0:3], r[7] = (x, y, z), cls
    return r


def test_the_step_cap_and_a_margin_at_or_above_a_rays_steps(T):
    """Cells of 1 m (view 64, px 64, identity).  A sensor 16 384 cells from its point casts a ray of exactly
    PCA_BEV_RAYS_MAX_STEPS steps, one 16 385 cells away is one over: dropped, it counts nowhere and is no candidate.  The first
    ray crosses the voxel of a candidate point of frame 3 (whose own ray has no step)."""
    frames = [np.array([row(0.5, 3.5, 0.5)]), np.array([row(0.5, -7.5, 1.5)]), np.array([row(-2.5, 9.5, 2.5)]),
              np.array([row(10.5, 3.5, 0.5), row(10.25, 3.25, 0.75)])]
    sensors = np.array([[0.5 + rc.MAX_STEPS, 3.5, 0.5], [1.5 + rc.MAX_STEPS, -7.5, 1.5], [-2.5, 9.5 - (rc.MAX_STEPS - 2), 0.5],
                        [10.75, 3.75, 0.25]])
    px, nz = 64, 4
    grid = ((0., 0., 0.), np.eye(3), 0., 0., 64., px)
    st = loaded(frames, capacity=1024)
    for rule, crossed in (((1, 1, 0.0), 1), ((9, 1, 0.0), 1), ((10, 1, 0.0), 0), ((rc.MAX_STEPS, 1, 0.0), 0)):
        out = st.bev_voxel_carve(params(*grid), 0., 1., nz, sensors, [13], *rule)
        want = cc.model(frames, sensors, *grid, 0., 1., nz, False, [13], *rule)
        assert want['N'].tolist() == [rc.MAX_STEPS, -1, rc.MAX_STEPS, 0, 0] and want['stats'][:5].tolist() == [5, 4, 0, 1, 4]
        # voxel (42, 35, 0) is step it = 16 374 of the first ray's 16 384: counted while it < N - end_margin, up to a margin of 9
        assert want['cross'][0, px - 1 - 35, 42] == crossed and want['flags'].tolist() == [0, 255, 0, crossed, crossed], rule
        cc.compare(out, want)
    st.check_status()


def test_window_above_max_points_is_cut_and_says_so(T):
    from pca_amd import _lib
    frames = frames_of(1)
    R, dx, dy, px, nz = rc.rotation(0.3), 0., 0., 20, 5
    st = loaded(frames)
    cut = 6700                                                    # inside the second frame
    out = st.bev_voxel_carve(params(ORIGIN, R, dx, dy, VIEW, px), -1., 0.5, nz, SENSORS, DYNOBJ, max_points=cut)
    want = cc.model(frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.5, nz, False, DYNOBJ, max_points=cut)
    cc.compare(out, want)
    assert out['flags'].shape == (cut, ) and st.ctx.status() == _lib.STATUS_STORE_OVERFLOW     # (read and cleared here)
    # flags beyond the cut are not written
    r, _, (hits, cross, flags, stats) = raw_call(st, params(ORIGIN, R, dx, dy, VIEW, px), max_points=cut, z_step=0.5, nz=nz)
    assert r == 0 and np.array_equal(flags[:cut].cpu().numpy(), want['flags']) and (flags[cut:] == 7).all().item()
    assert stats.tolist() == want['stats'].tolist() and st.ctx.status() == _lib.STATUS_STORE_OVERFLOW
    st.check_status()


# ---------------------------------------------------------------------------------------------- 4: mark_dyn
def test_mark_dyn_writes_dyn_alone_and_the_next_raster_sees_it(T):
    frames = frames_of(1)
    rows = np.concatenate(frames)
    R, dx, dy = ROT
    px, nz = 64, 32
    prm = params(ORIGIN, R, dx, dy, VIEW, px, 2.5)
    st = loaded(frames)
    st.retransform(np.eye(4), defer=True)                        # something owed: a call that writes flushes it first
    quiet = st.bev_voxel_carve(prm, -1., 0.125, nz, SENSORS, DYNOBJ)      # off by default: the store stays as it is
    assert len(st._pending) == 1 and np.array_equal(st.dyn[:rows.shape[0]].cpu().numpy(), rows[:, 9].astype(np.uint8))
    rows_before = [t[:rows.shape[0]].clone() for t in st._arrays()]
    out = st.bev_voxel_carve(prm, -1., 0.125, nz, SENSORS, DYNOBJ, mark_dyn=True)
    assert not st._pending and all(T.equal(out[k], quiet[k]) for k in out)
    want = want_of(('rot', px, nz, False, RULES[0]), frames, SENSORS, ORIGIN, R, dx, dy, VIEW, px, -1., 0.125, nz, False, DYNOBJ,
                   *RULES[0])
    cc.compare(out, want)
    dyn = np.where(want['flags'] == 1, 1., rows[:, 9])
    assert (dyn != rows[:, 9]).sum() == want['stats'][5] >= 50
    assert np.array_equal(st.dyn[:rows.shape[0]].cpu().numpy(), dyn.astype(np.uint8))
    for name, a, b in zip('x y z intensity rgbs inst'.split(), rows_before, st._arrays()):
        assert T.equal(a, b[:rows.shape[0]]), name
    # the rasters that follow: those of a store loaded with rows whose dyn was set by hand
    marked = [f.copy() for f in frames]
    k = 0
    for f in marked:
        f[:, 9] = dyn[k:k + f.shape[0]]
        k += f.shape[0]
    twin = loaded(marked)
    a16, a64 = st.bev(2, prm, want_f64=True)
    b16, b64 = twin.bev(2, prm, want_f64=True)
    assert T.equal(a64.view(T.int64), b64.view(T.int64)) and T.equal(a16.view(T.int16), b16.view(T.int16))
    # the flagged points take no part any more
    again = st.bev_voxel_carve(prm, -1., 0.125, nz, SENSORS, DYNOBJ)
    assert again['stats'][0].item() == want['stats'][0] - want['stats'][5]
    st.check_status()
    twin.check_status()


# ---------------------------------------------------------------------------------------------- 5: the top level
def test_carve_dynamic_on_a_kitti_sequence(T, tmp_path):
    from pca_amd import host_logic as hl
    acc, idx = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14), 9
    twin = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14)
    gen = acc.sem_bev_generator
    z_range, nz = (-2.0, 4.4), 32
    frames = acc.sem_pcs
    poses = np.array(acc.poses)
    origin = poses[idx]
    R = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:idx] - origin))
    view, px = 1. * gen.view_size, gen.pixel_size
    z_step = (z_range[1] - z_range[0]) / nz
    lifted = poses + np.array([0., 0., 1.5])                      # a sensor that does not sit at the pose
    assert gen.dynamic_classes() == DYNOBJ
    wants = {}
    for part, sl, sensors, kw in (('full', slice(0, None), None, {}), ('present', slice(0, idx), None, dict(classes=['car', 5])),
                                  ('future', slice(idx, None), lifted, dict(end_margin=2, min_cross=1, ratio=0.5))):
        rows, org = frames[sl], (poses if sensors is None else sensors)[sl]
        out = acc.carve_dynamic(idx, part=part, z_range=z_range, nz=nz, origins=None if sensors is None else sensors[sl], **kw)
        classes = [13, 5] if 'classes' in kw else DYNOBJ
        rule = (kw.get('end_margin', 1), kw.get('min_cross', 2), kw.get('ratio', 1.0))
        want = wants[part] = cc.model(rows, org, origin, R, 0., 0., view, px, z_range[0], z_step, nz, False, classes, *rule)
        cc.compare(out, want)
        assert want['stats'][4] > 50 and want['cross'].sum() > 50, part
        # the generator: host rows per frame in BEV-frame metres, one origin each, equal the window form
        rel = [f.copy() for f in rows]
        for f in rel:
            f[:, 0:3] -= origin
        host = gen.voxel_carve_device(rel, org - origin, R, 0., 0., view, z_range, nz, classes=kw.get('classes'), end_margin=rule[0],
                                      min_cross=rule[1], ratio=rule[2])
        assert all(T.equal(host[k], out[k]) for k in out), part
    with pytest.raises(ValueError):
        acc.carve_dynamic(idx, part='past')
    with pytest.raises(ValueError, match='origins'):
        acc.carve_dynamic(idx, part='present', origins=poses)     # one origin per frame of the part
    with pytest.raises(ValueError, match='per-frame'):
        gen.voxel_carve_device(np.concatenate(frames), poses, R, 0., 0., view, z_range, nz)
    with pytest.raises(ValueError, match='mark_dyn'):
        gen.voxel_carve_device(frames, poses, R, 0., 0., view, z_range, nz, mark_dyn=True)
    # mark_dyn=True: the next sample is that of a twin accumulator whose dyn was set on the host
    unmarked = acc.generate_bev(idx, 1, gen_future=True)[0]
    dyn0 = acc.store.dyn.clone()
    out = acc.carve_dynamic(idx, part='full', z_range=z_range, nz=nz, min_cross=1, ratio=0.25, mark_dyn=True)
    want = cc.model(frames, poses, origin, R, 0., 0., view, px, z_range[0], z_step, nz, False, DYNOBJ, 1, 1, 0.25)
    cc.compare(out, want)
    n_marked = int(want['stats'][5])
    assert n_marked > 20
    off = acc.store.offsets()
    lo, hi = int(off[0]), int(off[-1])
    expect = T.where(T.from_numpy(want['flags'] == 1).to(dyn0.device), T.ones_like(dyn0[lo:hi]), dyn0[lo:hi])
    assert T.equal(acc.store.dyn[lo:hi], expect) and int((expect != dyn0[lo:hi]).sum()) == n_marked
    toff = twin.store.offsets()
    assert int(toff[-1]) - int(toff[0]) == hi - lo
    twin.store.dyn[int(toff[0]):int(toff[-1])] = expect
    a, b = acc.generate_bev(idx, 1, gen_future=True)[0], twin.generate_bev(idx, 1, gen_future=True)[0]
    assert sorted(a) == sorted(b)
    planes = [k for k in a if isinstance(a[k], np.ndarray)]
    assert len(planes) >= 15
    for k in planes:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert any(a[k].tobytes() != unmarked[k].tobytes() for k in planes)      # (and the marks do show in the sample)
    acc.store.check_status()
    twin.store.check_status()


# ---------------------------------------------------------------------------------------------- 6: the C ABI's checks
def raw_call(st, prm, max_points=20000, z_lo=-1., z_step=0.5, nz=4, origins=True, only=True, outputs=(True, True, True, True),
             rule=(1, 2, 1.0), pending=None, slots=None, ws_bytes=None, workspace=True):
    """pca_bev_voxel_carve itself; returns (rc, message, (hits, cross, flags, stats))."""
    import torch

    from pca_amd import _lib
    ctx, lib = st.ctx, st.ctx.lib
    px = min(max(int(prm.px), 1), 64)
    hits = torch.full((32, px, px), 7, dtype=torch.int32, device=st.device)       # (a refused call writes nothing)
    cross = torch.full((32, px, px), 7, dtype=torch.int32, device=st.device)
    flags = torch.full((20000, ), 7, dtype=torch.uint8, device=st.device)
    stats = torch.full((6, ), 7, dtype=torch.int64, device=st.device)
    outs = [t.data_ptr() if on else None for t, on in zip((hits, cross, flags, stats), outputs)]
    org = torch.from_numpy(SENSORS[:st.n_frames].copy()).to(st.device)
    group = _lib.PcaClassGroup()
    group.mask[:] = list(_lib.class_mask(DYNOBJ))
    need = int(lib.pca_bev_carve_workspace_bytes(min(max_points, 1 << 20), px, min(max(nz, 1), 32)))
    ws = torch.empty(need, dtype=torch.uint8, device=st.device)
    store = st.c_store()
    b, e = (st.head, st.head + st.n_frames) if slots is None else slots
    if pending is None:
        pT, pE, nP = None, None, 0
    else:
        Ts, ends, nP = pending
        pT = None if Ts is None else (C.c_double * len(Ts))(*Ts)
        pE = None if ends is None else (C.c_int * len(ends))(*ends)
    r = lib.pca_bev_voxel_carve(ctx.h, C.byref(store), st.frame_off.data_ptr(), b, e, max_points, C.byref(prm), z_lo, z_step, nz, 0,
                                org.data_ptr() if origins else None, group if only else None, rule[0], rule[1], rule[2],
                                pT, pE, nP, ws.data_ptr() if workspace else None, need if ws_bytes is None else ws_bytes, *outs,
                                ctx.stream())
    torch.cuda.synchronize()
    return r, lib.pca_last_error(ctx.h).decode(), (hits, cross, flags, stats)


def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    frames = frames_of(1)
    R, px = rc.rotation(0.3), 32
    st = loaded(frames)
    prm = params(ORIGIN, R, 0., 0., VIEW, px)
    ctx = st.ctx
    want = cc.model(frames, SENSORS, ORIGIN, R, 0., 0., VIEW, px, -1., 0.5, 4, False, DYNOBJ)
    r, _, (hits, cross, flags, stats) = raw_call(st, prm)         # the call as such is fine
    assert r == 0 and np.array_equal(hits[:4].cpu().numpy(), want['hits']) and (hits[4:] == 7).all().item()
    assert np.array_equal(cross[:4].cpu().numpy(), want['cross']) and (cross[4:] == 7).all().item()
    assert np.array_equal(flags[:12000].cpu().numpy(), want['flags']) and (flags[12000:] == 7).all().item()
    assert stats.tolist() == want['stats'].tolist() and want['stats'][5] >= 50
    for k in range(4):                                            # any output alone
        only_k = tuple(j == k for j in range(4))
        r, _, outs = raw_call(st, prm, outputs=only_k)
        assert r == 0
        for j, (t, name) in enumerate(zip(outs, ('hits', 'cross', 'flags', 'stats'))):
            if j != k:
                assert (t == 7).all().item(), (k, name)
        n = {0: 4, 1: 4, 2: 12000, 3: 6}[k]
        assert np.array_equal(outs[k][:n].cpu().numpy(), want[('hits', 'cross', 'flags', 'stats')[k]]), k
    ctx.profile(1)
    bad_R = np.array([[1., 0., 0.], [0., np.cos(0.1), -np.sin(0.1)], [0., np.sin(0.1), np.cos(0.1)]])
    eye = [float(v) for v in np.eye(4).reshape(-1)]
    nan, inf = float('nan'), float('inf')
    h = st.head
    cases = [(dict(prm=params(ORIGIN, R, 0., 0., VIEW, 1025)), r'bev voxel carve: px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, R, 0., 0., VIEW, 0)), r'bev voxel carve: px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, bad_R, 0., 0., VIEW, px)), 'bev voxel carve: R must be a rotation about the z axis'),
             (dict(outputs=(False, ) * 4), 'bev voxel carve: bad arguments'),
             (dict(origins=False), 'bev voxel carve: bad arguments'),
             (dict(only=False), 'bev voxel carve: bad arguments'),
             (dict(workspace=False), 'bev voxel carve: bad arguments'),
             (dict(ws_bytes=1024), 'bev voxel carve: workspace too small'),
             (dict(max_points=1 << 32), 'bev voxel carve: max_points must be below 2\\^32'),
             (dict(slots=(h + 2, h + 1)), 'bev voxel carve: need slot_begin <= slot_end'),
             (dict(pending=(eye * 5, [h + 1] * 5, 5)), 'bev voxel carve: bad chain of owed transforms'),
             (dict(pending=(None, None, 1)), 'bev voxel carve: bad chain of owed transforms'),
             (dict(pending=(eye, [h + 4], 1)), 'bev voxel carve: a pending slot end lies beyond the window'),
             (dict(pending=(eye * 2, [h + 2, h + 1], 2)), 'bev voxel carve: pending slot ends must ascend')]
    cases += [(dict(nz=v), r'bev voxel carve: nz must be in 1\.\.32') for v in (0, -1, 33)]
    cases += [(dict(z_lo=v), 'bev voxel carve: z_lo must be finite') for v in (nan, inf, -inf)]
    cases += [(dict(z_step=v), 'bev voxel carve: z_step must be finite and > 0') for v in (0., -0.5, nan, inf)]
    cases += [(dict(rule=(v, 2, 1.0)), r'bev voxel carve: end_margin must be in 0\.\.16384') for v in (-1, rc.MAX_STEPS + 1)]
    cases += [(dict(rule=(1, 0, 1.0)), 'bev voxel carve: min_cross must be >= 1')]
    cases += [(dict(rule=(1, 2, v)), 'bev voxel carve: ratio must be finite and >= 0') for v in (-0.5, nan, inf)]
    for bad, msg in cases:
        args = dict(prm=prm)
        args.update(bad)
        r, err, outs = raw_call(st, **args)
        assert r == -1 and re.match(msg, err), (err, msg)
        assert all((t == 7).all().item() for t in outs), msg
    with pytest.raises(RuntimeError, match=r'bev voxel carve: nz must be in 1\.\.32'):
        st.bev_voxel_carve(prm, -1., 0.5, 33, SENSORS, DYNOBJ)
    with pytest.raises(RuntimeError, match='min_cross must be >= 1'):
        st.bev_voxel_carve(prm, -1., 0.5, 4, SENSORS, DYNOBJ, min_cross=0)
    with pytest.raises(ValueError, match='min_cross'):
        st.bev_voxel_carve(prm, -1., 0.5, 4, SENSORS, DYNOBJ, min_cross=-1)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert all(prof[k][1] == 0 for k in ('bev_carve_ends', 'bev_carve_rays', 'bev_carve_flags'))
    # the limits themselves are legal: end_margin 16 384 counts nothing, ratio 0 asks for min_cross alone
    r, _, (hits, cross, flags, stats) = raw_call(st, prm, rule=(rc.MAX_STEPS, 1, 0.0))
    assert r == 0 and not cross[:4].any().item() and stats[5].item() == 0 and stats[4].item() == want['stats'][4]
    st.check_status()
