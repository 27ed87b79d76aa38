"""GPU: the window of the store rendered into a pinhole camera (pca_render_camera, DeviceStore.render_camera,
SemanticPointCloudAccumulator.render_camera) against the numpy model of tests/render_camera_common.py (tied to the oracle by
tests/test_render_camera_model.py).  Every comparison is exact; every input is a valid call or a refused one."""
import ctypes as C
import re

import numpy as np
import pytest

import elev_partition_common as ec
import render_camera_common as rcc
from test_gpu_kernels import T  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, frames_of, kitti_accumulator, loaded, owe, params

pytestmark = pytest.mark.gpu

MID = (65, 33, 32.)                                               # the shape of the tests that need one: 47 chunks, ~14 points a pixel


def cam_of(P, W, H, radius=0, include_dyn=True, depth_range=(0., np.inf)):
    from pca_amd._lib import make_camera
    return make_camera(P, W, H, radius, include_dyn, depth_range)


_wants = {}


def want_of(key, *args, **kw):
    """The model's result for a case that several tests share, computed once."""
    if key not in _wants:
        _wants[key] = rcc.model(*args, **kw)
    return _wants[key]


# ---------------------------------------------------------------------------------------------- 1: the model, five shapes
@pytest.mark.parametrize('W,H,f', rcc.SHAPES)
def test_render_equals_the_model(T, W, H, f):
    """1 x 1: every point fights for one key; 5 x 7 at radius 2: most footprints are clipped; 1408 x 376: KITTI's image."""
    frames, P = frames_of(1), rcc.camera(W, H, f)
    st = loaded(frames)
    for radius in (0, 2):
        for include_dyn in (False, True):
            out = st.render_camera(cam_of(P, W, H, radius, include_dyn))
            want = want_of((W, H, radius, include_dyn), frames, P, W, H, radius, include_dyn)
            rcc.compare(out, want)
    plain = want_of((W, H, 0, True), frames, P, W, H, 0, True)
    assert plain['stats'][0] == 12000 and plain['stats'][1] > 2500      # (the case cannot silently go soft)
    assert (W, H) != MID[:2] or (plain['stats'][2] >= 1000 and plain['most'] >= 10)
    assert (W, H) != (1, 1) or plain['most'] == plain['stats'][1]
    st.check_status()


@pytest.mark.parametrize('always_atomic', ['0', '1'])
def test_few_workgroups_walk_the_window_in_rounds(T, monkeypatch, always_atomic):
    """PCA_RENDER_G=3: three workgroups take the 47 chunks of the window in 16 rounds (by default a window below 524 288 points
    is one round).  PCA_RENDER_ALWAYS_ATOMIC=1, the A/B form without the load in front of the atomic, gives the same result."""
    monkeypatch.setenv('PCA_RENDER_G', '3')
    monkeypatch.setenv('PCA_RENDER_ALWAYS_ATOMIC', always_atomic)
    W, H, f = MID
    frames, P = frames_of(1), rcc.camera(W, H, f)
    st = loaded(frames)
    for radius in (0, 2):
        rcc.compare(st.render_camera(cam_of(P, W, H, radius)), want_of((W, H, radius, True), frames, P, W, H, radius, True))
    st.check_status()


@pytest.mark.parametrize('radius,floor', [(0, 50), (2, 300)])
def test_exact_ties_go_to_the_smallest_index(T, radius, floor):
    """x, y, z on a 1/2 m lattice, the camera on it, yaw 0, f = 8: d = x - 1/2 is exactly equal for many points of a pixel.
    The floors: 61 and 350 pixels whose two nearest candidates tie, counted by the model when the test was written."""
    rng = np.random.default_rng(7)
    frames = []
    for _ in range(3):
        f = ec.random_rows(rng, 4000, 25.)
        f[:, 0:3] = np.rint(f[:, 0:3] * 2) / 2
        frames.append(f)
    W, H = MID[:2]
    P = rcc.camera(W, H, 8., position=(0.5, -0.5, 1.5), yaw=0.)
    st = loaded(frames)
    want = rcc.model(frames, P, W, H, radius)
    rcc.compare(st.render_camera(cam_of(P, W, H, radius)), want)
    assert want['ties'] > floor and want['stats'][1] > 5000
    st.check_status()


# ---------------------------------------------------------------------------------------------- 2: owed transforms
@pytest.mark.parametrize('ends', [(2, ), (1, 2, 2, 3)])
def test_owed_chain_over_part_of_the_window(T, ends):
    from test_gpu_kernels import _tilting_transform
    frames = frames_of(2)
    W, H, f = MID
    P = rcc.camera(W, H, f)
    cam = cam_of(P, W, H, 1)
    prm = params((0.3, -0.2, 0.125), -0.7, -0.5, 0.25, 40., 64, 2.5)
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
    got = lazy.render_camera(cam)
    want = rcc.model(eager, P, W, H, 1)
    rcc.compare(got, want)
    rcc.compare(twin.render_camera(cam), want)
    assert not np.array_equal(want['index'], rcc.model(frames, P, W, H, 1)['index'])
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


# ---------------------------------------------------------------------------------------------- 3: what takes part
def test_class_set_and_depth_range(T):
    W, H, f = MID
    frames, P = frames_of(1), rcc.camera(W, H, f)
    st = loaded(frames)
    classes = [0, 3, 13, 18, 200]
    out = st.render_camera(cam_of(P, W, H, 1, False, (5., 20.)), classes=classes)
    want = rcc.model(frames, P, W, H, 1, False, (5., 20.), classes)
    rcc.compare(out, want)
    assert 500 < want['stats'][0] < 3000 and 100 < want['stats'][1] < want['stats'][0] and want['stats'][2] > 300
    assert set(np.unique(want['sem'])) == {0, 3, 13, 18, 255}
    rcc.compare(st.render_camera(cam_of(P, W, H, 0, True, (5., 20.))), rcc.model(frames, P, W, H, 0, True, (5., 20.)))
    # an empty class set: the all-empty image
    out = st.render_camera(cam_of(P, W, H, 1), classes=[])
    rcc.compare(out, rcc.empty(W, H))
    st.check_status()


def test_non_finite_coordinates_drop_the_point(T):
    """A NaN or an infinity anywhere fails a comparison of the mask: no special case, and nothing is written for the point."""
    W, H, f = MID
    frames = [f.copy() for f in frames_of(1)]
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        frames[1][k::40, k] = v
    P = rcc.camera(W, H, f)
    st = loaded(frames)
    want = rcc.model(frames, P, W, H, 1)
    rcc.compare(st.render_camera(cam_of(P, W, H, 1)), want)
    assert want['stats'][0] == 12000 and 2000 < want['stats'][1] < want_of((W, H, 1, True), frames_of(1), P, W, H, 1, True)['stats'][1]
    st.check_status()


def test_empty_and_cut_windows(T):
    from pca_amd import _lib
    W, H, f = MID
    frames, P = frames_of(1), rcc.camera(W, H, f)
    st = loaded(frames)
    cam = cam_of(P, W, H, 1)
    ctx = st.ctx
    ctx.profile(1)
    out = st.render_camera(cam, first_frame=2, last_frame=2)      # a window without a slot: only the resolve is launched
    prof = ctx.profile_read()
    ctx.profile(0)
    rcc.compare(out, rcc.empty(W, H))
    assert prof['render_zbuffer'][1] == 0 and prof['render_resolve'][1] == 1
    # frames 1 and 2 alone: the index counts from the window's first point
    rcc.compare(st.render_camera(cam, first_frame=1), rcc.model(frames[1:], P, W, H, 1))
    assert st.ctx.status() == 0
    cut = 6700                                                    # inside the second frame
    out = st.render_camera(cam, max_points=cut)
    want = rcc.model(frames, P, W, H, 1, max_points=cut)
    rcc.compare(out, want)
    assert st.ctx.status() == _lib.STATUS_STORE_OVERFLOW         # (read and cleared here)
    assert want['stats'][0] == cut and want['index'].max() < cut
    assert want_of((W, H, 1, True), frames, P, W, H, 1, True)['stats'][1] > want['stats'][1] > 1000
    st.check_status()


# ---------------------------------------------------------------------------------------------- 4: the C ABI's checks
def raw_call(st, cam, max_points=20000, cam_ok=True, outputs=(True, ) * 6, pending=None, slots=None, store=None, frame_off=True):
    """pca_render_camera itself, with buffers of the 65 x 33 image; returns (rc, message, the six buffers)."""
    import torch
    ctx, lib = st.ctx, st.ctx.lib
    W, H = MID[:2]
    bufs = [torch.full((H, W), 7, dtype=torch.int64, device=st.device), torch.full((H, W), 7., dtype=torch.float32, device=st.device),
            torch.full((H, W), 7, dtype=torch.int64, device=st.device), torch.full((H, W, 3), 7, dtype=torch.uint8, device=st.device),
            torch.full((H, W), 7, dtype=torch.uint8, device=st.device), torch.full((3, ), 7, dtype=torch.int64, device=st.device)]
    store = st.c_store() if store is None else store
    b, e = (st.head, st.head + st.n_frames) if slots is None else slots
    if pending is None:
        pT, pE, nP = None, None, 0
    else:
        Ts, ends, nP = pending
        pT = None if Ts is None else (C.c_double * len(Ts))(*Ts)
        pE = None if ends is None else (C.c_int * len(ends))(*ends)
    r = lib.pca_render_camera(ctx.h, C.byref(store), st.frame_off.data_ptr() if frame_off else None, b, e, max_points,
                              C.byref(cam) if cam_ok else None, None, pT, pE, nP,
                              *(t.data_ptr() if ok else None for t, ok in zip(bufs, outputs)), ctx.stream())
    torch.cuda.synchronize()
    return r, lib.pca_last_error(ctx.h).decode(), bufs


def refusals(st, P):
    """(arguments of raw_call, the message) for every check of pca_render_camera."""
    W, H = MID[:2]
    eye = [float(v) for v in np.eye(4).reshape(-1)]
    nan, inf = float('nan'), float('inf')
    h, beyond = st.head, st.head + st.n_frames + 1
    good = cam_of(P, W, H, 1)
    cases = [(dict(cam_ok=False), 'render camera: bad arguments'), (dict(frame_off=False), 'render camera: bad arguments')]
    cases += [(dict(outputs=tuple(k != miss for k in range(6))), 'render camera: bad arguments') for miss in range(6)]
    for name in ('x', 'rgbs', 'dyn'):
        store = type(st.c_store())()                              # a copy: c_store() hands out the store's own block
        C.memmove(C.byref(store), C.byref(st.c_store()), C.sizeof(store))
        setattr(store, name, None)
        cases.append((dict(store=store), r"render camera: the store's x, y, z, rgbs and dyn arrays are needed"))
    cases += [(dict(slots=(h + 2, h + 1)), 'render camera: need slot_begin <= slot_end'),
              (dict(pending=(eye * 5, [h + 1] * 5, 5)), 'render camera: bad chain of owed transforms'),
              (dict(pending=(None, None, 1)), 'render camera: bad chain of owed transforms'),
              (dict(pending=(eye, [beyond], 1)), 'render camera: a pending slot end lies beyond the window'),
              (dict(pending=(eye * 2, [h + 2, h + 1], 2)), 'render camera: pending slot ends must ascend'),
              (dict(max_points=1 << 32), r'render camera: max_points must be below 2\^32')]
    size = r'render camera: need 1 <= width, height and width \* height <= 16777216'
    cases += [(dict(cam=cam_of(P, w, hh, 1)), size) for w, hh in ((0, H), (W, 0), (-1, H), (4097, 4096), (1 << 16, 1 << 16))]
    cases += [(dict(cam=cam_of(P, W, H, r)), r'render camera: radius must be in 0\.\.3') for r in (-1, 4)]
    cases += [(dict(cam=cam_of(P, W, H, 1, True, rng)), 'render camera: need 0 <= min_depth < max_depth')
              for rng in ((-1., 5.), (5., 5.), (6., 5.), (nan, 5.), (0., nan), (inf, inf))]
    for k, v in ((0, nan), (7, inf), (11, -inf)):
        bad = np.array(P, dtype=np.float64).reshape(-1).copy()
        bad[k] = v
        cases.append((dict(cam=cam_of(bad, W, H, 1)), 'render camera: every entry of P must be finite'))
    return [(dict(dict(cam=good), **bad), msg) for bad, msg in cases]


def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    W, H, f = MID
    frames, P = frames_of(1), rcc.camera(W, H, f)
    st = loaded(frames)
    ctx = st.ctx
    r, _, bufs = raw_call(st, cam_of(P, W, H, 1))                 # the call as such is fine
    assert r == 0
    rcc.compare(dict(zip(('depth', 'index', 'rgb', 'sem', 'stats'), bufs[1:])), want_of((W, H, 1, True), frames, P, W, H, 1, True))
    ctx.profile(1)
    for args, msg in refusals(st, P):
        r, err, bufs = raw_call(st, **args)
        assert r == -1 and re.match(msg, err), (err, msg)
        assert all((t == 7).all().item() for t in bufs), msg
    with pytest.raises(RuntimeError, match=r'render camera: radius must be in 0\.\.3'):
        st.render_camera(cam_of(P, W, H, 4))
    with pytest.raises(RuntimeError, match='render camera: need 1 <= width, height'):
        st.render_camera(cam_of(P, 1 << 15, 1 << 15))
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['render_zbuffer'][1] == 0 and prof['render_resolve'][1] == 0
    st.check_status()


def test_refused_calls_leave_the_noted_k1_and_the_owed_chain_usable(T, tmp_path, monkeypatch):
    """The pattern of test_gpu_window_passes.py: a K1 that integrate() noted is still noted after every refusal, and the
    render that follows is the one of an accumulator that was never refused."""
    monkeypatch.setenv('PCA_FUSE_K1', '1')
    out = []
    for refuse_first in (False, True):
        acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=6)
        st = acc.store
        chain = [(np.array(Tm).copy(), e) for Tm, e in st._pending]
        assert st._k1_noted is not None and chain                # a K1 is noted and re-transforms are owed
        if refuse_first:
            for args, msg in refusals(st, acc.P_velo_frame):
                r, err, _ = raw_call(st, **args)
                assert r == -1 and re.match(msg, err), (err, msg)
            with pytest.raises(RuntimeError, match='render camera: '):
                acc.render_camera(radius=4)
            assert st._k1_noted is not None                      # nothing ran: the K1 is still noted
        got = acc.render_camera(radius=1)
        out.append([v.cpu().numpy() for v in got.values()])
        assert st._k1_noted is None
        assert len(st._pending) == len(chain) and all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(st._pending, chain))
        st.check_status()
        st.set_defer_k1(False)
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(*out))
    assert out[0][4][2] > 500                                    # (stats: pixels covered)


# ---------------------------------------------------------------------------------------------- 5: the top level
def test_drop_in_on_a_kitti_sequence(T, tmp_path):
    acc = kitti_accumulator(tmp_path, dict(BEV_KITTI))
    P, (W, H) = acc.P_velo_frame, (96, 64)                        # the fake tree's images
    n = acc.store.n_frames
    out = acc.render_camera()                                     # the defaults: p_velo_frame, the last image's size
    splat = acc.render_camera(radius=2, depth_range=(2., 30.), classes=[0, 2, 8], include_dyn=False)
    newest = acc.render_camera(frames=(n - 1, n))
    rows = acc.sem_pcs                                            # (applies what is still owed: the rows as they stand now)
    assert len(rows) == n == 10 and tuple(out['depth'].shape) == (H, W)
    want = rcc.model(rows, P, W, H)
    rcc.compare(out, want)
    assert want['stats'][1] > 2000 and want['stats'][2] > 1500
    rcc.compare(splat, rcc.model(rows, P, W, H, 2, False, (2., 30.), [0, 2, 8]))
    # the newest frame alone, in the lidar coordinates K1 saw it in: every stored point of it that the camera sees is the
    # winner of its pixel or is beaten there by a nearer one (or an equally near one stored before it)
    last = rows[-1]
    kept, u, v, d = rcc.pixels(last, P, W, H)
    index, depth = newest['index'].cpu().numpy(), newest['depth'].cpu().numpy()
    rgb, sem = newest['rgb'].cpu().numpy(), newest['sem'].cpu().numpy()
    assert kept.sum() > 300 and newest['stats'].tolist() == [len(last), int(kept.sum()), int((index >= 0).sum())]
    p = np.flatnonzero(kept)
    w = index[v[p], u[p]]                                         # the winner at each kept point's pixel
    d32 = d.astype(np.float32)
    assert (w >= 0).all() and np.array_equal(depth[v[p], u[p]], d32[w])
    assert np.array_equal(u[w], u[p]) and np.array_equal(v[w], v[p])          # the index maps back to a point of that pixel
    assert ((d32[w] < d32[p]) | ((d32[w] == d32[p]) & (w <= p))).all()
    won = p[w == p]
    assert len(won) == (index >= 0).sum() > 300
    assert np.array_equal(rgb[v[won], u[won]], last[won, 4:7].astype(np.uint8)) and np.array_equal(sem[v[won], u[won]], last[won, 7].astype(np.uint8))
    with pytest.raises(ValueError, match='frames'):
        acc.render_camera(frames=(3, n + 1))
    from sem_pc_accum import SemanticPointCloudAccumulator
    assert SemanticPointCloudAccumulator._render_defaults(acc) == (None, None)  # the base class has no camera of its own
    acc._render_defaults = lambda: (None, None)
    with pytest.raises(ValueError, match='needs P'):
        acc.render_camera(size=(W, H))
    acc.store.check_status()
