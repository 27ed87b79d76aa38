"""GPU parity of K1 on the frustum-edge frames (tests/k1_edges_common.py; the oracle is pinned to the reference on the same
frames by test_k1_edges_golden.py): points on the five frustum planes and their f32 neighbours, magnitudes up to FLT_MAX, inf /
NaN / -0.0 / denormals, at the lanes, packed-pair halves and tile edges of every tile shape -- through every form of K1, the
stored rows, the segment sizes and the status word against the oracle, bit for bit."""
import numpy as np
import pytest

import k1_edges_common as kc
from test_gpu_kernels import DYNOBJ, P_KITTI, assert_planes_match, cu, dev_store

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


_want = {}


def oracle_rows(orc, name, pts=None, key='', bilinear=False, sem_gt=None):
    """The oracle's rows of a case's frame (or of `pts`, a piece of it, under `key`): computed once, shared, never written to."""
    k = (name, key, bilinear, sem_gt is not None)
    if k not in _want:
        fr = kc.frame(name)
        pts = fr.pts if pts is None else pts
        img, sem = fr.images()
        ost = orc.Store(max(len(pts), 1))
        orc.set_sample_mode(1 if bilinear else 0)
        try:
            orc.kitti_project_sample_filter(ost, pts, fr.P, None if sem_gt is not None else img, None if sem_gt is not None else sem,
                                            sem_gt, fr.H, fr.W, fr.filters)
        finally:
            orc.set_sample_mode(0)
        rows = ost.rows()
        rows.setflags(write=False)
        _want[k] = rows
    return _want[k]


def dev_frame(T, fr, pts=None):
    img, sem = fr.images()
    return dict(pts=cu(T, fr.pts if pts is None else pts), rgb=cu(T, img), sem=cu(T, sem))


def check(st, wants, name):
    """Segment sizes, rows (bit for bit: kept points are finite) and a clean status word."""
    st.check_status()
    assert st.sizes().tolist() == [len(w) for w in wants], name
    assert np.array_equal(st.rows(), np.concatenate(wants)), name
    st.check_status()


def test_the_kitti_camera_is_the_suite_s():
    assert np.array_equal(kc.CAMERAS['kitti'][0], P_KITTI)


@pytest.mark.parametrize('sample_mode', ['nearest', 'bilinear'])
@pytest.mark.parametrize('name', kc.CASES)
def test_k1_edges_fused_one_frame(T, orc, name, sample_mode):
    """One frame: the FUSED form, 256 x 4 tiles chained by look-back (the last tile holds 507 points)."""
    fr = kc.frame(name)
    st = dev_store(capacity=len(fr.pts), max_frames=4)
    st.append_kitti([dev_frame(T, fr)], fr.P, fr.H, fr.W, fr.filters, sample_mode=sample_mode)
    check(st, [oracle_rows(orc, name, bilinear=sample_mode == 'bilinear')], name)


@pytest.mark.parametrize('form', ['one_frame', 'inline', 'uploaded', 'bilinear_inline'])
@pytest.mark.parametrize('name', kc.CASES)
def test_k1_edges_split(T, orc, monkeypatch, name, form):
    """The SPLIT form (512 x 4 tiles + k1_append), forced: one frame (its descriptor in the argument block), the frame twice with
    the descriptors inline in the kernel arguments (equal frames, as that form needs), uploaded (PCA_K1_NO_INLINE=1), and inline
    with bilinear sampling.  test_the_switches_select_the_forms holds PCA_K1_MODE to what it selects."""
    monkeypatch.setenv('PCA_K1_MODE', 'split')
    if form == 'uploaded':
        monkeypatch.setenv('PCA_K1_NO_INLINE', '1')
    fr = kc.frame(name)
    n_frames = 1 if form == 'one_frame' else 2
    bilinear = form == 'bilinear_inline'
    st = dev_store(capacity=n_frames * len(fr.pts), max_frames=4)
    f = dev_frame(T, fr)
    st.append_kitti([f] * n_frames, fr.P, fr.H, fr.W, fr.filters, sample_mode='bilinear' if bilinear else 'nearest')
    check(st, [oracle_rows(orc, name, bilinear=bilinear)] * n_frames, (name, form))


@pytest.mark.parametrize('form', ['fused', 'one_frame', 'inline', 'uploaded'])
def test_the_switches_select_the_forms(T, orc, monkeypatch, form):
    """What the cases above rely on: without a switch one such frame takes the FUSED form, PCA_K1_MODE=split the SPLIT form.  Seen
    through the diagnostic stamps (PCA_K1_STAMPS=1: eight words per workgroup of the front grid), whose workgroup count is one
    per 1024-point tile FUSED and one per 2048-point tile and frame SPLIT; the rows are the oracle's with the stamps on as well.
    (Inline and uploaded descriptors launch the same grid: nothing the library reports tells them apart.)"""
    import ctypes as C
    from pca_amd import _lib
    name = 'axis'
    fr = kc.frame(name)
    n, n_frames = len(fr.pts), 2 if form in ('inline', 'uploaded') else 1
    if form != 'fused':
        monkeypatch.setenv('PCA_K1_MODE', 'split')
    if form == 'uploaded':
        monkeypatch.setenv('PCA_K1_NO_INLINE', '1')
    monkeypatch.setenv('PCA_K1_STAMPS', '1')
    st = dev_store(capacity=n_frames * n, max_frames=4)
    st.append_kitti([dev_frame(T, fr)] * n_frames, fr.P, fr.H, fr.W, fr.filters)
    check(st, [oracle_rows(orc, name)] * n_frames, (name, form))
    ctx = _lib.Context.get()
    buf = np.zeros((4096, 8), np.uint64)
    blocks = ctx.lib.pca_debug_k1_stamps(ctx.h, buf.ctypes.data_as(C.c_void_p), len(buf))
    assert blocks == (-(-n // 1024) if form == 'fused' else n_frames * -(-n // 2048)), form
    assert buf[:blocks, 0].all() and not buf[blocks:].any()           # every workgroup of that grid stamped its start


@pytest.mark.parametrize('mode', ['fused', 'split'])
@pytest.mark.parametrize('name', kc.CASES)
def test_k1_edges_ragged_batch(T, orc, monkeypatch, name, mode):
    """The edge frame, cut in two inside its u/d = W - 1/2 family at a point that is no tile boundary, between an empty frame, a
    one-point frame and a frame of exactly one tile of the form under test (1024 points FUSED, 2048 SPLIT): frames of unequal tile
    counts (the descriptor search by tile / by queue position), the plane family across the tile boundaries of both pieces, both
    pieces ending in a partial tile."""
    if mode == 'split':
        monkeypatch.setenv('PCA_K1_MODE', 'split')
    tile = 2048 if mode == 'split' else 1024
    fr = kc.frame(name)
    fam = fr.of('u_hi')
    fam = fam[fam >= 700]
    cut = int(fam[len(fam) // 2])
    assert cut % 1024 and (len(fr.pts) - cut) % 1024 and fam.min() < cut < fam.max()
    kept = np.intersect1d(fr.of('ladder_e36'), kc.fixture(name)['kept'])
    one = fr.pts[kept[:1]]                                 # (the one-point frame: a 1e36 point that the reference keeps)
    pieces = {'empty': fr.pts[:0], 'one': one, 'head': fr.pts[:cut], 'tail': fr.pts[cut:], 'tile': fr.pts[1000:1000 + tile]}
    order = ['empty', 'head', 'one', 'tail', 'tile']
    st = dev_store(capacity=2 * len(fr.pts), max_frames=8)
    st.append_kitti([dev_frame(T, fr, pieces[k]) for k in order], fr.P, fr.H, fr.W, fr.filters)
    wants = [oracle_rows(orc, name, pieces[k], key=f'tile{tile}' if k == 'tile' else k) for k in order]
    assert len(wants[0]) == 0 and len(wants[2]) == 1 and len(wants[1]) + len(wants[3]) == len(oracle_rows(orc, name))
    check(st, wants, (name, mode))


@pytest.mark.parametrize('mode', ['fused', 'split'])
@pytest.mark.parametrize('name', kc.CASES)
def test_k1_edges_use_gt_sem(T, orc, monkeypatch, name, mode):
    """use_gt_sem: no projection and no cull -- every point whose class passes the filter is kept, NaN and inf included
    (compared as bit patterns)."""
    if mode == 'split':
        monkeypatch.setenv('PCA_K1_MODE', 'split')
    fr = kc.frame(name)
    sem_gt = np.random.default_rng(fr.seed + 1).integers(0, 19, len(fr.pts)).astype(np.uint8)
    want = oracle_rows(orc, name, sem_gt=sem_gt)
    st = dev_store(capacity=len(fr.pts), max_frames=4)
    st.append_kitti([dict(pts=cu(T, fr.pts), sem_gt=cu(T, sem_gt))], fr.P, 1, 1, fr.filters)
    st.check_status()
    assert st.sizes().tolist() == [len(want)] == [int((~np.isin(sem_gt, fr.filters)).sum())]
    for e in kc.RUNGS:                                    # every point of the ladder whose class passes is kept
        assert (~np.isin(sem_gt[fr.of(f'ladder_e{e}')], fr.filters)).sum() > 200
    assert np.isnan(want).any() and np.isinf(want).any()
    assert np.array_equal(st.rows().view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize('name', kc.CASES)
def test_k1_edges_deferred_k1_rides_in_the_raster(T, orc, name):
    """pca_k1_defer: the frame's K1 runs as the first workgroups of the raster that follows it (1024 x 4 tiles).  No K1 launch
    of its own, the oracle's rows, and the raster's 21 planes (view culling on, as shipped) against the oracle's raster of the
    oracle's rows."""
    from pca_amd import _lib
    from pca_amd.device_store import make_bev_params
    fr = kc.frame(name)
    want = oracle_rows(orc, name)
    f = dev_frame(T, fr)
    st = dev_store(capacity=len(fr.pts), max_frames=4)
    C = -np.linalg.solve(fr.P[:, :3], fr.P[:, 3])
    args = ((float(C[0]), float(C[1]), 0.), np.eye(3), 0., 0., 40., 64, None, 20., 20., 0.5, 0, DYNOBJ, False)
    st.set_defer_k1(True)
    try:
        o = _lib.PcaKittiObs()
        o.pts, o.rgb, o.sem, o.sem_gt, o.n, o.host_mask = f['pts'].data_ptr(), f['rgb'].data_ptr(), f['sem'].data_ptr(), None, len(fr.pts), 0
        st.ctx.profile(True)
        st.append_kitti_obs(o, fr.P, fr.H, fr.W, fr.filters, keep=f)
        p16, p64 = st.bev(1, make_bev_params(*args), want_f64=True)
        launches = st.ctx.profile_read()['kitti_project_sample_filter'][1]
        st.ctx.profile(False)
    finally:
        st.set_defer_k1(False)
    assert launches == 0                                  # it rode
    check(st, [want], name)
    ost = orc.Store.from_rows(want)
    ref = orc.bev(ost, len(want), orc.make_bev_params(*args))
    assert np.count_nonzero(ref['planes'][14:21]) > 100   # (the window does see points)
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), ref, name)
