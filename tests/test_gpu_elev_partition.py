"""GPU: the BEV window partitioned by height above the cell minimum (pca_bev_elev_partition, DeviceStore.bev_elev_partition,
SemBEVGenerator.elev_partition_device / static_obj_partitioning_by_elev, SemanticPointCloudAccumulator.partition_by_elev)
against the reference's fixture and the numpy model of tests/elev_partition_common.py (pinned to the reference by
tests/test_elev_partition_golden.py).  Every comparison is exact."""
import ctypes as C
import re

import numpy as np
import pytest

import elev_partition_common as ec
from test_gpu_kernels import SEM_IDXS, T, dev_store  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, INTS, kitti_accumulator, params

pytestmark = pytest.mark.gpu

CASE_NAMES = [c[0] for c in ec.CASES]


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b):
    a, b = host(a), host(b)
    assert sorted(a) == sorted(b) == ['counts', 'elev', 'flags', 'observed']
    for k in a:
        x, y = (a[k].view(np.uint64), b[k].view(np.uint64)) if k == 'elev' else (a[k], b[k])
        assert a[k].dtype == b[k].dtype and np.array_equal(x, y), k


# ---------------------------------------------------------------------------------------------- 1: the reference's fixture
@pytest.mark.parametrize('case', CASE_NAMES)
def test_fixture_window_form_and_the_reference_method(T, golden, case):
    from bev_generator.sem_bev import SemBEVGenerator
    g = golden('elev_partition')
    view, px, _, rot, dx, dy = g['cfg']
    px = int(px)
    frames, origin, hf, thresh, include_dyn = ec.fixture_case(g, case)
    rows = np.concatenate(frames)
    st = dev_store(capacity=4096, max_frames=4)
    assert st.load_rows(frames) is None
    out = host(st.bev_elev_partition(params(origin, ec.rotation(rot), dx, dy, view, px, hf), thresh, include_dyn=include_dyn))
    st.check_status()
    assert out['observed'].dtype == np.bool_ and np.array_equal(out['observed'], g[f'mask_{case}'])
    assert out['elev'].dtype == np.float64 and np.array_equal(out['elev'].view(np.uint64), g[f'elev_{case}'].view(np.uint64))
    assert out['flags'].dtype == np.uint8 and out['flags'].shape == (rows.shape[0], )
    fate = g[f'fate_{case}']
    assert np.array_equal(ec.fates(out['flags'], rows[:, 8]), fate)
    n_in, n_el = int((fate != ec.FATE_OUT).sum()), int((out['flags'] == 1).sum())
    assert out['counts'].tolist() == [n_in, n_el, n_in - n_el] and n_el > 20
    # the reference's method on the gridded rows the reference handed to its own
    gen = SemBEVGenerator(SEM_IDXS, view, px, 0., 0., False, *INTS, hf)
    grid = g[ec.grid_name(case)]
    work = grid.copy()
    pc_static, pc_dynamic, elevmap, mask = gen.static_obj_partitioning_by_elev(work, thresh)
    assert gen.height_filter == hf
    f = fate[grid[:, 3].astype(int)]
    want = grid.copy()
    want[f == ec.FATE_DYNAMIC, 8] = 1                              # (set where elevated; a 1 that was there stays)
    assert np.array_equal(work, want)                              # the caller's rows: column 8 in place, nothing else
    assert pc_static.dtype == np.float64 and np.array_equal(pc_static, want[f == ec.FATE_STATIC])
    assert np.array_equal(pc_dynamic, want[f == ec.FATE_DYNAMIC])
    assert mask.dtype == np.bool_ and np.array_equal(mask, g[f'mask_{case}'])
    assert elevmap.dtype == np.float64 and np.array_equal(elevmap.view(np.uint64), g[f'elev_{case}'].view(np.uint64))


# ---------------------------------------------------------------------------------------------- 2: many workgroups, heavy tile
@pytest.mark.parametrize('cap_g', [None, '2'])
def test_many_level1_workgroups_a_heavy_cell_and_a_heavy_tile(T, monkeypatch, cap_g):
    """390 000 points at 256^2: 60 level-1 workgroups whose points stay in registers, or -- PCA_BEV_ELEV_G=2 -- two whose
    chunks (195 000 points) go past the register path.  One cell holds 70 000 points, its tile 40 000 more."""
    if cap_g:
        monkeypatch.setenv('PCA_BEV_ELEV_G', cap_g)
    rng = np.random.default_rng(19)
    view, px, hf, dx, dy = 100., 256, 3.0, 0.7, -1.3
    frames = ec.heavy_window(rng, view, px, dx, dy)
    rows = np.concatenate(frames)
    assert rows.shape[0] == 390000
    origin = (0., 0., 0.25)
    st = dev_store(capacity=1 << 19, max_frames=64)
    assert st.load_rows(frames) is None
    for thresh, include_dyn in ((0.3, False), (-0.05, True)):
        out = st.bev_elev_partition(params(origin, np.eye(3), dx, dy, view, px, hf), thresh, include_dyn=include_dyn)
        want = ec.model(rows, origin, np.eye(3), dx, dy, view, px, hf, thresh, include_dyn)
        ec.compare(out, want)
        assert np.bincount(want['cell'][want['cell'] >= 0]).max() > 50000
    st.check_status()


# ---------------------------------------------------------------------------------------------- 3: owed chain
@pytest.mark.parametrize('k', [1, 2, 3, 4])
def test_owed_chain_is_applied_to_what_is_read_and_stays_owed(T, k):
    from test_gpu_kernels import _tilting_transform
    rng = np.random.default_rng(60 + k)
    frames = [ec.random_rows(rng, 5000, 40.) for _ in range(3)]
    origin, view, px, hf = (0.3, -0.2, 0.1), 80., 64, 1.5     # (about 7 400 points in view in 4 096 cells: thousands above a minimum)
    lazy, twin = dev_store(capacity=1 << 15, max_frames=8), dev_store(capacity=1 << 15, max_frames=8)
    lazy.CHAIN_K = twin.CHAIN_K = 4
    assert lazy.load_rows(frames) is None and twin.load_rows(frames) is None
    for step in range(k):
        Tm = _tilting_transform(step)                            # changes z: minimum, threshold and filter see the transformed z
        lazy.retransform(Tm, defer=True)
        twin.retransform(Tm, defer=True)
    twin.flush_pending()                                         # eager: K2 writes the transforms into the store
    n_rows = sum(f.shape[0] for f in frames)
    before = [t[:n_rows].clone() for t in lazy._arrays()]
    prm = params(origin, ec.rotation(0.4), 0.5, -0.25, view, px, hf)
    got = lazy.bev_elev_partition(prm, 0.2)
    want = twin.bev_elev_partition(prm, 0.2)
    assert len(lazy._pending) == k and not twin._pending         # still owed
    same(got, want)
    assert int(got['counts'][1]) > 1000 and int(got['counts'][2]) > 1000
    assert all(T.equal(a, b[:n_rows]) for a, b in zip(before, lazy._arrays()))       # no store column was written
    assert not T.equal(lazy.z[:n_rows], twin.z[:n_rows])
    # what is owed is applied by the next consumer as before: a flush makes the two stores equal
    lazy.flush_pending()
    assert all(T.equal(a[:n_rows], b[:n_rows]) for a, b in zip(lazy._arrays(), twin._arrays()))
    lazy.check_status()
    twin.check_status()


# ---------------------------------------------------------------------------------------------- 4 and 7: the KITTI drop-in
def test_noted_k1_runs_before_the_partition(T, tmp_path, monkeypatch):
    prm = params((0., 0., 0.), ec.rotation(0.3), 0., 0., 50., 32, None)
    out = []
    for fuse in ('1', '0'):
        monkeypatch.setenv('PCA_FUSE_K1', fuse)
        acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=6)
        st = acc.store
        assert (st._k1_noted is not None) == (fuse == '1')       # integrate() left the newest frame's K1 for the next raster
        res = st.bev_elev_partition(prm, 0.2)                    # (the whole window: the C call itself runs the noted K1)
        assert st._k1_noted is None
        st.check_status()
        n_last = int(st.sizes()[-1])
        out.append((res, n_last))
        st.set_defer_k1(False)
    same(out[0][0], out[1][0])
    n_last = out[0][1]
    assert n_last == out[1][1] and (out[0][0]['flags'][-n_last:] != 255).sum().item() > 100   # the new frame's points take part


def test_partition_by_elev_is_the_elevation_plane_of_the_same_sample(T, tmp_path):
    from pca_amd import host_logic as hl
    acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14)
    gen, idx = acc.sem_bev_generator, 9
    bev = acc.generate_bev(idx, 1, gen_future=True)[0]
    pcs, trajs = acc._window_inputs(idx, True)
    rot_mat = hl.rotation_matrix_3d(hl.heading_rot_ang(trajs['ego_traj_present']))
    _, p64 = gen.rasterise(pcs['pc_present'], pcs['pc_future'], pcs['pc_full'], rot_mat, 0., 0., 1. * gen.view_size, want_f64=True)
    p64 = p64.cpu().numpy()
    assert np.array_equal(p64[6].astype(np.float16).view(np.uint16), bev['elevation_present'].view(np.uint16))
    sizes = acc.store.sizes()
    for part, plane, n in (('present', 6, sizes[:idx].sum()), ('future', 13, sizes[idx:].sum()), ('full', 20, sizes.sum())):
        out = host(acc.partition_by_elev(idx, 0.25, part=part))
        assert np.array_equal(out['elev'].view(np.uint64), p64[plane].view(np.uint64)), part
        assert (out['elev'][~out['observed']] == 0.).all() and out['observed'].sum() > 50
        assert out['flags'].shape == (n, ) and out['counts'][0] == (out['flags'] != 255).sum() > 100
        assert out['counts'][1] == (out['flags'] == 1).sum() > 10
    with pytest.raises(ValueError):
        acc.partition_by_elev(idx, 0.25, part='past')
    # mark_dyn through the accumulator: the elevated points leave the static partition of the next sample
    dyn0 = acc.store.dyn.clone()
    out = acc.partition_by_elev(idx, 0.25, part='full', mark_dyn=True)
    off = acc.store.offsets()
    lo, hi = int(off[0]), int(off[-1])
    assert T.equal(acc.store.dyn[lo:hi], T.where(out['flags'] == 1, T.ones_like(dyn0[lo:hi]), dyn0[lo:hi]))
    again = host(acc.partition_by_elev(idx, 0.25, part='full'))
    assert again['counts'][0] == out['counts'][2].item()
    acc.store.check_status()


# ---------------------------------------------------------------------------------------------- 5: grids, refusals, edges
def raw_call(st, prm, thresh, max_points, outputs=True, ws_bytes=None, first=0, last=None):
    """pca_bev_elev_partition itself; returns (rc, message, outputs)."""
    import torch
    ctx, lib = st.ctx, st.ctx.lib
    px = max(int(prm.px), 1)
    need = int(lib.pca_bev_elev_workspace_bytes(max_points, min(px, 1024)))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=st.device)
    elev = torch.full((min(px, 1024), min(px, 1024)), -7., dtype=torch.float64, device=st.device)
    flags = torch.full((max_points, ), 77, dtype=torch.uint8, device=st.device)
    counts = torch.full((3, ), -7, dtype=torch.int64, device=st.device)
    last = st.n_frames if last is None else last
    store = st.c_store()
    rc = lib.pca_bev_elev_partition(ctx.h, C.byref(store), st.frame_off.data_ptr(), st.head + first, st.head + last, max_points,
                                    C.byref(prm), thresh, 0, None, None, 0, ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                                    elev.data_ptr() if outputs else None, None, flags.data_ptr() if outputs else None,
                                    counts.data_ptr() if outputs else None, ctx.stream())
    return rc, lib.pca_last_error(ctx.h).decode(), (elev, flags, counts)


@pytest.mark.parametrize('px', [1, 7, 8, 9, 1024])
def test_grid_sizes_against_the_model(T, px):
    rng = np.random.default_rng(100 + px)
    frames = [ec.random_rows(rng, 1500, 12.) for _ in range(2)]
    rows = np.concatenate(frames)
    origin, R, dx, dy, view, hf = (0.5, -0.25, 0.125), ec.rotation(0.3), 0.3, -0.2, 20., 2.5
    st = dev_store(capacity=4096, max_frames=4)
    assert st.load_rows(frames) is None
    for thresh, include_dyn in ((0.25, False), (0., True), (-0.5, False)):
        out = st.bev_elev_partition(params(origin, R, dx, dy, view, px, hf), thresh, include_dyn=include_dyn)
        want = ec.model(rows, origin, R, dx, dy, view, px, hf, thresh, include_dyn)
        ec.compare(out, want)
        assert 800 < want['counts'][0] < 3000
    st.check_status()


def test_refusals_the_cut_window_and_empty_windows(T):
    from pca_amd import _lib
    rng = np.random.default_rng(5)
    frames = [ec.random_rows(rng, 1000, 12.) for _ in range(2)]
    rows = np.concatenate(frames)
    origin, R, view, px = (0., 0., 0.), ec.rotation(0.3), 20., 32
    st = dev_store(capacity=4096, max_frames=4)
    assert st.load_rows(frames) is None
    prm = params(origin, R, 0., 0., view, px, None)
    # a window above max_points is cut there; flags beyond the cut are not written
    cut = 700
    out = st.bev_elev_partition(prm, 0.2, max_points=cut)
    ec.compare(out, ec.model(rows[:cut], origin, R, 0., 0., view, px, None, 0.2, False))
    rc, _, (elev, flags, counts) = raw_call(st, prm, 0.2, cut)
    assert rc == 0 and (flags.cpu().numpy() != 77).all() and counts[0].item() == out['counts'][0].item()
    big = T.full((2000, ), 77, dtype=T.uint8, device=st.device)
    ctx, lib = st.ctx, st.ctx.lib
    ws = T.empty(int(lib.pca_bev_elev_workspace_bytes(cut, px)) + 256, dtype=T.uint8, device=st.device)
    store = st.c_store()
    assert lib.pca_bev_elev_partition(ctx.h, C.byref(store), st.frame_off.data_ptr(), 0, 2, cut, C.byref(prm), 0.2, 0, None, None,
                                      0, ws.data_ptr(), ws.numel(), None, None, big.data_ptr(), None, ctx.stream()) == 0
    big = big.cpu().numpy()
    assert np.array_equal(big[:cut], out['flags'].cpu().numpy()) and (big[cut:] == 77).all()
    # refusals: -1 with the message, nothing launched, the status word (STORE_OVERFLOW from the cut) as it was
    ctx.profile(1)
    bad_R = np.array([[1., 0., 0.], [0., np.cos(0.1), -np.sin(0.1)], [0., np.sin(0.1), np.cos(0.1)]])
    for bad, msg in ((dict(prm=params(origin, R, 0., 0., view, 1025, None)), r'bev elev partition: px must be in 1\.\.1024'),
                     (dict(prm=params(origin, R, 0., 0., view, 0, None)), r'bev elev partition: px must be in 1\.\.1024'),
                     (dict(thresh=float('nan')), 'bev elev partition: elev_thresh is NaN'),
                     (dict(prm=params(origin, bad_R, 0., 0., view, px, None)), 'bev elev partition: R must be a rotation about the z axis'),
                     (dict(outputs=False), 'bev elev partition: bad arguments'),
                     (dict(ws_bytes=1024), 'bev elev partition: workspace too small')):
        args = dict(prm=prm, thresh=0.2, max_points=2000)
        args.update(bad)
        rc, err, (elev, flags, counts) = raw_call(st, **args)
        assert rc == -1 and re.match(msg, err), (err, msg)
        assert (elev == -7.).all().item() and (flags == 77).all().item() and (counts == -7).all().item()
    with pytest.raises(RuntimeError, match=r'bev elev partition: px must be in 1\.\.1024'):
        st.bev_elev_partition(params(origin, R, 0., 0., view, 1025, None), 0.2)
    with pytest.raises(RuntimeError, match='elev_thresh is NaN'):
        st.bev_elev_partition(prm, float('nan'))
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['bev_elev_bin'][1] == 0 and prof['bev_elev_cells'][1] == 0
    assert ctx.status() == _lib.STATUS_STORE_OVERFLOW            # (read and cleared here)
    # a negative threshold is legal
    out = st.bev_elev_partition(prm, -1e300)
    assert out['counts'][1].item() == out['counts'][0].item() > 500
    # empty windows: no frame at all in the range, and a store that holds nothing
    for store, args in ((st, dict(first_frame=1, last_frame=1)), (dev_store(capacity=1024, max_frames=4), {})):
        out = host(store.bev_elev_partition(prm, 0.2, **args))
        assert out['elev'].shape == (px, px) and not out['elev'].any() and not np.signbit(out['elev']).any()
        assert not out['observed'].any() and out['flags'].shape == (0, ) and out['counts'].tolist() == [0, 0, 0]
        store.check_status()


# ---------------------------------------------------------------------------------------------- 6: mark_dyn
def test_mark_dyn_writes_dyn_alone_and_the_next_raster_sees_it(T):
    rng = np.random.default_rng(8)
    frames = [ec.random_rows(rng, 4000, 30.) for _ in range(3)]
    rows = np.concatenate(frames)
    origin, R, dx, dy, view, px, hf = (0.4, -0.3, 0.2), ec.rotation(2.1), 1.75, -2.5, 60., 64, 2.5
    prm = params(origin, R, dx, dy, view, px, hf)
    st, twin = dev_store(capacity=1 << 14, max_frames=4), dev_store(capacity=1 << 14, max_frames=4)
    assert st.load_rows(frames) is None
    st.retransform(np.eye(4), defer=True)                        # something owed: a call that writes flushes it first
    quiet = st.bev_elev_partition(prm, 0.3)                      # off by default: the store stays as it is
    assert len(st._pending) == 1
    rows_before = [t[:rows.shape[0]].clone() for t in st._arrays()]
    out = st.bev_elev_partition(prm, 0.3, mark_dyn=True)
    assert not st._pending
    same(out, quiet)
    want = ec.model(rows, origin, R, dx, dy, view, px, hf, 0.3, False)
    ec.compare(out, want)
    dyn = np.where(want['flags'] == 1, 1., rows[:, 9])
    assert (dyn != rows[:, 9]).sum() == want['counts'][1] > 1000
    assert np.array_equal(st.dyn[:rows.shape[0]].cpu().numpy(), dyn.astype(np.uint8))
    for name, a, b in zip('x y z intensity rgbs inst'.split(), rows_before, st._arrays()):
        assert T.equal(a, b[:rows.shape[0]]), name
    # the rasters that follow: those of a store whose dyn was set by hand
    marked = [f.copy() for f in frames]
    k = 0
    for f in marked:
        f[:, 9] = dyn[k:k + f.shape[0]]
        k += f.shape[0]
    assert twin.load_rows(marked) is None
    a16, a64 = st.bev(2, prm, want_f64=True)
    b16, b64 = twin.bev(2, prm, want_f64=True)
    assert T.equal(a64.view(T.int64), b64.view(T.int64)) and T.equal(a16.view(T.int16), b16.view(T.int16))
    # nothing is elevated among what is left of the static partition's elevated points: they are dynamic now
    again = st.bev_elev_partition(prm, 0.3)
    assert again['counts'][0].item() == want['counts'][2]
    st.check_status()
    twin.check_status()
