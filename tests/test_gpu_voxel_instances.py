"""GPU: the object voxels of the window clustered into instances (pca_bev_voxel_instances, DeviceStore.bev_voxel_instances,
SemBEVGenerator.voxel_instances_device, SemanticPointCloudAccumulator.voxel_instances) against the numpy model of
tests/voxel_instances_common.py (pinned by tests/test_voxel_instances_model.py).  Every comparison is exact; every input is a
valid call or a refused one."""
import ctypes as C
import re

import numpy as np
import pytest

import voxel_instances_common as ic
import voxel_labels_common as vl
from test_gpu_kernels import T  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, frames_of, kitti_accumulator, loaded, owe, params

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (8, 5), (20, 32), (64, 7)]
ORIGIN, VIEW = (0.3, -0.2, 0.125), 40.
ROT = (vl.rotation(0.4), 0.5, -0.25)                             # a rotated and shifted view
LABELS5 = vl.table_of([[13], [14], [15], [17], [0, 1, 2]])        # the four movable classes and a fifth, wide label
LABELS19 = (vl.identity_table(19), 19)                            # label = class, every class of the random frames
MODES = {'static': 0, 'all': 1, 'dynamic': 2}
KERNELS = {'bev_voxel_bin': 1, 'bev_voxel_cells': 1, 'bev_inst_init': 1, 'bev_inst_merge': 2, 'bev_inst_compress': 2,
           'bev_inst_sums': 1, 'bev_inst_offsets': 1, 'bev_inst_number': 1, 'bev_inst_write': 1, 'bev_inst_points': 1}

_wants = {}


def want_of(key, *args, **kw):
    """The model's result for a case that several tests share, computed once."""
    if key not in _wants:
        _wants[key] = ic.model(*args, **kw)
    return _wants[key]


def mask_prm(px):
    origin, R, dx, dy, view, px, hf = ic.grid_of(px, 1)[:7]
    return params(origin, R, dx, dy, view, px, hf)


def mask_call(st, px, nz, **kw):
    return st.bev_voxel_instances(mask_prm(px), 0., 1., nz, *ic.DYN_LABELS, **kw)


def random_case(px, nz):
    """frames_of(1) in the rotated and shifted view, bins of 1/2 m from -1 m, height_filter inside the z range."""
    R, dx, dy = ROT
    return params(ORIGIN, R, dx, dy, VIEW, px, 2.5), (ORIGIN, R, dx, dy, VIEW, px, 2.5, -1., 0.5, nz)


# ---------------------------------------------------------------------------------------------- 1: the masks
@pytest.mark.parametrize('connectivity', [6, 26])
@pytest.mark.parametrize('px,nz', SHAPES)
def test_every_mask_equals_the_model(T, px, nz, connectivity):
    rng = np.random.default_rng(px * 100 + nz)
    done = []
    for name in sorted(ic.MASKS):
        m = ic.MASKS[name](px, nz)
        if m is None:
            continue
        rows = ic.rows_for_mask(m, 1 + (np.arange(m.size).reshape(m.shape) % 3), rng=rng)
        want = ic.model(rows, *ic.grid_of(px, nz), *ic.DYN_LABELS, connectivity=connectivity, mask=m)
        st = loaded([rows[:rows.shape[0] // 2], rows[rows.shape[0] // 2:]])
        ic.compare(mask_call(st, px, nz, connectivity=connectivity), want)
        st.check_status()
        done.append((name, want['n'], int(want['stats'][5])))
    print(px, nz, connectivity, done)
    assert len(done) == (1 if px == 1 else 7)                     # (1 x 1 x 1 holds the checkerboard's single voxel alone)
    if (px, nz) == (64, 7):                                       # the long path: one component of thousands of voxels
        assert ('serpentine', 1, 4 * (32 * 64 + 31) + 3) in done


def test_checkerboard_of_8192_singletons_and_the_cap_of_the_tables(T):
    px, nz = 64, 4
    m = ic.checkerboard(px, nz)
    rows = ic.rows_for_mask(m, rng=np.random.default_rng(5))
    st = loaded([rows])
    want = ic.model(rows, *ic.grid_of(px, nz), *ic.DYN_LABELS, connectivity=6, max_instances=100, mask=m)
    out = mask_call(st, px, nz, connectivity=6, max_instances=100)
    ic.compare(out, want)
    assert want['stats'].tolist() == [8192, 8192, 8192, 8192, 8192, 1] and out['table'].shape == (100, 9)
    assert out['inst'].max().item() == 8191 == out['ids'].max().item() and out['table'][99, 0].item() == 3 * 64 + 7
    # min_voxels = 2: nothing survives
    out = mask_call(st, px, nz, connectivity=6, min_voxels=2)
    ic.compare(out, ic.model(rows, *ic.grid_of(px, nz), *ic.DYN_LABELS, connectivity=6, min_voxels=2))
    assert out['stats'].tolist() == [8192, 8192, 8192, 0, 0, 0] and (out['inst'] == -1).all().item()
    assert (out['ids'] == -1).all().item() and not out['table'].any().item() and not out['label_counts'].any().item()
    assert (out['top_label'] == 255).all().item()
    st.check_status()


def test_the_largest_grid(T):
    """1024 x 1024 x 2: the scan over 2 M flags (512 tiles) and places above 2^20.  frames_of(2) in the middle and a spiral arm
    across the whole of plane 0, a turn every 64 cells."""
    px, nz = 1024, 2
    arm = ic.rows_for_mask(ic.spiral(px, nz, pitch=64))
    frames = list(frames_of(2)) + [arm]
    table = vl.identity_table(19)
    st = loaded(frames, capacity=1 << 16)
    want = ic.model(frames, *ic.grid_of(px, nz), table, 19, connectivity=6)
    out = st.bev_voxel_instances(mask_prm(px), 0., 1., nz, table, 19, connectivity=6)
    ic.compare(out, want)
    assert want['stats'][5] > 15000 and want['table'][:want['n'], 0].max() > 1 << 20 and want['n'] > 100
    st.check_status()


# ---------------------------------------------------------------------------------------------- 2: random frames
@pytest.mark.parametrize('min_points', [1, 3])
@pytest.mark.parametrize('dyn', ['static', 'all', 'dynamic'])
def test_random_frames_in_a_rotated_view_and_the_counts_of_the_voxel_labels(T, dyn, min_points):
    frames = frames_of(1)
    st = loaded(frames)
    n = lost = 0
    for px, nz in ((20, 8), (64, 7)):
        prm, grid = random_case(px, nz)
        want = want_of(('19', px, nz, dyn, min_points), frames, *grid, *LABELS19, dyn_mode=MODES[dyn], min_points=min_points)
        out = st.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS19, min_points=min_points, dyn=dyn)
        ic.compare(out, want)
        n, lost = n + want['n'], lost + int(want['stats'][0] - want['stats'][4])
        if dyn != 'dynamic':                                      # the reuse claim: the thresholded counts ARE the voxel labels' counts
            counts = st.bev_voxel_labels(prm, -1., 0.5, nz, *LABELS19, include_dyn=dyn == 'all')['counts'].cpu().numpy()
            assert np.array_equal(counts.view(np.uint32), want['counts'])
            fg = want['counts'] >= min_points
            assert fg.sum() == want['stats'][1] and np.array_equal(out['inst'].cpu().numpy() >= 0, fg)
    print(dyn, min_points, 'components', n, 'kept points without an instance', lost)
    assert n >= 4 and (lost > 100) == (min_points == 3)           # (the case cannot go soft)
    st.check_status()


def test_the_order_of_the_points_and_of_the_frames_does_not_matter(T):
    frames, (px, nz) = frames_of(1), (64, 7)
    rows = np.concatenate(frames)
    prm, grid = random_case(px, nz)
    a = loaded(frames).bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, dyn='all')
    perm = np.random.default_rng(9).permutation(rows.shape[0])
    mixed = rows[perm]
    st = loaded([mixed[:100], mixed[100:100], mixed[100:7001], mixed[7001:]])
    b = st.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, dyn='all')
    for k in ('inst', 'table', 'label_counts', 'top_label', 'stats'):
        assert T.equal(a[k], b[k]), k
    assert T.equal(a['ids'][T.from_numpy(perm).to(a['ids'].device)], b['ids'])
    assert a['stats'][3].item() >= 5
    st.check_status()


@pytest.mark.parametrize('G', ['1', '3'])
def test_few_workgroups_walk_the_grid_and_the_window_in_rounds(T, monkeypatch, G):
    """PCA_BEV_INST_G: one and three workgroups take the 112 blocks of the 64 x 64 x 7 grid, its 7 scan tiles and the 47 chunks of
    the window in rounds."""
    monkeypatch.setenv('PCA_BEV_INST_G', G)
    frames, (px, nz) = frames_of(1), (64, 7)
    prm, grid = random_case(px, nz)
    st = loaded(frames)
    ic.compare(st.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, dyn='all'),
               want_of(('5', px, nz, 'all', 1), frames, *grid, *LABELS5, dyn_mode=1, min_points=1))
    m = ic.serpentine(px, nz)
    rows = ic.rows_for_mask(m, rng=np.random.default_rng(2))
    st = loaded([rows])
    ic.compare(mask_call(st, px, nz, connectivity=6), ic.model(rows, *ic.grid_of(px, nz), *ic.DYN_LABELS, connectivity=6, mask=m))
    st.check_status()


def test_the_launch_count_does_not_depend_on_the_data(T):
    """The structural claim: two voxel levels and ten launches, whatever the mask."""
    px, nz = 20, 32
    for name in ('serpentine', 'checkerboard'):
        st = loaded([ic.rows_for_mask(ic.MASKS[name](px, nz))])
        st.ctx.profile(1)
        mask_call(st, px, nz)
        prof = st.ctx.profile_read()
        st.ctx.profile(0)
        assert {k: prof[k][1] for k in KERNELS} == KERNELS, name
        st.check_status()


# ---------------------------------------------------------------------------------------------- 3: owed transforms, a noted K1
def test_owed_chain_over_part_of_the_window(T):
    from test_gpu_kernels import _tilting_transform
    frames, ends = frames_of(2), (1, 2, 2, 3)
    px, nz = 64, 7
    prm, grid = random_case(px, nz)
    lazy, twin = loaded(frames), loaded(frames)
    for st in (lazy, twin):
        st.CHAIN_K = 4
        for step, e in enumerate(ends):
            owe(st, _tilting_transform(step), e)
    eager = twin.frame_rows()                                    # K2 writes the transforms into the twin's store
    assert not twin._pending
    n_rows = sum(f.shape[0] for f in frames)
    before = [t[:n_rows].clone() for t in lazy._arrays()]
    pending = [(np.array(Tm).copy(), e) for Tm, e in lazy._pending]
    want = ic.model(eager, *grid, *LABELS5, dyn_mode=1)
    ic.compare(lazy.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, dyn='all'), want)
    ic.compare(twin.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, dyn='all'), want)
    assert not np.array_equal(want['inst'], ic.model(frames, *grid, *LABELS5, dyn_mode=1)['inst'])
    assert len(lazy._pending) == len(ends)                       # still owed, and the same list
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(pending, lazy._pending))
    assert all(T.equal(a, b[:n_rows]) for a, b in zip(before, lazy._arrays()))       # no store column was written
    for st in (lazy, twin):
        st.check_status()


def test_noted_k1_runs_before_the_pass(T, tmp_path, monkeypatch):
    """The pattern of test_gpu_window_passes.py."""
    table = vl.identity_table(19)
    out = []
    for fuse in ('1', '0'):
        monkeypatch.setenv('PCA_FUSE_K1', fuse)
        acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=6)
        st = acc.store
        assert (st._k1_noted is not None) == (fuse == '1')       # integrate() left the newest frame's K1 for the next raster
        prm = params((0., 0., 0.), 0.3, 0., 0., 50., 32, None)
        if fuse == '1':                                           # a refused call runs nothing: the K1 is still noted
            with pytest.raises(RuntimeError, match='bev voxel instances: connectivity must be 6 or 26'):
                st.bev_voxel_instances(prm, -2., 1.6, 4, table, 19, connectivity=18)
            assert st._k1_noted is not None
        res = st.bev_voxel_instances(prm, -2., 1.6, 4, table, 19)
        assert st._k1_noted is None
        out.append([v.cpu().numpy() for v in res.values()])
        st.check_status()
        st.set_defer_k1(False)
    assert all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(*out))
    assert all(x.any() for x in out[0])


# ---------------------------------------------------------------------------------------------- 4: cut and empty windows
def test_window_above_max_points_is_cut_and_says_so(T):
    from pca_amd import _lib
    frames, (px, nz) = frames_of(1), (20, 8)
    prm, grid = random_case(px, nz)
    st = loaded(frames)
    cut = 6700                                                    # inside the second frame
    want = ic.model(frames, *grid, *LABELS5, max_points=cut)
    out = st.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, max_points=cut)
    ic.compare(out, want)
    assert out['ids'].shape == (cut, ) and st.ctx.status() == _lib.STATUS_STORE_OVERFLOW       # (read and cleared here)
    assert not np.array_equal(want['inst'], ic.model(frames, *grid, *LABELS5)['inst'])
    # ids beyond the cut are not written
    r, _, (inst, ids, table, label_counts, stats) = raw_call(st, prm, max_points=cut, nz=nz, labels=LABELS5)
    assert r == 0 and np.array_equal(ids[:cut].cpu().numpy(), want['ids']) and (ids[cut:] == 7).all().item()
    assert stats.tolist() == want['stats'].tolist() and st.ctx.status() == _lib.STATUS_STORE_OVERFLOW
    st.check_status()


def test_empty_frames_and_empty_windows(T):
    rng = np.random.default_rng(11)
    a, b = vl.random_rows(rng, 3000, 25.), vl.random_rows(rng, 2000, 25.)
    frames = [a, np.zeros((0, 10)), b, np.zeros((0, 10)), np.zeros((0, 10))]
    px, nz = 20, 8
    prm, grid = random_case(px, nz)
    st = loaded(frames)
    ic.compare(st.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5), ic.model(frames, *grid, *LABELS5))
    ic.compare(st.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, first_frame=1), ic.model(frames[1:], *grid, *LABELS5))
    # the window of the empty frames alone, and of no frame at all: inst -1, zeros, no ids
    for f0, f1 in ((3, 5), (2, 2)):
        out = st.bev_voxel_instances(prm, -1., 0.5, nz, *LABELS5, first_frame=f0, last_frame=f1)
        assert (out['inst'] == -1).all().item() and out['stats'].tolist() == [0] * 6 and out['ids'].shape == (0, )
        assert not out['table'].any().item() and not out['label_counts'].any().item() and (out['top_label'] == 255).all().item()
    r, _, (inst, ids, table, label_counts, stats) = raw_call(st, prm, nz=nz, labels=LABELS5, slots=(st.head + 2, st.head + 2))
    assert r == 0 and (inst[:nz] == -1).all().item() and (ids == 7).all().item() and stats.tolist() == [0] * 6
    assert not table[:32].any().item() and not label_counts[:32 * 5].any().item()             # (max_instances = 32 rows are cleared)
    assert (table[32:] == 7).all().item() and (label_counts[32 * 5:] == 7).all().item()
    st.check_status()


# ---------------------------------------------------------------------------------------------- 5: the top level
def test_movers_and_parked_things_on_a_kitti_drive(T, tmp_path):
    """The street scene of the carve's tests (a wall, a parked block of car points in every frame, a second block in the first
    frame only) put into the store of a KITTI drop-in of three frames, in the un-augmented frame of its last sample: after
    carve_dynamic(mark_dyn=True) the movers are one instance, the block that left, and the static things are one, the parked."""
    import voxel_carve_common as cc
    from pca_amd import host_logic as hl
    acc, idx = kitti_accumulator(tmp_path, dict(BEV_KITTI, view_size=64, pixel_size=64), n_frames=3), 2
    gen = acc.sem_bev_generator
    poses = np.array(acc.poses)
    origin = poses[idx]
    R = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:idx] - origin))
    frames_v, sensors_v, kind = cc.street_scene()
    frames = []
    for f in frames_v:                                           # view frame -> store: X = R^T p + origin
        f = f.copy()
        f[:, 0:3] = f[:, 0:3] @ R + origin
        frames.append(f)
    sensors = sensors_v @ R + origin
    assert acc.store.load_rows(frames) is None
    z_range, nz, view, px = (0., 4.), 4, 64., 64
    carved = acc.carve_dynamic(idx, part='full', z_range=z_range, nz=nz, origins=sensors, mark_dyn=True)
    want_c = cc.model(frames, sensors, origin, R, 0., 0., view, px, 0., 1., nz, False, gen.dynamic_classes())
    cc.compare(carved, want_c)
    assert np.array_equal(want_c['flags'] == 1, kind == 1)        # the block that left is flagged whole, nothing else
    rows = np.concatenate(frames)
    rows[:, 9] = want_c['flags'] == 1
    assert np.array_equal(acc.store.dyn[:rows.shape[0]].cpu().numpy(), rows[:, 9].astype(np.uint8))
    grid = (origin, R, 0., 0., view, px, None, 0., 1., nz)
    for dyn, who in (('dynamic', 1), ('static', 2)):
        out = acc.voxel_instances(idx, part='full', z_range=z_range, nz=nz, dyn=dyn)
        want = ic.model(rows, *grid, *ic.DYN_LABELS, dyn_mode=MODES[dyn])
        ic.compare(out, want)
        assert want['n'] == 1 and np.array_equal(want['ids'] >= 0, kind == who), dyn
        assert want['table'][0, 2] == (kind == who).sum() and want['top_label'][0] == 0
        boxes = hl.instance_boxes(out['table'].cpu().numpy(), 1, view, px, 0., 1.)
        assert boxes.shape == (1, 6) and (boxes[0, 1::2] - boxes[0, 0::2] <= [2., 4., 2.]).all()
    # the generator on host rows in BEV-frame metres equals the window form; classes as lists, names taken too
    rel = rows.copy()
    rel[:, 0:3] -= origin
    host = gen.voxel_instances_device(rel, R, 0., 0., view, z_range, nz, classes=[['car'], [14], [15], [17]], dyn='static')
    assert all(T.equal(host[k], out[k]) for k in out)
    every = acc.voxel_instances(idx, part='present', z_range=z_range, nz=nz, classes=[[cc.WALL], ['car']], dyn='all', connectivity=6)
    n_present = frames[0].shape[0] + frames[1].shape[0]
    ic.compare(every, ic.model(rows[:n_present], *grid, *vl.table_of([[cc.WALL], [13]]), dyn_mode=1, connectivity=6))
    with pytest.raises(ValueError):
        acc.voxel_instances(idx, part='past')
    with pytest.raises(ValueError, match='dyn'):
        acc.voxel_instances(idx, dyn='moving')
    acc.store.check_status()


# ---------------------------------------------------------------------------------------------- 6: the C ABI's checks
def raw_call(st, prm, max_points=20000, z_lo=-1., z_step=0.5, nz=4, labels=LABELS5, label_of=True, dyn_mode=0, min_points=1,
             connectivity=26, min_voxels=1, max_instances=32, outputs=(True, ) * 5, pending=None, slots=None, ws_bytes=None,
             workspace=True):
    """pca_bev_voxel_instances itself; returns (rc, message, (inst, ids, table, label_counts, stats))."""
    import torch
    ctx, lib = st.ctx, st.ctx.lib
    px = min(max(int(prm.px), 1), 64)
    table_of, n_labels = labels
    inst = torch.full((32, px, px), 7, dtype=torch.int32, device=st.device)        # (a refused call writes nothing)
    ids = torch.full((20000, ), 7, dtype=torch.int32, device=st.device)
    table = torch.full((64, 9), 7, dtype=torch.int32, device=st.device)
    label_counts = torch.full((64 * 32, ), 7, dtype=torch.int32, device=st.device)     # (flat: the call's rows are n_labels long)
    stats = torch.full((6, ), 7, dtype=torch.int64, device=st.device)
    outs = [t.data_ptr() if on else None for t, on in zip((inst, ids, table, label_counts, stats), outputs)]
    need = int(lib.pca_bev_instances_workspace_bytes(min(max_points, 1 << 20), px, min(max(nz, 1), 32), 64))
    ws = torch.empty(need, dtype=torch.uint8, device=st.device)
    store = st.c_store()
    b, e = (st.head, st.head + st.n_frames) if slots is None else slots
    if pending is None:
        pT, pE, nP = None, None, 0
    else:
        Ts, ends, nP = pending
        pT = None if Ts is None else (C.c_double * len(Ts))(*Ts)
        pE = None if ends is None else (C.c_int * len(ends))(*ends)
    host_table = np.ascontiguousarray(table_of, dtype=np.uint8)
    r = lib.pca_bev_voxel_instances(ctx.h, C.byref(store), st.frame_off.data_ptr(), b, e, max_points, C.byref(prm), z_lo, z_step, nz,
                                    host_table.ctypes.data if label_of else None, n_labels, dyn_mode, min_points, connectivity,
                                    min_voxels, max_instances, pT, pE, nP, ws.data_ptr() if workspace else None,
                                    need if ws_bytes is None else ws_bytes, *outs, ctx.stream())
    torch.cuda.synchronize()
    return r, lib.pca_last_error(ctx.h).decode(), (inst, ids, table, label_counts, stats)


def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    frames = frames_of(1)
    R, px = vl.rotation(0.3), 32
    st = loaded(frames)
    prm = params(ORIGIN, R, 0., 0., VIEW, px)
    ctx = st.ctx
    want = ic.model(frames, ORIGIN, R, 0., 0., VIEW, px, None, -1., 0.5, 4, *LABELS5, max_instances=32)
    names = ('inst', 'ids', 'table', 'label_counts', 'stats')
    rows_of = {'inst': 4, 'ids': 12000, 'table': 32, 'label_counts': 32 * 5, 'stats': 6}

    def written(name, t):
        """The output holds the model's result, and what lies behind it is untouched (label_counts: 32 rows of 5 labels)."""
        n = rows_of[name]
        got = t[:n].cpu().numpy().astype(np.int64)
        return np.array_equal(got.reshape(want[name].shape), want[name]) and (t[n:] == 7).all().item()
    r, _, outs = raw_call(st, prm)                                # the call as such is fine
    assert r == 0 and all(written(n, t) for n, t in zip(names, outs)) and want['n'] > 32
    for k in range(5):                                            # any output alone
        r, _, outs = raw_call(st, prm, outputs=tuple(j == k for j in range(5)))
        assert r == 0 and written(names[k], outs[k]), names[k]
        assert all((t == 7).all().item() for j, t in enumerate(outs) if j != k), names[k]
    ctx.profile(1)
    bad_R = np.array([[1., 0., 0.], [0., np.cos(0.1), -np.sin(0.1)], [0., np.sin(0.1), np.cos(0.1)]])
    eye = [float(v) for v in np.eye(4).reshape(-1)]
    nan, inf = float('nan'), float('inf')
    h = st.head
    bad_table = LABELS5[0].copy()
    bad_table[200] = 5
    what = 'bev voxel instances: '
    cases = [(dict(prm=params(ORIGIN, R, 0., 0., VIEW, 1025)), r'px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, R, 0., 0., VIEW, 0)), r'px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, bad_R, 0., 0., VIEW, px)), 'R must be a rotation about the z axis'),
             (dict(outputs=(False, ) * 5), 'bad arguments'),
             (dict(label_of=False), 'bad arguments'),
             (dict(workspace=False), 'bad arguments'),
             (dict(ws_bytes=1024), 'workspace too small'),
             (dict(max_points=1 << 31), 'max_points must be below 2\\^31'),
             (dict(slots=(h + 2, h + 1)), 'need slot_begin <= slot_end'),
             (dict(labels=(bad_table, 5)), r'label_of\[200\] must be below n_labels, or 255'),
             (dict(pending=(eye * 5, [h + 1] * 5, 5)), 'bad chain of owed transforms'),
             (dict(pending=(eye, [h + 4], 1)), 'a pending slot end lies beyond the window'),
             (dict(pending=(eye * 2, [h + 2, h + 1], 2)), 'pending slot ends must ascend')]
    cases += [(dict(nz=v), r'nz must be in 1\.\.32') for v in (0, -1, 33)]
    cases += [(dict(labels=(LABELS5[0], v)), r'n_labels must be in 1\.\.32') for v in (0, 33)]
    cases += [(dict(z_lo=v), 'z_lo must be finite') for v in (nan, inf, -inf)]
    cases += [(dict(z_step=v), 'z_step must be finite and > 0') for v in (0., -0.5, nan, inf)]
    cases += [(dict(connectivity=v), 'connectivity must be 6 or 26') for v in (0, 4, 18, 27)]
    cases += [(dict(max_instances=v), r'max_instances must be in 1\.\.65536') for v in (0, -1, 65537)]
    cases += [(dict(min_points=v), 'min_points must be >= 1') for v in (0, -3)]
    cases += [(dict(min_voxels=v), 'min_voxels must be >= 1') for v in (0, -3)]
    cases += [(dict(dyn_mode=v), 'dyn_mode must be 0, 1 or 2') for v in (-1, 3)]
    for bad, msg in cases:
        args = dict(prm=prm)
        args.update(bad)
        r, err, outs = raw_call(st, **args)
        assert r == -1 and re.match(what + msg, err), (err, msg)
        assert all((t == 7).all().item() for t in outs), msg
    with pytest.raises(RuntimeError, match=r'bev voxel instances: nz must be in 1\.\.32'):
        st.bev_voxel_instances(prm, -1., 0.5, 33, *LABELS5)
    with pytest.raises(RuntimeError, match=r'max_instances must be in 1\.\.65536'):
        st.bev_voxel_instances(prm, -1., 0.5, 4, *LABELS5, max_instances=65537)
    with pytest.raises(ValueError, match='256 entries'):
        st.bev_voxel_instances(prm, -1., 0.5, 4, LABELS5[0][:100], 5)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert all(prof[k][1] == 0 for k in KERNELS)
    # the limits themselves are legal
    r, _, (inst, ids, table, label_counts, stats) = raw_call(st, prm, max_instances=1)
    assert r == 0 and stats.tolist() == want['stats'].tolist() and np.array_equal(table[:1].cpu().numpy(), want['table'][:1])
    assert (table[1:] == 7).all().item() and np.array_equal(inst[:4].cpu().numpy(), want['inst'])
    st.check_status()
