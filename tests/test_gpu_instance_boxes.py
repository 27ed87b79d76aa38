"""GPU: oriented metric boxes around the window's instances (pca_bev_instance_boxes, DeviceStore.bev_instance_boxes,
SemBEVGenerator.instance_boxes_device, SemanticPointCloudAccumulator.instance_boxes) against the numpy model of
tests/instance_boxes_common.py (pinned by tests/test_instance_boxes_model.py).  Every comparison with the model is exact;
every input is a valid call or a refused one."""
import ctypes as C
import re

import numpy as np
import pytest

import instance_boxes_common as bc
from test_gpu_kernels import T  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, frames_of, kitti_accumulator, loaded, owe, params

pytestmark = pytest.mark.gpu

VIEW, PX = 40., 32
KERNELS = {'bev_box_table': 1, 'bev_box_count': 1, 'bev_box_offsets': 1, 'bev_box_scatter': 1, 'bev_box_extents': 1,
           'bev_box_near': 1, 'bev_box_choose': 1}
CRITERIA = {0: 'area', 1: 'edge'}


def prm_of(px=PX):
    origin, R, dx, dy = bc.frame()
    return params(origin, R, dx, dy, VIEW, px)


def angles(n):
    from pca_amd.host_logic import fit_angles
    return fit_angles(n)


def cut_frames(rows, *cuts):
    """The rows as frames, cut at the given places (an empty frame where two cuts meet)."""
    edges = [0] + list(cuts) + [rows.shape[0]]
    return [rows[a:b] for a, b in zip(edges[:-1], edges[1:])]


def boxes_call(T, st, ids, n_rows, cs, criterion, **kw):
    ids = T.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
    kw.setdefault('extents', True)
    kw.setdefault('near', True)
    return st.bev_instance_boxes(prm_of(), ids, n_rows, cs, criterion=CRITERIA[criterion], **kw)


def check_boxes(out, cs):
    """'boxes' is host_logic.oriented_boxes of 'fit', to 1e-12 (a few f64 operations in another order), NaN where it is NaN."""
    from pca_amd.host_logic import oriented_boxes
    want, _ = oriented_boxes(out['fit'].cpu().numpy(), cs)
    got = out['boxes'].cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 1: the scenes
def scenes():
    theta17 = 17 * (0.5 * np.pi) / 90
    return {'rectangle': (bc.rectangle_scene(theta17), 90), 'l': (bc.l_scene(), bc.L_ANGLES), 'point': (bc.point_scene(1), 90),
            'two_points': (bc.point_scene(2), 90), 'random': (bc.random_scene(), 90)}


@pytest.mark.parametrize('criterion', [0, 1])
@pytest.mark.parametrize('name', ['rectangle', 'l', 'point', 'two_points', 'random'])
def test_every_scene_equals_the_model(T, name, criterion):
    (rows, ids, n_rows), n_angles = scenes()[name]
    cs = angles(n_angles)
    st = loaded(cut_frames(rows, rows.shape[0] // 3, rows.shape[0] // 3))
    want = bc.model(ids, rows, *bc.frame(), n_rows, cs, criterion, 0.2, want_near=True)
    out = boxes_call(T, st, ids, n_rows, cs, criterion)
    bc.compare(out, want)
    check_boxes(out, cs)
    if name == 'rectangle':
        assert want['t'][0] == 17
    if name == 'l':
        assert want['t'][0] == (6 if criterion else 1)
    # without the optional outputs: the same fit; near_t* is 0 where near_t was not needed
    lean = boxes_call(T, st, ids, n_rows, cs, criterion, extents=False, near=False)
    assert sorted(lean) == ['boxes', 'fit', 'fit_n', 'stats']
    bc.compare(lean, bc.model(ids, rows, *bc.frame(), n_rows, cs, criterion, 0.2))
    assert T.equal(lean['fit'].view(T.int64), out['fit'].view(T.int64)) and (criterion == 1 or not lean['fit_n'][:, 1].any().item())
    st.check_status()


@pytest.mark.parametrize('n_angles', [1, 7, 200, 256])
def test_tables_of_other_lengths(T, n_angles):
    """One direction; 36 lane groups of 7; more directions than half the threads (one lane group, two table launches)."""
    rows, ids, n_rows = bc.random_scene(n=3000, n_rows=9, seed=6)
    cs = angles(n_angles)
    st = loaded([rows])
    for criterion in (0, 1):
        bc.compare(boxes_call(T, st, ids, n_rows, cs, criterion), bc.model(ids, rows, *bc.frame(), n_rows, cs, criterion, 0.2, want_near=True))
    st.check_status()


# ---------------------------------------------------------------------------------------------- 2: several pieces, few workgroups
_big = {}


def big_want(criterion):
    if criterion not in _big:
        rows, ids, n_rows = bc.big_row_scene()
        _big[criterion] = bc.model(ids, rows, *bc.frame(), n_rows, angles(45), criterion, 0.2, want_near=True)
    return _big[criterion]


@pytest.mark.parametrize('G', [None, '1', '3'])
def test_a_row_of_several_pieces(T, monkeypatch, G):
    """5 000 points in one row: three pieces that combine by atomics.  PCA_BEV_BOXES_G: one and three workgroups take the 22
    chunks of the window, the pieces and the rows in rounds -- the same bits."""
    if G is not None:
        monkeypatch.setenv('PCA_BEV_BOXES_G', G)
    rows, ids, n_rows = bc.big_row_scene()
    st = loaded([rows])
    for criterion in (0, 1):
        want = big_want(criterion)
        assert want['stats'][3] > 2 * bc.PIECE
        bc.compare(boxes_call(T, st, ids, n_rows, angles(45), criterion), want)
    st.check_status()


def test_the_order_of_the_points_and_of_the_frames_does_not_matter(T):
    rows, ids, n_rows = bc.big_row_scene()
    cs = angles(45)
    perm = np.random.default_rng(9).permutation(rows.shape[0])
    a = boxes_call(T, loaded([rows]), ids, n_rows, cs, 1)
    st = loaded(cut_frames(rows[perm], 100, 100, 3001))
    b = boxes_call(T, st, ids[perm], n_rows, cs, 1)
    frames = cut_frames(rows, 1500, 4000)
    st2 = loaded(frames[::-1])
    c = boxes_call(T, st2, np.concatenate(cut_frames(ids, 1500, 4000)[::-1]), n_rows, cs, 1)
    for other in (b, c):
        for k in ('fit', 'extents'):
            assert T.equal(a[k].view(T.int64), other[k].view(T.int64)), k
        assert all(T.equal(a[k], other[k]) for k in ('fit_n', 'near', 'stats'))
    st.check_status()


def test_ids_behind_the_rows_are_skipped_and_nothing_is_written_behind_them(T):
    rows, ids, n_rows = bc.singles_scene()
    cs = angles(4)
    st = loaded([rows])
    want = bc.model(ids, rows, *bc.frame(), n_rows, cs, 1, 0.2, want_near=True)
    assert want['stats'].tolist() == [4096, 4096, 4096, 1]
    out = boxes_call(T, st, ids, n_rows, cs, 1)
    bc.compare(out, want)
    assert (out['fit'][:, 6] == 0).all().item() and (out['fit'][:, 7] == 0).all().item()       # a point alone: t* = 0
    r, _, outs = raw_call(st, ids, n_rows=n_rows, cs=cs, criterion=1, spare=16)
    assert r == 0
    for t, name in zip(outs, ('fit', 'fit_n', 'extents', 'near')):
        flat = t.reshape(n_rows + 16, -1)
        assert np.array_equal(flat[:n_rows].cpu().numpy().reshape(want[name].shape), want[name].astype(flat.cpu().numpy().dtype)), name
        assert (flat[n_rows:] == 7).all().item(), name
    assert outs[4].tolist() == want['stats'].tolist()
    st.check_status()


def test_the_launch_count_does_not_depend_on_the_data(T):
    """The structural claim: seven launches whatever the scene, six where near_t is not needed."""
    cs = angles(90)
    for scene in (bc.big_row_scene(), bc.singles_scene(), bc.point_scene()):
        rows, ids, n_rows = scene
        st = loaded([rows])
        for criterion, near in ((1, False), (0, True), (0, False)):
            st.ctx.profile(1)
            boxes_call(T, st, ids, n_rows, cs, criterion, extents=False, near=near)
            prof = st.ctx.profile_read()
            st.ctx.profile(0)
            want = dict(KERNELS, bev_box_near=1 if criterion == 1 or near else 0)
            assert {k: prof[k][1] for k in KERNELS} == want, (n_rows, criterion, near)
        st.check_status()


# ---------------------------------------------------------------------------------------------- 3: owed transforms, a noted K1
def frames_ids(n, n_rows, seed=12):
    return np.random.default_rng(seed).integers(-1, n_rows + 2, n).astype(np.int32)


def test_owed_chain_over_part_of_the_window(T):
    from test_gpu_kernels import _tilting_transform
    frames, ends = frames_of(2), (1, 2, 2, 3)
    lazy, twin = loaded(frames), loaded(frames)
    for st in (lazy, twin):
        st.CHAIN_K = 4
        for step, e in enumerate(ends):
            owe(st, _tilting_transform(step), e)
    eager = twin.frame_rows()                                    # K2 writes the transforms into the twin's store
    assert not twin._pending
    n_pts = sum(f.shape[0] for f in frames)
    ids, n_rows, cs = frames_ids(n_pts, 10), 10, angles(30)
    before = [t[:n_pts].clone() for t in lazy._arrays()]
    pending = [(np.array(Tm).copy(), e) for Tm, e in lazy._pending]
    want = bc.model(ids, eager, *bc.frame(), n_rows, cs, 1, 0.2, want_near=True)
    bc.compare(boxes_call(T, lazy, ids, n_rows, cs, 1), want)
    bc.compare(boxes_call(T, twin, ids, n_rows, cs, 1), want)
    assert not bc.same_f64(want['fit'], bc.model(ids, frames, *bc.frame(), n_rows, cs, 1, 0.2)['fit'])
    assert len(lazy._pending) == len(ends)                       # still owed, and the same list
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(pending, lazy._pending))
    assert all(T.equal(a, b[:n_pts]) for a, b in zip(before, lazy._arrays()))        # no store column was written
    for st in (lazy, twin):
        st.check_status()


def test_noted_k1_runs_before_the_pass(T, tmp_path, monkeypatch):
    """The pattern of test_gpu_window_passes.py."""
    out = []
    for fuse in ('1', '0'):
        monkeypatch.setenv('PCA_FUSE_K1', fuse)
        acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=6)
        st = acc.store
        assert (st._k1_noted is not None) == (fuse == '1')       # integrate() left the newest frame's K1 for the next raster
        prm = params((0., 0., 0.), 0.3, 0., 0., 50., 32, None)
        ids = T.zeros(st.max_window_points(), dtype=T.int32, device=st.device)      # every point in row 0
        ids[::3] = 1
        if fuse == '1':                                           # a refused call runs nothing: the K1 is still noted
            bad = angles(8)
            bad[3, 1] = np.nan
            with pytest.raises(RuntimeError, match='bev instance boxes: every entry of cos_sin must be finite'):
                st.bev_instance_boxes(prm, ids, 2, bad)
            assert st._k1_noted is not None
        res = st.bev_instance_boxes(prm, ids, 2, angles(8), criterion='edge', extents=True, near=True)
        assert st._k1_noted is None
        out.append({k: v.cpu().numpy() for k, v in res.items()})
        st.check_status()
        st.set_defer_k1(False)
    assert all(out[0][k].tobytes() == out[1][k].tobytes() for k in out[0])
    lo, hi = st.frame_off[[st.head, st.head + st.n_frames]].tolist()
    assert out[0]['stats'].tolist()[:3] == [hi - lo, 0, 2] and np.isfinite(out[0]['fit']).all()


# ---------------------------------------------------------------------------------------------- 4: cut and empty windows
def test_window_above_max_points_is_cut_and_says_so(T):
    from pca_amd import _lib
    rows, ids, n_rows = bc.random_scene()
    cs = angles(12)
    st = loaded(cut_frames(rows, 2500))
    cut = 2700                                                    # inside the second frame
    want = bc.model(ids, rows, *bc.frame(), n_rows, cs, 1, 0.2, want_near=True, max_points=cut)
    out = boxes_call(T, st, ids, n_rows, cs, 1, max_points=cut)
    bc.compare(out, want)
    assert want['stats'][0] < cut and st.ctx.status() == _lib.STATUS_STORE_OVERFLOW           # (read and cleared here)
    assert not bc.same_f64(want['fit'], bc.model(ids, rows, *bc.frame(), n_rows, cs, 1, 0.2)['fit'])
    # ids of exactly the cut's length are enough: nothing behind the cut is read
    bc.compare(boxes_call(T, st, ids[:cut], n_rows, cs, 1, max_points=cut), want)
    assert st.ctx.status() == _lib.STATUS_STORE_OVERFLOW
    with pytest.raises(ValueError, match='one entry per point'):
        boxes_call(T, st, ids[:cut - 1], n_rows, cs, 1, max_points=cut)
    st.check_status()


def test_empty_frames_and_empty_windows(T):
    rows, ids, n_rows = bc.random_scene(n=3000, n_rows=9, seed=6)
    cs = angles(12)
    empty = np.zeros((0, 10))
    frames = [rows[:1200], empty, rows[1200:], empty, empty]
    st = loaded(frames)
    bc.compare(boxes_call(T, st, ids, n_rows, cs, 1), bc.model(ids, rows, *bc.frame(), n_rows, cs, 1, 0.2, want_near=True))
    bc.compare(boxes_call(T, st, ids[1200:], n_rows, cs, 1, first_frame=1),
               bc.model(ids[1200:], rows[1200:], *bc.frame(), n_rows, cs, 1, 0.2, want_near=True))
    # the window of the empty frames alone, and of no frame at all: empty rows, zero stats
    nothing = bc.model(ids[:0], empty, *bc.frame(), n_rows, cs, 1, 0.2, want_near=True)
    assert nothing['stats'].tolist() == [0] * 4 and np.isnan(nothing['fit'][:, :7]).all() and (nothing['fit'][:, 7] == -1).all()
    for f0, f1 in ((3, 5), (2, 2)):
        out = boxes_call(T, st, ids[:0], n_rows, cs, 1, first_frame=f0, last_frame=f1)
        bc.compare(out, nothing)
        assert np.isnan(out['boxes'].cpu().numpy()).all()
    r, _, outs = raw_call(st, ids, n_rows=n_rows, cs=cs, criterion=1, spare=4, slots=(st.head + 2, st.head + 2))
    assert r == 0 and outs[4].tolist() == [0] * 4
    assert np.isnan(outs[0][:n_rows, :7].cpu().numpy()).all() and (outs[0][:n_rows, 7] == -1).all().item() and (outs[0][n_rows:] == 7).all().item()
    assert not outs[1][:n_rows].any().item() and not outs[3][:n_rows].any().item() and (outs[1][n_rows:] == 7).all().item()
    assert bc.same_f64(outs[2][:n_rows].cpu().numpy(), nothing['extents']) and (outs[2][n_rows:] == 7).all().item()
    st.check_status()


# ---------------------------------------------------------------------------------------------- 5: the top level
def test_boxes_of_the_movers_and_the_parked_things_on_a_kitti_drive(T, tmp_path):
    """The drive of test_gpu_voxel_instances.py's last test: after carve_dynamic(mark_dyn=True) the block that left and the
    parked block are one instance each; their boxes equal the model fed with the call's own ids, lie inside the voxel boxes
    and are what host_logic.oriented_boxes makes of the fit."""
    import voxel_carve_common as cc
    from pca_amd import host_logic as hl
    acc, idx = kitti_accumulator(tmp_path, dict(BEV_KITTI, view_size=64, pixel_size=64), n_frames=3), 2
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
    acc.carve_dynamic(idx, part='full', z_range=z_range, nz=nz, origins=sensors, mark_dyn=True)
    rows = np.concatenate(frames)
    cs = hl.fit_angles(90)
    for dyn, who in (('dynamic', 1), ('static', 2)):
        for criterion in ('area', 'edge'):
            out = acc.instance_boxes(idx, part='full', z_range=z_range, nz=nz, dyn=dyn, max_instances=16, criterion=criterion)
            assert sorted(out) == ['box_stats', 'boxes', 'fit', 'fit_n', 'ids', 'inst', 'label_counts', 'stats', 'table', 'top_label']
            ids = out['ids'].cpu().numpy()
            assert np.array_equal(ids >= 0, kind == who) and out['stats'][3].item() == 1
            want = bc.model(ids, rows, origin, R, 0., 0., 16, cs, criterion == 'edge', 0.2)
            bc.compare({k: out[k] for k in ('fit', 'fit_n')} | {'stats': out['box_stats']}, want)
            assert want['stats'].tolist() == [(kind == who).sum(), 0, 1, (kind == who).sum()]
            check_boxes(out, cs)
            # every corner and the height range lie inside the instance's voxel box
            vox = hl.instance_boxes(out['table'].cpu().numpy(), 1, view, px, 0., 1.)[0]
            _, corners = hl.oriented_boxes(want['fit'], cs)
            assert (corners[0, :, 0] >= vox[0] - 1e-9).all() and (corners[0, :, 0] <= vox[1] + 1e-9).all()
            assert (corners[0, :, 1] >= vox[2] - 1e-9).all() and (corners[0, :, 1] <= vox[3] + 1e-9).all()
            assert vox[4] <= want['fit'][0, 4] <= want['fit'][0, 5] <= vox[5]
            assert np.isnan(out['boxes'][1:].cpu().numpy()).all()
    # the dict of an earlier voxel_instances call is taken as it is
    inst = acc.voxel_instances(idx, part='full', z_range=z_range, nz=nz, dyn='static', max_instances=16)
    again = acc.instance_boxes(idx, part='full', criterion='edge', instances=inst)
    assert all(T.equal(again[k], out[k]) for k in ('fit_n', 'box_stats', 'ids')) and again['inst'] is inst['inst']
    assert T.equal(again['fit'].view(T.int64), out['fit'].view(T.int64))
    with pytest.raises(ValueError, match='criterion'):
        acc.instance_boxes(idx, criterion='variance')
    acc.store.check_status()


# ---------------------------------------------------------------------------------------------- 6: the C ABI's checks
def raw_call(st, ids, n_rows=9, cs=None, criterion=0, edge_dist=0.2, prm=None, max_points=20000, outputs=(True, ) * 5, pending=None,
             slots=None, ws_bytes=None, workspace=True, n_angles=None, spare=4, with_ids=True, with_table=True):
    """pca_bev_instance_boxes itself; returns (rc, message, (fit, fit_n, extents, near, stats)).  The outputs hold `spare`
    rows more than n_rows, all filled with 7 (a refused call writes nothing, an accepted one nothing behind its rows)."""
    import torch
    ctx, lib = st.ctx, st.ctx.lib
    cs = angles(12) if cs is None else np.ascontiguousarray(cs, dtype=np.float64)
    A = cs.shape[0]
    rows_cap = min(max(n_rows, 1), 65536) + spare
    fit = torch.full((rows_cap, 8), 7., dtype=torch.float64, device=st.device)
    fit_n = torch.full((rows_cap, 2), 7, dtype=torch.int32, device=st.device)
    ext = torch.full((rows_cap, A, 4), 7., dtype=torch.float64, device=st.device)
    near = torch.full((rows_cap, A), 7, dtype=torch.int32, device=st.device)
    stats = torch.full((4, ), 7, dtype=torch.int64, device=st.device)
    outs = [t.data_ptr() if on else None for t, on in zip((fit, fit_n, ext, near, stats), outputs)]
    need = int(lib.pca_bev_instance_boxes_workspace_bytes(min(max_points, 1 << 20), min(max(n_rows, 1), 65536), A))
    ws = torch.empty(need, dtype=torch.uint8, device=st.device)
    dev_ids = torch.zeros(20000, dtype=torch.int32, device=st.device)
    dev_ids[:len(ids)] = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(st.device)
    store = st.c_store()
    b, e = (st.head, st.head + st.n_frames) if slots is None else slots
    if pending is None:
        pT, pE, nP = None, None, 0
    else:
        Ts, ends, nP = pending
        pT = None if Ts is None else (C.c_double * len(Ts))(*Ts)
        pE = None if ends is None else (C.c_int * len(ends))(*ends)
    prm = prm_of() if prm is None else prm
    r = lib.pca_bev_instance_boxes(ctx.h, C.byref(store), st.frame_off.data_ptr(), b, e, max_points, C.byref(prm),
                                   dev_ids.data_ptr() if with_ids else None, n_rows, cs.ctypes.data if with_table else None,
                                   A if n_angles is None else n_angles, criterion, edge_dist, pT, pE, nP,
                                   ws.data_ptr() if workspace else None, need if ws_bytes is None else ws_bytes, *outs, ctx.stream())
    torch.cuda.synchronize()
    return r, lib.pca_last_error(ctx.h).decode(), (fit, fit_n, ext, near, stats)


def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    rows, ids, n_rows = bc.random_scene(n=3000, n_rows=9, seed=6)
    st = loaded(cut_frames(rows, 1000, 2000))
    ctx = st.ctx
    cs = angles(12)
    want = bc.model(ids, rows, *bc.frame(), n_rows, cs, 0, 0.2, want_near=True)
    names = ('fit', 'fit_n', 'extents', 'near', 'stats')

    def written(name, t):
        """The output holds the model's result, and what lies behind its rows is untouched."""
        if name == 'stats':
            return t.tolist() == want['stats'].tolist()
        got = t[:n_rows].cpu().numpy()
        if name in ('fit', 'extents'):
            return bc.same_f64(got, want[name]) and (t[n_rows:] == 7).all().item()
        w = want[name].copy()
        return np.array_equal(got.view(np.uint32).astype(np.int64), w) and (t[n_rows:] == 7).all().item()
    r, _, outs = raw_call(st, ids)                                # the call as such is fine
    assert r == 0 and all(written(n, t) for n, t in zip(names, outs))
    for k in range(5):                                            # any output alone (fit_n alone: near_t was not needed)
        r, _, outs = raw_call(st, ids, outputs=tuple(j == k for j in range(5)))
        assert r == 0 and all((t == 7).all().item() for j, t in enumerate(outs) if j != k), names[k]
        if names[k] == 'fit_n':
            assert np.array_equal(outs[1][:n_rows, 0].cpu().numpy(), want['fit_n'][:, 0]) and not outs[1][:n_rows, 1].any().item()
        else:
            assert written(names[k], outs[k]), names[k]
    ctx.profile(1)
    bad_R = np.array([[1., 0., 0.], [0., np.cos(0.1), -np.sin(0.1)], [0., np.sin(0.1), np.cos(0.1)]])
    eye = [float(v) for v in np.eye(4).reshape(-1)]
    nan, inf = float('nan'), float('inf')
    h = st.head
    what = 'bev instance boxes: '
    origin, R, dx, dy = bc.frame()

    def bad_table(i, v):
        t = cs.copy()
        t.reshape(-1)[i] = v
        return t
    cases = [(dict(prm=params(origin, bad_R, dx, dy, VIEW, PX)), 'R must be a rotation about the z axis'),
             (dict(outputs=(False, ) * 5), 'bad arguments'),
             (dict(with_ids=False), 'bad arguments'),
             (dict(with_table=False), 'bad arguments'),
             (dict(workspace=False), 'bad arguments'),
             (dict(ws_bytes=1024), 'workspace too small'),
             (dict(max_points=1 << 31), 'max_points must be below 2\\^31'),
             (dict(slots=(h + 2, h + 1)), 'need slot_begin <= slot_end'),
             (dict(pending=(eye * 5, [h + 1] * 5, 5)), 'bad chain of owed transforms'),
             (dict(pending=(eye, [h + 4], 1)), 'a pending slot end lies beyond the window'),
             (dict(pending=(eye * 2, [h + 2, h + 1], 2)), 'pending slot ends must ascend')]
    cases += [(dict(n_angles=v), r'n_angles must be in 1\.\.256') for v in (0, -1, 257)]
    cases += [(dict(n_rows=v), r'n_rows must be in 1\.\.65536') for v in (0, -1, 65537)]
    cases += [(dict(criterion=v), 'criterion must be 0 or 1') for v in (2, -1)]
    cases += [(dict(edge_dist=v), 'edge_dist must be finite and >= 0') for v in (-0.5, nan, inf)]
    cases += [(dict(cs=bad_table(i, v)), 'every entry of cos_sin must be finite') for i, v in ((0, nan), (7, inf), (23, -inf))]
    for bad, msg in cases:
        r, err, outs = raw_call(st, ids, **bad)
        assert r == -1 and re.match(what + msg, err), (err, msg)
        assert all((t == 7).all().item() for t in outs), msg
    with pytest.raises(RuntimeError, match=r'bev instance boxes: n_rows must be in 1\.\.65536'):
        boxes_call(T, st, ids, 65537, cs, 0)
    with pytest.raises(RuntimeError, match=r'bev instance boxes: n_angles must be in 1\.\.256'):
        boxes_call(T, st, ids, n_rows, angles(257), 0)
    with pytest.raises(ValueError, match='criterion'):
        st.bev_instance_boxes(prm_of(), T.zeros(3000, dtype=T.int32).cuda(), n_rows, cs, criterion='variance')
    with pytest.raises(ValueError, match='int32'):
        st.bev_instance_boxes(prm_of(), T.zeros(3000, dtype=T.int64).cuda(), n_rows, cs)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert all(prof[k][1] == 0 for k in KERNELS)
    # the limits themselves are legal: one row, edge_dist 0, px plays no part
    r, _, outs = raw_call(st, ids, n_rows=1, criterion=1, edge_dist=0., prm=params(origin, R, dx, dy, VIEW, 4096))
    one = bc.model(ids, rows, *bc.frame(), 1, cs, 1, 0., want_near=True)
    assert r == 0 and bc.same_f64(outs[0][:1].cpu().numpy(), one['fit']) and outs[4].tolist() == one['stats'].tolist()
    assert (outs[0][1:] == 7).all().item() and outs[1][0].tolist() == one['fit_n'][0].tolist()
    st.check_status()
