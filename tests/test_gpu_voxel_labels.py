"""GPU: the BEV window voxelised into semantic occupancy labels (pca_bev_voxel_labels, DeviceStore.bev_voxel_labels,
SemBEVGenerator.voxel_labels_device, SemanticPointCloudAccumulator.voxel_labels) against the numpy model of
tests/voxel_labels_common.py (pinned by tests/test_voxel_labels_model.py).  Every comparison is exact."""
import ctypes as C
import re

import numpy as np
import pytest

import test_voxel_labels_model as hand
import voxel_labels_common as vc
from test_gpu_kernels import SEM_IDXS, T, dev_store  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, frames_of, kitti_accumulator, loaded, params

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1, 1), (8, 5, 19), (20, 5, 19), (20, 32, 32), (64, 32, 32), (64, 7, 20)]
ORIGIN, VIEW = (0.3, -0.2, 0.125), 40.


def table_for(n_labels):
    """The 19 classes of random_rows onto labels that reach n_labels - 1; with one label, class 0 alone takes part."""
    t = np.full(256, 255, dtype=np.uint8)
    if n_labels == 1:
        t[0] = 0
    elif n_labels == 19:
        t[:19] = np.arange(19)
    else:
        t[:19] = n_labels - 1 - np.arange(19)
    return t


# ---------------------------------------------------------------------------------------------- 1: the model, small shapes
@pytest.mark.parametrize('px,nz,n_labels', SHAPES)
def test_lattice_heights_on_bin_edges(T, px, nz, n_labels):
    """z_lo = -1, z_step = 1 / 8 and heights on a 1 / 1024 lattice: every 128th height sits exactly on a bin edge.  A rotated
    view with a shift; a single partial tile, partial tiles at the right and bottom edges, nz that is no multiple of the
    slab, the largest counter block."""
    frames = frames_of(1)
    rows = np.concatenate(frames)
    R, dx, dy, table = vc.rotation(0.4), 0.5, -0.25, table_for(n_labels)
    st = loaded(frames)
    for include_dyn in (False, True):
        out = st.bev_voxel_labels(params(ORIGIN, R, dx, dy, VIEW, px, None), -1., 0.125, nz, table, n_labels, include_dyn=include_dyn)
        want = vc.model(rows, ORIGIN, R, dx, dy, VIEW, px, None, -1., 0.125, nz, table, n_labels, include_dyn)
        vc.compare(out, want)
        assert want['counts'].sum() > (0 if n_labels == 1 else 300)
    on_edge = ((rows[:, 2] - ORIGIN[2]) * 8 % 1 == 0) & (want['voxel'] >= 0)
    assert nz < 32 or on_edge.sum() > 20
    st.check_status()


@pytest.mark.parametrize('px,nz,n_labels', SHAPES)
def test_inexact_quotients_match_the_f64_division(T, px, nz, n_labels):
    """z_lo = -2, z_step = 0.2, plus rows at z_lo + k z_step (k = 0 .. nz) and their two f64 neighbours: the quotient is
    inexact and within an ulp or two of an integer -- the bin has to be the one numpy's division gives, bit for bit."""
    rng = np.random.default_rng(100 + px + nz)
    frames = [f.copy() for f in frames_of(2)]
    frames[2] = np.concatenate([frames[2], vc.edge_rows(rng, 4, 15., ORIGIN[2], -2.0, 0.2, nz, [0] if n_labels == 1 else range(19))])
    rows = np.concatenate(frames)
    R, dx, dy, table = vc.rotation(-1.1), -0.75, 0.3, table_for(n_labels)
    st = loaded(frames)
    out = st.bev_voxel_labels(params(ORIGIN, R, dx, dy, VIEW, px, None), -2.0, 0.2, nz, table, n_labels)
    want = vc.model(rows, ORIGIN, R, dx, dy, VIEW, px, None, -2.0, 0.2, nz, table, n_labels, False)
    vc.compare(out, want)
    t = (((rows[:, 2] - ORIGIN[2]) + 0.0) - -2.0) / 0.2
    near = (np.abs(t - np.rint(t)) < 1e-9) & (want['voxel'] >= 0)
    assert near.sum() > 3 * nz
    st.check_status()


def test_height_filter_inside_the_z_range(T):
    frames = frames_of(1)
    rows = np.concatenate(frames)
    R, px, nz, n_labels, hf = vc.rotation(2.0), 20, 32, 19, 1.5
    table = table_for(n_labels)
    st = loaded(frames)
    out = st.bev_voxel_labels(params(ORIGIN, R, 1.5, -2.5, VIEW, px, hf), -1., 0.125, nz, table, n_labels)
    want = vc.model(rows, ORIGIN, R, 1.5, -2.5, VIEW, px, hf, -1., 0.125, nz, table, n_labels, False)
    vc.compare(out, want)
    assert want['counts'][:20].sum() > 1000 and not want['counts'][20:].any()    # (-1 + 20 / 8 = 1.5: the filter's height)
    free = st.bev_voxel_labels(params(ORIGIN, R, 1.5, -2.5, VIEW, px, None), -1., 0.125, nz, table, n_labels)
    assert free['counts'][20:].sum().item() > 1000
    st.check_status()


def test_largest_grid_uses_every_key_bit(T):
    """1024^2: 16 384 tiles, whose 14 bits sit above the record's 16 in level 1's key; level 1's histogram is 64 KiB of LDS."""
    frames = frames_of(2)
    rows = np.concatenate(frames)
    R, px, nz, n_labels = vc.rotation(0.9), 1024, 2, 32
    table = table_for(n_labels)
    st = loaded(frames)
    out = st.bev_voxel_labels(params(ORIGIN, R, -0.5, 0.75, VIEW, px, None), -1.5, 2.5, nz, table, n_labels)
    want = vc.model(rows, ORIGIN, R, -0.5, 0.75, VIEW, px, None, -1.5, 2.5, nz, table, n_labels, False)
    vc.compare(out, want)
    seen = np.flatnonzero(want['counts'].sum(axis=0).reshape(-1))
    assert want['counts'].sum() > 4000 and seen.min() < 8 * px and seen.max() > (px - 8) * px
    st.check_status()


# ---------------------------------------------------------------------------------------------- 2: ties, wide counters
def test_ties_go_to_the_smallest_label_and_counters_are_32_bits_wide(T):
    view, px = 8., 4
    at, other = (1., 1.), (-1., 1.)                               # cells (row 1, column 2) and (row 1, column 1)
    rows = np.concatenate([vc.pile(at, 0.1, 3, 7), vc.pile(at, 0.2, 1, 7), vc.pile(at, 0.3, 5, 6),
                           vc.pile(other, 1.5, 4, 70000), vc.pile(other, 1.25, 2, 66000), vc.pile(other, 1.75, 7, 5000)])
    rows = rows[np.random.default_rng(3).permutation(rows.shape[0])]
    frames = [rows[:50000], rows[50000:]]
    st = loaded(frames, capacity=1 << 18)
    table = vc.identity_table(8)
    out = st.bev_voxel_labels(params((0., 0., 0.), np.eye(3), 0., 0., view, px, None), 0., 1., 2, table, 8)
    # (wrapping 16-bit counters would make label 7 the winner of the second voxel, saturating ones label 2)
    hand.expect(vc.model(rows, (0., 0., 0.), np.eye(3), 0., 0., view, px, None, 0., 1., 2, table, 8, False), 2,
                {(0, 1, 2): (1, 20, 7), (1, 1, 1): (4, 141000, 70000)})
    got = {k: v.cpu().numpy() for k, v in out.items()}
    hand.expect({'labels': got['labels'], 'counts': got['counts'].view(np.uint32), 'top': got['top'].view(np.uint32)}, 2,
                {(0, 1, 2): (1, 20, 7), (1, 1, 1): (4, 141000, 70000)})
    st.check_status()


def test_heavy_window_beyond_the_register_path(T, monkeypatch):
    """390 000 points at 256^2 under PCA_BEV_VOXEL_G=4: four level-1 workgroups whose chunks (97 500 points) go past the
    register path.  One cell holds 70 000 points, its tile 40 000 more."""
    monkeypatch.setenv('PCA_BEV_VOXEL_G', '4')
    rng = np.random.default_rng(19)
    view, px, hf, dx, dy, nz, n_labels = 100., 256, 3.0, 0.7, -1.3, 32, 19
    frames = vc.heavy_window(rng, view, px, dx, dy)
    rows = np.concatenate(frames)
    assert rows.shape[0] == 390000
    origin, table = (0., 0., 0.25), table_for(n_labels)
    st = loaded(frames, capacity=1 << 19, max_frames=64)
    out = st.bev_voxel_labels(params(origin, np.eye(3), dx, dy, view, px, hf), -2.0, 0.2, nz, table, n_labels)
    want = vc.model(rows, origin, np.eye(3), dx, dy, view, px, hf, -2.0, 0.2, nz, table, n_labels, False)
    vc.compare(out, want)
    assert want['counts'].sum(axis=0).max() > 40000 and want['top'].max() > 100
    st.check_status()


# ---------------------------------------------------------------------------------------------- 3: label table and flags
def test_label_table_dyn_non_finite_and_out_of_range_heights(T):
    view, px = hand.VIEW, hand.PX
    prm = params(hand.ORIGIN, hand.R, 0., 0., view, px, None)

    def device(rows, z_lo, z_step, nz, label_of=None, n_labels=8, include_dyn=False):
        label_of = vc.identity_table(n_labels) if label_of is None else label_of
        rows = np.array(rows)
        st = loaded([rows[:2], rows[2:]], capacity=1024)
        out = st.bev_voxel_labels(prm, z_lo, z_step, nz, label_of, n_labels, include_dyn=include_dyn)
        vc.compare(out, hand.run(rows, z_lo, z_step, nz, label_of, n_labels, include_dyn))
        st.check_status()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        return {'labels': got['labels'], 'counts': got['counts'].view(np.uint32), 'top': got['top'].view(np.uint32)}
    row = hand.row
    # classes mapped to 255 are ignored, two classes share a label
    table, n_labels = vc.table_of([[4, 9], [2]])
    rows = [row(1., 1., 0.1, 4), row(1., 1., 0.1, 9), row(1., 1., 0.1, 2), row(1., 1., 0.1, 0), row(1., 1., 0.1, 200),
            row(-1., -1., 0.1, 7)]
    hand.expect(device(rows, 0., 1., 1, table, n_labels), 1, {(0, 1, 2): (0, 3, 2)})
    # dyn == 1 is dropped, and kept with include_dyn
    rows = [row(1., 1., 0.1, 1, dyn=1.), row(1., 1., 0.1, 1, dyn=1.), row(1., 1., 0.1, 2), row(1., 1., 0.1, 3, dyn=2.)]
    hand.expect(device(rows, 0., 1., 1), 1, {(0, 1, 2): (2, 2, 1)})
    hand.expect(device(rows, 0., 1., 1, include_dyn=True), 1, {(0, 1, 2): (1, 4, 2)})
    # NaN / +-inf z is dropped; -0.0 lands in bin 0; a hair below z_lo is out
    rows = [row(1., 1., -0.0, 1), row(1., 1., -1e-300, 2), row(1., 1., np.nan, 3), row(1., 1., np.inf, 3),
            row(1., 1., -np.inf, 3), row(1., 1., 1.75, 4), row(1., 1., 1.5, 5)]
    hand.expect(device(rows, 0., 1., 2), 2, {(0, 1, 2): (1, 1, 1), (1, 1, 2): (4, 2, 1)})
    # below z_lo and at or above the top: dropped, not clamped
    rows = [row(1., 1., -1.0, 2), row(1., 1., -0.5, 2), row(1., 1., -0.5000001, 3), row(-3.5, -3.5, 0.999, 1),
            row(-3.5, -3.5, 1.0, 1), row(-3.5, -3.5, -1.0000001, 1), row(3.9, 3.9, 0.25, 0), row(3.9, 3.9, 1e300, 0),
            row(3.9, 3.9, -1e300, 0)]
    hand.expect(device(rows, -1., 0.5, 4), 4,
                {(0, 1, 2): (2, 2, 1), (1, 1, 2): (2, 1, 1), (3, 3, 0): (1, 1, 1), (2, 0, 3): (0, 1, 1)})


# ---------------------------------------------------------------------------------------------- 4: owed chain
@pytest.mark.parametrize('k', [1, 2, 3, 4])
def test_owed_chain_is_applied_to_what_is_read_and_stays_owed(T, k):
    from test_gpu_kernels import _tilting_transform
    rng = np.random.default_rng(60 + k)
    frames = [vc.random_rows(rng, 5000, 40.) for _ in range(3)]
    origin, view, px, hf, nz, n_labels = (0.3, -0.2, 0.1), 80., 64, 2.5, 32, 19
    lazy, twin = loaded(frames), loaded(frames)
    lazy.CHAIN_K = twin.CHAIN_K = 4
    for step in range(k):
        Tm = _tilting_transform(step)                            # changes z: the bin and the filter see the transformed z
        lazy.retransform(Tm, defer=True)
        twin.retransform(Tm, defer=True)
    eager = twin.rows()                                          # K2 writes the transforms into the twin's store
    assert not twin._pending
    n_rows = eager.shape[0]
    before = [t[:n_rows].clone() for t in lazy._arrays()]
    pending = [(np.array(Tm).copy(), e) for Tm, e in lazy._pending]
    R, table = vc.rotation(0.4), table_for(n_labels)
    prm = params(origin, R, 0.5, -0.25, view, px, hf)
    got = lazy.bev_voxel_labels(prm, -2.0, 0.2, nz, table, n_labels)
    want = vc.model(eager, origin, R, 0.5, -0.25, view, px, hf, -2.0, 0.2, nz, table, n_labels, False)
    vc.compare(got, want)
    vc.compare(twin.bev_voxel_labels(prm, -2.0, 0.2, nz, table, n_labels), want)
    assert want['counts'].sum() > 3000
    assert len(lazy._pending) == k                               # still owed, and the same list
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(pending, lazy._pending))
    assert all(T.equal(a, b[:n_rows]) for a, b in zip(before, lazy._arrays()))       # no store column was written
    assert not T.equal(lazy.z[:n_rows], twin.z[:n_rows])
    lazy.check_status()
    twin.check_status()


# ---------------------------------------------------------------------------------------------- 5: empty and cut windows
def test_empty_windows_and_the_cut_window(T):
    from pca_amd import _lib
    frames = frames_of(1)[:2]
    rows = np.concatenate(frames)
    R, px, nz, n_labels = vc.rotation(0.3), 20, 5, 19
    table = table_for(n_labels)
    prm = params(ORIGIN, R, 0., 0., VIEW, px, None)
    st = loaded(frames)
    far = np.concatenate(frames)
    far[:, 0] += 1000.
    # no frame at all in the range, a store that holds nothing, a window whose points are all out of view
    for store, args in ((st, dict(first_frame=1, last_frame=1)), (dev_store(capacity=1024, max_frames=4), {}),
                        (loaded([far]), {})):
        out = {k: v.cpu().numpy() for k, v in store.bev_voxel_labels(prm, -1., 0.5, nz, table, n_labels, **args).items()}
        assert out['labels'].shape == out['counts'].shape == out['top'].shape == (nz, px, px)
        assert (out['labels'] == 255).all() and not out['counts'].any() and not out['top'].any()
        store.check_status()
    # a window above max_points is cut there and says so
    cut = 2700
    out = st.bev_voxel_labels(prm, -1., 0.5, nz, table, n_labels, max_points=cut)
    vc.compare(out, vc.model(rows[:cut], ORIGIN, R, 0., 0., VIEW, px, None, -1., 0.5, nz, table, n_labels, False))
    assert st.ctx.status() == _lib.STATUS_STORE_OVERFLOW         # (read and cleared here)
    whole = st.bev_voxel_labels(prm, -1., 0.5, nz, table, n_labels)
    assert whole['counts'].sum().item() > out['counts'].sum().item() > 500
    st.check_status()


# ---------------------------------------------------------------------------------------------- 6: an existing device path
def test_one_bin_over_everything_equals_the_class_planes_counts(T):
    frames = frames_of(2)
    R, px, hf = vc.rotation(0.7), 64, 2.5
    prm = params(ORIGIN, R, 0.4, -0.6, VIEW, px, hf)
    groups = [[0, 1], [2], [5, 6, 7], [18]]                       # disjoint
    table, n_labels = vc.table_of(groups)
    st = loaded(frames)
    out = st.bev_voxel_labels(prm, -1000., 2000., 1, table, n_labels)
    _, _, cnt = st.bev_class_planes(2, prm, groups, want_counts=True)
    full = cnt[2].cpu().numpy().view(np.uint32).astype(np.int64)  # [groups + all static points, px, px] of the set 'full'
    per_label = full[:len(groups)]
    counts, top, labels = (out[k][0].cpu().numpy() for k in ('counts', 'top', 'labels'))
    assert np.array_equal(counts.view(np.uint32), per_label.sum(axis=0)) and per_label.sum() > 1000
    assert (per_label.sum(axis=0) <= full[len(groups)]).all()
    assert np.array_equal(top.view(np.uint32), per_label.max(axis=0))
    assert np.array_equal(labels, np.where(per_label.sum(axis=0) > 0, per_label.argmax(axis=0), 255))
    # every class its own label, none left out: the all-static slot itself
    out = st.bev_voxel_labels(prm, -1000., 2000., 1, vc.identity_table(19), 19)
    assert np.array_equal(out['counts'][0].cpu().numpy().view(np.uint32), full[len(groups)])
    st.check_status()


# ---------------------------------------------------------------------------------------------- 7: the C ABI's checks
def raw_call(st, prm, max_points, z_lo=-1., z_step=0.5, nz=4, table=None, n_labels=19, outputs=True, ws_bytes=None):
    """pca_bev_voxel_labels itself; returns (rc, message, outputs)."""
    import torch
    ctx, lib = st.ctx, st.ctx.lib
    px = min(max(int(prm.px), 1), 1024)
    need = int(lib.pca_bev_voxel_workspace_bytes(max_points, px))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=st.device)
    shape = (32, min(px, 64), min(px, 64))                       # (a refused call writes nothing: the size does not matter)
    labels = torch.full(shape, 77, dtype=torch.uint8, device=st.device)
    counts = torch.full(shape, -7, dtype=torch.int32, device=st.device)
    top = torch.full(shape, -7, dtype=torch.int32, device=st.device)
    table = table_for(19) if table is None else table
    store = st.c_store()
    rc = lib.pca_bev_voxel_labels(ctx.h, C.byref(store), st.frame_off.data_ptr(), st.head, st.head + st.n_frames, max_points,
                                  C.byref(prm), z_lo, z_step, nz, None if table is False else table.ctypes.data, n_labels, 0,
                                  None, None, 0, ws.data_ptr(), need if ws_bytes is None else ws_bytes,
                                  labels.data_ptr() if outputs else None, counts.data_ptr() if outputs else None,
                                  top.data_ptr() if outputs else None, ctx.stream())
    return rc, lib.pca_last_error(ctx.h).decode(), (labels, counts, top)


def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    frames = frames_of(1)[:1]
    R, px = vc.rotation(0.3), 32
    st = loaded(frames)
    prm = params(ORIGIN, R, 0., 0., VIEW, px, None)
    ctx = st.ctx
    rc, _, (labels, counts, top) = raw_call(st, prm, 8000)       # the call as such is fine
    assert rc == 0 and (labels[:4] != 77).all().item() and (counts[:4] >= 0).all().item() and (labels[4:] == 77).all().item()
    ctx.profile(1)
    bad_R = np.array([[1., 0., 0.], [0., np.cos(0.1), -np.sin(0.1)], [0., np.sin(0.1), np.cos(0.1)]])
    too_big = table_for(19).copy()
    too_big[3] = 19
    nan, inf = float('nan'), float('inf')
    cases = [(dict(prm=params(ORIGIN, R, 0., 0., VIEW, 1025, None)), r'bev voxel labels: px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, R, 0., 0., VIEW, 0, None)), r'bev voxel labels: px must be in 1\.\.1024'),
             (dict(prm=params(ORIGIN, bad_R, 0., 0., VIEW, px, None)), 'bev voxel labels: R must be a rotation about the z axis'),
             (dict(outputs=False), 'bev voxel labels: bad arguments'),
             (dict(table=False), 'bev voxel labels: bad arguments'),
             (dict(ws_bytes=1024), 'bev voxel labels: workspace too small'),
             (dict(table=too_big), r'bev voxel labels: label_of\[3\] must be below n_labels, or 255')]
    cases += [(dict(nz=v), r'bev voxel labels: nz must be in 1\.\.32') for v in (0, -1, 33)]
    cases += [(dict(n_labels=v), r'bev voxel labels: n_labels must be in 1\.\.32') for v in (0, 33)]
    cases += [(dict(z_lo=v), 'bev voxel labels: z_lo must be finite') for v in (nan, inf, -inf)]
    cases += [(dict(z_step=v), 'bev voxel labels: z_step must be finite and > 0') for v in (0., -0.5, nan, inf)]
    for bad, msg in cases:
        args = dict(prm=prm, max_points=8000)
        args.update(bad)
        rc, err, (labels, counts, top) = raw_call(st, **args)
        assert rc == -1 and re.match(msg, err), (err, msg)
        assert (labels == 77).all().item() and (counts == -7).all().item() and (top == -7).all().item()
    with pytest.raises(RuntimeError, match=r'bev voxel labels: nz must be in 1\.\.32'):
        st.bev_voxel_labels(prm, -1., 0.5, 33, table_for(19), 19)
    with pytest.raises(RuntimeError, match='z_step must be finite and > 0'):
        st.bev_voxel_labels(prm, -1., 0., 4, table_for(19), 19)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['bev_voxel_bin'][1] == 0 and prof['bev_voxel_cells'][1] == 0
    st.check_status()


# ---------------------------------------------------------------------------------------------- 8: the drop-ins
def same_bev(a, b):
    assert set(a.keys()) == set(b.keys())
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), key
        elif isinstance(x, (list, tuple)):
            assert len(x) == len(y) and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x, y)), key
        else:
            assert x is None and y is None, key


def check_dropin(T, acc, idx):
    """acc.voxel_labels of all three parts against the model on the host rows of acc.sem_pcs in the sample's frame; the
    host-rows form of voxel_labels_device against the window form; generate_bev before and after."""
    from pca_amd import host_logic as hl
    gen = acc.sem_bev_generator
    def sample():
        return {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in acc.generate_bev(idx, 1, gen_future=True)[0].items()}
    before = sample()
    z_range, nz, classes = (-2.0, 4.4), 32, [[0, 1, 2], [13, 14, 15, 17], [5], [8, 9]]
    got = {part: acc.voxel_labels(idx, part=part, z_range=z_range, nz=nz, classes=classes) for part in ('present', 'future', 'full')}
    default = acc.voxel_labels(idx)
    after = sample()
    same_bev(before, after)
    frames = acc.sem_pcs
    poses = np.array(acc.poses)
    origin = poses[idx]
    R = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:idx] - origin))
    view, px, hf = 1. * gen.view_size, gen.pixel_size, gen.height_filter
    table, n_labels = vc.table_of(classes)
    z_step = (z_range[1] - z_range[0]) / nz
    for part, rows in (('present', frames[:idx]), ('future', frames[idx:]), ('full', frames)):
        rows = np.concatenate(rows)
        want = vc.model(rows, origin, R, 0., 0., view, px, hf, z_range[0], z_step, nz, table, n_labels, False)
        vc.compare(got[part], want)
        assert want['counts'].sum() > 200, part
        # host rows in BEV-frame metres through the generator equal the window form
        rel = rows.copy()
        rel[:, 0:3] -= origin
        host = gen.voxel_labels_device(rel, R, 0., 0., view, z_range, nz, classes=classes)
        assert all(T.equal(host[k], got[part][k]) for k in ('labels', 'counts', 'top')), part
    rows = np.concatenate(frames)
    vc.compare(default, vc.model(rows, origin, R, 0., 0., view, px, hf, -2.0, (4.4 - -2.0) / 32, 32, vc.identity_table(32), 32, False))
    with pytest.raises(ValueError):
        acc.voxel_labels(idx, part='past')
    with pytest.raises(ValueError):
        acc.voxel_labels(idx, classes=[[1, 2], [2]])             # a class named in two lists
    acc.store.check_status()


def test_kitti_dropin(T, tmp_path):
    check_dropin(T, kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14), 9)


def test_nuscenes_dropin(T, tmp_path, monkeypatch):
    """A scene of fake_nuscenes.synth_tables' records (lidar points and ego poses) through the NuScenes oracle accumulator."""
    from PIL import Image

    import fake_nuscenes as fk
    import sem_pc_accum
    from nuscenes_oracle_sem_pc_accum import NuScenesOracleSemanticPointCloudAccumulator
    from test_gpu_dropin import BEV_NUSC, NUSC_FILTERS, FakeSemSeg
    monkeypatch.setattr(sem_pc_accum, 'SemSegONNX', lambda path: FakeSemSeg())
    F, n, ncam, H, W = 8, 2500, 2, 90, 160
    t = fk.synth_tables(seed=11, n_records=F, n_pts=n)
    rng = np.random.default_rng(12)
    pils = [Image.fromarray(im) for im in rng.integers(0, 256, (ncam, H, W, 3), dtype=np.uint8)]
    acc = NuScenesOracleSemanticPointCloudAccumulator('fake.onnx', NUSC_FILTERS, SEM_IDXS, False, dict(BEV_NUSC), 'boston',
                                                      False, None)
    for k in range(F):
        Tk = np.eye(4)
        Tk[:3, :3] = fk.FakeQuaternion(t['ego_q'][k]).rotation_matrix
        Tk[:3, 3] = t['ego_t'][k]
        pts = t['points'][k].astype(np.float64)
        pc = np.stack([pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3], rng.uniform(1.01, W - 1.01, n), rng.uniform(1.01, H - 1.01, n),
                       rng.integers(-1, 3, n).astype(float)], 1)
        obs = dict(images=pils, pc=pc, pc_cam_idx=rng.integers(-1, ncam, n), ego_at_lidar_ts=Tk, ego_global_x=Tk[0, 3],
                   ego_global_y=Tk[1, 3], inst_tokens=['parked', 'moving'], inst_cls=[0, 0],
                   inst_center=[t['ego_t'][0] + [6., 3., 0.5], t['ego_t'][0] + [2. + 0.5 * k, -4., 0.5]])
        assert acc.integrate([obs]) is None
    check_dropin(T, acc, 5)
