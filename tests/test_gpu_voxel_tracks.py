"""GPU: the instances of one sample matched to those of the sample before it (pca_voxel_instance_match,
DeviceStore.voxel_instance_match, SemBEVGenerator.voxel_instance_match_device, SemanticPointCloudAccumulator.track_instances /
store_frame) against the brute-force numpy model of tests/voxel_tracks_common.py (pinned by tests/test_voxel_tracks_model.py).
Every comparison is exact; `pairs` is compared after sorting, its order being the one thing the contract leaves open.

Shapes (px, nz): (8, 1) a single line; (33, 7) odd sizes that leave partial waves; (72, 5) wider than one wave per line;
(136, 32) the full height.  Each scene runs by default and with PCA_VOXEL_MATCH_G=1, one workgroup round all its loops."""
import re

import numpy as np
import pytest

import voxel_tracks_common as vt
from test_gpu_kernels import KITTI_FILTERS, SEM_IDXS, T, dev_store  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, kitti_accumulator, kitti_tree

pytestmark = pytest.mark.gpu

# letter -> (name, dtype, shape of the buffer for (n_prev, n_cur, cells shape, n_ids, cap))
OUTPUTS = {'c': ('cur_track', 'int32'), 'm': ('match', 'int32'), 'i': ('cur_info', 'uint32'), 'p': ('prev_info', 'uint32'),
           'v': ('track_vol', 'int32'), 't': ('track_ids', 'int32'), 'k': ('pairs', 'uint32'), 's': ('stats', 'int64')}
ALL = 'cmipvtks'
FILL = 7


def set_g(monkeypatch, g, fold=None):
    monkeypatch.delenv('PCA_VOXEL_MATCH_G', raising=False) if g is None else monkeypatch.setenv('PCA_VOXEL_MATCH_G', g)
    monkeypatch.delenv('PCA_VOXEL_MATCH_FOLD', raising=False) if fold is None else monkeypatch.setenv('PCA_VOXEL_MATCH_FOLD', fold)


def raw(T, prev, n_prev, cur, n_cur, M, min_overlap=1, min_iou=0.0, cap_pairs=None, prev_track=None, t0=0, ids=None, outputs=ALL,
        counter=None, sync=True, **bad):
    """pca_voxel_instance_match itself.  outputs: the letters of OUTPUTS that are wanted; every output buffer starts out filled with
    bytes of 7, so does the workspace.  bad: px, nz, rows_prev, rows_cur (for n_prev, n_cur), ws_bytes replaced; null_counter.  counter: a cuda int32 [1] to
    chain calls (else a fresh one holding t0).  Returns (rc, message, {name: array or tensor}, outputs, counter tensor)."""
    from pca_amd import _lib
    ctx = _lib.Context.get()
    nz, px, _ = cur.shape
    if cap_pairs is None:
        cap_pairs = 16
        while cap_pairs < 4 * max(n_prev, n_cur):
            cap_pairs *= 2
    dev = lambda a: None if a is None else (a if isinstance(a, T.Tensor) else T.from_numpy(np.array(a)).cuda())      # noqa: E731
    d_prev, d_cur, d_track, d_ids = dev(prev), dev(cur), dev(prev_track), dev(ids)
    M = np.ascontiguousarray(M, dtype=np.float64).reshape(12)
    need = int(ctx.lib.pca_voxel_instance_match_workspace_bytes(n_prev, n_cur, cap_pairs))
    ws = T.full((max(need, 256), ), FILL, dtype=T.uint8, device='cuda')
    if counter is None:
        counter = T.full((1, ), t0, dtype=T.int32, device='cuda')
    n_ids = 0 if ids is None else int(d_ids.numel())
    rp, rc = min(max(n_prev, 1), 65536), min(max(n_cur, 1), 65536)
    shapes = {'c': (rc, ), 'm': (rc, ), 'i': (rc, 4), 'p': (rp, 4), 'v': tuple(cur.shape), 't': (max(n_ids, 1), ),
              'k': (cap_pairs if need > 0 else 16, 3), 's': (10, )}
    outs = {}
    for c, (name, dt) in OUTPUTS.items():
        words = int(np.prod(shapes[c])) * np.dtype(dt).itemsize
        outs[name] = T.full((words, ), FILL, dtype=T.uint8, device='cuda')
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    r = ctx.lib.pca_voxel_instance_match(
        ctx.h, bad.get('px', px), bad.get('nz', nz), d_prev.data_ptr(), bad.get('rows_prev', n_prev), d_cur.data_ptr(),
        bad.get('rows_cur', n_cur), M.ctypes.data, int(min_overlap), float(min_iou), int(cap_pairs), ptr(d_track),
        None if bad.get('null_counter') else counter.data_ptr(), ptr(d_ids), n_ids, ws.data_ptr(), bad.get('ws_bytes', need),
        *(outs[OUTPUTS[c][0]].data_ptr() if c in outputs else None for c in ALL), ctx.stream())
    if not sync:
        return r, None, outs, outputs, counter
    T.cuda.synchronize()
    host = {OUTPUTS[c][0]: outs[OUTPUTS[c][0]].cpu().numpy().view(OUTPUTS[c][1]).reshape(shapes[c]) for c in ALL}
    if ids is None:
        host['track_ids'] = host['track_ids'][:0]
    return r, ctx.lib.pca_last_error(ctx.h).decode(), host, outputs, counter


FILLED = {dt: np.frombuffer(bytes([FILL]) * 8, dtype=dt)[0] for dt in ('int32', 'uint32', 'int64')}


def same(got, want, full_table=False):
    """Every output that was asked for equals the model's; the others still hold their 7s; the counter has moved on."""
    r, err, outs, outputs, counter = got
    assert r == 0, err
    for c, (name, dt) in OUTPUTS.items():
        a = outs[name]
        if c not in outputs:
            assert (a == FILLED[dt]).all(), name
            continue
        if full_table:                                       # only these are defined once an increment was dropped
            if c == 's':
                assert a[4] > 0 and a[[0, 1, 8, 9]].tolist() == want['stats'][[0, 1, 8, 9]].tolist()
            elif c == 'i':
                assert np.array_equal(a[:, :2], want[name][:, :2])
            elif c == 'p':
                assert np.array_equal(a[:, 0], want[name][:, 0])
            continue
        b = want[name]
        if c == 'k':
            assert a.shape[0] >= b.shape[0]
            a = vt.sorted_pairs(a)
            b = vt.sorted_pairs(b)
        assert a.dtype == b.dtype == np.dtype(dt), name
        assert a.shape == b.shape and np.array_equal(a, b), (name, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape),
                                                              np.argwhere(a != b)[:4].tolist() if a.shape == b.shape else None)
    if not full_table:
        assert int(counter.item()) == int(want['counter'])


# ---------------------------------------------------------------------------------------------- 1: the scenes
@pytest.mark.parametrize('px,nz', vt.SHAPES)
def test_random_scenes_equal_the_model(T, monkeypatch, px, nz):
    """Blob volumes at two densities under the identity, a whole-voxel shift, a rigid turn and a general affine map, with
    ids outside the rows, prev_track, a counter that does not start at 0 and per-point ids: all eight outputs."""
    for density in vt.DENSITIES:
        s = vt.random_scene(px, nz, density)
        for name, M in vt.scene_maps(px, nz).items():
            want = vt.scene_model(px, nz, density, name)
            for g in (None, '1'):
                set_g(monkeypatch, g)
                same(raw(T, s['prev'], s['n_prev'], s['cur'], s['n_cur'], M, prev_track=s['prev_track'], t0=s['t0'], ids=s['ids']), want)
    # the scenes hold what they are meant to hold: pairs, matches, new and lost tracks, voxels out of view, skipped ids
    if px >= 33:
        st = vt.scene_model(px, nz, 'dense', 'rigid')['stats']
        assert st[3] > 16 and st[5] > 0 and st[6] > 0 and st[7] > 0 and st[1] < st[0] and st[8] > 0 and st[9] > 0


def test_thresholds_and_defaults(T, monkeypatch):
    """min_overlap and min_iou at work on a scene where they decide, and prev_track NULL: the track of a is a."""
    set_g(monkeypatch, None)
    px, nz = 33, 7
    s = vt.random_scene(px, nz, 'dense')
    M = vt.scene_maps(px, nz)['rigid']
    base = vt.model(s['prev'], s['n_prev'], s['cur'], s['n_cur'], M)
    assert base['stats'][5] >= 2
    c = np.sort(base['cur_info'][base['match'] >= 0, 2])
    for how in (dict(), dict(min_overlap=int(c[-1])), dict(min_overlap=int(c[-1]) + 1), dict(min_iou=0.2), dict(min_iou=1.0),
                dict(min_overlap=3, min_iou=0.05)):
        want = vt.model(s['prev'], s['n_prev'], s['cur'], s['n_cur'], M, **how)
        same(raw(T, s['prev'], s['n_prev'], s['cur'], s['n_cur'], M, outputs='cmipvks', **how), want)
    assert vt.model(s['prev'], s['n_prev'], s['cur'], s['n_cur'], M, min_overlap=int(c[-1]))['stats'][5] >= 1
    assert vt.model(s['prev'], s['n_prev'], s['cur'], s['n_cur'], M, min_overlap=int(c[-1]) + 1)['stats'][5] == 0


# ---------------------------------------------------------------------------------------------- 2: NULL outputs
@pytest.mark.parametrize('outputs', [ALL, 'c', 'm', 'i', 'p', 'v', 't', 'k', 's', 'cv', 'ks', 'mt', 'ip', 'cmipvks'])
def test_null_output_subsets(T, monkeypatch, outputs):
    """Asked-for outputs equal the model, the others keep their fill byte."""
    set_g(monkeypatch, None)
    px, nz = 33, 7
    s = vt.random_scene(px, nz, 'dense')
    same(raw(T, s['prev'], s['n_prev'], s['cur'], s['n_cur'], vt.scene_maps(px, nz)['rigid'], prev_track=s['prev_track'], t0=s['t0'],
             ids=s['ids'], outputs=outputs), vt.scene_model(px, nz, 'dense', 'rigid'))


# ---------------------------------------------------------------------------------------------- 3: key folding
@pytest.mark.parametrize('px,nz', [(33, 7), (72, 5)])
def test_key_folding(T, monkeypatch, px, nz):
    """One instance filling whole lines (a wave has ONE run per segment) and a checkerboard of two ids (every lane its own
    run), matched to themselves under a shift: both equal the model, folded, unfolded and with one workgroup."""
    for build in (vt.whole_lines, vt.checker):
        vol, n = build(px, nz)
        other, n_other = vt.blobs(px, nz, 12, 6.0, seed=px)
        for prev, n_prev, M in ((vol, n, vt.shift_map(1, 0, 0)), (vol, n, vt.shift_map(2, 2, 0)), (other, n_other, vt.turn_map(20., (10., 10.)))):
            want = vt.model(prev, n_prev, vol, n, M, cap_pairs=None)
            assert want['stats'][2] > 0
            for g, fold in ((None, None), ('1', None), (None, '0'), ('2', '0')):
                set_g(monkeypatch, g, fold)
                same(raw(T, prev, n_prev, vol, n, M, outputs='cmipvks'), want)
    # the situations: one run per segment against one run per lane
    lines, _ = vt.whole_lines(px, nz)
    assert (np.diff(lines[:, ::2, :], axis=2) == 0).all() and (np.diff(vt.checker(px, nz)[0], axis=2) != 0).all()


# ---------------------------------------------------------------------------------------------- 4: a full pair table
def test_full_pair_table_gives_up_and_counts(T, monkeypatch):
    """cap_pairs = 16 and 33 distinct pairs: the call returns, stats[4] > 0, what is defined then equals the model and the
    Python binding raises."""
    px, nz = 33, 7
    vol, n = vt.many_pairs(px, nz)
    want = vt.model(vol, n, vol, n, vt.shift_map())
    assert want['stats'][3] == n > 16
    for g in (None, '1'):
        set_g(monkeypatch, g)
        got = raw(T, vol, n, vol, n, vt.shift_map(), cap_pairs=16, outputs='cmipvks')
        same(got, want, full_table=True)
        assert got[2]['stats'][4] >= n - 16
    st = dev_store(capacity=1 << 10, max_frames=2)
    with pytest.raises(RuntimeError, match='voxel instance match: .* found no slot'):
        st.voxel_instance_match(vol, n, vol, n, vt.shift_map(), cap_pairs=16)
    out = st.voxel_instance_match(vol, n, vol, n, vt.shift_map(), cap_pairs=64)          # enough slots: the same call is fine
    assert np.array_equal(out['pairs'].cpu().numpy().view(np.uint32), want['pairs'])


# ---------------------------------------------------------------------------------------------- 5: refused calls
def test_refused_calls_write_nothing(T, monkeypatch):
    set_g(monkeypatch, None)
    px, nz = 8, 1
    s = vt.random_scene(px, nz, 'sparse')
    ok = dict(prev_track=s['prev_track'], ids=s['ids'], t0=5)
    from pca_amd import _lib
    need = int(_lib.load().pca_voxel_instance_match_workspace_bytes(s['n_prev'], s['n_cur'], 16))
    bad_M = vt.shift_map()
    bad_M[1, 2] = np.inf
    nan_M = vt.shift_map()
    nan_M[2, 3] = np.nan
    cases = [(dict(px=0), r'px must be in 1\.\.1024'), (dict(px=1025), r'px must be in 1\.\.1024'), (dict(nz=33), r'nz must be in 1\.\.32'),
             (dict(nz=0), r'nz must be in 1\.\.32'),
             (dict(rows_prev=0), r'n_prev and n_cur must be in 1\.\.65536'), (dict(rows_cur=0), r'n_prev and n_cur must be in 1\.\.65536'),
             (dict(rows_prev=65537), r'n_prev and n_cur must be in 1\.\.65536'), (dict(rows_cur=65537), r'n_prev and n_cur must be in 1\.\.65536'),
             (dict(M=bad_M), 'every entry of M must be finite'), (dict(M=nan_M), 'every entry of M must be finite'),
             (dict(cap_pairs=24), r'cap_pairs must be a power of two in 16\.\.2\^22'), (dict(cap_pairs=8), 'cap_pairs must be a power of two'),
             (dict(cap_pairs=1 << 23), 'cap_pairs must be a power of two'),
             (dict(cap_pairs=16, ws_bytes=need - 1), 'workspace too small'), (dict(outputs=''), 'at least one output is needed'),
             (dict(min_iou=1.5), r'min_iou must be finite and in 0\.\.1'), (dict(min_iou=-0.1), 'min_iou must be finite'),
             (dict(min_iou=float('nan')), 'min_iou must be finite'), (dict(min_overlap=0), 'min_overlap must be >= 1'),
             (dict(null_counter=True), 'track_counter must not be NULL')]
    for how, message in cases:
        how = dict(ok, **how)
        M = how.pop('M', vt.shift_map())
        r, err, outs, _, counter = raw(T, s['prev'], s['n_prev'], s['cur'], s['n_cur'], M, **how)
        assert r == -1, how
        assert re.search('^voxel instance match: .*' + message, err), (err, message)
        for c, (name, dt) in OUTPUTS.items():
            assert (outs[name] == FILLED[dt]).all(), (how, name)
        assert counter.item() == 5
    # track_ids without ids
    r, err, outs, _, _ = raw(T, s['prev'], s['n_prev'], s['cur'], s['n_cur'], vt.shift_map(), ids=None, outputs='ct')
    assert r == -1 and err == 'voxel instance match: track_ids needs ids' and (outs['cur_track'] == FILLED['int32']).all()


# ---------------------------------------------------------------------------------------------- 6: chaining on the device
def test_three_calls_chain_without_a_host_read(T, monkeypatch):
    """Three volumes, three calls back to back on one stream: each call's cur_track is the next one's prev_track, the counter
    stays on the device, and nothing is read before the end; tracks and counter are the model's."""
    set_g(monkeypatch, None)
    px, nz = 72, 5
    vols = [vt.blobs(px, nz, 40, 6.0, seed=100 + i) for i in range(2)]
    vols.append((vt.moved(vols[1][0], (3, -2, 0)), vols[1][1]))
    maps = [vt.shift_map(), vt.turn_map(10., (30., 40.), (2., 1., 0.)), vt.shift_map(-3, 2, 0)]
    empty = np.full_like(vols[0][0], -1)
    want, prev, n_prev, track, t0 = [], empty, 1, None, 0
    for (vol, n), M in zip(vols, maps):
        want.append(vt.model(prev, n_prev, vol, n, M, prev_track=track, t0=t0))
        prev, n_prev, track, t0 = vol, n, want[-1]['cur_track'], int(want[-1]['counter'])
    assert want[0]['stats'][6] > 10 and want[1]['stats'][5] > 0 and want[1]['stats'][6] > 0
    assert want[2]['stats'][5] > 10 and want[2]['stats'][6] == 0                        # the shifted copy keeps every track in view
    counter = T.zeros(1, dtype=T.int32, device='cuda')
    prev, n_prev, track, got = T.from_numpy(empty).cuda(), 1, None, []
    for (vol, n), M in zip(vols, maps):
        cur = T.from_numpy(np.array(vol)).cuda()
        r, _, outs, _, counter = raw(T, prev, n_prev, cur, n, M, prev_track=track, counter=counter, outputs='cs', sync=False)
        assert r == 0
        got.append(outs)
        prev, n_prev, track = cur, n, outs['cur_track'].view(T.int32)
    T.cuda.synchronize()
    for g, w in zip(got, want):
        assert np.array_equal(g['cur_track'].view(T.int32).cpu().numpy(), w['cur_track'])
        assert np.array_equal(g['stats'].view(T.int64).cpu().numpy()[[0, 1, 2, 3, 5, 6, 7, 8, 9]], w['stats'][[0, 1, 2, 3, 5, 6, 7, 8, 9]])
    assert counter.item() == want[-1]['counter']
    used = np.concatenate([w['cur_track'] for w in want])
    assert used.max() == counter.item() - 1                  # numbers are handed out densely and never twice


# ---------------------------------------------------------------------------------------------- 7: the Python layers
def test_device_store_and_generator_layers(T, monkeypatch):
    set_g(monkeypatch, None)
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import host_logic as hl
    from pca_amd.tracks import grid_geom
    px, nz = 33, 7
    s = vt.random_scene(px, nz, 'dense')
    M = vt.scene_maps(px, nz)['rigid']
    want = vt.scene_model(px, nz, 'dense', 'rigid')
    st = dev_store(capacity=1 << 10, max_frames=2)
    counter = T.full((1, ), s['t0'], dtype=T.int32, device='cuda')
    out = st.voxel_instance_match(s['prev'], s['n_prev'], T.from_numpy(np.array(s['cur'])).cuda(), s['n_cur'], M,
                                  prev_track=s['prev_track'], counter=counter, ids=s['ids'])
    assert sorted(out) == ['counter', 'cur_info', 'cur_track', 'match', 'pairs', 'prev_info', 'stats', 'track_ids', 'track_vol']
    for k in ('cur_track', 'match', 'track_vol', 'track_ids', 'stats'):
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    for k in ('cur_info', 'prev_info', 'pairs'):             # (int32 tensors that hold u32; pairs compacted and sorted by (b, a))
        assert np.array_equal(out[k].cpu().numpy().view(np.uint32), want[k]), k
    assert out['counter'] is counter and counter.item() == want['counter']
    with pytest.raises(ValueError, match='the shape of prev_inst'):
        st.voxel_instance_match(s['prev'], s['n_prev'], s['cur'][:3], s['n_cur'], M)
    with pytest.raises(RuntimeError, match='voxel instance match: min_iou'):
        st.voxel_instance_match(s['prev'], s['n_prev'], s['cur'], s['n_cur'], M, min_iou=1.5)
    # the generator builds M from two grids and the rigid map between them
    gen = SemBEVGenerator(SEM_IDXS, 33., px, 0., 0., False, 20., 20., 0.5, None)
    prev_geom = grid_geom([1., -2., 0.3], hl.rotation_matrix_3d(0.3), 0., 0., 33., px, -2., 0.5)
    cur_geom = grid_geom([2.5, -1., 0.3], hl.rotation_matrix_3d(0.45), 0., 0., 33., px, -2., 0.5)
    Tm = np.eye(4)
    Tm[:3, :3], Tm[:3, 3] = hl.rotation_matrix_3d(-0.1), (-1.5, 0.2, 0.)
    got = gen.voxel_instance_match_device((s['prev'], s['n_prev'], prev_geom), (s['cur'], s['n_cur'], cur_geom), Tm)
    model = vt.model(s['prev'], s['n_prev'], s['cur'], s['n_cur'], hl.voxel_index_map(prev_geom, cur_geom, Tm))
    assert model['stats'][3] > 10
    assert np.array_equal(got['cur_track'].cpu().numpy(), model['cur_track']) and np.array_equal(got['stats'].cpu().numpy(), model['stats'])
    with pytest.raises(ValueError, match='share px and nz'):
        gen.voxel_instance_match_device((s['prev'], s['n_prev'], prev_geom), (s['cur'][:5], s['n_cur'], cur_geom), Tm)


def test_store_frame_over_a_kitti_run(T, tmp_path):
    """store_frame() is the product of the T_new_prev that moved stored points, the same through integrate and integrate_many,
    and the stored points are what they were without the bookkeeping (the run itself is held to the oracle elsewhere)."""
    from kitti360_sem_pc_accum import Kitti360SemanticPointCloudAccumulator
    from obs_dataloaders.kitti360_obs_dataloader import Kitti360Dataloader
    n = 7
    one = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=n)
    root, seq, calib, Ts = kitti_tree(tmp_path, n)
    want = np.eye(4)
    for k in range(1, n):                                    # (the first frame finds nothing stored to move)
        want = Ts[k] @ want
    assert np.array_equal(one.store_frame(), want) and not np.array_equal(want, np.eye(4))
    many = Kitti360SemanticPointCloudAccumulator(50., calib, 1e3, 'none', KITTI_FILTERS, SEM_IDXS, True, dict(BEV_KITTI))
    it = iter(Ts)
    many.pose_provider = lambda pc: next(it)
    batch = list(Kitti360Dataloader(root, 1, [seq], [0], [n]))
    for lo, hi in ((0, 1), (1, 4), (4, n)):
        many.integrate_many(batch[lo:hi])
        part = np.eye(4)
        for k in range(1, hi):
            part = Ts[k] @ part
        assert np.array_equal(many.store_frame(), part)
    assert np.array_equal(many.store.rows(), one.store.rows())


# ---------------------------------------------------------------------------------------------- 8: end to end
def car_block(centre, size, spacing=0.2, cls=13):
    """Stored rows of a filled block of car-class points around `centre` (view-frame metres)."""
    ax = [np.arange(-0.5 * s, 0.5 * s + 1e-9, spacing) + c for s, c in zip(size, centre)]
    g = np.stack(np.meshgrid(*ax, indexing='ij'), axis=-1).reshape(-1, 3)
    rows = np.zeros((g.shape[0], 10))
    rows[:, 0:3], rows[:, 7] = g, cls
    return rows


def test_tracks_hold_over_a_kitti_drive(T, tmp_path):
    """A static scene of car-class blocks seen from three moments of a drive: the blocks in view of two consecutive samples keep
    their track although voxel_instances numbers them anew, a block that only the later frames hold gets a new number, the
    per-point tracks are those of the model run on the volumes read back, and boxes=True carries the boxes alongside."""
    from pca_amd import host_logic as hl
    acc = kitti_accumulator(tmp_path, dict(BEV_KITTI, view_size=64, pixel_size=64), n_frames=3)
    px, nz, z_range = 64, 4, (0., 4.)
    poses = np.array(acc.poses)
    # the scene in the store's coordinates of the first moment: five blocks in frame 0, a sixth in frame 1 only, one far block in
    # frame 2; block 0 lies behind the ego, where the drive's later views no longer reach
    centres = [(-28., 8., 1.), (8., 6., 1.), (-6., -9., 1.5), (3., -14., 1.), (-12., 10., 1.), (-2., 3., 1.), (14., -4., 1.)]
    blocks = [car_block(np.array(c) + poses[1], (3.6, 1.6, 1.2)) for c in centres]
    frames = [np.concatenate(blocks[:5]), blocks[5], blocks[6]]
    who = [np.concatenate([np.full(b.shape[0], i) for i, b in enumerate(blocks[:5])]), np.full(blocks[5].shape[0], 5),
           np.full(blocks[6].shape[0], 6)]
    assert acc.store.load_rows(frames) is None
    frame0 = acc.store_frame()
    how = dict(z_range=z_range, nz=nz, max_instances=16, part='present')

    def geom_of(idx):
        p = np.array(acc.poses)
        return (p[idx], hl.rotation_matrix_3d(hl.heading_rot_ang(p[:idx] - p[idx])), 0., 0., 64., px, 0., 1.)

    def block_tracks(out, frames_in):
        """{block: its track}: every point of a block in view carries ONE track"""
        ids, tr = out['ids'].cpu().numpy(), out['track_ids'].cpu().numpy()
        w = np.concatenate(who[:frames_in])
        assert ids.shape == tr.shape == w.shape
        assert np.array_equal(tr >= 0, ids >= 0)
        found = {}
        for b in np.unique(w[ids >= 0]):
            t = np.unique(tr[(w == b) & (ids >= 0)])
            assert t.size == 1, (b, t)
            found[int(b)] = int(t[0])
        assert len(set(found.values())) == len(found)        # the blocks are far apart: one instance, one track each
        return found

    def move(Tm):
        """what integrate() does to what is stored, without a new frame: the points and the poses are re-expressed, the ego's
        new pose [0, 0, 0] joins the track and the oldest one leaves it (the store keeps its three frames)"""
        acc.update_sem_pcs(Tm)
        acc.update_poses(Tm)
        acc.poses = [list(p) for p in acc.poses][1:] + [[0., 0., 0.]]

    # sample 1: frame 0 only, from the first pose on; a sequence starts, every block in view is new
    s1 = acc.track_instances(1, None, **how)
    assert sorted(set(s1) - {'inst', 'ids', 'table', 'label_counts', 'top_label', 'stats'}) == ['match', 'match_stats', 'state',
                                                                                                'track', 'track_ids', 'track_vol']
    t1 = block_tracks(s1, 1)
    assert sorted(t1) == [0, 1, 2, 3, 4] and sorted(t1.values()) == [0, 1, 2, 3, 4]
    assert s1['match_stats'].tolist()[5:8] == [0, 5, 0] and s1['state'].next_track() == 5
    # two known steps on (the stored points are re-expressed; the blocks are static), then frames 0 and 1 from the second pose
    steps = [np.eye(4), np.eye(4)]
    steps[0][:3, :3], steps[0][:3, 3] = hl.rotation_matrix_3d(-0.15), (-6., 0.5, 0.)
    steps[1][:3, :3], steps[1][:3, 3] = hl.rotation_matrix_3d(-0.2), (-7., -1., 0.)
    for Tm in steps:
        move(Tm)
    assert np.array_equal(acc.store_frame(), steps[1] @ (steps[0] @ frame0))
    prev_state = s1['state']
    s2 = acc.track_instances(2, prev_state, **how)
    t2 = block_tracks(s2, 2)
    assert 0 not in t2 and 5 in t2                           # block 0 has left the view, block 5 has come with frame 1
    kept = [b for b in t2 if b in t1]
    assert len(kept) >= 3 and all(t2[b] == t1[b] for b in kept)
    assert t2[5] == 5 and s2['state'].next_track() == 6      # the new block takes the next number
    # ... although the instance numbers themselves changed between the samples
    id1 = {b: int(np.unique(s1['ids'].cpu().numpy()[(np.concatenate(who[:1]) == b)])[-1]) for b in kept}
    id2 = {b: int(np.unique(s2['ids'].cpu().numpy()[(np.concatenate(who[:2]) == b)])[-1]) for b in kept}
    assert id1 != id2
    # the per-point tracks are those of the model on the volumes read back
    Tm = acc.store_frame() @ np.linalg.inv(prev_state.frame)
    M = hl.voxel_index_map(prev_state.geom, s2['state'].geom, Tm)
    assert np.allclose(np.array(s2['state'].geom[0]), geom_of(2)[0]) and np.array_equal(s2['state'].geom[1], geom_of(2)[1])
    want = vt.model(prev_state.inst.cpu().numpy(), 16, s2['inst'].cpu().numpy(), 16, M, prev_track=prev_state.track.cpu().numpy(),
                    t0=5, ids=s2['ids'].cpu().numpy())
    for k, name in (('track', 'cur_track'), ('track_vol', 'track_vol'), ('track_ids', 'track_ids'), ('match', 'match'),
                    ('match_stats', 'stats')):
        assert np.array_equal(s2[k].cpu().numpy(), want[name]), k
    assert want['stats'][5] == len(kept) and want['stats'][6] == 1
    # a third moment three samples apart from the first, the whole window, with the boxes alongside
    move(steps[0])
    s3 = acc.track_instances(2, s2['state'], boxes=True, **dict(how, part='full'))
    assert {'fit', 'fit_n', 'boxes', 'box_stats', 'track', 'state'} <= set(s3)
    t3 = block_tracks(s3, 3)
    both = [b for b in t3 if b in t2]
    assert len(both) >= 3 and all(t3[b] == t2[b] for b in both)
    assert t3[6] == 6                                        # the block of the last frame: the next number
    n3 = int(s3['stats'][3].item())
    boxes, track = s3['boxes'].cpu().numpy(), s3['track'].cpu().numpy()
    assert np.isfinite(boxes[:n3]).all() and (track[:n3] >= 0).all() and (track[n3:] == -1).all() and np.isnan(boxes[n3:]).all()
    # nothing was written to the store, and grids of another size are refused
    with pytest.raises(ValueError, match='share px and nz'):
        acc.track_instances(2, s3['state'], **dict(how, nz=8))
    acc.store.check_status()
