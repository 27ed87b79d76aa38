"""GPU parity for grids above 1024 x 1024 (up to 4096 x 4096): the rasteriser runs them as bands of whole tile rows (at
most 16 384 tiles each), one level-1 pass and one launch of the tile kernels per band.  Same bar as tests/test_gpu_kernels.py:
bit-exact against the CPU oracle except the intensity planes (1e-12)."""
import numpy as np
import pytest

from test_gpu_kernels import DYNOBJ, KITTI_FILTERS, SEM_IDXS, assert_planes_match, dev_store, run_dev_bev, run_orc_bev

pytestmark = pytest.mark.gpu

INTS = (20., 20., 0.5)
NUSC_FILTERS = [10, 11, 12, 16, 18]


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def band_rows(px):
    """Tile rows per band (csrc/pca_bev.hip band_rows)."""
    tx = (px + 7) // 8
    return tx if tx * tx <= 16384 else 16384 // tx


def x_of_col(i, px, view):
    return ((i + 0.5) / px - 0.5) * view


def y_of_row(r, px, view):
    return ((px - 1 - r + 0.5) / px - 0.5) * view


def grid_rows(rng, px, view, n=150_000, cluster_tile=None, n_cluster=3000):
    """(M,10) rows on an axis-aligned raster (R = I, no shift): uniform points over the view, points in the cell rows on
    both sides of every band boundary, on the crop edges and in the clamp case (floor(...) == px), and a dense cluster of
    n_cluster records in one tile (tile row, tile column) -- a heavy-queue tile when it holds more than 2 560."""
    h = 0.5 * view
    parts = [np.stack([rng.uniform(-h, h, n), rng.uniform(-h, h, n)], 1)]
    step = 8 * band_rows(px)
    for r0 in range(step, px, step):                          # the last cell row of a band and the first of the next
        for r in (r0 - 1, r0):
            cols = rng.integers(0, px, 400)
            parts.append(np.stack([x_of_col(cols, px, view) + rng.uniform(-0.4, 0.4, 400) * view / px,
                                   np.full(400, y_of_row(r, px, view))], 1))
    inner = np.nextafter(h, 0.)                                # x / view * px + px / 2 rounds to px: clamped to px - 1
    e = rng.uniform(-h, h, 200)
    parts.append(np.stack([np.r_[np.full(50, inner), np.full(50, -inner), e[:100]],
                           np.r_[e[100:], np.full(50, inner), np.full(50, -inner)]], 1))
    parts.append(np.array([[h, 0.], [-h, 0.], [0., h], [0., -h], [inner, inner], [-inner, -inner]]))   # on the edge: out
    if cluster_tile is not None:
        tr, tc = cluster_tile
        cell = view / px
        r_last = min(8 * tr + 7, px - 1)                       # (a partial last tile has fewer cell rows / columns)
        x0, y0 = x_of_col(8 * tc, px, view) - 0.5 * cell, y_of_row(r_last, px, view) - 0.5 * cell
        w = min(8, px - 8 * tc) * cell
        hgt = (r_last - 8 * tr + 1) * cell
        parts.append(np.stack([x0 + rng.uniform(0.01, 0.99, n_cluster) * w, y0 + rng.uniform(0.01, 0.99, n_cluster) * hgt], 1))
    xy = np.concatenate(parts)
    m = xy.shape[0]
    rows = np.zeros((m, 10))
    rows[:, :2] = xy
    rows[:, 2] = rng.uniform(-2, 4, m)
    rows[:, 3] = rng.uniform(0, 1, m).astype(np.float32)
    rows[:, 4:7] = rng.integers(0, 256, (m, 3))
    rows[:, 7] = rng.choice([0, 1, 13, 17], m)
    rows[:, 9] = rng.random(m) < 0.05
    return rows[rng.permutation(m)]


def last_band_tile(px):
    """(tile row, tile column) of a tile in the last tile row: the last band (not band 0), a partial tile where px % 8 != 0."""
    tx = (px + 7) // 8
    return tx - 1, tx // 2


# ------------------------------------------------------------------------------------------ 1: grid sizes vs the oracle
@pytest.mark.parametrize('px', [1025, 1032, 1536, 2048, 4096])
def test_banded_grid_sizes_against_the_oracle(T, orc, px):
    """The first sizes past 1024 (a partial last tile, a partial last band), 1536, 2048 and 4096; points straddle every
    band boundary, sit on the crop edges and in the clamp case, and one tile of a band other than 0 goes through the heavy
    queue.  f16 and f64 planes."""
    rng = np.random.default_rng(px)
    view = 80.0
    rows = grid_rows(rng, px, view, cluster_tile=last_band_tile(px))
    cut = rows.shape[0] // 3
    p16, p64, used = run_dev_bev(T, rows[:cut], rows[cut:], view, px, 3.0, INTS, False, 0.0)
    assert not used
    ref = run_orc_bev(orc, rows[:cut], rows[cut:], view, px, 3.0, INTS, False, 0.0)
    assert_planes_match(p16, p64, ref, f'px={px}')


def test_banded_grid_with_rotation_and_shift(T, orc):
    """A rotated, shifted raster at 2048 (the general view transform) against the oracle."""
    rng = np.random.default_rng(77)
    rows = grid_rows(rng, 2048, 70.0, n=120_000, cluster_tile=(200, 100))
    rows[:, 3] = rng.integers(0, 256, rows.shape[0]) / 255.   # the NuScenes encoding (intensity_div255)
    p16, p64, _ = run_dev_bev(T, rows[:50_000], rows[50_000:], 60.0, 2048, None, (1., 30., 0.12), True, 0.7, 1.3, -2.1,
                              (0.4, -0.3, 0.1))
    ref = run_orc_bev(orc, rows[:50_000], rows[50_000:], 60.0, 2048, None, (1., 30., 0.12), True, 0.7, 1.3, -2.1,
                      (0.4, -0.3, 0.1))
    assert_planes_match(p16, p64, ref, 'rotated 2048')


# ------------------------------------------------------------------------------------------ 2: f64 intensities, memory path
@pytest.mark.parametrize('groups', [None, '4'])
def test_banded_f64_intensity_and_memory_path(T, orc, monkeypatch, groups):
    """Column 3 not f32-representable (the RecD side channel) at 2048, with level 1's default pieces and with four pieces
    (PCA_BEV_G: chunks far beyond level 1's register path, the memory path); and the f32 records on the memory path."""
    if groups:
        monkeypatch.setenv('PCA_BEV_G', groups)
        monkeypatch.setenv('PCA_BEV_CHUNK', '1024')
    from pca_amd import host_logic as hl
    rng = np.random.default_rng(5)
    px, view = 2048, 40.0
    rows = grid_rows(rng, px, view, n=100_000, cluster_tile=last_band_tile(px))
    cut = 40_000
    f32_rows = rows.copy()
    rows[:, 3] = rng.uniform(0, 1, rows.shape[0])             # genuine f64
    p16, p64, used = run_dev_bev(T, rows[:cut], rows[cut:], view, px, None, INTS, False, 0.3)
    assert used
    prm = orc.make_bev_params([0, 0, 0], hl.rotation_matrix_3d(0.3), 0, 0, view, px, None, *INTS, 0, DYNOBJ, False)
    ref = orc.bev(orc.Store.from_rows(rows), cut, prm, intensity64=rows[:, 3])
    assert_planes_match(p16, p64, ref, 'f64 intensity')
    p16, p64, used = run_dev_bev(T, f32_rows[:cut], f32_rows[cut:], view, px, None, INTS, False, 0.3)
    assert not used
    ref = run_orc_bev(orc, f32_rows[:cut], f32_rows[cut:], view, px, None, INTS, False, 0.3)
    assert_planes_match(p16, p64, ref, 'f32 intensity')


# ------------------------------------------------------------------------------------------ 3: owed chain
@pytest.mark.parametrize('write_back', [1, 0])
def test_banded_owed_chain(T, orc, write_back):
    """Two owed re-transforms at 2048: with write_back = 1 band 0 applies and stores them and the later bands read the
    updated store; with 0 every band applies them on the fly and the store keeps its coordinates.  The planes equal the
    oracle's on eagerly re-transformed rows either way; no point is transformed twice."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    rng = np.random.default_rng(11 + write_back)
    px, view = 2048, 80.0
    rows = grid_rows(rng, px, view, n=120_000, cluster_tile=last_band_tile(px))
    cut = 50_000
    Ts = []
    for k in range(2):
        a = 0.02 * (k + 1)
        Tm = np.eye(4)
        Tm[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        Tm[:3, 3] = [0.9, -0.3 * k, 0.01]
        Ts.append(Tm)
    st = dev_store(capacity=rows.shape[0], max_frames=4)
    assert st.load_rows([rows[:cut], rows[cut:]]) is None
    st.CHAIN_K = 2 if write_back else 4
    for Tm in Ts:
        st.retransform(Tm, defer=True)
    assert len(st._pending) == 2
    n_pend, _, _, wb = st.bev_pending(0, st.n_frames)
    assert (n_pend, wb) == (2, write_back)
    prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.2), 0., 0., view, px, 3.0, *INTS, 0, DYNOBJ, False)
    p16, p64 = st.bev(1, prm, want_f64=True)
    st.check_status()
    ost = orc.Store.from_rows(rows)
    for Tm in Ts:
        orc.retransform(ost, Tm)
    oprm = orc.make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.2), 0., 0., view, px, 3.0, *INTS, 0, DYNOBJ, False)
    ref = orc.bev(ost, cut, oprm)
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), ref, f'chain write_back={write_back}')
    n = rows.shape[0]
    stored = np.stack([st.x[:n].cpu().numpy(), st.y[:n].cpu().numpy(), st.z[:n].cpu().numpy()], 1)
    want = ost.rows()[:, :3] if write_back else rows[:, :3]
    assert np.array_equal(stored, want)
    assert len(st._pending) == (0 if write_back else 2)
    assert np.array_equal(st.rows(), ost.rows())               # (flushes what is still owed)


# ------------------------------------------------------------------------------------------ 4: extra planes
def test_banded_extra_reducers_max_mean(T):
    """The opt-in extra reducers at 2048 against the numpy model of test_bev_extra_reducers_max_mean (R = I, no shift),
    light tiles and a heavy tile outside band 0."""
    from pca_amd import _lib, host_logic as hl
    from pca_amd.device_store import make_bev_params
    rng = np.random.default_rng(31)
    px, view = 2048, 64.0
    rows = grid_rows(rng, px, view, n=150_000, cluster_tile=last_band_tile(px), n_cluster=4000)
    n = rows.shape[0]
    cut = 60_000
    st = dev_store(capacity=n, max_frames=4)
    assert st.load_rows([rows[:cut], rows[cut:]]) is None
    prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.0), 0., 0., view, px, None, *INTS, 0, DYNOBJ, False)
    extra = T.zeros((3, len(_lib.BEV_EXTRA_PLANES), px, px), dtype=T.float64, device='cuda')
    p16, p64 = st.bev(1, prm, want_f64=True, extra=extra)
    st.check_status()
    ex = extra.cpu().numpy()
    elev = p64.cpu().numpy()
    x, y, z, inten, sem, dyn = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 7], rows[:, 9]
    keep = (x > -view / 2) & (x < view / 2) & (y > -view / 2) & (y < view / 2) & (dyn != 1)
    i = np.clip(np.floor(x / view * px + 0.5 * px).astype(int), 0, px - 1)
    j = np.clip(np.floor(y / view * px + 0.5 * px).astype(int), 0, px - 1)
    cell = (px - 1 - j) * px + i
    is_future = np.arange(n) >= cut
    for s, sel in enumerate((~is_future, is_future, np.ones(n, bool))):
        m = keep & sel
        cnt = np.bincount(cell[m], minlength=px * px).astype(float)
        zmax = np.full(px * px, -np.inf)
        np.maximum.at(zmax, cell[m], z[m])
        zmax[cnt == 0] = 0.0
        zsum = np.bincount(cell[m], weights=z[m], minlength=px * px)
        zmean = np.where(cnt > 0, zsum / np.maximum(cnt, 1), 0.0)
        mr = m & (sem == 0)
        cr = np.bincount(cell[mr], minlength=px * px).astype(float)
        isum = np.bincount(cell[mr], weights=inten[mr], minlength=px * px)
        imean = np.where(cr > 0, isum / np.maximum(cr, 1), 0.0)
        assert np.array_equal(ex[s, 0].ravel(), zmax), f'max z set {s}'
        np.testing.assert_allclose(ex[s, 1].ravel(), zmean, rtol=0, atol=1e-11)
        np.testing.assert_allclose(ex[s, 2].ravel(), imean, rtol=0, atol=1e-11)
        obs = cnt > 0
        assert np.all(ex[s, 1].ravel()[obs] >= elev[7 * s + 6].ravel()[obs] - 1e-12)
    p16b, p64b = st.bev(1, prm, want_f64=True)
    assert T.equal(p64, p64b) and T.equal(p16, p16b)


# ------------------------------------------------------------------------------------------ 5: batched
def test_banded_bev_many_equals_single_calls(T):
    """DeviceStore.bev_many with three jobs at 2048 (different windows, splits, views) equals three bev() calls bit for bit."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    rng = np.random.default_rng(8)
    px = 2048
    frames = [grid_rows(rng, px, 60.0, n=40_000, cluster_tile=last_band_tile(px) if k == 2 else None) for k in range(5)]
    st = dev_store(capacity=sum(f.shape[0] for f in frames), max_frames=8)
    assert st.load_rows(frames) is None
    jobs = []
    for k, (split, first, last, view, rot) in enumerate(((2, 0, None, 60.0, 0.0), (3, 1, 5, 50.0, 0.4), (1, 0, 3, 64.0, -0.2))):
        prm = make_bev_params((0.3 * k, -0.2, 0.), hl.rotation_matrix_3d(rot), 0.1 * k, 0., view, px, 3.0 if k else None,
                              *INTS, 0, DYNOBJ, False)
        jobs.append((split, prm, first, last))
    out = T.empty((3, 21, px, px), dtype=T.float16, device='cuda')
    st.bev_many(jobs, out)
    st.check_status()
    for k, (split, prm, first, last) in enumerate(jobs):
        one = st.bev(split, prm, first_frame=first, last_frame=last)[0]
        assert T.equal(out[k].view(T.int16), one.view(T.int16)), k
    assert (out[:, 14].float() != 0.5).float().mean() > 0.005


# ------------------------------------------------------------------------------------------ 6: KITTI drop-in stream
def test_kitti_dropin_stream_at_pixel_size_2048(monkeypatch):
    """The KITTI-360 drop-in accumulator with pixel_size 2048 and the defaults (K1 deferred, view hints on): a 200 m horizon
    and an 80 m view, so frames are left out; 14 steps of integrate() + generate_bev(), one step without a raster, so that
    owed chains of 1..4 and a write-back occur.  Every step's planes and the final stored rows against the oracle pipeline."""
    import torch

    import sem_pc_accum
    from kitti360_sem_pc_accum import Kitti360SemanticPointCloudAccumulator
    from oracle import oracle as orc
    from pca_amd import host_logic as hl
    from test_gpu_dropin import BEV_KITTI
    H, W, N = 96, 320, 20_000
    cam_to_velo = np.array([[0.04307104361, -0.08829286498, 0.995162929, 0.8043914418],
                            [-0.999004371, 0.007784614041, 0.04392796942, 0.2993489574],
                            [-0.01162548558, -0.9960641394, -0.08786966659, -0.1770225824], [0, 0, 0, 1]])
    P = np.array([[130.0, 0, 160.0, 0], [0, 130.0, 48.0, 0], [0, 0, 1, 0]]) @ np.linalg.inv(cam_to_velo)

    def frame(k):
        rng = np.random.default_rng(7000 + k)
        pc = np.stack([rng.uniform(-30, 30, N), rng.uniform(-30, 30, N), rng.uniform(-2, 3, N), rng.uniform(0, 1, N)],
                      1).astype(np.float32)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        sem = rng.integers(0, 19, (H, W)).astype(np.uint8)
        sem[rng.random((H, W)) < 0.01] = 255
        return pc, img, sem
    pool = [frame(k) for k in range(3)]
    dev_pool = [(torch.from_numpy(i).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(s).cuda()) for p, i, s in pool]

    class Resident:
        def pred(self, rgb):
            return by_ptr[rgb.data_ptr()][None, None]
    by_ptr = {d[0].data_ptr(): d[2] for d in dev_pool}
    monkeypatch.setattr(sem_pc_accum, 'SemSegONNX', lambda path: Resident())
    a = -0.004
    Tm = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.]]) @ \
        np.array([[1, 0, 0, -2.0], [0, 1, 0, 0.01], [0, 0, 1, 0.002], [0, 0, 0, 1.]])
    horizon, bev_h, view, px = 200.0, 30.0, 80, 2048
    bev_params = dict(BEV_KITTI, view_size=view, pixel_size=px)
    calib = {'h_velo_cam': None, 'p_cam_frame': None, 'p_velo_frame': P}
    acc = Kitti360SemanticPointCloudAccumulator(horizon, calib, 1e3, 'resident', KITTI_FILTERS, SEM_IDXS, False, bev_params)
    acc._store_args = dict(capacity=1 << 22, max_frames=256)
    acc.pose_provider = lambda pc: Tm
    ost = orc.Store(120 * N)
    track = hl.PoseTrack()
    sizes, lo, removed_dev, removed_orc = [], 0, [], []

    def oracle_step(k):
        nonlocal sizes, lo
        pc, img, sem = pool[k % 3]
        if len(track):
            track.apply_transform(Tm)
            orc.retransform(ost, Tm, lo, ost.n)
        sizes.append(orc.kitti_project_sample_filter(ost, pc, P, img, sem, None, H, W, KITTI_FILTERS))
        track.append([0., 0., 0.])
        ev = 0
        if len(track) > 1:
            ev = track.evict_beyond(horizon, track.push_segment())
            lo += int(np.sum(sizes[:ev]))
            sizes = sizes[ev:]
        removed_orc.append(ev)
    fill = 60
    for k in range(fill):
        removed_dev.append(acc.integrate([(dev_pool[k % 3][0], dev_pool[k % 3][1], None)]))
        oracle_step(k)
    chains = set()
    for k in range(fill, fill + 14):
        removed_dev.append(acc.integrate([(dev_pool[k % 3][0], dev_pool[k % 3][1], None)]))
        oracle_step(k)
        if k == fill + 6:                                   # a step without a raster: the chain is one longer next time
            continue
        d = acc.get_incremental_path_dists()
        pidx = int(((d - bev_h) > 0).argmax())
        chains.add(len(acc.store._pending))
        bev = acc.generate_bev(pidx, 1, gen_future=True)[0]
        origin = np.array(track.poses[pidx])
        R = hl.rotation_matrix_3d(hl.heading_rot_ang(np.array(track.poses[:pidx]) - origin))
        prm = orc.make_bev_params(origin, R, 0., 0., view, px, None, 20., 20., 0.5, 0, [13, 14, 15, 17], False)
        sub = orc.Store(1)
        for name in ('x', 'y', 'z', 'intensity', 'rgbs', 'inst', 'dyn'):
            setattr(sub, name, getattr(ost, name)[lo:ost.n])
        sub.n = sub.cap = ost.n - lo
        F = orc.bev(sub, int(np.sum(sizes[:pidx])), prm)['f16']
        for s, name in enumerate(('present', 'future', 'full')):
            for key, pl in (('road', 0), ('dynamic', 5), ('elevation', 6)):
                assert np.array_equal(bev[f'{key}_{name}'].view(np.uint16), F[7 * s + pl].view(np.uint16)), (k, key, name)
            assert np.array_equal(bev[f'rgb_{name}'].view(np.uint16), F[7 * s + 2:7 * s + 5].view(np.uint16)), (k, name)
            di = np.abs(bev[f'intensity_{name}'].view(np.uint16).astype(int) - F[7 * s + 1].view(np.uint16).astype(int))
            assert di.max() <= 1 and (di != 0).mean() < 1e-3, (k, name)
        assert (bev['road_full'] != np.float16(0.5)).mean() > 0.001
    assert chains >= {1, 2, 3, 4}, chains
    assert acc.store.hints_taken > 0
    assert removed_dev == removed_orc
    assert np.array_equal(np.concatenate(acc.sem_pcs), ost.rows(lo))
    acc.store.check_status()


# ------------------------------------------------------------------------------------------ 7: NuScenes drop-in
def test_nuscenes_dropin_generate_bev_at_2048(monkeypatch):
    """One generate_bev of the NuScenes oracle-semantics accumulator at pixel_size 2048 (the / 255 intensity path, height
    filter) against the oracle pipeline."""
    from PIL import Image

    from nuscenes_oracle_sem_pc_accum import NuScenesOracleSemanticPointCloudAccumulator
    from oracle import oracle as orc
    from pca_amd import host_logic as hl
    from pca_amd.tracker import InstanceTracker
    import sem_pc_accum
    from test_gpu_dropin import FakeSemSeg
    monkeypatch.setattr(sem_pc_accum, 'SemSegONNX', lambda path: FakeSemSeg())
    F, n, ncam, H, W = 12, 30_000, 2, 180, 320
    rng = np.random.default_rng(2048)
    fake = FakeSemSeg()
    imgs = rng.integers(0, 256, (ncam, H, W, 3), dtype=np.uint8)
    sems = np.stack([fake.pred(im)[0, 0] for im in imgs]).astype(np.uint8)
    pils = [Image.fromarray(im) for im in imgs]
    px = 2048
    bev_params = dict(type='sem', view_size=51.2, pixel_size=px, max_trans_radius=0., zoom_thresh=0., do_warp=False,
                      int_scaler=1., int_sep_scaler=30., int_mid_threshold=0.12, height_filter=3.)
    acc = NuScenesOracleSemanticPointCloudAccumulator('fake.onnx', NUSC_FILTERS, SEM_IDXS, False, bev_params, 'boston',
                                                      False, None)
    st = orc.Store(F * n, intensity_div255=True)
    track, tracker, offs, T_global_world = hl.PoseTrack(), InstanceTracker(), [0], None
    for k in range(F):
        a = 0.002 * k
        Tk = np.eye(4)
        Tk[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        Tk[:3, 3] = [1000. + 1.5 * k, 500., 0.]
        pc = np.stack([rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-2, 4, n),
                       rng.integers(0, 256, n).astype(float), rng.uniform(1.01, W - 1.01, n),
                       rng.uniform(1.01, H - 1.01, n), rng.integers(-1, 5, n).astype(float)], 1)
        cam = rng.integers(-1, ncam, n)
        tokens, cls = ['parked', 'moving'], [0, 0]
        centers = [np.array([1010., 505., 0.5]), np.array([1005. + 0.5 * k, 495., 0.5])]
        obs = dict(images=pils, pc=pc, pc_cam_idx=cam, ego_at_lidar_ts=Tk, ego_global_x=Tk[0, 3],
                   ego_global_y=Tk[1, 3], inst_tokens=tokens, inst_cls=cls, inst_center=centers)
        assert acc.integrate([obs]) is None
        if T_global_world is None:
            T_global_world = np.linalg.inv(Tk)
        T_ego_world = T_global_world @ Tk
        pose = T_ego_world[:3, -1].tolist()
        pose[2] += 1.
        m = orc.nusc_sample_filter_transform(st, pc, cam, imgs, sems, T_ego_world, NUSC_FILTERS)
        offs.append(offs[-1] + m)
        track.append(pose)
        for ts, inst_idx in tracker.observe(k, tokens, cls, [orc.homo_transform(T_global_world, c[None])[0] for c in centers]):
            orc.mark_dynamic(st, offs[ts], offs[ts + 1], inst_idx)
        if len(track.poses) > 1:
            track.push_segment()
    acc.store.check_status()
    sizes = np.diff(offs)
    assert np.array_equal(acc.store.rows(), st.rows())
    pi = 6
    bev = acc.generate_bev(pi, 1, gen_future=True)[0]
    origin = np.array(track.poses[pi])
    poses = np.array(track.poses)
    R = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:pi] - origin))
    prm = orc.make_bev_params(origin, R, 0., 0., 51.2, px, 3., 1., 30., 0.12, 0, [13, 14, 15, 17], True)
    ref = orc.bev(st, int(sizes[:pi].sum()), prm)['f16']
    for s, name in enumerate(('present', 'future', 'full')):
        for k, key in ((0, 'road'), (5, 'dynamic'), (6, 'elevation')):
            assert np.array_equal(bev[f'{key}_{name}'].view(np.uint16), ref[7 * s + k].view(np.uint16)), (key, name)
        assert np.array_equal(bev[f'rgb_{name}'].view(np.uint16), ref[7 * s + 2:7 * s + 5].view(np.uint16)), name
        d = np.abs(bev[f'intensity_{name}'].view(np.uint16).astype(int) - ref[7 * s + 1].view(np.uint16).astype(int))
        assert d.max() <= 1
    assert (bev['road_full'] != np.float16(0.5)).mean() > 0.001


# ------------------------------------------------------------------------------------------ 8: warp
def test_warp_kernel_at_2048(T):
    """pca_bev_warp on 2048^2 planes against the numpy gather."""
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import host_logic as hl
    rng = np.random.default_rng(40)
    px = 2048
    for iw, jw in ((1100.3, 930.8), (800.2, 1200.6)):
        a1, a2 = hl.cal_warp_params(iw, int(px / 2), px - 1)
        b1, b2 = hl.cal_warp_params(jw, int(px / 2), px - 1)
        planes = rng.random((3, px, px))
        want = hl.warp_dense_probmaps(planes, a1, a2, b1, b2).astype(np.float16)
        got = SemBEVGenerator.warp_planes_device(T.from_numpy(planes.astype(np.float16)).cuda(), a1, a2, b1, b2)
        assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16)), (iw, jw)


# ------------------------------------------------------------------------------------------ 9: bounds
def test_grid_above_4096_is_rejected(T):
    from pca_amd.device_store import make_bev_params
    rows = np.zeros((10, 10))
    with pytest.raises(Exception, match=r'px must be in 1\.\.4096'):
        run_dev_bev(T, rows[:5], rows[5:], 80.0, 4097, None, INTS, False, 0.0)
    st = dev_store(capacity=16, max_frames=4)
    assert st.load_rows([rows[:5], rows[5:]]) is None
    prm = make_bev_params((0., 0., 0.), np.eye(3), 0., 0., 80., 4097, None, *INTS, 0, DYNOBJ, False)
    with pytest.raises(Exception, match=r'px must be in 1\.\.4096'):
        st.bev_many([(1, prm, 0, None)], T.empty((1, 21, 4097, 4097), dtype=T.float16, device='cuda'))
