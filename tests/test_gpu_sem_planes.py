"""GPU: BEV planes of any semantic class group (pca_bev_class_planes, DeviceStore.bev_class_planes, SemBEVGenerator
sem_planes / gen_sem_probmap / gen_gridmap_count_map) against the reference's fixture, the main raster, the C oracle
(pinned per group by tests/test_sem_planes_golden.py) and plain numpy."""
import pickle
import random

import numpy as np
import pytest

from test_gpu_kernels import DYNOBJ, SEM_IDXS, T, dev_store, orc  # noqa: F401  (T, orc: fixtures)
from window_pass_common import BEV_KITTI, INTS, kitti_accumulator, params

pytestmark = pytest.mark.gpu

SETS = ('present', 'future', 'full')
SEM_PLANES = {'sidewalk': [1], 'vehicle': ['car', 'truck', 'bus', 'motorcycle'], 'roadway': ['road']}


def closed_form(n, n_g):
    n, n_g = np.asarray(n, dtype=np.float64), np.asarray(n_g, dtype=np.float64)
    return (n_g + 1.) / ((n_g + 1.) + ((n - n_g) + 1.))


def host(p16, p64, cnt):
    return p16.cpu().numpy(), p64.cpu().numpy(), None if cnt is None else cnt.cpu().numpy().view(np.uint32)


def random_rows(rng, n, lim, classes=tuple(range(19)) + (255, )):
    rows = np.zeros((n, 10))
    rows[:, 0:2] = rng.uniform(-lim, lim, (n, 2))
    rows[:, 2] = rng.uniform(-2, 4, n)
    rows[:, 3] = rng.integers(0, 256, n)
    rows[:, 4:7] = rng.integers(0, 256, (n, 3))
    rows[:, 7] = rng.choice(classes, n)
    rows[:, 9] = (rng.random(n) < 0.15).astype(float)
    return rows


# ---------------------------------------------------------------------------------------------- 1: the reference's fixture
def test_fixture_store_call_and_pregridded_helpers(T, golden):
    from bev_generator.sem_bev import SemBEVGenerator
    g = golden('sem_planes')
    view, px, hf, rot, dx, dy, zoom = g['cfg']
    px = int(px)
    groups = [[int(c) for c in row if c >= 0] for row in g['groups']]
    st = dev_store(capacity=4096, max_frames=4)
    assert st.load_rows([g['pc_present'], g['pc_future']]) is None
    p16, p64, cnt = host(*st.bev_class_planes(1, params((0., 0., 0.), rot, dx, dy, zoom * view, px, hf), groups,
                                              want_counts=True))
    st.check_status()
    assert p16.shape == p64.shape == (3, 5, px, px) and cnt.shape == (3, 6, px, px)
    for s, name in enumerate(SETS):
        assert np.array_equal(cnt[s, 5], g[f'count_{name}'])
        for k in range(5):
            assert np.array_equal(p64[s, k], g[f'prob_{name}'][k]), (name, k)
            assert np.array_equal(p16[s, k].view(np.uint16), g[f'prob16_{name}'][k].view(np.uint16)), (name, k)
            assert np.array_equal(cnt[s, k], g[f'count_{name}_g{k}']), (name, k)
    # the public helpers on the reference's own pre-gridded rows (its static partition)
    gen = SemBEVGenerator(SEM_IDXS, view, px, 0., 0., False, *INTS, hf)
    for name in ('present', 'future'):
        grid = g[f'grid_{name}']
        static = grid[grid[:, 9] != 1]
        keep = static.copy()
        count = gen.gen_gridmap_count_map(static)
        assert count.dtype == np.float64 and np.array_equal(count, g[f'count_{name}'])
        for k in range(5):
            prob = gen.gen_sem_probmap(static, groups[k])
            assert prob.dtype == np.float64 and np.array_equal(prob, g[f'prob_{name}'][k]), (name, k)
        assert np.array_equal(gen.gen_sem_probmap(static, ['car', 'truck', 'bus', 'motorcycle']), g[f'prob_{name}'][1])
        w = static[:, 3]
        want = np.flip(np.histogram2d(static[:, 1], static[:, 0], range=[[0, px], [0, px]], bins=[px, px], weights=w)[0], 0)
        np.testing.assert_allclose(gen.gen_gridmap_count_map(static, weights=w), want, rtol=1e-13, atol=0)
        assert np.array_equal(static, keep)                      # inputs are not touched
    assert gen.height_filter == hf
    with pytest.raises(KeyError):
        gen.gen_sem_probmap(static, ['sidewalk'])


# ---------------------------------------------------------------------------------------------- 2: main raster and oracle
def test_groups_equal_main_raster_planes_and_oracle_in_an_augmented_frame(T, orc):
    from pca_amd import host_logic as hl
    rng = np.random.default_rng(77)
    frames = [random_rows(rng, 4000, 40.) for _ in range(3)]
    origin, rot, dx, dy, view, px, hf = (0.4, -0.3, 0.2), 2.1, 1.75, -2.5, 1.07 * 60., 64, 2.5
    groups = [[0], DYNOBJ, [1], [2, 8, 13], [0, 255]]
    st = dev_store(capacity=1 << 14, max_frames=4)
    assert st.load_rows(frames) is None
    prm = params(origin, rot, dx, dy, view, px, hf)
    m16, m64 = st.bev(2, prm, want_f64=True)
    m16, m64 = m16.cpu().numpy(), m64.cpu().numpy()
    p16, p64, cnt = host(*st.bev_class_planes(2, prm, groups, want_counts=True))
    st.check_status()
    for s in range(3):
        for k, plane in ((0, 0), (1, 5)):                        # [road] = the road plane, DYNOBJ = the dynamic plane
            assert np.array_equal(p64[s, k], m64[7 * s + plane]), (s, k)
            assert np.array_equal(p16[s, k].view(np.uint16), m16[7 * s + plane].view(np.uint16)), (s, k)
    ost = orc.Store.from_rows(np.concatenate(frames))
    n_split = frames[0].shape[0] + frames[1].shape[0]
    for k, grp in enumerate(groups):
        oprm = orc.make_bev_params(origin, hl.rotation_matrix_3d(rot), dx, dy, view, px, hf, *INTS, 0, grp, False)
        ref = orc.bev(ost, n_split, oprm)
        for s in range(3):
            assert np.array_equal(p64[s, k], ref['planes'][7 * s + 5]), (s, k)
            assert np.array_equal(p16[s, k].view(np.uint16), ref['f16'][7 * s + 5].view(np.uint16)), (s, k)
            assert np.array_equal(closed_form(cnt[s, 5], cnt[s, k]), p64[s, k])
    assert np.array_equal(cnt[2], cnt[0] + cnt[1]) and cnt[2, 5].sum() > 3000


# ---------------------------------------------------------------------------------------------- 3: many workgroups, big cell
@pytest.mark.parametrize('cap_g', [None, '2'])
def test_many_level1_workgroups_and_a_cell_beyond_16_bit(T, monkeypatch, cap_g):
    """40 frames x 8 000 rows + 70 000 rows in one cell, 256^2, 16 groups: 48 level-1 workgroups whose points stay in
    registers, or -- PCA_BEV_CLASS_G=2 -- two whose chunks (195 000 points) go past the register path.  Identity rotation
    and zero origin: the view coordinates are x + dx, y + dy exactly, so numpy's unfused cell expression is the kernel's."""
    if cap_g:
        monkeypatch.setenv('PCA_BEV_CLASS_G', cap_g)
    rng = np.random.default_rng(9)
    view, px, hf, dx, dy = 100., 256, 2.0, 0.7, -1.3
    frames = [random_rows(rng, 8000, 60.) for _ in range(40)]
    pile = random_rows(rng, 70000, 1.)
    cell_lo = np.array([(140 - 128) * view / px - dx, (90 - 128) * view / px - dy])
    pile[:, 0:2] = cell_lo + rng.uniform(0.05, 0.3, (70000, 2))
    pile[:, 2], pile[:, 9] = 0.5, 0.
    frames[25] = np.concatenate([frames[25], pile])
    split = 22
    groups = [sorted(rng.choice(20, size=rng.integers(1, 6), replace=False).tolist()) for _ in range(14)] + [[255], [3]]
    groups = [[255 if c == 19 else c for c in grp] for grp in groups]
    st = dev_store(capacity=1 << 19, max_frames=64)
    assert st.load_rows(frames) is None
    p16, p64, cnt = host(*st.bev_class_planes(split, params((0., 0., 0.), 0., dx, dy, view, px, hf), groups,
                                              want_counts=True))
    st.check_status()
    rows = np.concatenate(frames)
    n_present = sum(f.shape[0] for f in frames[:split])
    ax, ay = rows[:, 0] + dx, rows[:, 1] + dy
    keep = (ax > -0.5 * view) & (ax < 0.5 * view) & (ay > -0.5 * view) & (ay < 0.5 * view) & (rows[:, 2] < hf) & (rows[:, 9] != 1)
    i = np.clip(np.floor(ax / view * px + 0.5 * px).astype(np.int64), 0, px - 1)
    j = np.clip(np.floor(ay / view * px + 0.5 * px).astype(np.int64), 0, px - 1)
    cell = (px - 1 - j) * px + i
    future = np.arange(rows.shape[0]) >= n_present
    want = np.zeros((3, 17, px * px), np.int64)
    for s, in_set in enumerate((~future, future)):
        want[s, 16] = np.bincount(cell[keep & in_set], minlength=px * px)
        for k, grp in enumerate(groups):
            want[s, k] = np.bincount(cell[keep & in_set & np.isin(rows[:, 7], grp)], minlength=px * px)
    want[2] = want[0] + want[1]
    want = want.reshape(3, 17, px, px)
    assert want[1, 16].max() > 65535                             # beyond 16-bit counters
    assert np.array_equal(cnt, want)
    prob = closed_form(want[:, 16:17], want[:, :16])
    assert np.array_equal(p64, prob)
    assert np.array_equal(p16.view(np.uint16), prob.astype(np.float16).view(np.uint16))


# ---------------------------------------------------------------------------------------------- 4: owed chain
@pytest.mark.parametrize('k', [1, 2, 3, 4])
def test_owed_chain_is_applied_to_what_is_read_and_stays_owed(T, orc, k):
    from pca_amd import host_logic as hl
    from test_gpu_kernels import _tilting_transform
    rng = np.random.default_rng(40 + k)
    frames = [random_rows(rng, 5000, 40.) for _ in range(3)]
    groups = [[0], DYNOBJ, [1, 2], [255]]
    origin, view, px, hf = (0.3, -0.2, 0.1), 80., 128, 1.5
    lazy, twin = dev_store(capacity=1 << 15, max_frames=8), dev_store(capacity=1 << 15, max_frames=8)
    lazy.CHAIN_K = twin.CHAIN_K = 4
    assert lazy.load_rows(frames) is None and twin.load_rows(frames) is None
    ost = orc.Store.from_rows(np.concatenate(frames))
    for step in range(k):
        Tm = _tilting_transform(step)                            # changes z: the height filter sees the transformed z
        lazy.retransform(Tm, defer=True)
        twin.retransform(Tm, defer=True)
        orc.retransform(ost, Tm)
    twin.flush_pending()
    n_rows = sum(f.shape[0] for f in frames)
    before = [t[:n_rows].clone() for t in (lazy.x, lazy.y, lazy.z)]
    prm = params(origin, 0., 0., 0., view, px, hf)
    got = host(*lazy.bev_class_planes(2, prm, groups, want_counts=True))
    want = host(*twin.bev_class_planes(2, prm, groups, want_counts=True))
    assert len(lazy._pending) == k and not twin._pending
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint16) if a.dtype == np.float16 else a, b.view(np.uint16) if b.dtype == np.float16 else b)
    assert got[2][2, 4].sum() > 3000
    assert all(T.equal(a, b[:n_rows]) for a, b in zip(before, (lazy.x, lazy.y, lazy.z)))   # the store was not written
    # the transforms are still owed: the main raster applies them now and matches the oracle
    _, m64 = lazy.bev(2, prm, want_f64=True)
    oprm = orc.make_bev_params(origin, hl.rotation_matrix_3d(0.), 0., 0., view, px, hf, *INTS, 0, DYNOBJ, False)
    ref = orc.bev(ost, frames[0].shape[0] + frames[1].shape[0], oprm)['planes']
    m64 = m64.cpu().numpy()
    for s in range(3):
        for plane in (0, 2, 3, 4, 5, 6):
            assert np.array_equal(m64[7 * s + plane], ref[7 * s + plane]), (s, plane)
        assert np.array_equal(got[1][s, 0], ref[7 * s + 0]) and np.array_equal(got[1][s, 1], ref[7 * s + 5])
    lazy.check_status()
    twin.check_status()


# ---------------------------------------------------------------------------------------------- 5 and 7: the KITTI drop-in
def test_noted_k1_runs_before_the_class_planes(T, tmp_path, monkeypatch):
    groups = [[0], DYNOBJ, [1]]
    prm = params((0., 0., 0.), 0.3, 0., 0., 50., 32, None)
    out = []
    for fuse in ('1', '0'):
        monkeypatch.setenv('PCA_FUSE_K1', fuse)
        acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=6)
        st = acc.store
        assert (st._k1_noted is not None) == (fuse == '1')       # integrate() left the newest frame's K1 for the next raster
        n = st.n_frames
        out.append(host(*st.bev_class_planes(n - 1, prm, groups, want_counts=True)))
        assert st._k1_noted is None
        st.check_status()
        st.set_defer_k1(False)
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.uint16) if a.dtype == np.float16 else a, b.view(np.uint16) if b.dtype == np.float16 else b)
    assert out[0][2][1, 3].sum() > 100                           # 'future' = the newest frame alone: its points are counted


def same_sample(a, b, keys):
    for k in keys:
        if k.startswith('trajs'):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert a[k].dtype == np.float16 and np.array_equal(a[k].view(np.uint16), b[k].view(np.uint16)), k


def test_dropin_sem_planes_keys_warp_and_refusals(T, tmp_path):
    from pca_amd import host_logic as hl
    px = BEV_KITTI['pixel_size']
    ref_keys = [f'{a}_{s}' for a in ('road', 'trajs', 'intensity', 'rgb', 'dynamic', 'elevation') for s in SETS]
    plain = kitti_accumulator(tmp_path, dict(BEV_KITTI)).generate_bev(5, 1, gen_future=True)[0]
    assert sorted(plain.keys()) == sorted(ref_keys)
    acc = kitti_accumulator(tmp_path, dict(BEV_KITTI, sem_planes=SEM_PLANES))
    assert acc.sem_bev_generator.sem_planes == SEM_PLANES and not acc._fast_bev_ok(5)
    bev = acc.generate_bev(5, 1, gen_future=True)[0]
    assert type(bev) is dict and type(pickle.loads(pickle.dumps(bev))) is dict
    same_sample(bev, plain, ref_keys)                            # the 15 reference keys are what they were
    extra = [f'{name}_{s}' for name in SEM_PLANES for s in SETS]
    assert sorted(bev.keys()) == sorted(ref_keys + extra)
    for k in extra:
        assert bev[k].dtype == np.float16 and bev[k].shape == (px, px)
    for s in SETS:                                               # the same class sets as two of the sample's own planes
        assert np.array_equal(bev[f'vehicle_{s}'].view(np.uint16), bev[f'dynamic_{s}'].view(np.uint16))
        assert np.array_equal(bev[f'roadway_{s}'].view(np.uint16), bev[f'road_{s}'].view(np.uint16))
    assert any(not np.array_equal(bev[f'sidewalk_{s}'], bev[f'roadway_{s}']) for s in SETS)
    many = acc.generate_bev_many([4, 5])
    assert type(many[1]) is dict
    same_sample(many[1], bev, ref_keys + extra)
    # do_warp: the class planes go through the same warp as the 21 planes
    gen = acc.sem_bev_generator
    gen.do_warp = True
    np.random.seed(11)
    random.seed(11)                                              # (the warp's signs come from `random`)
    warped = acc.generate_bev(5, 1, gen_future=True)[0]
    np.random.seed(11)
    random.seed(11)
    i_warp, j_warp = gen.get_random_warp_params(0.15, 0.30, px, px)
    a1, a2 = hl.cal_warp_params(i_warp, int(px / 2), px - 1)
    b1, b2 = hl.cal_warp_params(j_warp, int(px / 2), px - 1)
    for k in extra + ['road_full', 'dynamic_present']:
        want = hl.warp_dense_probmaps(bev[k].astype(np.float64)[None], a1, a2, b1, b2)[0].astype(np.float16)
        assert np.array_equal(warped[k].view(np.uint16), want.view(np.uint16)), k
    assert any(not np.array_equal(warped[k], bev[k]) for k in extra)
    gen.do_warp = False
    # refusals at the call
    gen.sem_planes = {'road': [0]}
    with pytest.raises(ValueError, match='road'):
        acc.generate_bev(5, 1, gen_future=True)
    gen.sem_planes = {'kerb': ['sidewalk']}
    with pytest.raises(KeyError):
        acc.generate_bev(5, 1, gen_future=True)
    gen.sem_planes = {}
    same_sample(acc.generate_bev(5, 1, gen_future=True)[0], plain, ref_keys)
    acc.store.check_status()


def test_host_array_inputs_go_through_the_temporary_stores(T, golden):
    """generate_bev called with host arrays (not a WindowPart): the class planes equal the fixture's."""
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import host_logic as hl
    g = golden('sem_planes')
    view, px, hf, rot, dx, dy, zoom = g['cfg']
    px = int(px)
    gen = SemBEVGenerator(SEM_IDXS, view, px, 0., 0., False, *INTS, hf)
    gen.sem_planes = {'vehicle': ['car', 'truck', 'bus', 'motorcycle'], 'c1': [1]}
    gen._frame = (hl.rotation_matrix_3d(rot), dx, dy, zoom * view)
    present, future = g['pc_present'], g['pc_future']
    bev = gen.generate_bev(present, future, np.concatenate([present, future]), [], [], [])
    for name in SETS:
        assert np.array_equal(bev[f'vehicle_{name}'].view(np.uint16), g[f'prob16_{name}'][1].view(np.uint16))
        assert np.array_equal(bev[f'c1_{name}'].view(np.uint16), g[f'prob16_{name}'][0].view(np.uint16))
        assert np.array_equal(bev[f'vehicle_{name}'].view(np.uint16), bev[f'dynamic_{name}'].view(np.uint16))


# ---------------------------------------------------------------------------------------------- 6: edges and refusals
def test_edges_and_refusals(T):
    rng = np.random.default_rng(3)
    frames = [random_rows(rng, 1000, 12.) for _ in range(2)]
    rows = np.concatenate(frames)
    groups = [[0], DYNOBJ]
    st = dev_store(capacity=4096, max_frames=4)
    assert st.load_rows(frames) is None
    static_in = lambda r, view: ((np.abs(r[:, 0]) < 0.5 * view) & (np.abs(r[:, 1]) < 0.5 * view) & (r[:, 9] != 1))  # noqa: E731
    # px = 1: one cell holds everything in the view
    p16, p64, cnt = host(*st.bev_class_planes(1, params((0., 0., 0.), 0., 0., 0., 20., 1, None), groups, want_counts=True))
    k0, k1 = static_in(frames[0], 20.), static_in(frames[1], 20.)
    assert cnt.shape == (3, 3, 1, 1)
    assert cnt[:, 2, 0, 0].tolist() == [k0.sum(), k1.sum(), k0.sum() + k1.sum()]
    assert cnt[0, 0, 0, 0] == (k0 & (frames[0][:, 7] == 0)).sum()
    assert np.array_equal(p64, closed_form(cnt[:, 2:3], cnt[:, :2]))
    # px = 1024: 16 384 tiles for 2 000 points
    p16, p64, cnt = host(*st.bev_class_planes(1, params((0., 0., 0.), 0., 0., 0., 20., 1024, None), groups, want_counts=True))
    assert cnt[2, 2].sum() == static_in(rows, 20.).sum() and cnt[2, 2].max() >= 1
    assert cnt[2, 1].sum() == (static_in(rows, 20.) & np.isin(rows[:, 7], DYNOBJ)).sum()
    assert np.array_equal(p64, closed_form(cnt[:, 2:3], cnt[:, :2]))
    assert np.array_equal(p16.view(np.uint16), p64.astype(np.float16).view(np.uint16))
    # refusals, before anything is launched
    prm = params((0., 0., 0.), 0., 0., 0., 20., 32, None)
    with pytest.raises(RuntimeError, match=r'bev class planes: px must be in 1\.\.1024'):
        st.bev_class_planes(1, params((0., 0., 0.), 0., 0., 0., 20., 1025, None), groups)
    with pytest.raises(RuntimeError, match=r'bev class planes: n_groups must be in 1\.\.16'):
        st.bev_class_planes(1, prm, [])
    with pytest.raises(RuntimeError, match=r'bev class planes: n_groups must be in 1\.\.16'):
        st.bev_class_planes(1, prm, [[k] for k in range(17)])
    # split at the window's begin / end
    full = host(*st.bev_class_planes(1, prm, groups, want_counts=True))
    at_begin = host(*st.bev_class_planes(0, prm, groups, want_counts=True))
    at_end = host(*st.bev_class_planes(2, prm, groups, want_counts=True))
    for got, empty_set, other in ((at_begin, 0, 1), (at_end, 1, 0)):
        assert (got[1][empty_set] == 0.5).all() and (got[0][empty_set] == np.float16(0.5)).all() and not got[2][empty_set].any()
        assert np.array_equal(got[1][other], got[1][2]) and np.array_equal(got[2][other], got[2][2])
        assert np.array_equal(got[1][2], full[1][2]) and np.array_equal(got[2][2], full[2][2])
    st.check_status()
    # empty windows: no frame at all in the range, and a store that holds nothing
    for store, args in ((st, dict(first_frame=1, last_frame=1)), (dev_store(capacity=1024, max_frames=4), {})):
        p16, p64, cnt = host(*store.bev_class_planes(1 if args else 0, prm, groups, want_counts=True, **args))
        assert (p64 == 0.5).all() and (p16 == np.float16(0.5)).all() and not cnt.any()
        store.check_status()
