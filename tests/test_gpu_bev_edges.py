"""GPU parity of the BEV rasteriser on the edge fixtures (tests/golden/bev_edges_*.npz: hand-built inputs run through the
real reference): points on cell boundaries and one ulp to either side, on the crop edge, z at the height filter, -0.0,
even-count medians, cells of exactly 64 values, intensities at the threshold, empty sets.  Every case on every route that
shares level 1 but differs afterwards, against the oracle and straight against the reference's own planes."""
import numpy as np
import pytest

from bev_edges_common import EDGE_CASES, EdgeCase
from test_gpu_kernels import DYNOBJ, assert_planes_match, dev_store, run_dev_bev, run_orc_bev

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


_oracle_planes = {}


def oracle_planes(orc, g):
    """The oracle's planes of a case: computed once, shared by the routes, never written to."""
    if g.name not in _oracle_planes:
        ref = run_orc_bev(orc, g['pc_present'], g['pc_future'], g.zoom * g.view, g.px, g.hf, g.ints, g.div255, g.rot, g.dx, g.dy)
        for v in ref.values():
            v.setflags(write=False)
        _oracle_planes[g.name] = ref
    return _oracle_planes[g.name]


def assert_f16_matches_reference(p16, g):
    """The device's fp16 planes against the reference's own outputs (as test_bev_golden_and_oracle)."""
    for s, name in enumerate(('present', 'future', 'full')):
        for k, key in ((0, 'road'), (5, 'dynamic'), (6, 'elevation')):
            assert np.array_equal(p16[7 * s + k].view(np.uint16), g[f'bev_{key}_{name}'].view(np.uint16)), (g.name, key, name)
        assert np.array_equal(p16[7 * s + 2:7 * s + 5].view(np.uint16), g[f'bev_rgb_{name}'].view(np.uint16)), (g.name, name)
        d = np.abs(p16[7 * s + 1].view(np.uint16).astype(int) - g[f'bev_intensity_{name}'].view(np.uint16).astype(int))
        assert d.max() <= 1, (g.name, name)


def assert_f64_matches_reference(p64, g):
    """The pre-cast f64 planes: the 1e-5 contract."""
    for s, name in enumerate(('present', 'future', 'full')):
        for k, key in ((0, 'road'), (1, 'intensity'), (5, 'dynamic'), (6, 'elevation')):
            np.testing.assert_allclose(p64[7 * s + k], g[f'pre_{key}_{name}'], rtol=0, atol=1e-5)
        np.testing.assert_allclose(p64[7 * s + 2:7 * s + 5], g[f'pre_rgb_{name}'], rtol=0, atol=1e-5)


def assert_f16_matches_oracle(p16, ref, name):
    """The fp16 half of assert_planes_match, for the routes that return no f64 planes."""
    F = ref['f16']
    for s in range(3):
        for k in range(7):
            a, b = p16[7 * s + k].view(np.uint16), F[7 * s + k].view(np.uint16)
            if k == 1:
                d = np.abs(a.astype(int) - b.astype(int))
                assert d.max() <= 1 and (d != 0).mean() < 1e-3, (name, s)
            else:
                assert np.array_equal(a, b), (name, s, k)


def check(p16, p64, g, orc):
    assert_planes_match(p16, p64, oracle_planes(orc, g), g.name)
    assert_f16_matches_reference(p16, g)
    assert_f64_matches_reference(p64, g)


@pytest.mark.parametrize('route', ['default', 'memory_path'])
@pytest.mark.parametrize('case', EDGE_CASES)
def test_bev_edges_single_call(T, orc, monkeypatch, case, route):
    """bev() as shipped, and with level 1 as ONE workgroup (PCA_BEV_G=1): what a chunk holds beyond 12 288 points -- the
    counts case does -- takes the memory path of pass B."""
    g = EdgeCase(case)
    if route == 'memory_path':
        monkeypatch.setenv('PCA_BEV_G', '1')
    p16, p64, used_i64 = run_dev_bev(T, g['pc_present'], g['pc_future'], g.zoom * g.view, g.px, g.hf, g.ints, g.div255, g.rot,
                                     g.dx, g.dy)
    assert not used_i64                              # fixture intensities are representable
    check(p16, p64, g, orc)


@pytest.mark.parametrize('case', EDGE_CASES)
def test_bev_edges_f64_intensity_route(T, orc, case):
    """The f64 intensity side channel (24-byte records, no register path) fed with the very values the store holds."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    g = EdgeCase(case)
    rows_p, rows_f = g['pc_present'], g['pc_future']
    st = dev_store(capacity=max(rows_p.shape[0] + rows_f.shape[0], 1), max_frames=4, intensity_div255=g.div255)
    assert st.load_rows([rows_p, rows_f]) is None
    inten = np.concatenate([rows_p[:, 3], rows_f[:, 3], [0.]])          # (one spare value: never an empty tensor)
    i64 = T.from_numpy(np.ascontiguousarray(inten)).cuda()
    prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(g.rot), g.dx, g.dy, g.zoom * g.view, g.px, g.hf, *g.ints, 0,
                          DYNOBJ, g.div255)
    p16, p64 = st.bev(1, prm, want_f64=True, intensity64=i64)
    st.check_status()
    check(p16.cpu().numpy(), p64.cpu().numpy(), g, orc)


def partner_of(case):
    """Another case with the same grid size and intensity encoding (bev_many: one px per launch, one encoding per store)."""
    name, k = case.split('/')
    if name.startswith('lattice_'):
        cfg, r = name[len('lattice_'):].rsplit('_r', 1)
        return f'lattice_{cfg}_r{(int(r) + 1) % 5}/{k}'
    return {'counts': 'lattice_nusc_r3/k1', 'intensity_kitti': 'lattice_kitti_r3/k1', 'intensity_nusc': 'counts/k0',
            'empty_sets': 'lattice_nusc_r4/k0'}[name]


@pytest.mark.parametrize('case', EDGE_CASES)
def test_bev_edges_as_one_job_of_bev_many(T, orc, case):
    """Two cases in one store (four frames), rastered as two jobs of one bev_many launch, each with its own parameters."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    pair = [EdgeCase(case), EdgeCase(partner_of(case))]
    assert pair[0].px == pair[1].px and pair[0].div255 == pair[1].div255 and pair[0].name != pair[1].name
    frames = [g[k] for g in pair for k in ('pc_present', 'pc_future')]
    st = dev_store(capacity=max(sum(f.shape[0] for f in frames), 1), max_frames=8, intensity_div255=pair[0].div255)
    assert st.load_rows(frames) is None
    jobs = []
    for k, g in enumerate(pair):
        prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(g.rot), g.dx, g.dy, g.zoom * g.view, g.px, g.hf, *g.ints, 0,
                              DYNOBJ, g.div255)
        jobs.append((2 * k + 1, prm, 2 * k, 2 * k + 2))
    out = T.empty((2, 21, pair[0].px, pair[0].px), dtype=T.float16, device='cuda')
    st.bev_many(jobs, out)
    st.check_status()
    out = out.cpu().numpy()
    for k, g in enumerate(pair):
        assert_f16_matches_oracle(out[k], oracle_planes(orc, g), g.name)
        assert_f16_matches_reference(out[k], g)


@pytest.mark.parametrize('write_back', [False, True])
@pytest.mark.parametrize('case', [c for c in EDGE_CASES if c.startswith('lattice_') and '_r0/' in c])
def test_bev_edges_reached_through_an_owed_transform(T, orc, case, write_back):
    """R = identity: the raster itself moves the points onto the lattice -- one owed re-transform, a pure translation by
    dyadic amounts, applied to what level 1 reads (and, with write_back, stored).  A translation is exact only for a
    point that x - d + d gives back bit for bit: those points make up the frame that owes it; the others (next to zero,
    or where x - d reaches the next binade) and the future set are stored where they are, in frames that count as
    appended after the transform was recorded."""
    from pca_amd.device_store import make_bev_params
    g = EdgeCase(case)
    assert g.rot == 0.
    d = np.array([0.5, -0.25, 0.125])
    rows_p, rows_f = g['pc_present'], g['pc_future']
    back = rows_p[:, :3] - d
    exact = ((back + d).view(np.uint64) == rows_p[:, :3].view(np.uint64)).all(1)       # (bit for bit: -0.0 stays -0.0)
    assert exact.mean() > 0.8                        # (most of the set, boundary points included, goes through the transform)
    moved = rows_p[exact].copy()
    moved[:, :3] = back[exact]
    st = dev_store(capacity=rows_p.shape[0] + rows_f.shape[0], max_frames=4, intensity_div255=g.div255)
    st.CHAIN_K = 1 if write_back else 4
    assert st.load_rows([moved, rows_p[~exact], rows_f]) is None
    Tm = np.eye(4)
    Tm[:3, 3] = d
    st.retransform(Tm, defer=True)
    owed, _ = st._pending[-1]
    st._pending[-1] = (owed, st.head + 1)            # frames 1 and 2 came after it
    prm = make_bev_params((0., 0., 0.), np.eye(3), g.dx, g.dy, g.zoom * g.view, g.px, g.hf, *g.ints, 0, DYNOBJ, g.div255)
    p16, p64 = st.bev(2, prm, want_f64=True)
    st.check_status()
    assert len(st._pending) == (0 if write_back else 1)
    check(p16.cpu().numpy(), p64.cpu().numpy(), g, orc)
    want = np.concatenate([rows_p[exact], rows_p[~exact], rows_f])
    assert np.array_equal(st.rows()[:, :3].view(np.uint64), want[:, :3].view(np.uint64))
