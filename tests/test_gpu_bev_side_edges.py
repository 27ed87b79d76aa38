"""GPU: the edge fixtures (tests/golden/bev_edges_*.npz, see test_gpu_bev_edges.py) through the two side passes that share
the main raster's view test, cell function and owed chain (csrc/pca_bev_view.h): the class planes against the main raster's
road / dynamic planes and the reference's own, the elevation partition against the main raster's elevation plane -- as
shipped, with level 1 as ONE workgroup (chunks beyond the register path), and reached through an owed transform."""
import numpy as np
import pytest

from bev_edges_common import EDGE_CASES, EdgeCase
from test_gpu_kernels import DYNOBJ, T, dev_store  # noqa: F401  (T: fixture)

pytestmark = pytest.mark.gpu

SETS = ('present', 'future', 'full')
OWED_CASES = [c for c in EDGE_CASES if c.startswith('lattice_') and '_r0/' in c]


def bits(a):
    return a.view({2: np.uint16, 8: np.uint64}[a.dtype.itemsize])


def check_side_passes(st, split, prm, g):
    """Both side passes over the whole window of `st` against the main raster of the same store and the fixture."""
    _, m64 = st.bev(split, prm, want_f64=True)
    st.check_status()
    m64 = m64.cpu().numpy()
    # ---- the class planes: [road], DYNOBJ = the main raster's planes 0 and 5
    c16, c64, cnt = st.bev_class_planes(split, prm, [[0], DYNOBJ], want_counts=True)
    st.check_status()
    c16, c64, cnt = c16.cpu().numpy(), c64.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)
    for s, name in enumerate(SETS):
        for k, (plane, key) in enumerate(((0, 'road'), (5, 'dynamic'))):
            assert np.array_equal(bits(c64[s, k]), bits(m64[7 * s + plane])), (g.name, key, name)
            assert np.array_equal(bits(c16[s, k]), bits(g[f'bev_{key}_{name}'])), (g.name, key, name)
            np.testing.assert_allclose(c64[s, k], g[f'pre_{key}_{name}'], rtol=0, atol=1e-5)
    # ---- the elevation partition of the static points: the main raster's elevation plane of the `full` set
    out = st.bev_elev_partition(prm, 0.5, include_dyn=False)
    st.check_status()
    elev, observed, flags, counts = (out[k].cpu().numpy() for k in ('elev', 'observed', 'flags', 'counts'))
    assert np.array_equal(bits(elev), bits(m64[7 * 2 + 6])), g.name
    assert np.array_equal(observed, cnt[2, 2] > 0), g.name
    assert counts[0] == flags.size - (flags == 255).sum(), g.name


def loaded_store(g):
    """The case's two sets as two frames, as test_bev_edges_f64_intensity_route loads them."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    rows_p, rows_f = g['pc_present'], g['pc_future']
    st = dev_store(capacity=max(rows_p.shape[0] + rows_f.shape[0], 1), max_frames=4, intensity_div255=g.div255)
    assert st.load_rows([rows_p, rows_f]) is None
    prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(g.rot), g.dx, g.dy, g.zoom * g.view, g.px, g.hf, *g.ints, 0,
                          DYNOBJ, g.div255)
    return st, prm


def owing_store(g):
    """As test_bev_edges_reached_through_an_owed_transform builds it: frame 0 owes a translation that puts it onto the
    lattice, and goes on owing it (CHAIN_K = 4: nothing is written back)."""
    from pca_amd.device_store import make_bev_params
    assert g.rot == 0.
    d = np.array([0.5, -0.25, 0.125])
    rows_p, rows_f = g['pc_present'], g['pc_future']
    back = rows_p[:, :3] - d
    exact = ((back + d).view(np.uint64) == rows_p[:, :3].view(np.uint64)).all(1)
    assert exact.mean() > 0.8
    moved = rows_p[exact].copy()
    moved[:, :3] = back[exact]
    st = dev_store(capacity=rows_p.shape[0] + rows_f.shape[0], max_frames=4, intensity_div255=g.div255)
    st.CHAIN_K = 4
    assert st.load_rows([moved, rows_p[~exact], rows_f]) is None
    Tm = np.eye(4)
    Tm[:3, 3] = d
    st.retransform(Tm, defer=True)
    owed, _ = st._pending[-1]
    st._pending[-1] = (owed, st.head + 1)            # frames 1 and 2 came after it
    prm = make_bev_params((0., 0., 0.), np.eye(3), g.dx, g.dy, g.zoom * g.view, g.px, g.hf, *g.ints, 0, DYNOBJ, g.div255)
    return st, prm


@pytest.mark.parametrize('route', ['default', 'one_workgroup'])
@pytest.mark.parametrize('case', EDGE_CASES)
def test_side_passes_on_the_edge_cases(T, monkeypatch, case, route):
    """As shipped, and with level 1 of both passes as ONE workgroup (PCA_BEV_CLASS_G = PCA_BEV_ELEV_G = 1): what the chunk
    holds beyond 12 288 points -- the counts case does -- is recomputed in pass B."""
    if route == 'one_workgroup':
        monkeypatch.setenv('PCA_BEV_CLASS_G', '1')
        monkeypatch.setenv('PCA_BEV_ELEV_G', '1')
    g = EdgeCase(case)
    st, prm = loaded_store(g)
    check_side_passes(st, 1, prm, g)


@pytest.mark.parametrize('route', ['default', 'one_workgroup'])
@pytest.mark.parametrize('case', OWED_CASES)
def test_side_passes_reached_through_an_owed_transform(T, monkeypatch, case, route):
    if route == 'one_workgroup':
        monkeypatch.setenv('PCA_BEV_CLASS_G', '1')
        monkeypatch.setenv('PCA_BEV_ELEV_G', '1')
    g = EdgeCase(case)
    st, prm = owing_store(g)
    check_side_passes(st, 2, prm, g)
    assert len(st._pending) == 1                     # (still owed: every pass applied it to what it read)
