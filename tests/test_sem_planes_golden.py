"""The class-group fixture (tests/golden/sem_planes.npz, made by running the reference: tools/make_golden.py) against plain
numpy and against the C oracle used per group -- no GPU.  The oracle's `dynamic` plane with a group as its dynobj_classes
is the reference's gen_sem_probmap of that group, so the GPU tests may use it for inputs the reference never saw."""
import numpy as np
import pytest

from oracle import oracle as orc

SETS = ('present', 'future', 'full')


def rot_z(ang):
    c, s = np.cos(ang), np.sin(ang)
    return np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]])


def fixture_groups(g):
    return [[int(c) for c in row if c >= 0] for row in g['groups']]


def closed_form(n, n_g):
    """(n_g + 1) / ((n_g + 1) + ((n - n_g) + 1)): dirichlet expectation of {in the group, not in it}, uniform prior."""
    n, n_g = np.asarray(n, dtype=np.float64), np.asarray(n_g, dtype=np.float64)
    return (n_g + 1.) / ((n_g + 1.) + ((n - n_g) + 1.))


def test_fixture_planes_are_the_closed_form_of_its_counts(golden):
    g = golden('sem_planes')
    groups = fixture_groups(g)
    assert len(groups) == 5 and groups[0] == [1] and groups[3] and set(groups[4]) == {0, 255}
    for name in SETS:
        n = g[f'count_{name}']
        assert n.dtype == np.float64 and n.sum() > 0
        for k in range(len(groups)):
            n_g = g[f'count_{name}_g{k}']
            assert (n_g <= n).all()
            p = closed_form(n, n_g)
            assert np.array_equal(p, g[f'prob_{name}'][k]), (name, k)
            assert np.array_equal(p.astype(np.float16).view(np.uint16), g[f'prob16_{name}'][k].view(np.uint16)), (name, k)
        if name == 'full':
            assert np.array_equal(n, g['count_present'] + g['count_future'])
    assert g['count_full_g3'].sum() == 0                       # the group no point belongs to: the prior everywhere it is empty
    assert ((g['count_full_g2'] > 0) & (g['count_full_g4'] > 0)).any()   # the overlapping groups share cells (class 0)


def test_fixture_holds_the_edge_rows(golden):
    g = golden('sem_planes')
    view, px, hf, rot, dx, dy, zoom = g['cfg']
    rows = np.concatenate([g['pc_present'], g['pc_future']])
    assert (rows[:, 9] == 1).sum() > 50 and (rows[:, 2] >= hf).sum() > 100
    grid = np.concatenate([g['grid_present'], g['grid_future']])
    assert (grid[:, 0] == px).any()                            # one ulp inside +view/2 floors to px: counted in the last cell
    assert set(np.unique(rows[:, 7]).astype(int)) >= {0, 1, 13, 14, 15, 17, 255}


@pytest.mark.parametrize('k', range(5))
def test_oracle_dynamic_plane_with_a_group_is_the_reference(golden, k):
    g = golden('sem_planes')
    view, px, hf, rot, dx, dy, zoom = g['cfg']
    group = fixture_groups(g)[k]
    st = orc.Store.from_rows(np.concatenate([g['pc_present'], g['pc_future']]))
    prm = orc.make_bev_params((0., 0., 0.), rot_z(rot), dx, dy, zoom * view, int(px), hf, 20., 20., 0.5, 0, group, False)
    out = orc.bev(st, g['pc_present'].shape[0], prm)
    for s, name in enumerate(SETS):
        assert np.array_equal(out['planes'][7 * s + 5], g[f'prob_{name}'][k]), name
        assert np.array_equal(out['f16'][7 * s + 5].view(np.uint16), g[f'prob16_{name}'][k].view(np.uint16)), name
