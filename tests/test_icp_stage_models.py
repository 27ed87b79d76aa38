"""The CPU models of tests/icp_stage_common.py against plain formulations of the same operations, and the conditions the
device tests (tests/test_gpu_icp_stages.py) rely on for their scenes.  No GPU needed.

Measured here (sparse / dense scene with the planted clusters): valid normals with a small eigen-gap 73 of 9 322 (0.8 %: the
collinear returns of the far rings) / 0 of 10 706 targets of the sweeps; brute-forced neighbourhoods (the 30 nearest reach past the
64 of the k-d tree or out of the box) 3.9 % / 0.1 %; the normal summed in reversed order and in longdouble moves by at most
1.3e-8 / 4.7e-9 of the angle bound (a quarter is asked)."""
import ctypes as C

import numpy as np
import pytest

import icp_stage_common as m


@pytest.fixture(scope='module', params=['sparse', 'dense'])
def scene(request):
    tgt = m.normals_scene(request.param)
    return request.param, tgt, m.normals_model(tgt)


def test_cells_at_the_faces_and_borders():
    f32 = np.float32
    up = lambda v: np.nextafter(f32(v), f32(0))              # noqa: E731
    pts = np.array([(-128, -128, -16), (128, 0, 0), (up(128), up(128), up(16)), (0, 0, 16), (0, 0, -16), (-64, -64, -8), (64, 0, 0),
                    (up(64), up(64), up(8)), (0, 0, 8), (np.nan, 0, 0), (np.inf, 0, 0), (0, -np.inf, 0), (0.0, -0.0, 0.25), (up(0.25), up(-0.25), 0)],
                   dtype=np.float32)
    in0, c0, i0 = m.cells(pts, 0)
    in1, c1, i1 = m.cells(pts, 1)
    assert in0.tolist() == [True, False, True, False, True, True, True, True, True, False, False, False, True, True]
    assert in1.tolist() == [False, False, False, False, False, True, False, True, False, False, False, False, True, True]
    assert i0[0] == 0 and c0[2].tolist() == [511, 511, 63] and i0[2] == m.NX * m.NY * m.NZ - 1
    assert i1[5] == 0 and c1[7].tolist() == [511, 511, 63]
    assert c1[12].tolist() == [256, 256, 33] and c1[13].tolist() == [256, 255, 32] and c0[13].tolist() == [256, 255, 32]
    assert i0[9] == -1 and i1[10] == -1


def test_box_model_is_plain_30nn_inside_3m(scene):
    """Wherever the 30th distance is below 3 m (and the 30th and 31st differ by more than rounding) the box model's set is the
    30 nearest neighbours of a k-d tree; the tree-assisted path equals the brute-force box on a sample."""
    from scipy.spatial import cKDTree
    name, tgt, mod = scene
    xyz = tgt[:, :3].astype(np.float64)
    d, nb = cKDTree(xyz).query(xyz, k=31)
    clear = (d[:, 29] < 3.0) & (d[:, 30] > d[:, 29] * (1 + 1e-6))
    assert clear.mean() > 0.85                                # (the rest: the sparse far rings and the lattice's ties)
    for i in np.flatnonzero(clear):
        assert np.array_equal(np.sort(nb[i, :30]), np.sort(mod['sets'][i])), i
    sample = np.random.default_rng(0).choice(len(tgt), 400, replace=False)
    inside, c, _ = m.cells(tgt[:, :3], 0)
    for i in sample:                                         # (the brute-force box, written out once more)
        cand = np.flatnonzero(inside & np.all(np.abs(c - c[i]) <= m.NORMAL_RINGS, axis=1))
        d2 = m.f32_dist2(tgt[cand, :3], tgt[i, :3])
        kk = np.sort(d2)[m.K - 1] if len(cand) >= m.K else d2.max()
        assert kk == mod['kth'][i] and np.array_equal(np.sort(cand[d2 <= kk]), np.sort(mod['sets'][i])), i


def test_conditions_of_the_normal_scenes(scene):
    name, tgt, mod = scene
    n_plants = len(m.normal_plants())
    is_sweep = np.ones(len(tgt), bool)
    perm = np.random.default_rng(5).permutation(len(tgt))     # (normals_scene's own shuffle)
    where = np.empty(len(tgt), np.int64)
    where[perm] = np.arange(len(tgt))                         # row of the unshuffled cloud -> row of the scene
    plants = where[len(tgt) - n_plants:]
    is_sweep[plants] = False
    assert tgt[is_sweep, 2].max() < 2.5 and tgt[~is_sweep, 2].min() >= 5.5
    assert mod['valid'][is_sweep].mean() > 0.99               # (a few far returns have fewer than three points in their box)
    gap = m.small_gap(mod['lam'])
    print(name, 'small gaps: sweep', int(gap[is_sweep].sum()), 'of', int(is_sweep.sum()), 'all valid', int((gap & mod['valid']).sum()),
          'brute', float(mod['brute'].mean()))
    assert gap[is_sweep].mean() <= 0.02 and (gap & mod['valid']).mean() <= 0.02
    assert (mod['brute'][is_sweep].mean() > 0.03) if name == 'sparse' else (mod['brute'][is_sweep].mean() < 0.002)
    # the planted clusters: (rows of normal_plants from the back) lone, one, two, ten, the lattice patches before them
    size = np.array([len(s) for s in mod['sets']])
    lone, one, two, ten = plants[-1], plants[-2], plants[-4:-2], plants[-14:-4]
    assert size[lone] == 1 and size[one] == 1 and size[two].tolist() == [2, 2] and (size[ten] == 10).all()
    assert not mod['valid'][[lone, one, *two]].any() and mod['valid'][ten].all() and not gap[ten].any()
    lattice = plants[:-14]
    assert len(lattice) > 500 and mod['valid'][lattice].all()
    assert (size[lattice] > m.K).mean() > 0.3                 # the 30th distance is shared: every tied point counts
    assert gap[lattice].mean() < 0.1
    in_fine_box = (np.abs(tgt[lattice, 2]) < 7.0) & (np.abs(tgt[lattice, 0]) < 63)
    assert 0.2 < in_fine_box.mean() < 0.8                     # both the fine and the coarse path of the search
    for i in lattice[:200]:
        s = mod['sets'][i]
        if size[i] > m.K:                                    # the tied points are not coplanar with the query
            d2 = m.f32_dist2(tgt[s, :3], tgt[i, :3])
            tied = s[d2 == mod['kth'][i]]
            assert len(tied) >= 2
    # the bound: the model summed in reversed order and in longdouble stays four times inside it
    bound = m.angle_bound(mod['kth'], mod['lam'])
    check = np.flatnonzero(mod['valid'] & ~gap)
    check = check[np.random.default_rng(1).choice(len(check), 1500, replace=False)]
    worst = 0.0
    for i in check:
        s = mod['sets'][i]
        D = tgt[s, :3] - tgt[i, :3]
        for kw in (dict(order=np.arange(len(s))[::-1]), dict(dtype=np.longdouble)):
            nrm, _ = m.normal_of(D, **kw)
            worst = max(worst, float(m.sine_between(nrm, mod['normal'][i]) / bound[i]))
    print(name, 'reversed / longdouble: worst share of the bound', worst)
    assert worst <= 0.25


def test_partner_model_is_the_kdtree_where_the_nearest_is_unique():
    from scipy.spatial import cKDTree
    from test_gpu_icp import pose_T
    src, tgt, info = m.partner_scene()
    T = np.linalg.inv(pose_T(0.9, 0.03, 0.008))
    q = m.transform(T, src)
    mod = m.partners_model(q, tgt)
    # the conditions: nothing but the planted rows falls outside the grid; the far sources straddle both caps; ties exist
    outside = np.flatnonzero(~mod['in_grid'])
    assert outside.tolist() == info['high'].tolist() + [info['nan_row'], info['inf_row']]
    d = np.sqrt(mod['d2'][mod['in_grid']])
    assert ((d > 2.2) & (d < 3.9)).sum() > 30 and ((d >= 3.9) & (d < 4.0)).sum() >= 1 and (d >= 4.0).sum() > 10
    assert (mod['ties'][mod['in_grid']] == 2).sum() >= 20 and (mod['ties'] >= m.DUP_COPIES).sum() >= m.DUP_GROUPS - 1
    cand = np.flatnonzero(m.cells(tgt[:, :3], 0)[0])
    fin = np.flatnonzero(np.all(np.isfinite(q), axis=1))
    dd, j = cKDTree(tgt[cand, :3].astype(np.float64)).query(q[fin], k=2)
    unique = dd[:, 1] > dd[:, 0] * (1 + 1e-9) + 1e-12
    assert unique.mean() > 0.95
    assert np.array_equal(cand[j[unique, 0]], mod['nearest'][fin][unique])
    assert np.allclose(np.sqrt(mod['d2'][fin]), dd[:, 0], rtol=1e-12, atol=0)
    # among equals the lowest index
    tied = fin[~unique]
    for i in tied:
        same = np.flatnonzero(m.f64_dist2(tgt[:, :3], q[i]) == mod['d2'][i])
        assert mod['nearest'][i] == same.min()


def test_accumulator_and_step_models():
    """The sums against a row-by-row loop; solve + exp_step on them reproduce a known small motion of a synthetic system."""
    rng = np.random.default_rng(2)
    tgt = m.rows(rng.uniform(-5, 5, (50, 3)))
    nrm = rng.normal(size=(50, 4)).astype(np.float32)
    nrm[:, 3] = rng.integers(0, 2, 50)
    q = rng.uniform(-5, 5, (40, 3))
    partner = rng.integers(-1, 50, 40)
    sums, mag = m.accumulators_model(q, tgt, partner, nrm)
    ref = np.zeros(30)
    for i in range(40):
        if partner[i] < 0:
            continue
        t, n = tgt[partner[i], :3].astype(np.float64), nrm[partner[i], :3].astype(np.float64)
        ref[27] += ((q[i] - t) ** 2).sum()
        ref[28] += 1
        if nrm[partner[i], 3] == 0:
            continue
        J, r = np.concatenate([np.cross(q[i], n), n]), (q[i] - t) @ n
        ref[:21] += [J[a] * J[b] for a, b in m.PAIRS]
        ref[21:27] += J * r
        ref[29] += r * r
    assert np.allclose(sums, ref, rtol=1e-12, atol=1e-12) and np.all(mag >= np.abs(sums) * (1 - 1e-12))
    A, b = m.system_of(sums)
    assert np.array_equal(A, A.T) and A[0, 1] == sums[1] and A[1, 1] == sums[6] and A[5, 5] == sums[20]
    U = m.exp_step(np.array([0.0, 0.0, np.pi / 2, 1.0, 2.0, 3.0]))
    assert np.allclose(U, [[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], atol=1e-15)


def test_layout_accessor_reports_the_workspace_map():
    """pca_debug_icp_layout (host only): ascending, 256-aligned regions of the sizes the kernels index, total + the room to
    align the base = pca_icp_workspace_bytes."""
    from pca_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 16)()
    assert lib.pca_debug_icp_layout(0, 5, out) == -1 and lib.pca_debug_icp_layout(5, 5, None) == -1
    for n_src, n_tgt in ((1, 1), (255, 257), (9001, 120000), (120000, 9001)):
        assert lib.pca_debug_icp_layout(n_src, n_tgt, out) == 0
        v = list(out)
        off, total = v[:11], v[11]
        assert off[0] == 0 and all(a < b for a, b in zip(off, off[1:])) and off[-1] < total and all(o % 256 == 0 for o in off + [total])
        cells_ = v[15]
        assert cells_ == m.NX * m.NY * m.NZ and v[14] == 30 and v[12] * 8 + 16 <= 128 * 8 and v[13] + v[14] <= 128
        assert off[1] - off[0] >= (cells_ + 1) * 4 and off[2] - off[1] >= n_tgt * 16 and off[4] - off[3] >= n_tgt * 16
        assert off[5] - off[4] >= n_tgt * 16 and off[6] - off[5] >= n_src * 4 and total - off[10] >= (v[13] + v[14]) * 8
        mx = max(n_src, n_tgt)
        assert lib.pca_debug_icp_layout(mx, mx, out) == 0 and out[11] + 512 == lib.pca_icp_workspace_bytes(mx)
