"""The models and scenes of tests/nusc_front_edges_common.py on the CPU: the numpy models and the C oracle against what the
reference itself gave on every scene (tests/golden/nusc_front_edges.npz), bit for bit; the conditions the scenes must meet,
checked on the reference's own outputs; and every wrong reading of a rule told apart from the right one by at least one scene.
The conditions are conditions, not measurements: if a seed misses one, the seed changes, not the floor."""
import numpy as np
import pytest

import nusc_front_edges_common as ec
from oracle import oracle as orc


@pytest.fixture(scope='module')
def fx(golden):
    return golden('nusc_front_edges')


def sel_of(fx, name):
    return ec.sel_from(fx, name)


def k0n_fixture(fx, name):
    p = 'k0n_%s_' % name
    return fx[p + 'pc_in_ego'], fx[p + 'uv'], fx[p + 'cam_idx'].astype(np.int64)


def oracle_k0n(pc, r):
    return orc.nusc_project_cams(pc, r['ego_from_lidar'], r['glob_from_ego'], r['cam_from_glob'].reshape(-1, 16) if len(r['wh']) else np.zeros((0, 16)),
                                 r['K'].reshape(-1, 9), r['wh'])


def assert_k0n_equal(got, want):
    # pc_in_ego of a special (0 x inf, inf - inf) is a NaN whose sign the order of the operands decides: NaN == NaN there
    assert ec.same_bits_or_nan(got[0], want[0]), np.flatnonzero(np.any(got[0] != want[0], axis=1))[:8]
    assert ec.same_bits(got[0][np.isfinite(want[0])], want[0][np.isfinite(want[0])])
    assert ec.same_bits(got[1], want[1]), np.flatnonzero(np.any(got[1] != want[1], axis=1))[:8]
    assert np.array_equal(got[2], want[2]), np.flatnonzero(got[2] != want[2])[:8]


# ---- K0n ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ec.RIGS)
def test_k0n_model_and_oracle_equal_the_reference(fx, name):
    sc = ec.k0n_scene(name, sel_of(fx, name))
    want = k0n_fixture(fx, name)
    assert len(sc['pc']) == len(want[2])
    assert_k0n_equal(ec.k0n_model_rig(sc['pc'], sc['rig']), want)
    assert_k0n_equal(oracle_k0n(sc['pc'], sc['rig']), want)
    sp = sc['sections']['specials']
    assert np.all(want[2][sp][np.any(~np.isfinite(sc['pc'][sp]), axis=1)] == -1)      # no NaN / inf point is assigned


@pytest.mark.parametrize('name', ec.RIGS)
def test_k0n_scene_conditions_on_the_reference_outputs(fx, name):
    sc = ec.k0n_scene(name, sel_of(fx, name))
    r, sec = sc['rig'], sc['sections']
    ego, uv, cam = k0n_fixture(fx, name)
    n, ncam = len(cam), len(r['wh'])
    masks = np.unpackbits(fx['k0n_%s_masks' % name], axis=1)[:, :n].astype(bool)
    assert np.array_equal(np.where(masks.any(0), ncam - 1 - np.argmax(masks[::-1], axis=0), -1), cam)       # the last camera that takes a point
    for j in range(ncam):
        for bound in ec.BOUNDS:
            s = sec['fam_%d_%s' % (j, bound)]
            assert s.stop - s.start == 2 * ec.N_SIDE
            assert masks[j, s][:ec.N_SIDE].all() and not masks[j, s][ec.N_SIDE:].any(), (j, bound)          # >= 200 on either side
    assert sec['fam_0_u_lo'].start == 0                      # families from point 0 on: lanes 0, 63, 64, 255 hold family points
    assert masks[ncam - 1, n - 1] and cam[n - 1] == ncam - 1                                              # the last point: kept side of an edge
    assert np.isfinite(fx['k0n_%s_fam_ulps' % name]).all() and fx['k0n_%s_fam_ulps' % name].max() < 1e6
    for cams in ec.overlap_sets(r):
        s = sec['ovl_' + '_'.join(map(str, cams))]
        assert s.stop - s.start >= 200 and all(masks[j, s].all() for j in cams)
        assert np.all(cam[s] == cams[-1])                  # the later camera wins
    assert len(ec.overlap_sets(r)) == {'nusc': 6, 'mixed': 3, 'axis': 0}[name]
    for j in range(ncam):
        assert not masks[j, sec['behind_%d' % j]].any()
    if name == 'axis':
        pts, kept = ec.axis_exact_points()
        assert np.array_equal(cam[sec['exact']] >= 0, kept) and kept.sum() >= 30 and (~kept).sum() >= 30    # every exact hit is refused
        u = uv[sec['exact']][kept]
        assert set(u[:-1, 0]) <= {2.0, 254.0, 128.0} and set(u[:-1, 1]) <= {2.0, 126.0, 64.0}
    if name == 'mixed':
        assert len({tuple(w) for w in r['wh']}) == 3 and r['wh'][1][0] < r['wh'][1][1]                     # three sizes, one portrait
        assert masks[0, masks[1]].mean() > 0.99              # camera 0 contains camera 1


K0N_VARIANTS = ('ge_u_lo', 'ge_u_hi', 'ge_v_lo', 'ge_v_hi', 'ge_cz', 'first_wins', 'wh0', 'w_not_w1')


@pytest.mark.parametrize('variant', K0N_VARIANTS)
def test_k0n_scenes_tell_a_wrong_rule_from_the_right_one(fx, variant):
    differs = []
    for name in ec.RIGS:
        sc = ec.k0n_scene(name, sel_of(fx, name))
        _, uv, cam = ec.k0n_model_rig(sc['pc'], sc['rig'], variant)
        _, uv0, cam0 = k0n_fixture(fx, name)
        if not (np.array_equal(cam, cam0) and ec.same_bits(uv, uv0)):
            differs.append(name)
    assert differs, variant
    if variant.startswith('ge_'):
        assert 'axis' in differs                             # only an exact hit separates >= from >


@pytest.mark.parametrize('ncam', [0, 1, 8])
def test_k0n_model_equals_oracle_at_the_camera_counts_the_device_suite_runs(fx, ncam):
    sc = ec.k0n_scene('nusc', sel_of(fx, 'nusc'))
    r = ec.sub_rig(ec.rig('eight'), ncam)
    got = ec.k0n_model_rig(sc['pc'], r)
    assert_k0n_equal(oracle_k0n(sc['pc'], r), got)
    assert set(np.unique(got[2])) == set(range(-1, ncam))


def test_k0n_second_trip_scene_model_equals_oracle(fx):
    sc = ec.k0n_second_trip_scene(sel_of(fx, 'mixed'))
    got = ec.k0n_model_rig(sc['pc'], sc['rig'])
    assert_k0n_equal(oracle_k0n(sc['pc'], sc['rig']), got)
    assert len(sc['pc']) == ec.K0N_TRIP + 1 and got[2][-1] == 2 and got[2][0] == 0


# ---- K1n ----------------------------------------------------------------------------------------
def oracle_k1n(pc, cam, name, T, filters, mode=0):
    imgs, sems = ec.stack(name)
    st = orc.Store(max(len(pc), 1))
    orc.set_sample_mode(mode)
    try:
        orc.nusc_sample_filter_transform(st, pc, cam, imgs, sems, T, filters)
    finally:
        orc.set_sample_mode(0)
    return st.rows()


def same_rows(a, b):
    sa, sb = ec.soa(a), ec.soa(b)
    return a.shape == b.shape and all(ec.same_bits(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize('name', list(ec.K1N_STACKS))
def test_k1n_model_and_oracle_equal_the_reference(fx, name):
    sc = ec.k1n_scene(name)
    p = 'k1n_%s_' % name
    assert ec.same_bits(sc['pc'], fx[p + 'pc']) and np.array_equal(sc['cam'], fx[p + 'cam_idx']) and sc['filters'] == fx[p + 'filters'].tolist()
    imgs, sems = ec.stack(name)
    rows, asserts = ec.k1n_model(sc['pc'], sc['cam'], imgs, sems, sc['T'], sc['filters'])
    assert not asserts and ec.same_bits(rows, fx[p + 'rows'])
    assert same_rows(oracle_k1n(sc['pc'], sc['cam'], name, sc['T'], sc['filters']), fx[p + 'rows'])
    assert {c >> 6 for c in sc['filters']} == {0, 1, 2, 3}


@pytest.mark.parametrize('name', list(ec.K1N_STACKS))
def test_k1n_scene_conditions_on_the_reference_outputs(fx, name):
    """Every edge point is stored, with the colour and class of the pixel it is there for: column 1 / W - 1, row 1 / H - 1 of
    every camera, the even neighbour of a tie, the first legal and the last pixel; a filtered class occurs where the stack
    has room for one; cam_idx outside [0, ncam) stores nothing."""
    sc = ec.k1n_scene(name)
    ncam, H, W = ec.K1N_STACKS[name]
    imgs, sems = ec.stack(name)
    rows, kept = fx['k1n_%s_rows' % name], fx['k1n_%s_kept' % name].tolist()
    um, vm = sc['pc'][0, 4], sc['pc'][0, 5]
    seen = set()
    for i in sc['stored']:
        assert i in kept, (i, sc['tags'][i])
        c, tag, (u, v) = int(sc['cam'][i]), sc['tags'][i], sc['pc'][i, 4:6]
        x, y = {'edge_u_lo': (1, round(vm)), 'edge_u_hi': (W - 1, round(vm)), 'edge_v_lo': (round(um), 1), 'edge_v_hi': (round(um), H - 1),
                'first_pixel': (1, 1), 'last_pixel': (W - 1, H - 1)}.get(tag, (None, None))
        if tag == 'tie':
            x, y = (int(2 * round(u / 2)), round(vm)) if u != um else (round(um), int(2 * round(v / 2)))
        assert rows[kept.index(i), 4:8].tolist() == imgs[c, y, x].tolist() + [int(sems[c, y, x])], (i, tag)
        seen.add((tag, c))
    assert {(t, c) for t in ('edge_u_lo', 'edge_u_hi', 'edge_v_lo', 'edge_v_hi', 'last_pixel') for c in range(ncam)} <= seen
    ties = sc['pc'][[i for i, t in enumerate(sc['tags']) if t == 'tie'], 4:6]
    ks = np.floor(ties[ties != np.round(ties)])              # (the tied coordinate of each)
    assert name == 's3' or ({0, 1} == set((ks % 2).tolist()) and 1 in ks and W - 2 in ks and H - 2 in ks)
    for i, t in enumerate(sc['tags']):
        if t.startswith('cam_'):
            assert (i in kept) == (0 <= sc['cam'][i] < ncam)
        if t == 'filtered':
            assert i not in kept
    words = {int(sems[sc['cam'][i], round(sc['pc'][i, 5]), round(sc['pc'][i, 4])]) >> 6 for i, t in enumerate(sc['tags']) if t == 'filtered'}
    assert {'s3': words == set(), 's8': len(words) >= 1, 'nusc': words == {0, 1, 2, 3}}[name]      # nusc: a dropped point per word of the mask
    assert {-ec.BIG, -1, 0, ncam - 1, ncam, 7, ec.BIG} <= set(sc['cam'].tolist())


def test_position_encoding_tells_neighbouring_pixels_and_cameras_apart():
    for name in ec.K1N_STACKS:
        imgs, sems = ec.stack(name)
        full = np.concatenate([imgs, sems[..., None]], axis=-1).astype(np.int64)
        assert np.all(np.any(full[:, :, 1:] != full[:, :, :-1], axis=-1)) and np.all(np.any(full[:, 1:] != full[:, :-1], axis=-1))
        assert np.all(np.any(full[:, 1:, 1:] != full[:, :-1, :-1], axis=-1)) and np.all(np.any(full[:, 1:, :-1] != full[:, :-1, 1:], axis=-1))
        assert all(np.all(imgs[a, ..., 2] != imgs[b, ..., 2]) for a in range(len(imgs)) for b in range(a))


@pytest.mark.parametrize('variant', ['half_up', 'trunc', 'swap_uv', 'bilinear_class', 'keep_ge_ncam'])
def test_k1n_scenes_tell_a_wrong_rule_from_the_right_one(fx, variant):
    differs = []
    for name in ec.K1N_STACKS:
        sc = ec.k1n_scene(name)
        imgs, sems = ec.stack(name)
        rows, asserts = ec.k1n_model(sc['pc'], sc['cam'], imgs, sems, sc['T'], sc['filters'], variant)
        if asserts or not ec.same_bits(rows, fx['k1n_%s_rows' % name]):
            differs.append(name)
    assert differs, variant


@pytest.mark.parametrize('name', list(ec.K1N_STACKS))
@pytest.mark.parametrize('kind', ec.OFFENDERS)
def test_k1n_offending_frames_and_their_twins(name, kind):
    """The reference asserts on the offending frame (the model says so, the oracle raises); the twin -- the same point with
    cam_idx -1 or ncam -- passes and stores the rows of the other points, which are also what the model gives for the offender."""
    sc = ec.k1n_scene(name)
    imgs, sems = ec.stack(name)
    pc, cam = ec.k1n_offender(name, kind)
    rows, asserts = ec.k1n_model(pc, cam, imgs, sems, sc['T'], sc['filters'])
    assert asserts
    with pytest.raises(AssertionError):
        oracle_k1n(pc, cam, name, sc['T'], sc['filters'])
    pct, camt = ec.k1n_offender(name, kind, twin=True)
    rows_t, asserts_t = ec.k1n_model(pct, camt, imgs, sems, sc['T'], sc['filters'])
    assert not asserts_t and ec.same_bits(rows_t, rows) and same_rows(oracle_k1n(pct, camt, name, sc['T'], sc['filters']), rows)
    full, _ = ec.k1n_model(sc['pc'], sc['cam'], imgs, sems, sc['T'], sc['filters'])
    assert len(rows) == len(full) - 1                        # the scene stores its victim; the offender and the twin do not


# ---- sampler and normaliser ----------------------------------------------------------------------
def test_strict_bilinear_model_and_oracle_equal_the_reference(fx):
    fmap, uv = ec.bilinear_scene()
    assert ec.same_bits(fmap, fx['bil_map']) and ec.same_bits(uv, fx['bil_uv'])
    want = fx['bil_out']
    nan = np.isnan(want)
    integer = np.any(uv == np.floor(uv), axis=1)
    assert np.array_equal(nan, integer) and nan.sum() >= 9   # the reference divides 0 by 0 exactly there
    for got in (ec.bilinear_model(fmap, uv), orc.sample_bilinear(fmap, uv)):
        assert np.array_equal(np.isnan(got), nan) and ec.same_bits(got[~nan], want[~nan])
    H, W = ec.BIL_HW
    for b, col in ((1.0, 0), (W - 1.0, 0), (1.0, 1), (H - 1.0, 1)):
        assert np.any(uv[:, col] == np.nextafter(b, 5.0))   # one step inside every bound


def test_nchw_model_is_totensor_and_normalize_in_f32():
    """Every byte value in every channel against the same expression with each operation rounded from f64 by hand."""
    img = ec.nchw_image(16, 16)
    assert all(set(img[..., c].ravel().tolist()) == set(range(256)) for c in range(3))
    for mean, std in ((ec.MEAN, ec.STD), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))):
        got = ec.nchw_model(img, mean, std)
        assert got.dtype == np.float32 and got.shape == (3, 16, 16)
        for c in range(3):
            x = (img[..., c].astype(np.float64) / 255.0).astype(np.float32)
            d = (x.astype(np.float64) - np.float64(np.float32(mean[c]))).astype(np.float32)
            assert ec.same_bits(got[c], (d.astype(np.float64) / np.float64(np.float32(std[c]))).astype(np.float32))
