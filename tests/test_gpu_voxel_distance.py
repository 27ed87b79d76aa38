"""GPU: the exact distance transform of voxel volumes (pca_voxel_distance, DeviceStore.voxel_distance,
SemBEVGenerator.voxel_distance_device, SemanticPointCloudAccumulator.voxel_distance / voxel_ssc_sample_filled) against the
brute-force numpy model of tests/voxel_distance_common.py (pinned by tests/test_voxel_distance_model.py, which also shows that
the scenes hold the ties and the far voxels they are meant to hold).  Every comparison is exact, tsdf as uint32 views; every
input is a valid call or a refused one.

Shapes: the issue's, plus (200, 8) and one call at (1024, 32).  The line kernel takes a row of the volume and a round of its k
values per workgroup, a round being min(ceil(nz / 4), 6144 // px) values: 33 / 7 has rounds of 2, 2, 2 and 1, 136 / 32 four of 8,
and only 1024 / 32 meets the cap (rounds of 6, the last one of 2).  The row kernel's tile is min(64, 6144 // px) columns wide: 72 =
64 + 8 is a whole tile and a narrow one, 136 has tiles of 45 (the last one 1 wide), 200 tiles of 30, 1024 tiles of 6 with a last
one of 4.  Each scene runs by default and with PCA_VOXEL_DIST_G=1, one workgroup for all the rows and tiles."""
import ctypes as C
import re

import numpy as np
import pytest

import voxel_distance_common as vd
import voxel_ssc_common as sc_
from test_gpu_kernels import SEM_IDXS, T, dev_store  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, kitti_accumulator

pytestmark = pytest.mark.gpu

OUTPUTS = {'d': ('dist2', 'int32'), 'n': ('nearest', 'int32'), 'l': ('nearest_label', 'uint8'), 'f': ('filled', 'uint8'),
           't': ('tsdf', 'float32')}


def raw(T, labels, seen=None, sites=None, weights=(1, 1), max_dist2=None, fill_dist2=None, fill_free=False, tsdf=None,
        outputs='dnlft', **bad):
    """pca_voxel_distance itself.  outputs: which of dist2 / nearest / nearest_label / filled / tsdf are wanted ('f' and 't'
    are dropped where fill_dist2 / tsdf is None, unless bad['keep'] says otherwise); bad: px, nz, ws_bytes replaced,
    null_labels for a null pointer.  All five outputs start out filled with 7.  Returns (rc, message, {name: array})."""
    from pca_amd import _lib
    ctx = _lib.Context.get()
    nz, px, _ = labels.shape
    if not bad.get('keep'):
        outputs = ''.join(c for c in outputs if not ((c == 'f' and fill_dist2 is None) or (c == 't' and tsdf is None)))
    dev_labels = T.from_numpy(np.array(labels)).cuda()              # (a copy: the scenes are read-only)
    dev_seen = None if seen is None else T.from_numpy(np.array(seen)).cuda()
    need = int(ctx.lib.pca_voxel_distance_workspace_bytes(px, nz))
    ws = T.full((need, ), 7, dtype=T.uint8, device='cuda')
    outs = {name: T.full(labels.shape, 7, dtype=getattr(T, dt), device='cuda') for name, dt in OUTPUTS.values()}
    group = None
    if sites is not None:
        group = _lib.PcaClassGroup()
        group.mask[:] = list(_lib.class_mask(sites))
    unit, trunc, flip = (0., 0., False) if tsdf is None else tsdf
    r = ctx.lib.pca_voxel_distance(ctx.h, bad.get('px', px), bad.get('nz', nz), None if bad.get('null_labels') else dev_labels.data_ptr(),
                                   None if dev_seen is None else dev_seen.data_ptr(), None if group is None else C.byref(group),
                                   int(weights[0]), int(weights[1]), -1 if max_dist2 is None else int(max_dist2),
                                   -1 if fill_dist2 is None else int(fill_dist2), 1 if fill_free else 0, float(unit), float(trunc),
                                   1 if flip else 0, ws.data_ptr(), bad.get('ws_bytes', need),
                                   *(outs[OUTPUTS[c][0]].data_ptr() if c in outputs else None for c in 'dnlft'), ctx.stream())
    T.cuda.synchronize()
    return r, ctx.lib.pca_last_error(ctx.h).decode(), {k: t.cpu().numpy() for k, t in outs.items()}, outputs


def same(got, want):
    """Every output that was asked for equals the model's; the others still hold their 7s."""
    r, err, outs, outputs = got
    assert r == 0, err
    for c, (name, dt) in OUTPUTS.items():
        if c in outputs:
            a, b = outs[name], want[name]
            assert a.dtype == b.dtype == np.dtype(dt)
            if c == 't':
                a, b = a.view(np.uint32), b.view(np.uint32)
            assert np.array_equal(a, b), (name, int((a != b).sum()), np.argwhere(a != b)[:4].tolist())
        else:
            assert (outs[name] == 7).all(), name


# ---------------------------------------------------------------------------------------------- 1: the scenes
@pytest.mark.parametrize('px,nz', vd.SHAPES)
def test_random_scenes_equal_the_model(T, monkeypatch, px, nz):
    """Two densities, every label a site and a subset, seen given: all five outputs, by default and with ONE workgroup."""
    for density in vd.densities(px, nz):
        labels, seen, subset = vd.random_scene(px, nz, density)
        for sites in (None, subset):
            base = vd.scene_base(px, nz, density, sites)
            how = dict(sites=sites, fill_dist2=3, tsdf=(0.5, 2.5, True))
            want = vd.model(labels, seen, base=base, **how)
            monkeypatch.delenv('PCA_VOXEL_DIST_G', raising=False)
            same(raw(T, labels, seen, **how), want)
            monkeypatch.setenv('PCA_VOXEL_DIST_G', '1')
            same(raw(T, labels, seen, **how), want)


@pytest.mark.parametrize('px,nz', vd.SHAPES)
def test_plain_contents(T, monkeypatch, px, nz):
    """No site at all (bytes >= 32 and 255 only); a single site in a corner; every voxel a site."""
    rng = np.random.default_rng(px * 100 + nz)
    seen = (rng.random((nz, px, px)) < 0.5).astype(np.uint8)
    none = np.where(rng.random((nz, px, px)) < 0.1, 77, 255).astype(np.uint8)
    one = np.full((nz, px, px), 255, dtype=np.uint8)
    one[nz - 1, px - 1, 0] = 6
    full = rng.integers(0, 32, size=(nz, px, px), dtype=np.uint8)
    for g in (None, '1'):
        monkeypatch.delenv('PCA_VOXEL_DIST_G', raising=False) if g is None else monkeypatch.setenv('PCA_VOXEL_DIST_G', g)
        for flip in (False, True):
            got = raw(T, none, seen, fill_dist2=100, tsdf=(1., 3., flip))
            same(got, vd.model(none, seen, fill_dist2=100, tsdf=(1., 3., flip)))
            out = got[2]
            assert (out['dist2'] == -1).all() and (out['nearest'] == -1).all() and (out['nearest_label'] == 255).all()
            assert (out['filled'] == 255).all()                     # (an own byte >= 32 is empty and is not copied)
            assert np.array_equal(np.abs(out['tsdf']), np.full(none.shape, 0. if flip else 1., np.float32))
            assert np.array_equal(np.signbit(out['tsdf']), seen == 0)
        same(raw(T, one, seen, fill_dist2=5, tsdf=(1., 3., True)), vd.model(one, seen, fill_dist2=5, tsdf=(1., 3., True)))
        # (every voxel its own site: the brute-force model would cost voxels^2 pairs, and the contract says what comes out)
        same(raw(T, full, seen, fill_dist2=5, tsdf=(1., 3., False)),
             {'dist2': np.zeros(full.shape, np.int32), 'nearest': np.arange(full.size, dtype=np.int32).reshape(full.shape),
              'nearest_label': full, 'filled': full, 'tsdf': np.zeros(full.shape, np.float32)})


def test_longest_line_and_the_bound(T, monkeypatch):
    """px = 1024, nz = 1, 32 sites with the four corners: the longest line and the largest D; then weights (1000, 1), where
    1000 * 2 * 1023^2 = 2 093 058 000 is just inside 2^31 - 2 and a 32-bit intermediate that wraps would show."""
    labels, seen = vd.long_line_scene()
    for weights in ((1, 1), (1000, 1)):
        base = vd.transform(labels, None, weights)
        how = dict(weights=weights, fill_dist2=50 * 50 * weights[0], tsdf=(0.01, 8., True))
        monkeypatch.delenv('PCA_VOXEL_DIST_G', raising=False)
        same(raw(T, labels, seen, **how), vd.model(labels, seen, base=base, **how))
        for m in (0, 3 * weights[0], 300 * 300 * weights[0]):
            same(raw(T, labels, seen, max_dist2=m, **how), vd.model(labels, seen, base=base, max_dist2=m, **how))
    monkeypatch.setenv('PCA_VOXEL_DIST_G', '3')
    same(raw(T, labels, seen, **how), vd.model(labels, seen, base=base, **how))


def test_largest_volume_single_site(T):
    """1024 x 1024 x 32 with one site, unbounded: the longest walk there is, every voxel's, the k rounds cut by the LDS cap, and
    still two launches.  One site needs no search: D is its distance, everywhere."""
    from pca_amd import _lib
    labels = np.full((32, 1024, 1024), 255, dtype=np.uint8)
    labels[30, 1000, 17] = 8
    ctx = _lib.Context.get()
    ctx.profile(1)
    got = raw(T, labels, None, weights=(625, 256), outputs='d')
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['voxel_dist_lines'][1] == 1 and prof['voxel_dist_rows'][1] == 1
    k, r, c = (np.arange(n, dtype=np.int32) for n in (32, 1024, 1024))
    want = 256 * ((k - 30) ** 2)[:, None, None] + 625 * (((r - 1000) ** 2)[None, :, None] + ((c - 17) ** 2)[None, None, :])
    same(got, {'dist2': want.astype(np.int32)})


def test_anisotropic_weights(T):
    """weights (625, 256) at (72, 16): metres in units of 0.0125 m on the default grid's voxels; the bounds times the weight."""
    px, nz = 72, 16
    for density in vd.densities(px, nz):
        labels, seen, subset = vd.random_scene(px, nz, density)
        base = vd.scene_base(px, nz, density, None, (625, 256))
        for m in (None, ) + tuple(625 * v for v in vd.MAX_DIST2) + (256, 4 * 256):
            how = dict(weights=(625, 256), max_dist2=m, fill_dist2=2 * 625, tsdf=(0.0125, 1., True))
            same(raw(T, labels, seen, **how), vd.model(labels, seen, base=base, **how))


@pytest.mark.parametrize('px,nz', [(5, 3), (33, 7), (72, 16)])
def test_max_dist2(T, monkeypatch, px, nz):
    """Sites beyond max_dist2 do not exist: 0 leaves the sites only."""
    for density in vd.densities(px, nz):
        labels, seen, subset = vd.random_scene(px, nz, density)
        base = vd.scene_base(px, nz, density, subset)
        for g in (None, '1'):
            monkeypatch.delenv('PCA_VOXEL_DIST_G', raising=False) if g is None else monkeypatch.setenv('PCA_VOXEL_DIST_G', g)
            for m in vd.MAX_DIST2:
                how = dict(sites=subset, max_dist2=m, fill_dist2=9, tsdf=(1., 2., False))
                got = raw(T, labels, seen, **how)
                same(got, vd.model(labels, seen, base=base, **how))
                if m == 0:
                    assert np.array_equal(got[2]['dist2'] == 0, vd.site_mask(labels, subset)) and (got[2]['dist2'] <= 0).all()


# ---------------------------------------------------------------------------------------------- 2: fill and tsdf
def fill_scene():
    labels = np.full((2, 6, 6), 255, dtype=np.uint8)
    seen = np.zeros_like(labels)
    labels[0, 2, 2] = 4                      # a site
    labels[0, 2, 3], seen[0, 2, 3] = 255, 1  # free, beside the site
    labels[0, 2, 1] = 200                    # a byte >= 32 beside the site: empty, unseen, eligible
    labels[0, 3, 2], seen[0, 3, 2] = 200, 1  # the same byte where a beam passed
    labels[1, 5, 5] = 9                      # occupied, outside the site subset (4, )
    return labels, seen


def test_fill(T):
    labels, seen = fill_scene()
    for sites in (None, (4, )):
        for how in (dict(fill_dist2=1), dict(fill_dist2=1, fill_free=True), dict(fill_dist2=2), dict(fill_dist2=0),
                    dict(fill_dist2=2, max_dist2=1), dict(fill_dist2=2 ** 40, fill_free=True)):
            same(raw(T, labels, seen, sites=sites, **how), vd.model(labels, seen, sites, **how))
            same(raw(T, labels, None, sites=sites, **how), vd.model(labels, None, sites, **how))
    f = raw(T, labels, seen, sites=(4, ), fill_dist2=1)[2]['filled']
    assert f[0, 2, 2] == 4 and f[1, 5, 5] == 9                       # own labels, a site or not
    assert f[0, 2, 3] == 255                                         # a free voxel next to a site stays free by default
    assert f[0, 2, 1] == 4 and f[0, 3, 2] == 255                     # the byte 200 is empty: filled where unseen, else 255, never 200
    assert f[1, 2, 2] == 4 and f[0, 1, 1] == 255                     # within 1 across k; the diagonal is at 2
    f = raw(T, labels, seen, sites=(4, ), fill_dist2=1, fill_free=True)[2]['filled']
    assert f[0, 2, 3] == 4 and f[0, 3, 2] == 4
    f = raw(T, labels, None, sites=(4, ), fill_dist2=1)[2]['filled']
    assert f[0, 2, 3] == 4 and f[0, 3, 2] == 4                       # without `seen` every empty voxel is eligible
    f = raw(T, labels, seen, sites=(4, ), fill_dist2=0)[2]['filled']
    assert np.array_equal(f, np.where(labels < 32, labels, 255))


def test_tsdf(T):
    """Plain and flipped, with and without seen, trunc smaller and larger than the largest distance, odd units."""
    px, nz = 33, 7
    density = vd.densities(px, nz)[0]
    labels, seen, subset = vd.random_scene(px, nz, density)
    base = vd.scene_base(px, nz, density, subset)
    far = float(np.sqrt(base[0].max()))
    assert far >= 4                          # (the slab)
    for flip in (False, True):
        for sn in (seen, None):
            for unit, trunc in ((1., 2.), (1., 3. * far), (0.0125, 0.3), (1. / 3, far / 7), (0.7, 1e-3), (1e-3, 1e6)):
                how = dict(sites=subset, tsdf=(unit, trunc, flip))
                got = raw(T, labels, sn, **how)
                same(got, vd.model(labels, sn, base=base, **how))
    t = raw(T, labels, seen, sites=subset, tsdf=(1., 2., True))[2]['tsdf']
    site = vd.site_mask(labels, subset)
    assert (t[site] == 1).all() and (np.signbit(t) == ((labels >= 32) & (seen == 0))).all() and (np.abs(t) <= 1).all()
    assert (t[base[0] >= 4] == 0).all() and ((t != 0) & (np.abs(t) != 1)).any()


# ---------------------------------------------------------------------------------------------- 3: the C ABI's rules
@pytest.mark.parametrize('outputs', ['d', 'n', 'l', 'f', 't', 'dn', 'lf', 'nt'])
def test_absent_outputs(T, outputs):
    """Every output alone and some together: the rest is left as it was."""
    px, nz = 33, 7
    density = vd.densities(px, nz)[1]
    labels, seen, _ = vd.random_scene(px, nz, density)
    how = dict(fill_dist2=2, tsdf=(1., 2., True))
    got = raw(T, labels, seen, outputs=outputs, **how)
    assert got[3] == outputs
    same(got, vd.model(labels, seen, base=vd.scene_base(px, nz, density), **how))


def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    from pca_amd import _lib
    ctx = _lib.Context.get()
    ctx.profile(1)
    px, nz = 16, 4
    density = vd.densities(px, nz)[1]
    labels, seen, _ = vd.random_scene(px, nz, density)
    ok = dict(fill_dist2=2, tsdf=(1., 2., True))
    need = int(ctx.lib.pca_voxel_distance_workspace_bytes(px, nz))
    big = np.full((1, 1024, 1024), 255, dtype=np.uint8)
    cases = [(labels, dict(ok, px=0), r'voxel distance: px must be in 1\.\.1024'),
             (labels, dict(ok, px=1025), r'voxel distance: px must be in 1\.\.1024'),
             (labels, dict(ok, nz=0), r'voxel distance: nz must be in 1\.\.32'),
             (labels, dict(ok, nz=33), r'voxel distance: nz must be in 1\.\.32'),
             (labels, dict(ok, weights=(0, 1)), 'voxel distance: w_xy and w_z must be >= 1'),
             (labels, dict(ok, weights=(1, 0)), 'voxel distance: w_xy and w_z must be >= 1'),
             (labels, dict(ok, weights=(1, -3)), 'voxel distance: w_xy and w_z must be >= 1'),
             # 1026 * 2 * 1023^2 = 2 147 477 508 is inside; one more w_xy is 2 093 058 above 2^31 - 2
             (big, dict(ok, weights=(1027, 1)), r'voxel distance: w_xy 2 \(px-1\)\^2 \+ w_z \(nz-1\)\^2 must not exceed 2\^31 - 2'),
             (labels, dict(ok, weights=(1, (2 ** 31 - 2 - 2 * 15 * 15) // 9 + 1)), r'voxel distance: w_xy 2 \(px-1\)\^2'),
             (labels, dict(ok, null_labels=True), 'voxel distance: labels must not be NULL'),
             (labels, dict(ok, outputs=''), 'voxel distance: at least one output is needed'),
             (labels, dict(ok, tsdf=(1., 0., True)), 'voxel distance: tsdf needs tsdf_unit and tsdf_trunc finite and > 0'),
             (labels, dict(ok, tsdf=(1., float('nan'), True)), 'voxel distance: tsdf needs tsdf_unit and tsdf_trunc finite and > 0'),
             (labels, dict(ok, tsdf=(float('inf'), 1., True)), 'voxel distance: tsdf needs tsdf_unit and tsdf_trunc finite and > 0'),
             (labels, dict(ok, tsdf=(-1., 1., True)), 'voxel distance: tsdf needs tsdf_unit and tsdf_trunc finite and > 0'),
             (labels, dict(ok, fill_dist2=None, keep=True), 'voxel distance: filled needs fill_dist2 >= 0'),
             (labels, dict(ok, ws_bytes=need - 1), 'voxel distance: workspace too small')]
    for vol, bad, msg in cases:
        r, err, outs, _ = raw(T, vol, None if vol is big else seen, **bad)
        assert r == -1 and re.match(msg, err), (err, msg)
        assert all((a == 7).all() for a in outs.values()), msg
    prof = ctx.profile_read()
    assert prof['voxel_dist_lines'][1] == 0 and prof['voxel_dist_rows'][1] == 0
    # the weights one below the bound are served, and the call is two launches whatever the volume holds
    want = vd.model(labels, seen, base=vd.scene_base(px, nz, density), **ok)
    same(raw(T, labels, seen, **ok), want)
    w_z = (2 ** 31 - 2 - 2 * 15 * 15) // 9
    same(raw(T, labels, seen, weights=(1, w_z)), vd.model(labels, seen, weights=(1, w_z)))
    same(raw(T, big, None, weights=(1026, 1), outputs='d'), {'dist2': np.full(big.shape, -1, np.int32)})
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['voxel_dist_lines'][1] == 3 and prof['voxel_dist_rows'][1] == 3 and prof['voxel_pool'][1] == 0


def test_two_calls_give_identical_bytes(T):
    px, nz = 72, 16
    labels, seen, subset = vd.random_scene(px, nz, vd.densities(px, nz)[1])
    how = dict(sites=subset, weights=(3, 7), fill_dist2=12, tsdf=(0.3, 2., True))
    a, b = raw(T, labels, seen, **how), raw(T, labels, seen, **how)
    assert a[0] == b[0] == 0 and all(a[2][k].tobytes() == b[2][k].tobytes() for k in a[2])


# ---------------------------------------------------------------------------------------------- 4: the upper layers
def test_through_the_store(T):
    px, nz = 33, 7
    density = vd.densities(px, nz)[1]
    labels, seen, subset = vd.random_scene(px, nz, density)
    st = dev_store(capacity=1024, max_frames=2)
    out = st.voxel_distance(np.array(labels), np.array(seen), site_labels=subset, max_dist2=9, fill_dist2=2, tsdf=(0.5, 2., True))
    want = vd.model(labels, seen, max_dist2=9, fill_dist2=2, tsdf=(0.5, 2., True), base=vd.scene_base(px, nz, density, subset))
    assert sorted(out) == sorted(want) and all(out[k].is_cuda and tuple(out[k].shape) == labels.shape for k in out)
    assert all(np.array_equal(out[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)) for k in want)
    # only what was asked for; cuda inputs; a smaller volume reuses the workspace
    ws = st._dist_ws
    out = st.voxel_distance(T.from_numpy(labels[:3, :16, :16].copy()).cuda())
    assert sorted(out) == ['dist2', 'nearest', 'nearest_label'] and st._dist_ws is ws
    assert np.array_equal(out['dist2'].cpu().numpy(), vd.model(labels[:3, :16, :16])['dist2'])
    with pytest.raises(ValueError, match='seen'):
        st.voxel_distance(labels, seen[:3])
    with pytest.raises(RuntimeError, match='voxel distance: w_xy and w_z'):
        st.voxel_distance(labels, weights=(0, 1))
    st.check_status()


def test_generator_metrics(T):
    """metric='metres' on the default grid: weights (625, 256), unit 0.0125; distances become floor((d / unit)^2)."""
    from bev_generator.sem_bev import SemBEVGenerator
    gen = SemBEVGenerator(SEM_IDXS, **{k: v for k, v in dict(BEV_KITTI, view_size=80, pixel_size=256).items() if k != 'type'})
    labels = np.full((32, 256, 256), 255, dtype=np.uint8)
    labels[3, 100, 100], labels[3, 100, 104], labels[9, 7, 200] = 2, 5, 31
    seen = np.zeros_like(labels)
    out = gen.voxel_distance_device(labels, seen, 80., (-2.0, 4.4), 32, max_dist=1.0, fill_dist=0.7, tsdf_trunc=1.0)
    assert out['weights'] == (625, 256) and out['unit'] == 0.0125
    # 1 m is 80 units, 6400; 0.7 m is 56 units less a rounding, floor((0.7 / 0.0125)^2) = 3135: three bins up (9 * 256) and two
    # cells away (4 * 625) are inside, so is (2, 1) cells away (5 * 625 = 3125); four bins up and (2, 2) cells away are not
    bound = lambda d: int(np.floor((d / 0.0125) ** 2))      # noqa: E731
    assert bound(1.0) == 6400 and 3125 <= bound(0.7) <= 3136
    want = vd.model(labels, seen, None, (625, 256), bound(1.0), bound(0.7), False, (0.0125, 1.0, True))
    assert all(np.array_equal(out[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)) for k in want)
    f = out['filled'].cpu().numpy()
    assert f[6, 100, 100] == 2 and f[7, 100, 100] == 255 and f[3, 100, 102] == 2 and f[3, 100, 103] == 5
    assert f[3, 98, 99] == 2 and f[3, 98, 98] == 255
    # 'voxel': unit weights, distances in voxels; flip=False
    small = np.ascontiguousarray(labels[:4, 96:112, 96:112])
    out = gen.voxel_distance_device(small, None, 5., (0., 1.), 4, sites=[5], metric='voxel', max_dist=2.5, tsdf_trunc=2., flip=False)
    assert out['weights'] == (1, 1) and out['unit'] == 1. and 'filled' not in out
    want = vd.model(small, None, (5, ), (1, 1), 6, None, False, (1., 2., False))
    assert all(np.array_equal(out[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)) for k in want)
    with pytest.raises(ValueError, match='metric'):
        gen.voxel_distance_device(small, None, 5., (0., 1.), 4, metric='feet')


def test_accumulator_on_a_kitti_sequence(T, tmp_path):
    acc, idx = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14), 9
    z_range, nz, classes = (-2.0, 4.4), 8, [[0, 1, 2], [13, 14, 15, 17], [5], [8, 9]]
    px = acc.sem_bev_generator.pixel_size
    occ = acc.voxel_occupancy(idx, z_range=z_range, nz=nz, classes=classes)
    before = [t.clone() for t in acc.store._arrays()]
    # cells of 30 / 32 m, bins of 0.8 m: 75 / 64
    from pca_amd.host_logic import voxel_metric
    w_xy, w_z, unit = voxel_metric(30. / 32, 0.8, px=px, nz=nz)
    assert (w_xy, w_z) == (5625, 4096) and unit == 0.0125
    b = lambda d: int(np.floor((d / unit) ** 2))      # noqa: E731
    opts = dict(z_range=z_range, nz=nz, classes=classes, max_dist=4.0, fill_dist=1.5, tsdf_trunc=3.0)

    def check(out, source, sites, flip=True):
        assert sorted(out) == sorted(list(occ) + ['dist2', 'nearest', 'nearest_label', 'filled', 'tsdf', 'weights', 'unit']
                                     + (['input_occ'] if source is not None else []))
        assert all(T.equal(out[k], occ[k]) for k in occ)
        assert out['weights'] == (w_xy, w_z) and out['unit'] == unit
        labels = out['labels'].cpu().numpy() if source is None else source
        want = vd.model(labels, out['seen'].cpu().numpy(), sites, (w_xy, w_z), b(4.0), b(1.5), False, (unit, 3.0, flip))
        for k in want:
            assert np.array_equal(out[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)), k
        return want

    want = check(acc.voxel_distance(idx, **opts), None, None)
    labels = occ['labels'].cpu().numpy()
    assert ((want['filled'] != labels) & (want['filled'] < 32)).any()
    check(acc.voxel_distance(idx, site_classes=[1, 3], flip=False, **opts), None, (1, 3), flip=False)
    inp = acc.voxel_distance(idx, sites='input', **opts)
    scan = acc.voxel_ssc_sample(idx, z_range=z_range, nz=nz, classes=classes, occluded=False, scales=(1, ))['input_occ']
    assert T.equal(inp['input_occ'], scan) and 0 < int(scan.sum()) < int((occ['counts'] != 0).sum())
    check(inp, np.where(scan.cpu().numpy() != 0, 0, 255).astype(np.uint8), None)
    with pytest.raises(ValueError, match='sites'):
        acc.voxel_distance(idx, sites='scan', **opts)
    # the SSC sample with the pinholes closed: pooled and packed from `filled`
    plain = acc.voxel_ssc_sample(idx, z_range=z_range, nz=nz, classes=classes, occluded=False, scales=(1, 2))
    out = acc.voxel_ssc_sample_filled(idx, 1.5, z_range=z_range, nz=nz, classes=classes, occluded=False, scales=(1, 2))
    assert sorted(out) == sorted(list(plain) + ['filled', 'dist2', 'nearest']) and T.equal(out['labels'], plain['labels'])
    seen = occ['seen'].cpu().numpy()
    want = vd.model(labels, seen, None, (w_xy, w_z), b(1.5), b(1.5))
    assert all(np.array_equal(out[k].cpu().numpy(), want[k]) for k in ('filled', 'dist2', 'nearest'))
    filled = want['filled']
    assert np.array_equal(out['levels'][1]['labels'].cpu().numpy(), filled)
    pooled = sc_.pool_model(filled, seen, None, 2)
    assert all(np.array_equal(out['levels'][2][k].cpu().numpy(), pooled[k]) for k in pooled)
    packed = sc_.pack_model(filled, seen, None, plain['input_occ'].cpu().numpy())
    assert all(np.array_equal(out['packed'][1][k].cpu().numpy(), packed[k]) for k in packed)
    packed2 = sc_.pack_model(pooled['labels'], pooled['state'])
    assert all(np.array_equal(out['packed'][2][k].cpu().numpy(), packed2[k]) for k in packed2)
    # a filled voxel's bit is clear in .invalid, and it was set before
    newly = sc_.places((filled < 32) & (labels >= 32))
    assert newly.any()
    assert not (np.unpackbits(out['packed'][1]['invalid'].cpu().numpy())[:newly.size][newly]).any()
    assert (np.unpackbits(plain['packed'][1]['invalid'].cpu().numpy())[:newly.size][newly]).all()
    same_sample = acc.voxel_ssc_sample_filled(idx, None, z_range=z_range, nz=nz, classes=classes, occluded=False, scales=(1, 2))
    assert sorted(same_sample) == sorted(plain) and T.equal(same_sample['packed'][1]['invalid'], plain['packed'][1]['invalid'])
    assert all(T.equal(a.view(T.uint8), b_.view(T.uint8)) for a, b_ in zip(before, acc.store._arrays()))
    acc.store.check_status()
