"""GPU: voxel volumes pooled to coarser scales and packed into SemanticKITTI-SSC's file payloads (pca_voxel_pool, pca_voxel_pack,
DeviceStore.voxel_pool / voxel_pack, SemBEVGenerator.voxel_pyramid_device, SemanticPointCloudAccumulator.voxel_ssc_sample,
pca_amd.ssc) against the numpy model of tests/voxel_ssc_common.py (pinned by tests/test_voxel_ssc_model.py, which also shows
that the random scenes hold the thresholds and ties they are meant to hold).  Every comparison is exact; every input is a valid
call or a refused one.

The pool kernel's tile is 8 x 8 x 64 (k, row, col), so the shapes are the issue's: 8 / 8 one block and all three scales, 24 / 8
less than a tile wide, 72 / 16 one tile plus a partial one and two blocks in k, 136 / 32 two tiles and more along rows and cols;
6 / 2 and 10 / 2 (scale 2 alone) take the byte loads of a px that is no multiple of 4.  The pack kernel's tile is 64 columns x
(128 / nz) values of j."""
import re

import numpy as np
import pytest

import voxel_ssc_common as sc_
from test_gpu_kernels import T, dev_store  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, kitti_accumulator

pytestmark = pytest.mark.gpu

POOL_SHAPES = [(8, 8), (24, 8), (72, 16), (136, 32)]
PACK_SHAPES = [(3, 5), (5, 3), (16, 4), (33, 7), (64, 32)]

_scenes = {}


def scene_of(px, nz, planted=True):
    """(scene, {(s, fraction): the model's result}) of a shape, made once and never changed."""
    if (px, nz) not in _scenes:
        _scenes[px, nz] = (sc_.random_scene(px, nz, planted=planted), {})
    return _scenes[px, nz]


def want_of(px, nz, s, fraction=(1, 20)):
    sc, wants = scene_of(px, nz)
    if (s, fraction) not in wants:
        wants[s, fraction] = sc_.pool_model(sc['labels'], sc['seen'], sc['visible'], s, fraction)
    return wants[s, fraction]


def raw_pool(T, sc, levels, fraction=(1, 20), visible=True, **bad):
    """pca_voxel_pool itself.  levels: [(scale, 'lsv' -- which of labels / state / visible are wanted)]; bad: px, nz, occ_num,
    occ_den, n_levels replaced, labels / seen / descs = None for a null pointer.  The outputs start out filled with 7.
    Returns (rc, message, {scale: {name: array}})."""
    from pca_amd import _lib
    ctx = _lib.Context.get()
    nz, px, _ = sc['labels'].shape
    dev = {k: T.from_numpy(sc[k]).cuda() for k in ('labels', 'seen', 'visible')}
    descs = (_lib.PcaVoxelPoolLevel * max(len(levels), 1))()
    outs = []
    for d, (s, which) in zip(descs, levels):
        shape = (max(nz // s, 1), max(px // s, 1), max(px // s, 1)) if s > 0 else (1, 1, 1)
        o = {k: T.full(shape, 7, dtype=T.uint8, device='cuda') for k in ('labels', 'state', 'visible')}
        d.scale = s
        d.labels, d.state, d.visible = (o[k].data_ptr() if k[0] in which else None for k in ('labels', 'state', 'visible'))
        outs.append((s, o))
    ptr = {k: (None if k in bad else t.data_ptr()) for k, t in dev.items()}
    r = ctx.lib.pca_voxel_pool(ctx.h, bad.get('px', px), bad.get('nz', nz), ptr['labels'], ptr['seen'],
                               ptr['visible'] if visible else None, bad.get('occ_num', fraction[0]), bad.get('occ_den', fraction[1]),
                               None if 'descs' in bad else descs, bad.get('n_levels', len(levels)), ctx.stream())
    T.cuda.synchronize()
    return r, ctx.lib.pca_last_error(ctx.h).decode(), [(s, {k: t.cpu().numpy() for k, t in o.items()}) for s, o in outs]


def same_pool(got, px, nz, levels, fraction=(1, 20)):
    r, err, outs = got
    assert r == 0, err
    for (s, which), (s_got, o) in zip(levels, outs):
        want = want_of(px, nz, s, fraction)
        for k in ('labels', 'state', 'visible'):
            if k[0] in which:
                assert np.array_equal(o[k], want[k]), (s, k, int((o[k] != want[k]).sum()))
            else:
                assert (o[k] == 7).all(), (s, k)


# ---------------------------------------------------------------------------------------------- 1: the pool against the model
@pytest.mark.parametrize('px,nz', POOL_SHAPES)
def test_pool_equals_the_model(T, monkeypatch, px, nz):
    """All three scales in one call, by default and with ONE workgroup going round its loop for all the tiles."""
    sc, _ = scene_of(px, nz)
    levels = [(2, 'lsv'), (4, 'lsv'), (8, 'lsv')]
    same_pool(raw_pool(T, sc, levels), px, nz, levels)
    monkeypatch.setenv('PCA_VOXEL_POOL_G', '1')
    same_pool(raw_pool(T, sc, levels), px, nz, levels)


@pytest.mark.parametrize('px,nz', [(6, 2), (10, 2)])
def test_pool_a_px_that_is_no_multiple_of_4(T, monkeypatch, px, nz):
    sc = sc_.random_scene(px, nz, planted=False)
    want = sc_.pool_model(sc['labels'], sc['seen'], sc['visible'], 2)
    for g in (None, '1'):
        if g:
            monkeypatch.setenv('PCA_VOXEL_POOL_G', g)
        r, err, outs = raw_pool(T, sc, [(2, 'lsv')])
        assert r == 0, err
        assert all(np.array_equal(outs[0][1][k], want[k]) for k in want)


@pytest.mark.parametrize('levels', [[(8, 'lsv')], [(4, 'ls')], [(8, 's'), (2, 'l')], [(4, 'v'), (8, 'l'), (2, 'sv')], [(2, 'lsv'), (8, 'lv')]])
def test_pool_subsets_orders_and_absent_outputs(T, levels):
    sc, _ = scene_of(72, 16)
    same_pool(raw_pool(T, sc, levels), 72, 16, levels)


def test_pool_without_visible_and_other_fractions(T):
    sc, _ = scene_of(24, 8)
    levels = [(2, 'ls'), (4, 'ls'), (8, 'ls')]
    same_pool(raw_pool(T, sc, levels, visible=False), 24, 8, levels)
    for fraction in ((1, 8), (0, 1), (1, 1)):
        same_pool(raw_pool(T, sc, levels, fraction=fraction), 24, 8, levels, fraction)
    assert any((want_of(24, 8, s, (1, 8))['state'] != want_of(24, 8, s)['state']).any() for s in (4, 8))
    assert any((want_of(24, 8, s, (0, 1))['state'] != want_of(24, 8, s)['state']).any() for s in (4, 8))


def test_pool_through_the_store_is_one_launch(T):
    """DeviceStore.voxel_pool: numpy inputs and cuda tensors, the dict it returns, and ONE launch for the three scales."""
    from pca_amd import _lib
    sc, _ = scene_of(72, 16)
    st = dev_store(capacity=1024, max_frames=2)
    ctx = _lib.Context.get()
    ctx.profile(1)
    out = st.voxel_pool(sc['labels'], sc['seen'], sc['visible'])
    prof = ctx.profile_read()
    assert prof['voxel_pool'][1] == 1 and prof['voxel_pack'][1] == 0
    out2 = st.voxel_pool(T.from_numpy(sc['labels']).cuda(), T.from_numpy(sc['seen']).cuda(), scales=(4, ), occupied_fraction=(1, 8))
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['voxel_pool'][1] == 2
    assert sorted(out) == [2, 4, 8] and sorted(out2) == [4] and sorted(out2[4]) == ['labels', 'state']
    for s in (2, 4, 8):
        want = want_of(72, 16, s)
        assert sorted(out[s]) == ['labels', 'state', 'visible'] and out[s]['labels'].dtype == T.uint8
        assert tuple(out[s]['state'].shape) == (16 // s, 72 // s, 72 // s)
        assert all(np.array_equal(out[s][k].cpu().numpy(), want[k]) for k in want)
    assert np.array_equal(out2[4]['labels'].cpu().numpy(), want_of(72, 16, 4, (1, 8))['labels'])
    with pytest.raises(ValueError, match='seen'):
        st.voxel_pool(sc['labels'], sc['seen'][:8])
    with pytest.raises(RuntimeError, match='voxel pool: scale must be 2, 4 or 8'):
        st.voxel_pool(sc['labels'], sc['seen'], scales=(3, ))
    st.check_status()


# ---------------------------------------------------------------------------------------------- 2: the pack against the model
def raw_pack(T, sc, outputs='lioc', inputs='svi', label_map=sc_.LABEL_MAP, empty_value=sc_.EMPTY_VALUE, **bad):
    """pca_voxel_pack itself.  outputs: which of label / invalid / occluded / bin ('c' for the .bin) are wanted; inputs: which of
    seen / visible / input_occ are given; bad: px, nz replaced, labels = None.  The outputs start out filled with 7.
    Returns (rc, message, {name: array})."""
    from pca_amd import _lib
    ctx = _lib.Context.get()
    nz, px, _ = sc['labels'].shape
    n = px * px * nz
    dev = {k: T.from_numpy(sc[k]).cuda() for k in ('labels', 'seen', 'visible', 'input_occ')}
    out = {'label': T.full((n, ), 0x0707, dtype=T.uint16, device='cuda')}
    out.update({k: T.full(((n + 7) // 8, ), 7, dtype=T.uint8, device='cuda') for k in ('invalid', 'occluded', 'bin')})
    table = None if label_map is None else np.ascontiguousarray(label_map, dtype=np.uint16)
    r = ctx.lib.pca_voxel_pack(ctx.h, bad.get('px', px), bad.get('nz', nz), None if 'labels' in bad else dev['labels'].data_ptr(),
                               dev['seen'].data_ptr() if 's' in inputs else None, dev['visible'].data_ptr() if 'v' in inputs else None,
                               dev['input_occ'].data_ptr() if 'i' in inputs else None,
                               None if table is None else table.ctypes.data, empty_value,
                               out['label'].data_ptr() if 'l' in outputs else None, out['invalid'].data_ptr() if 'i' in outputs else None,
                               out['occluded'].data_ptr() if 'o' in outputs else None, out['bin'].data_ptr() if 'c' in outputs else None,
                               ctx.stream())
    T.cuda.synchronize()
    return r, ctx.lib.pca_last_error(ctx.h).decode(), {k: t.cpu().numpy() for k, t in out.items()}


def same_pack(got, want, outputs='lioc'):
    r, err, out = got
    assert r == 0, err
    for key, letter in (('label', 'l'), ('invalid', 'i'), ('occluded', 'o'), ('bin', 'c')):
        if letter in outputs:
            assert out[key].dtype == want[key].dtype and np.array_equal(out[key], want[key]), (key, int((out[key] != want[key]).sum()))
        else:
            assert (out[key] == (0x0707 if key == 'label' else 7)).all(), key


_packs = {}


def pack_want(px, nz):
    if (px, nz) not in _packs:
        sc = sc_.pack_scene(px, nz)
        _packs[px, nz] = (sc, sc_.pack_model(sc['labels'], sc['seen'], sc['visible'], sc['input_occ'], sc_.LABEL_MAP, sc_.EMPTY_VALUE))
    return _packs[px, nz]


@pytest.mark.parametrize('px,nz', PACK_SHAPES)
def test_pack_equals_the_model(T, monkeypatch, px, nz):
    """A label_map with values above 255 (the byte order shows), by default and with ONE workgroup for all the tiles."""
    sc, want = pack_want(px, nz)
    same_pack(raw_pack(T, sc), want)
    monkeypatch.setenv('PCA_VOXEL_PACK_G', '1')
    same_pack(raw_pack(T, sc), want)
    got = raw_pack(T, sc)[2]['label']
    assert got.view(np.uint8)[0::2].tolist() == (want['label'] & 255).tolist()       # little-endian


@pytest.mark.parametrize('outputs', ['l', 'i', 'o', 'c', 'lo', 'ic', 'ioc', 'lic'])
def test_pack_absent_outputs(T, outputs):
    """Every output alone and some together; the rest is left as it was.  Inputs nobody asked a stream of may be absent."""
    sc, want = pack_want(33, 7)
    same_pack(raw_pack(T, sc, outputs=outputs), want, outputs)
    needed = ''.join({'i': 's', 'o': 'v', 'c': 'i'}.get(c, '') for c in outputs)
    same_pack(raw_pack(T, sc, outputs=outputs, inputs=needed), want, outputs)


def test_pack_through_the_store(T):
    from pca_amd import _lib
    sc, want = pack_want(33, 7)
    st = dev_store(capacity=1024, max_frames=2)
    ctx = _lib.Context.get()
    ctx.profile(1)
    out = st.voxel_pack(sc['labels'], sc['seen'], sc['visible'], sc['input_occ'], label_map=sc_.LABEL_MAP, empty_value=sc_.EMPTY_VALUE)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['voxel_pack'][1] == 1 and prof['voxel_pool'][1] == 0
    assert sorted(out) == ['bin', 'invalid', 'label', 'occluded'] and out['label'].dtype == T.uint16 and out['bin'].dtype == T.uint8
    assert all(np.array_equal(out[k].cpu().numpy(), want[k]) for k in want)
    # the default map: label l -> l + 1, empty -> 0; only the streams whose input was given
    out = st.voxel_pack(T.from_numpy(sc['labels']).cuda(), visible=sc['visible'])
    assert sorted(out) == ['label', 'occluded']
    assert np.array_equal(out['label'].cpu().numpy(), sc_.pack_model(sc['labels'])['label'])
    assert np.array_equal(out['occluded'].cpu().numpy(), want['occluded'])
    with pytest.raises(ValueError, match='label_map'):
        st.voxel_pack(sc['labels'], label_map=np.arange(31))
    with pytest.raises(ValueError, match='visible'):
        st.voxel_pack(sc['labels'], visible=sc['visible'][:3])
    st.check_status()


# ---------------------------------------------------------------------------------------------- 3: the C ABI's checks
def test_refusals_launch_nothing_and_leave_the_outputs_alone(T):
    from pca_amd import _lib
    ctx = _lib.Context.get()
    ctx.profile(1)
    sc, _ = scene_of(24, 8)
    all3 = [(2, 'lsv'), (4, 'lsv'), (8, 'lsv')]
    pool = [(dict(px=0), all3, r'voxel pool: px must be in 1\.\.1024'), (dict(px=1025), all3, r'voxel pool: px must be in 1\.\.1024'),
            (dict(nz=0), all3, r'voxel pool: nz must be in 1\.\.32'), (dict(nz=33), all3, r'voxel pool: nz must be in 1\.\.32'),
            (dict(), [(3, 'lsv')], 'voxel pool: scale must be 2, 4 or 8'), (dict(), [(16, 'l')], 'voxel pool: scale must be 2, 4 or 8'),
            (dict(), [(0, 'l')], 'voxel pool: scale must be 2, 4 or 8'),
            (dict(), [(2, 'l'), (4, 's'), (2, 's')], 'voxel pool: a scale must not be requested twice'),
            (dict(px=20), [(2, 'l'), (8, 'l')], 'voxel pool: px and nz must be multiples of every requested scale'),
            (dict(nz=4), [(8, 'l')], 'voxel pool: px and nz must be multiples of every requested scale'),
            (dict(px=23), [(2, 'l')], 'voxel pool: px and nz must be multiples of every requested scale'),
            (dict(occ_den=0), all3, 'voxel pool: occ_den must be >= 1 and occ_num in 0..occ_den'),
            (dict(occ_num=-1), all3, 'voxel pool: occ_den must be >= 1 and occ_num in 0..occ_den'),
            (dict(occ_num=21), all3, 'voxel pool: occ_den must be >= 1 and occ_num in 0..occ_den'),
            (dict(labels=None), all3, 'voxel pool: labels must not be NULL'), (dict(seen=None), all3, 'voxel pool: seen must not be NULL'),
            (dict(descs=None), all3, 'voxel pool: levels must hold 1 to 3 descriptors'),
            (dict(n_levels=0), all3, 'voxel pool: levels must hold 1 to 3 descriptors'),
            (dict(n_levels=4), all3, 'voxel pool: levels must hold 1 to 3 descriptors'),
            (dict(), [(2, 'ls'), (4, '')], 'voxel pool: a level needs at least one output')]
    for bad, levels, msg in pool:
        r, err, outs = raw_pool(T, sc, levels, **bad)
        assert r == -1 and re.match(msg, err), (err, msg)
        assert all((a == 7).all() for _, o in outs for a in o.values()), msg
    r, err, outs = raw_pool(T, sc, [(2, 'ls'), (4, 'lsv')], visible=False)
    assert r == -1 and err == 'voxel pool: a visible output needs the visible input' and all((a == 7).all() for _, o in outs for a in o.values())
    psc, pwant = pack_want(16, 4)
    pack = [(dict(px=0), {}, r'voxel pack: px must be in 1\.\.1024'), (dict(px=1025), {}, r'voxel pack: px must be in 1\.\.1024'),
            (dict(nz=0), {}, r'voxel pack: nz must be in 1\.\.32'), (dict(nz=33), {}, r'voxel pack: nz must be in 1\.\.32'),
            (dict(labels=None), {}, 'voxel pack: labels must not be NULL'),
            (dict(), dict(outputs=''), 'voxel pack: at least one output is needed'),
            (dict(), dict(label_map=None), 'voxel pack: label_out needs label_map'),
            (dict(), dict(inputs='vi'), 'voxel pack: invalid_bits needs seen'),
            (dict(), dict(inputs='si'), 'voxel pack: occluded_bits needs visible'),
            (dict(), dict(inputs='sv'), 'voxel pack: bin_bits needs input_occ')]
    for bad, how, msg in pack:
        r, err, out = raw_pack(T, psc, **how, **bad)
        assert r == -1 and re.match(msg, err), (err, msg)
        assert (out['label'] == 0x0707).all() and all((out[k] == 7).all() for k in ('invalid', 'occluded', 'bin')), msg
    prof = ctx.profile_read()
    assert prof['voxel_pool'][1] == 0 and prof['voxel_pack'][1] == 0
    same_pool(raw_pool(T, sc, all3), 24, 8, all3)                 # the calls as such are fine, and their launches are counted
    same_pack(raw_pack(T, psc), pwant)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['voxel_pool'][1] == 1 and prof['voxel_pack'][1] == 1 and prof['bev_camera_rays'][1] == 0


# ---------------------------------------------------------------------------------------------- 4: the top level
def test_pyramid_of_the_generator(T):
    """SemBEVGenerator.voxel_pyramid_device on numpy volumes: one pool launch, one pack launch per level."""
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from test_gpu_kernels import SEM_IDXS
    sc, _ = scene_of(24, 8)
    gen = SemBEVGenerator(SEM_IDXS, **{k: v for k, v in BEV_KITTI.items() if k != 'type'})
    ctx = _lib.Context.get()
    ctx.profile(1)
    out = gen.voxel_pyramid_device(sc['labels'], sc['seen'], sc['visible'], sc['input_occ'], label_map=sc_.LABEL_MAP, empty_value=9)
    prof = ctx.profile_read()
    ctx.profile(0)
    assert prof['voxel_pool'][1] == 1 and prof['voxel_pack'][1] == 4
    want = sc_.pyramid_model(sc['labels'], sc['seen'], sc['visible'], sc['input_occ'], label_map=sc_.LABEL_MAP, empty_value=9)
    compare_pyramid(out, want)
    out = gen.voxel_pyramid_device(sc['labels'], sc['seen'], scales=(4, 1))
    compare_pyramid(out, sc_.pyramid_model(sc['labels'], sc['seen'], scales=(4, 1)))
    assert sorted(out['packed'][1]) == ['invalid', 'label'] and list(out['levels']) == [4, 1]


def compare_pyramid(out, want):
    assert sorted(out['levels']) == sorted(want['levels']) and sorted(out['packed']) == sorted(want['packed'])
    for kind in ('levels', 'packed'):
        for s in want[kind]:
            assert sorted(out[kind][s]) == sorted(want[kind][s]), (kind, s)
            for k, w in want[kind][s].items():
                got = out[kind][s][k].cpu().numpy()
                assert got.dtype == w.dtype and np.array_equal(got, w), (kind, s, k)


def test_voxel_ssc_sample_on_a_kitti_sequence(T, tmp_path):
    from pca_amd import ssc
    from pca_amd.writer import AsyncBevWriter
    acc, idx = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=14), 9
    z_range, nz, classes = (-2.0, 4.4), 32, [[0, 1, 2], [13, 14, 15, 17], [5], [8, 9]]
    px = acc.sem_bev_generator.pixel_size
    vis = acc.voxel_visibility(idx, z_range=z_range, nz=nz, classes=classes)
    before = [t.clone() for t in acc.store._arrays()]
    out = acc.voxel_ssc_sample(idx, z_range=z_range, nz=nz, classes=classes)
    # nothing was written to the store (bytes: rows behind the stored points hold whatever the allocation held)
    assert all(T.equal(a.view(T.uint8), b.view(T.uint8)) for a, b in zip(before, acc.store._arrays()))
    assert sorted(out) == sorted(list(vis) + ['input_occ', 'levels', 'packed'])
    assert all(T.equal(out[k], vis[k]) for k in vis if isinstance(vis[k], T.Tensor))
    # the single-scan input: the labels pass over the last frame of the present part
    gen = acc.sem_bev_generator
    pc, rot_mat, view = acc._unaugmented_part(idx, 'present')
    lo, hi = pc.frames()
    assert hi - lo > 1
    one = acc.store.bev_voxel_labels(gen._pass_params(pc, rot_mat, 0., 0., view), *gen._voxel_grid(z_range, nz),
                                     *gen.voxel_label_table(classes), first_frame=hi - 1, last_frame=hi)
    input_occ = (one['counts'].cpu().numpy() != 0).astype(np.uint8)
    assert np.array_equal(out['input_occ'].cpu().numpy(), input_occ) and 0 < input_occ.sum() < (vis['counts'] != 0).sum().item()
    labels, seen, visible = (vis[k].cpu().numpy() for k in ('labels', 'seen', 'visible'))
    want = sc_.pyramid_model(labels, seen, visible, input_occ)
    compare_pyramid(out, want)
    assert np.array_equal(out['levels'][1]['state'].cpu().numpy(), vis['state'].cpu().numpy())
    assert (want['levels'][2]['state'] == 2).any() and (want['levels'][2]['state'] == 1).any()
    # two input frames, no camera, fewer scales
    two = acc.voxel_ssc_sample(idx, z_range=z_range, nz=nz, classes=classes, scales=(1, 2), input_frames=2, occluded=False)
    assert 'visible' not in two and sorted(two['packed'][1]) == ['bin', 'invalid', 'label'] and sorted(two['levels']) == [1, 2]
    assert (two['input_occ'] >= out['input_occ']).all() and (two['input_occ'] != out['input_occ']).any()
    compare_pyramid(two, sc_.pyramid_model(labels, seen, None, two['input_occ'].cpu().numpy(), scales=(1, 2)))
    # the files: written from the device payloads by the writer's threads, read back by the host inverse
    writer = AsyncBevWriter(n_threads=2)
    try:
        paths = ssc.write_ssc_sample(out, str(tmp_path / 'voxels'), 7, writer=writer)
        writer.flush()
        assert writer.files_written == len(paths) == 10
    finally:
        writer.close()
    back = ssc.read_ssc_sample(str(tmp_path / 'voxels'), 7, px, nz, (1, 2, 4, 8))
    assert np.array_equal(back[1]['occluded'], visible == 0) and np.array_equal(back[1]['bin'], input_occ)
    for s in (1, 2, 4, 8):
        lv = want['levels'][s]
        assert np.array_equal(back[s]['label'], np.where(lv['labels'] < 32, lv['labels'].astype(np.uint16) + 1, 0)), s
        assert np.array_equal(back[s]['invalid'], lv['state'] == 0), s
    acc.store.check_status()
