"""CPU: the bindings of pca_voxel_pool / pca_voxel_pack exist, and the numpy model of tests/voxel_ssc_common.py -- which the GPU
tests of tests/test_gpu_voxel_ssc.py hold the kernels to -- is right on hand-built cases, is not hierarchical by accident, packs
as a per-voxel loop does, and its random scenes hold the situations they are meant to hold.  The host side of the file form
(pca_amd/ssc.py, AsyncBevWriter.submit_files) makes its round trip without a device."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import voxel_ssc_common as sc_
from conftest import ROOT

POOL_SHAPES = [(8, 8), (24, 8), (72, 16), (136, 32)]             # the shapes of tests/test_gpu_voxel_ssc.py


def test_bindings_and_signatures():
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib, ssc
    from pca_amd.device_store import DeviceStore
    from pca_amd.writer import AsyncBevWriter
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    for name, n_args in (('pca_voxel_pool', 11), ('pca_voxel_pack', 14)):
        assert name in _lib.EXPORTS and isinstance(getattr(lib, name), C._CFuncPtr) and len(getattr(lib, name).argtypes) == n_args
    assert _lib.KERNEL_IDS_SSC == ('voxel_pool', 'voxel_pack')
    text = open(os.path.join(ROOT, 'include', 'pca.h')).read()
    # the second block is what it was, and a third one follows it and ends the profiler's tables
    second = text[text.index('PCA_K_BEV_INST_INIT = PCA_K_COUNT'):text.index('PCA_K_TOTAL')].replace('= PCA_K_COUNT', '')
    ids = second.replace(',', ' ').split()
    assert len(ids) == len(_lib.KERNEL_IDS_INST) + len(_lib.KERNEL_IDS_CAMERA) and ids[-1] == 'PCA_K_BEV_CAMERA_RAYS'
    third = text[text.index('PCA_K_VOXEL_POOL = PCA_K_TOTAL'):]
    third = third[:third.index('}')].replace('= PCA_K_TOTAL', '').replace(',', ' ').split()
    assert third == ['PCA_K_VOXEL_POOL', 'PCA_K_VOXEL_PACK', 'PCA_K_END']
    assert [f[0] for f in _lib.PcaVoxelPoolLevel._fields_] == ['scale', 'labels', 'state', 'visible']
    assert C.sizeof(_lib.PcaVoxelPoolLevel) == 32
    p = inspect.signature(DeviceStore.voxel_pool).parameters
    assert list(p)[1:] == ['labels', 'seen', 'visible', 'scales', 'occupied_fraction']
    assert p['scales'].default == (2, 4, 8) and p['occupied_fraction'].default == (1, 20)
    p = inspect.signature(DeviceStore.voxel_pack).parameters
    assert list(p)[1:] == ['labels', 'seen', 'visible', 'input_occ', 'label_map', 'empty_value'] and p['empty_value'].default == 0
    p = inspect.signature(SemBEVGenerator.voxel_pyramid_device).parameters
    assert list(p)[1:] == ['labels', 'seen', 'visible', 'input_occ', 'scales', 'label_map', 'empty_value', 'occupied_fraction']
    assert p['scales'].default == (1, 2, 4, 8)
    p = inspect.signature(SemanticPointCloudAccumulator.voxel_ssc_sample).parameters
    assert list(p)[1:] == ['present_idx', 'part', 'z_range', 'nz', 'classes', 'include_dyn', 'origins', 'cameras', 'stride',
                           'max_depth', 'scales', 'input_frames', 'label_map', 'occluded']
    assert p['input_frames'].default == 1 and p['occluded'].default is True and p['nz'].default == 32
    assert list(inspect.signature(ssc.write_ssc_sample).parameters) == ['sample', 'directory', 'frame_id', 'writer']
    assert list(inspect.signature(ssc.read_ssc_sample).parameters) == ['directory', 'frame_id', 'px', 'nz', 'scales']
    assert 'LMSCNet' in ssc.write_ssc_sample.__doc__ and callable(AsyncBevWriter.submit_files)


# ---------------------------------------------------------------------------------------------- the pooling rule, by hand
def one_block(s, n_occ, n_free=0, label=5):
    """An 8 x 8 x 8 volume, empty and unseen, whose coarse voxel 0 of scale s holds n_occ voxels of `label` and n_free free ones."""
    v = sc_.empty_scene(8, 8)
    at = np.arange(n_occ + n_free)
    k, r, c = at // (s * s), (at // s) % s, at % s
    v['labels'][k[:n_occ], r[:n_occ], c[:n_occ]] = label
    v['seen'][k[n_occ:], r[n_occ:], c[n_occ:]] = 9
    return v


@pytest.mark.parametrize('s,thr', [(2, 1), (4, 4), (8, 26)])
def test_the_threshold_of_every_scale(s, thr):
    """occupied_fraction (1, 20): n_occ = 0 | 1 at s = 2, 3 | 4 at s = 4, 25 | 26 at s = 8 -- "more than 0.95 n empty -> empty"."""
    assert sc_.THRESHOLD[s] == thr == min(n for n in range(1, s ** 3 + 1) if not (s ** 3 - n) > 0.95 * s ** 3)
    below = sc_.pool_model(**one_block(s, thr - 1), s=s)
    at = sc_.pool_model(**one_block(s, thr), s=s)
    assert below['labels'][0, 0, 0] == 255 and below['state'][0, 0, 0] == 0
    assert at['labels'][0, 0, 0] == 5 and at['state'][0, 0, 0] == 2
    assert (at['labels'].ravel()[1:] == 255).all() and (at['state'].ravel()[1:] == 0).all() and not at['visible'].any()
    # other fractions: (1, 8) asks for an eighth, (0, 1) for one occupied voxel
    assert sc_.pool_model(**one_block(s, s ** 3 // 8 - 1), s=s, fraction=(1, 8))['state'][0, 0, 0] == 0
    assert sc_.pool_model(**one_block(s, s ** 3 // 8), s=s, fraction=(1, 8))['state'][0, 0, 0] == 2
    assert sc_.pool_model(**one_block(s, 1), s=s, fraction=(0, 1))['state'][0, 0, 0] == 2
    assert sc_.pool_model(**one_block(s, 0), s=s, fraction=(0, 1))['state'][0, 0, 0] == 0


@pytest.mark.parametrize('s', sc_.SCALES)
def test_free_against_unseen_a_tie_is_unseen(s):
    n = s ** 3
    n_occ = sc_.THRESHOLD[s] - 1 - (n - sc_.THRESHOLD[s] + 1) % 2          # below the threshold, an even rest
    assert sc_.pool_model(**one_block(s, n_occ, (n - n_occ) // 2), s=s)['state'][0, 0, 0] == 0
    assert sc_.pool_model(**one_block(s, n_occ, (n - n_occ) // 2 + 1), s=s)['state'][0, 0, 0] == 1
    assert sc_.pool_model(**one_block(s, n_occ, (n - n_occ) // 2 + 1), s=s)['labels'][0, 0, 0] == 255


def test_a_label_tie_goes_to_the_smallest_and_a_byte_of_40_is_empty():
    v = sc_.empty_scene(8, 8)
    v['labels'][0, 0, :2] = 9
    v['labels'][1, 1, :2] = 4
    v['labels'][0, 1, 0] = 17
    out = sc_.pool_model(**v, s=2)
    assert out['labels'][0, 0, 0] == 4 and out['state'][0, 0, 0] == 2
    v['labels'][0, 1, 1] = 9                                      # one more voxel of 9 ends the tie
    assert sc_.pool_model(**v, s=2)['labels'][0, 0, 0] == 9
    # 40 is no label: the voxel is empty -- free or unseen by its `seen` byte -- and takes no part in the vote
    w = sc_.empty_scene(8, 8)
    w['labels'][0, 0, 0] = 40
    assert sc_.pool_model(**w, s=2)['labels'][0, 0, 0] == 255 and sc_.pool_model(**w, s=2)['state'][0, 0, 0] == 0
    w['seen'][:2, :2, :2] = 1
    w['seen'][0, 0, 1] = 0                                        # 7 free (the 40 among them) against 1 unseen
    assert sc_.pool_model(**w, s=2)['state'][0, 0, 0] == 1
    assert sc_.state_of(w['labels'], w['seen'])[0, 0, 0] == 1
    packed = sc_.pack_model(w['labels'], w['seen'])
    assert packed['label'][0 * 8 * 8 + 7 * 8 + 0] == 0 and not np.unpackbits(packed['invalid'])[7 * 8]     # voxel (0, 7, 0): free


def test_scale_4_is_decided_from_the_fine_voxels_not_from_scale_2():
    """Five 2 x 2 x 2 cells hold {A, A, B}, three are full of B: the fine voxels vote 10 A against 29 B; the scale-2 results
    would vote five A against three B."""
    A, B = 7, 3
    v = sc_.empty_scene(8, 8)
    cells = [(k, r, c) for k in (0, 2) for r in (0, 2) for c in (0, 2)]
    for k, r, c in cells[:5]:
        v['labels'][k, r, c:c + 2] = A
        v['labels'][k + 1, r, c] = B
    for k, r, c in cells[5:]:
        v['labels'][k:k + 2, r:r + 2, c:c + 2] = B
    two = sc_.pool_model(**v, s=2)['labels'][:2, :2, :2].ravel()
    assert sorted(two.tolist()) == [B] * 3 + [A] * 5
    assert sc_.pool_model(**v, s=4)['labels'][0, 0, 0] == B
    assert sc_.pool_hierarchical(v['labels'], v['seen'], 4)['labels'][0, 0, 0] == A
    assert sc_.pool_model(**v, s=8)['labels'][0, 0, 0] == B and sc_.pool_model(**v, s=8)['state'][0, 0, 0] == 2


def test_visible_is_any_fine_voxel():
    v = sc_.empty_scene(8, 8)
    v['visible'][5, 6, 7] = 200
    for s in sc_.SCALES:
        vis = sc_.pool_model(**v, s=s)['visible']
        assert vis.sum() == 1 and vis[5 // s, 6 // s, 7 // s] == 1
    assert 'visible' not in sc_.pool_model(v['labels'], v['seen'], None, 2)


# ---------------------------------------------------------------------------------------------- the random scenes
@pytest.mark.parametrize('px,nz', POOL_SHAPES)
def test_random_scenes_are_what_they_claim(px, nz):
    """Every scene the GPU tests pool holds, at every scale, a coarse voxel exactly at its threshold and one exactly one
    below, a label tie in an occupied voxel and a free / unseen tie in one that is not.  The one exception is forced: the
    8 x 8 x 8 volume has a single coarse voxel of scale 8, which cannot be all four -- scale 8 has them in the other shapes."""
    sc = sc_.random_scene(px, nz)
    for s in sc_.SCALES:
        if (px // s) * (px // s) * (nz // s) < 4:
            assert (px, nz, s) == (8, 8, 8)
            continue
        got = sc_.situations(sc, s)
        assert all(got[k] >= 1 for k in sc_.PLANTS), (s, got)
    lab = sc['labels']
    # (all 32 labels wherever the volume is large enough to be expected to hold them: the single block has 512 voxels)
    assert ((lab >= 32) & (lab < 255)).sum() >= 1 and len(np.unique(lab[lab < 32])) >= (32 if px > 8 else 16)
    # and flat pooling differs from hierarchical pooling somewhere (except in the single block)
    if px > 8:
        assert (sc_.pool_model(lab, sc['seen'], None, 4)['labels'] != sc_.pool_hierarchical(lab, sc['seen'], 4)['labels']).any()


# ---------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize('px,nz', [(3, 5), (5, 3)])
def test_packing_against_a_per_voxel_loop(px, nz):
    sc = sc_.pack_scene(px, nz)
    want = sc_.pack_loop(sc['labels'], sc['seen'], sc['visible'], sc['input_occ'], sc_.LABEL_MAP, sc_.EMPTY_VALUE)
    got = sc_.pack_model(sc['labels'], sc['seen'], sc['visible'], sc['input_occ'], sc_.LABEL_MAP, sc_.EMPTY_VALUE)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    n = px * px * nz                                              # 45 or 75 places: the last byte is padded
    assert got['invalid'].size == (n + 7) // 8 and n % 8 in (5, 3)
    assert all(got[k][-1] & ((1 << (8 - n % 8)) - 1) == 0 for k in ('invalid', 'occluded', 'bin'))      # the padding bits
    assert 0 < np.unpackbits(got['invalid']).sum() < px * px * nz
    assert sorted(sc_.pack_model(sc['labels'])) == ['label']
    default = sc_.pack_model(sc['labels'])['label']
    assert set(np.unique(default)) <= set(range(33)) and (default == 0).any() and (default == 1).any() == (sc['labels'] == 0).any()


# ---------------------------------------------------------------------------------------------- the files, on the host
def test_host_round_trip_through_submit_files(tmp_path):
    from pca_amd import ssc
    from pca_amd.writer import AsyncBevWriter
    px, nz = 8, 8
    sc = sc_.random_scene(px, nz)
    pyr = sc_.pyramid_model(sc['labels'], sc['seen'], sc['visible'], sc['input_occ'])
    sample = {'packed': {s: {k: v.tobytes() for k, v in p.items()} for s, p in pyr['packed'].items()}}
    writer = AsyncBevWriter(n_threads=2)
    try:
        paths = ssc.write_ssc_sample(sample, str(tmp_path / 'voxels'), 42, writer=writer)
        writer.flush()
        assert writer.files_written == 10 and writer.previews_written == 0
    finally:
        writer.close()
    names = ['000042.label', '000042.invalid', '000042.occluded', '000042.bin'] + \
        [f'000042_1_{s}.{ext}' for s in (2, 4, 8) for ext in ('label', 'invalid')]
    assert [os.path.basename(p) for p in paths] == names and sorted(os.listdir(tmp_path / 'voxels')) == sorted(names)
    for s in (1, 2, 4, 8):
        n = (px // s) ** 2 * (nz // s)
        stem = '000042' if s == 1 else f'000042_1_{s}'
        assert os.path.getsize(tmp_path / 'voxels' / f'{stem}.label') == 2 * n
        assert os.path.getsize(tmp_path / 'voxels' / f'{stem}.invalid') == (n + 7) // 8
    back = ssc.read_ssc_sample(str(tmp_path / 'voxels'), 42, px, nz, (1, 2, 4, 8))
    lv = pyr['levels']
    assert sorted(back[1]) == ['bin', 'invalid', 'label', 'occluded'] and all(sorted(back[s]) == ['invalid', 'label'] for s in (2, 4, 8))
    assert np.array_equal(back[1]['occluded'], lv[1]['visible'] == 0) and np.array_equal(back[1]['bin'], lv[1]['input_occ'] != 0)
    for s in (1, 2, 4, 8):
        assert back[s]['label'].shape == (nz // s, px // s, px // s) and back[s]['label'].dtype == np.uint16
        occ = lv[s]['labels'] < 32
        assert np.array_equal(back[s]['label'], np.where(occ, lv[s]['labels'].astype(np.uint16) + 1, 0))
        assert np.array_equal(back[s]['invalid'], lv[s]['state'] == 0)
    assert np.array_equal(ssc.unpack_bits(pyr['packed'][1]['invalid'], px, nz), lv[1]['state'] == 0)
    with pytest.raises(ValueError, match='bit stream'):
        ssc.unpack_bits(b'\x00' * 3, px, nz)
