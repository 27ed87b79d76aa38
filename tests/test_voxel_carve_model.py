"""The numpy model of free-space carving (tests/voxel_carve_common.py, the contract of pca_bev_voxel_carve in include/pca.h):
tied to the rays model it repeats (tests/voxel_rays_common.py, itself pinned by tests/test_voxel_rays_model.py), on hand-written
rays, and on the synthetic street scene the defaults were chosen on.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np

import voxel_carve_common as cc
import voxel_rays_common as rc
from window_pass_common import frames_of


def test_the_entry_points_and_their_bindings_exist():
    """(missing before this feature)"""
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    for name in ('pca_bev_carve_workspace_bytes', 'pca_bev_voxel_carve'):
        assert name in _lib.EXPORTS and isinstance(getattr(lib, name), C._CFuncPtr)
    assert _lib.KERNEL_IDS_CARVE == ('bev_carve_ends', 'bev_carve_rays', 'bev_carve_flags')
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pca.h')) as f:
        text = f.read()
    ids = text[text.index('PCA_K_KITTI = 0'):text.index('PCA_K_COUNT')].replace('= 0', '').replace(',', ' ').split()
    names = _lib.KERNEL_IDS + _lib.KERNEL_IDS_VOXEL + _lib.KERNEL_IDS_RAYS + _lib.KERNEL_IDS_RENDER + _lib.KERNEL_IDS_CARVE
    assert len(ids) == len(names) and ids[-4:] == ['PCA_K_RENDER_RESOLVE', 'PCA_K_BEV_CARVE_ENDS', 'PCA_K_BEV_CARVE_RAYS',
                                                   'PCA_K_BEV_CARVE_FLAGS']
    assert lib.pca_version() == 2
    p = inspect.signature(DeviceStore.bev_voxel_carve).parameters
    assert list(p)[:7] == ['self', 'prm', 'z_lo', 'z_step', 'nz', 'origins', 'classes']
    assert (p['end_margin'].default, p['min_cross'].default, p['ratio'].default) == cc.DEFAULTS and p['mark_dyn'].default is False
    for fn in (SemBEVGenerator.voxel_carve_device, SemanticPointCloudAccumulator.carve_dynamic):
        p = inspect.signature(fn).parameters
        assert (p['end_margin'].default, p['min_cross'].default, p['ratio'].default) == cc.DEFAULTS
        assert p['classes'].default is None and p['mark_dyn'].default is False
    # the workspace: vox, cand, hits and cross
    assert lib.pca_bev_carve_workspace_bytes(1000, 16, 4) >= 4 * 1000 + 9 * 16 * 16 * 4


def one(s, e, in_class, px=4, nz=4, prm=cc.DEFAULTS):
    return cc.carve(np.array(s, dtype=np.float64).reshape(-1, 3), np.array(e, dtype=np.float64).reshape(-1, 3), in_class, px, nz, *prm)


def test_end_margin_takes_the_last_steps_before_the_end_voxel():
    """Ray A along u from voxel 0 to voxel 3 (N = 3, steps at 0, 1, 2); a candidate point in each of the voxels 1, 2 (rays B, C:
    N = 0, no step)."""
    s = [[0.5, 1.5, 2.5], [1.2, 1.5, 2.5], [2.2, 1.5, 2.5]]
    e = [[3.5, 1.5, 2.5], [1.8, 1.5, 2.5], [2.8, 1.5, 2.5]]
    cls = [False, True, True]
    row = lambda out, name: out[name][2, 4 - 1 - 1].tolist()     # noqa: E731  (place [k][px - 1 - j][i])
    out = one(s, e, cls, prm=(0, 1, 0.0))
    assert row(out, 'hits') == [0, 1, 1, 1] and row(out, 'cross') == [0, 1, 1, 0]      # voxel 0: crossed, but no candidate
    assert out['flags'].tolist() == [255, 1, 1] and out['stats'].tolist() == [3, 3, 0, 0, 2, 2]
    out = one(s, e, cls, prm=(1, 1, 0.0))
    assert row(out, 'cross') == [0, 1, 0, 0] and out['flags'].tolist() == [255, 1, 0]  # step 2 of 3 no longer counts
    out = one(s, e, cls, prm=(2, 1, 0.0))
    assert row(out, 'cross') == [0, 0, 0, 0] and out['flags'].tolist() == [255, 0, 0]
    out = one(s, e, cls, prm=(3, 1, 0.0))                        # end_margin at the ray's N and above: nothing counts
    assert not out['cross'].any() and not one(s, e, cls, prm=(rc.MAX_STEPS, 1, 0.0))['cross'].any()
    # a ray's own end voxel is never counted by itself: the candidate in voxel 3 is ray A's own end
    out = one(s, e, [True, False, False], prm=(0, 1, 0.0))
    assert row(out, 'cross') == [0, 0, 0, 0] and out['flags'].tolist() == [0, 255, 255]


def test_the_rule_is_min_cross_and_one_product():
    """Voxel 1 holds h candidate points and is crossed by c rays along u."""
    def case(h, c, prm):
        s = [[1.2, 1.5, 0.5]] * h + [[0.5, 1.5, 0.5]] * c
        e = [[1.8, 1.5, 0.5]] * h + [[3.5, 1.5, 0.5]] * c
        out = one(s, e, [True] * h + [False] * c, prm=prm)
        assert out['hits'][0, 2, 1] == h and out['cross'][0, 2, 1] == c
        return out['flags'][:h].tolist()
    assert case(3, 3, (1, 2, 1.0)) == [1, 1, 1]                  # cross == ratio * hits: flagged
    assert case(3, 2, (1, 2, 1.0)) == [0, 0, 0]
    assert case(1, 1, (1, 2, 1.0)) == [0]                        # ratio met, min_cross not
    assert case(1, 2, (1, 2, 1.0)) == [1]
    assert case(2, 3, (1, 3, 1.5)) == [1, 1] and case(2, 3, (1, 3, 1.75)) == [0, 0]
    assert case(2, 1, (1, 1, 0.0)) == [1, 1]


def test_dropped_rays_take_part_but_count_nowhere():
    s = [[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]]
    e = [[1.5, 0.5, 0.5], [1.5, 0.5, 0.5], [1.5 + rc.MAX_STEPS, 0.5, 0.5], [-0.5, 0.5, 0.5]]
    out = one(s, e, [True] * 4, prm=(0, 1, 0.0))
    assert out['stats'].tolist() == [4, 2, 1, 1, 1, 0] and out['flags'].tolist() == [0, 255, 255, 255]
    assert out['place'].tolist() == [(0 * 4 + 3) * 4 + 1, -1, -1, -1] and out['hits'].sum() == 1


def test_without_a_margin_cross_is_the_rays_models_visits_of_candidate_voxels():
    frames, px, nz = frames_of(1), 20, 32
    sensors = np.array([[1.0, 2.0, 0.5], [-8.0, 5.0, 1.0], [30.0, -3.0, 0.75]])
    args = (frames, sensors, (0.3, -0.2, 0.125), rc.rotation(0.4), 0.5, -0.25, 40., px, -1., 0.125, nz, False)
    want = cc.model(*args, [13, 14, 15, 17], end_margin=0, min_cross=1, ratio=0.0)
    rays = rc.traverse(want['s'], want['e'], px, nz, record=True)
    assert np.array_equal(rays['stats'], want['stats'][:4]) and np.array_equal(rays['N'], want['N'])
    vis = rays['visited']
    visits = np.bincount((vis[:, 3] * px + (px - 1 - vis[:, 2])) * px + vis[:, 1], minlength=nz * px * px).reshape(nz, px, px)
    cand = np.zeros(nz * px * px, dtype=bool)
    cand[want['place'][want['flags'] != 255]] = True
    cand = cand.reshape(nz, px, px)
    assert cand.sum() > 300 and np.array_equal(want['cross'], np.where(cand, visits, 0))
    assert (rays['seen'][want['cross'] > 0] == 1).all() and (want['cross'] > 0).sum() > 300
    # a margin only takes away
    assert (cc.model(*args, [13, 14, 15, 17], end_margin=1)['cross'] <= want['cross']).all()


def test_the_street_scene_a_car_that_left_is_flagged_a_parked_one_is_not():
    """The scene the defaults were chosen on (they are this project's choice; no real-data number exists)."""
    frames, origins, kind = cc.street_scene()
    assert [(kind == k).sum() for k in (1, 2)] == [300, 900] and (kind == 0).sum() > 5000
    want = cc.model(frames, origins, include_dyn=False, classes=[cc.CAR], **cc.STREET_GRID)
    assert want['stats'][1] == want['stats'][0] == kind.size and want['stats'][4] == 1200
    flags = want['flags']
    assert (flags[kind == 1] == 1).sum() == 300                  # the car that left, whole
    assert (flags[kind == 2] == 1).sum() == 0 and (flags[kind == 2] == 0).all()       # the parked one: kept, whole
    assert (flags[kind == 0] == 255).all()                       # the wall is no candidate
    # without the margin and the ratio, neighbouring beams of the parked car's own surface carve it
    loose = cc.model(frames, origins, include_dyn=False, classes=[cc.CAR], end_margin=0, min_cross=1, ratio=0.0, **cc.STREET_GRID)
    assert (loose['flags'][kind == 2] == 1).sum() > 0 and (loose['flags'][kind == 1] == 1).all()
    # with the wall's class in the set the wall is a candidate, and stays
    both = cc.model(frames, origins, include_dyn=False, classes=[cc.CAR, cc.WALL], **cc.STREET_GRID)
    assert (both['flags'][kind == 0] == 0).all() and np.array_equal(both['flags'][kind != 0], flags[kind != 0])
