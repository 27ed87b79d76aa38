"""CPU: the bindings of pca_voxel_instance_match exist, and the numpy model of tests/voxel_tracks_common.py -- which the GPU tests
of tests/test_gpu_voxel_tracks.py hold the kernels to -- does what include/pca.h says on hand-made cases.  Every case asserts
that its scene holds the situation it is named after (a test that cannot see a tie-rule bug proves nothing): a shift with an
instance that leaves and one that enters, a split with an exact tie, a merge, a best that is not mutual, the two thresholds
at and one below their value, ids outside the rows, a turn about a point off the centre against a per-voxel loop, three
chained volumes, pca_amd.host_logic.voxel_index_map against the cell rule of the voxel passes, and the store-frame mark."""
import ctypes as C
import inspect

import numpy as np
import pytest

import voxel_tracks_common as vt


def test_bindings_and_signatures():
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib, tracks
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    lib = _lib.load()
    for name, n_args in (('pca_voxel_instance_match_workspace_bytes', 3), ('pca_voxel_instance_match', 26)):
        assert name in _lib.EXPORTS and isinstance(getattr(lib, name), C._CFuncPtr) and len(getattr(lib, name).argtypes) == n_args
    ws = lib.pca_voxel_instance_match_workspace_bytes
    # keys 8 B and counts 4 B per slot, two 8 B bests, 16 counters, four 4 B arrays per cur row and two per prev row, each on a
    # 256-byte boundary; -1 outside the limits; no device needed
    assert ws(64, 128, 1024) == 8192 + 4096 + 1024 + 512 + 256 + 4 * 512 + 2 * 256
    assert ws(1, 1, 16) == 256 * 11
    assert [ws(*s) for s in ((0, 1, 16), (1, 0, 16), (65537, 1, 16), (1, 65537, 16), (1, 1, 8), (1, 1, 24), (1, 1, 1 << 23))] == [-1] * 7
    assert ws(65536, 65536, 1 << 22) > 0
    p = inspect.signature(DeviceStore.voxel_instance_match).parameters
    assert list(p)[1:] == ['prev_inst', 'n_prev', 'cur_inst', 'n_cur', 'index_map', 'prev_track', 'counter', 'min_overlap', 'min_iou',
                           'cap_pairs', 'ids']
    assert p['min_overlap'].default == 1 and p['min_iou'].default == 0.0 and p['cap_pairs'].default is None
    p = inspect.signature(SemBEVGenerator.voxel_instance_match_device).parameters
    assert list(p)[1:4] == ['prev', 'cur', 'T_cur_from_prev']
    p = inspect.signature(SemanticPointCloudAccumulator.track_instances).parameters
    assert list(p)[1:4] == ['present_idx', 'state', 'part'] and p['state'].default is None and p['boxes'].default is False
    assert p['min_overlap'].default == 1 and p['min_iou'].default == 0.0
    assert callable(SemanticPointCloudAccumulator.store_frame) and hasattr(tracks, 'TrackState')


def boxes(px, nz, *items, fill=-1):
    """A volume with box `i` = (id, k0, k1, r0, r1, c0, c1) set to its id (half-open ranges), `fill` elsewhere."""
    vol = np.full((nz, px, px), fill, dtype=np.int32)
    for i, k0, k1, r0, r1, c0, c1 in items:
        vol[k0:k1, r0:r1, c0:c1] = i
    return vol


# ---------------------------------------------------------------------------------------------- (a) an integer shift
def test_shift_keeps_partners_loses_and_gains():
    px, nz = 16, 3
    # prev: three instances; the scene moves 5 columns to the right: instance 2 (at the right edge) leaves the grid.  cur is
    # numbered in ITS order of smallest place, which differs from prev's, and holds one instance that was not there before.
    prev = boxes(px, nz, (0, 0, 2, 1, 3, 1, 4), (1, 1, 3, 8, 11, 3, 6), (2, 0, 1, 5, 7, 12, 16))
    cur = np.full_like(prev, -1)
    shifted = vt.moved(prev, (5, 0, 0))
    cur[shifted == 0], cur[shifted == 1] = 1, 2             # renumbered
    cur[0, 13:15, 0:2] = 0                                   # enters on the left; its image lies outside prev
    cur[2, 14:16, 13:16] = 3                                 # in view of prev but on empty space: new as well
    assert not (shifted == 2).any()                          # the one that leaves is gone from cur
    want = vt.model(prev, 3, cur, 5, vt.shift_map(-5, 0, 0))
    assert want['match'].tolist() == [-1, 0, 1, -1, -1]
    info = want['cur_info'].astype(np.int64)
    assert info[0].tolist() == [4, 0, 0, 0]                  # entered: no voxel in view
    assert info[3, 0] == 6 and info[3, 1] == 6 and info[3, 2] == 0       # in view, nothing under it
    assert (info[1:3, 0] == info[1:3, 1]).all() and (info[1:3, 0] == info[1:3, 2]).all()     # every voxel kept its partner
    assert want['cur_track'].tolist() == [0, 0, 1, 1, -1]    # prev_track None: the track of a is a; t0 = 0: new numbers 0, 1
    # (new numbers from 0 collide with rows-as-tracks by design of the NULL default: a sequence passes prev_track and t0)
    chained = vt.model(prev, 3, cur, 5, vt.shift_map(-5, 0, 0), prev_track=[10, 11, 12], t0=13)
    assert chained['cur_track'].tolist() == [13, 10, 11, 14, -1] and chained['counter'] == 15
    assert want['prev_info'][:, 3].tolist() == [2, 3, 0] and want['stats'][7] == 1      # prev 2 is lost
    assert want['stats'].tolist() == [int((cur >= 0).sum()), int(info[:, 1].sum()), int(info[1:3, 0].sum()), 2, 0, 2, 2, 1, 0, 0]


# ---------------------------------------------------------------------------------------------- (b) a split, (c) a merge
def test_split_larger_overlap_wins_and_tie_goes_to_smaller_b():
    px, nz = 12, 1
    prev = boxes(px, nz, (0, 0, 1, 2, 4, 0, 10))
    cur = boxes(px, nz, (0, 0, 1, 2, 4, 0, 3), (1, 0, 1, 2, 4, 4, 10))          # 6 and 12 voxels of the 20
    want = vt.model(prev, 1, cur, 2, vt.shift_map())
    assert want['pairs'].tolist() == [[0, 0, 6], [0, 1, 12]]
    assert want['match'].tolist() == [-1, 0] and want['cur_track'].tolist() == [0, 0]   # (the other is new: t0 = 0)
    assert want['prev_info'][0].tolist() == [20, 12, 2, 2]
    assert want['cur_info'][0].tolist() == [6, 6, 6, 1]      # its best is prev 0, whose best is the other: no match
    tie = boxes(px, nz, (0, 0, 1, 2, 4, 0, 5), (1, 0, 1, 2, 4, 5, 10))
    want = vt.model(prev, 1, tie, 2, vt.shift_map(), t0=7)
    assert want['pairs'][:, 2].tolist() == [10, 10]          # an exact tie
    assert want['match'].tolist() == [0, -1] and want['cur_track'].tolist() == [0, 7]


def test_merge_two_prev_under_one_cur():
    px, nz = 12, 2
    prev = boxes(px, nz, (0, 0, 2, 1, 3, 0, 4), (1, 0, 2, 1, 3, 5, 11))         # 16 and 24 voxels
    cur = boxes(px, nz, (0, 0, 2, 1, 3, 0, 11))
    want = vt.model(prev, 2, cur, 1, vt.shift_map(), prev_track=[4, 9])
    assert want['pairs'].tolist() == [[0, 0, 16], [1, 0, 24]]
    assert want['match'].tolist() == [1] and want['cur_track'].tolist() == [9]
    assert want['prev_info'][:, 3].tolist() == [0, 1] and want['stats'][7] == 1          # prev 0 is lost
    # an exact tie goes to the smaller a
    prev = boxes(px, nz, (0, 0, 2, 1, 3, 0, 5), (1, 0, 2, 1, 3, 5, 10))
    want = vt.model(prev, 2, boxes(px, nz, (0, 0, 2, 1, 3, 0, 10)), 1, vt.shift_map())
    assert want['pairs'][:, 2].tolist() == [20, 20] and want['match'].tolist() == [0]


# ---------------------------------------------------------------------------------------------- (d) not mutual
def test_best_that_is_not_mutual_matches_nothing():
    px, nz = 16, 1
    # cur 0 overlaps prev 0 with 2 voxels and nothing else; prev 0's best is cur 1 (6 voxels), whose best is prev 1 (8 voxels)
    prev = boxes(px, nz, (0, 0, 1, 0, 2, 0, 4), (1, 0, 1, 0, 2, 5, 9))
    cur = boxes(px, nz, (0, 0, 1, 0, 2, 0, 1), (1, 0, 1, 0, 2, 1, 9))
    cur[0, 0:2, 4] = -1
    want = vt.model(prev, 2, cur, 2, vt.shift_map())
    assert want['pairs'].tolist() == [[0, 0, 2], [0, 1, 6], [1, 1, 8]]
    assert want['cur_info'][:, 3].tolist() == [1, 2] and want['prev_info'][:, 2].tolist() == [2, 2]
    assert want['match'].tolist() == [-1, 1]
    assert want['prev_info'][0, 3] == 0                      # prev 0: its best (cur 1) prefers prev 1, so prev 0 is lost
    assert want['stats'][5:8].tolist() == [1, 1, 1]


# ---------------------------------------------------------------------------------------------- (e) thresholds
def test_thresholds_at_and_one_below():
    px, nz = 16, 1
    prev = boxes(px, nz, (0, 0, 1, 0, 2, 0, 8))              # 16 voxels
    cur = boxes(px, nz, (0, 0, 1, 0, 2, 4, 16))              # 24 voxels, 8 shared: union 32, IoU 1/4
    M = vt.shift_map()
    assert vt.model(prev, 1, cur, 1, M)['pairs'].tolist() == [[0, 0, 8]]
    assert vt.model(prev, 1, cur, 1, M, min_overlap=8)['match'].tolist() == [0]
    assert vt.model(prev, 1, cur, 1, M, min_overlap=9)['match'].tolist() == [-1]
    # 8 >= min_iou * 32 in f64: a product by a power of two is exact, so 1/4 holds and its successor does not
    above = np.nextafter(0.25, 1.)
    assert 0.25 * 32. == 8.0 and above * 32. > 8.0
    assert vt.model(prev, 1, cur, 1, M, min_iou=0.25)['match'].tolist() == [0]
    assert vt.model(prev, 1, cur, 1, M, min_iou=above)['match'].tolist() == [-1]
    assert vt.model(prev, 1, cur, 1, M, min_iou=np.nextafter(0.25, 0.))['match'].tolist() == [0]
    unmatched = vt.model(prev, 1, cur, 1, M, min_iou=0.5, t0=3)
    assert unmatched['cur_track'].tolist() == [3] and unmatched['stats'][5:8].tolist() == [0, 1, 1]
    assert unmatched['cur_info'][0].tolist() == [24, 24, 8, 1]           # the best is still reported


# ---------------------------------------------------------------------------------------------- (f) ids outside the rows
def test_ids_outside_rows_are_skipped_and_counted():
    px, nz = 8, 2
    prev = boxes(px, nz, (0, 0, 2, 0, 2, 0, 2), (5, 0, 1, 4, 6, 4, 6), (-2, 1, 2, 6, 8, 6, 8), (2, 0, 1, 0, 1, 7, 8))
    cur = boxes(px, nz, (0, 0, 2, 0, 2, 0, 2), (3, 0, 1, 4, 6, 4, 6), (-7, 1, 2, 6, 8, 0, 2), (2 ** 31 - 1, 0, 1, 7, 8, 7, 8))
    want = vt.model(prev, 2, cur, 3, vt.shift_map())         # prev ids 5, 2 and -2, cur ids 3, -7 and 2^31 - 1 lie outside
    assert want['stats'][8] == 4 + 4 + 1 and want['stats'][9] == 4 + 4 + 1
    assert want['stats'][0] == 8 and want['pairs'].tolist() == [[0, 0, 8]]
    assert want['cur_info'][:, 0].tolist() == [8, 0, 0] and want['cur_track'].tolist() == [0, -1, -1]
    assert (want['track_vol'][cur != 0] == -1).all() and (want['track_vol'][cur == 0] == 0).all()
    ids = np.array([0, 1, 2, 3, -1, -2, 2 ** 31 - 1, -2 ** 31], dtype=np.int32)
    assert vt.model(prev, 2, cur, 3, vt.shift_map(), ids=ids, prev_track=[6, 7])['track_ids'].tolist() == [6, -1, -1, -1, -1, -1, -1, -1]


# ---------------------------------------------------------------------------------------------- (g) a turn, per-voxel loop
def test_turn_about_an_off_centre_point_against_a_loop():
    px, nz = 20, 3
    prev, n_prev = vt.blobs(px, nz, 30, 4.5, seed=11)
    cur, n_cur = vt.blobs(px, nz, 24, 4.5, seed=12)
    M = vt.turn_map(30., (6.5, 12.25), (1.5, -2.25, 0.4))
    want = vt.model(prev, n_prev, cur, n_cur, M)
    loop = vt.loop_counts(prev, n_prev, cur, n_cur, M)
    assert len(loop) >= 5                                    # the scene has pairs to speak of
    assert {(int(a), int(b)): int(c) for a, b, c in want['pairs']} == loop
    q0, q1, q2, view = vt.images(cur.shape, M)
    assert 0 < view.sum() < view.size                        # some images leave the grid, some stay
    info = want['cur_info'].astype(np.int64)
    assert (info[:, 1] < info[:, 0]).any() and (info[:, 1] > 0).any()


# ---------------------------------------------------------------------------------------------- (h) chaining
def test_chain_of_three_volumes_never_reuses_a_number():
    px, nz = 16, 2
    v0 = boxes(px, nz, (0, 0, 2, 0, 3, 0, 3), (1, 0, 2, 6, 9, 6, 9))
    v1 = boxes(px, nz, (0, 0, 2, 12, 15, 12, 15), (1, 0, 2, 0, 3, 1, 4), (3, 0, 2, 6, 9, 7, 10))    # row 2 has no voxel
    v2 = boxes(px, nz, (0, 0, 2, 6, 9, 8, 11), (1, 0, 2, 12, 14, 0, 2))
    M = vt.shift_map()
    empty = np.full_like(v0, -1)
    s0 = vt.model(empty, 1, v0, 2, M)                        # the start of a sequence: everything is new, from 0
    assert s0['cur_track'].tolist() == [0, 1] and s0['counter'] == 2
    s1 = vt.model(v0, 2, v1, 4, M, prev_track=s0['cur_track'], t0=s0['counter'])
    assert s1['cur_track'].tolist() == [2, 0, -1, 1] and s1['counter'] == 3              # a row without a voxel: -1, no number
    s2 = vt.model(v1, 4, v2, 2, M, prev_track=s1['cur_track'], t0=s1['counter'])
    assert s2['cur_track'].tolist() == [1, 3] and s2['counter'] == 4
    # track 0 (lost in the third sample) and track 2 (lost as well) are never handed out again
    assert s2['stats'][7] == 2 and sorted(set(s0['cur_track']) | set(s1['cur_track']) | set(s2['cur_track'])) == [-1, 0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------- (i) voxel_index_map
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_voxel_index_map_against_the_cell_rule(seed):
    from pca_amd import host_logic as hl
    rng = np.random.default_rng(seed)
    px, nz = 24, 6

    def geom():
        return (rng.uniform(-2, 2, 3) * (1., 1., 0.15), hl.rotation_matrix_3d(rng.uniform(-np.pi, np.pi)), 0., 0., rng.uniform(20., 40.), px,
                rng.uniform(-2.2, -1.8), rng.uniform(0.5, 0.7))
    prev_geom, cur_geom = geom(), geom()
    if seed == 2:                                            # an augmented view: dx, dy are part of the rule
        prev_geom = prev_geom[:2] + (0.7, -1.3) + prev_geom[4:]
        cur_geom = cur_geom[:2] + (-0.4, 0.9) + cur_geom[4:]
    T = np.eye(4)
    T[:3, :3] = hl.rotation_matrix_3d(rng.uniform(-0.6, 0.6))
    T[:3, 3] = rng.uniform(4, 8, 3) * rng.choice([-1., 1.], 3) * (1., 1., 0.05)       # far enough for some centres to leave
    M = hl.voxel_index_map(prev_geom, cur_geom, T)
    assert M.shape == (3, 4) and M.dtype == np.float64
    assert np.allclose(hl.voxel_index_to_store(cur_geom), vt.index_to_store(cur_geom), rtol=0, atol=1e-12)
    # a cur voxel centre pushed through M ...
    q0, q1, q2, view = vt.images((nz, px, px), M)
    k, row, col = np.meshgrid(np.arange(nz), np.arange(px), np.arange(px), indexing='ij')
    centre = np.stack([col + 0.5, row + 0.5, k + 0.5, np.ones_like(k)], axis=-1).reshape(-1, 4).astype(np.float64)
    # ... against the cell rule applied to the centre's store point moved by inv(T)
    p_cur = centre @ vt.index_to_store(cur_geom).T
    own, _ = vt.cell_of(p_cur[:, :3], cur_geom)
    assert np.array_equal(own, np.stack([k, row, col], axis=-1).reshape(-1, 3))           # A inverts the rule on its own grid
    p_prev = p_cur @ np.linalg.inv(T).T
    cell, edge = vt.cell_of(p_prev[:, :3], prev_geom)
    far = edge >= 1e-9
    assert (~far).mean() < 0.01
    got = np.stack([np.floor(q2), np.floor(q1), np.floor(q0)], axis=-1).reshape(-1, 3)
    assert np.array_equal(got[far], cell[far])
    inside = (cell[:, 0] >= 0) & (cell[:, 0] < nz) & (cell[:, 1] >= 0) & (cell[:, 1] < px) & (cell[:, 2] >= 0) & (cell[:, 2] < px)
    assert np.array_equal(view.reshape(-1)[far], inside[far]) and 0 < inside.sum() < inside.size
    # the identity between equal grids is the identity map
    same = hl.voxel_index_map(cur_geom, cur_geom, np.eye(4))
    assert np.allclose(same, vt.shift_map(), rtol=0, atol=1e-9)


# ---------------------------------------------------------------------------------------------- (j) the store-frame mark
def test_store_frame_follows_update_sem_pcs():
    """The base class's bookkeeping with a store that only records (the run over a fake KITTI tree, through integrate and
    integrate_many, needs the device: tests/test_gpu_voxel_tracks.py)."""
    import fake_kitti as fk
    from sem_pc_accum import SemanticPointCloudAccumulator

    class Recorder:
        def __init__(self):
            self.seen = []

        def retransform(self, T, defer=False):
            self.seen.append((np.array(T), defer))
    acc = SemanticPointCloudAccumulator(50., 1e3, 'none', [], {}, True, dict(type='none'))
    assert np.array_equal(acc.store_frame(), np.eye(4))
    acc._store = Recorder()
    want = np.eye(4)
    for k in range(1, 6):
        acc.update_sem_pcs(fk.t_new_prev(k))
        want = fk.t_new_prev(k) @ want
        assert np.array_equal(acc.store_frame(), want)
    assert len(acc._store.seen) == 5 and all(d for _, d in acc._store.seen)               # the re-transform itself is unchanged
    frame = acc.store_frame()
    frame[0, 0] = 99.                                        # a copy: read-only from outside
    assert np.array_equal(acc.store_frame(), want)
    # two moments give the map between them, whatever came before the earlier one
    F_prev = fk.t_new_prev(2) @ fk.t_new_prev(1)
    assert np.allclose(want @ np.linalg.inv(F_prev), fk.t_new_prev(5) @ fk.t_new_prev(4) @ fk.t_new_prev(3), rtol=0, atol=1e-12)
