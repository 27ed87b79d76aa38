"""The CPU models of tests/store_edges_common.py on hand-written cases, the conditions the device tests
(tests/test_gpu_store_edges.py) rely on for their scenes, and -- in place of mutating the kernels on the GPU -- for each kernel a
list of deliberately wrong variants of its model, each of which must differ from the right model on at least one scene of the
device suite: a kernel with that defect could not pass it.  No GPU needed."""
import numpy as np
import pytest

import store_edges_common as m


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def rows_of(xyz, inst=None, dyn=None):
    r = np.zeros((len(xyz), 10))
    r[:, :3] = xyz
    r[:, 3] = np.arange(len(xyz))                    # (tells the points apart)
    if inst is not None:
        r[:, 8] = inst
    if dyn is not None:
        r[:, 9] = dyn
    return r


# ---- the models on cases small enough to write the result out --------------------------------------------------------
def test_k2_models_by_hand(orc):
    """A shift by (1, 2, 3), then a scaling by 2: exact in f64, so the results can be written down."""
    shift, scale = np.eye(4), np.diag([2., 2., 2., 1.])
    shift[:3, 3] = [1, 2, 3]
    rows = rows_of([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]])
    off = np.array([0, 1, 3, 3, 4])
    got = m.k2_model(rows, off, 1, 3, [shift, scale], orc)
    assert got[:, :3].tolist() == [[0, 0, 0], [4, 6, 8], [6, 8, 10], [3, 3, 3]]
    assert np.array_equal(got[:, 3:], rows[:, 3:])
    assert np.array_equal(m.k2_model(rows, off, 2, 3, [shift], orc), rows)                 # an empty frame
    # the tail: frame i of the batch owes Ts[i+1:] -- here shift, scale, shift | scale, shift | (empty) | nothing; Ts[0] nobody
    got = m.k2_tail_model(rows, off, 0, 4, [scale, shift, scale, shift], orc)
    assert got[:, :3].tolist() == [[3, 6, 9], [3, 4, 5], [5, 6, 7], [3, 3, 3]]
    got = m.k2_tail_model(rows, off, 1, 3, [scale, shift, scale], orc)      # from slot 1 on: slot 0 is no part of the batch
    assert got[:, :3].tolist() == [[0, 0, 0], [4, 6, 8], [6, 8, 10], [3, 3, 3]]
    assert np.array_equal(m.k2_tail_model(rows, off, 1, 1, [scale], orc), rows)
    assert np.array_equal(m.k2_tail_model(rows, off, 1, 0, [scale], orc), rows)


def test_k3_model_by_hand():
    rows = rows_of(np.zeros((4, 3)), inst=[-1, 2, 2, -1], dyn=[0, 0, 1, 0])
    off = np.array([0, 1, 3, 3, 4])
    assert m.k3_model(rows, off, [1], [2])[:, 9].tolist() == [0, 1, 1, 0]
    assert m.k3_model(rows, off, [3, 2], [-1, 2])[:, 9].tolist() == [0, 0, 1, 1]          # -1: the unlabelled; an empty frame
    assert m.k3_model(rows, off, [0, 0], [2, 5])[:, 9].tolist() == [0, 0, 1, 0]            # nothing matches; dyn stays
    assert np.array_equal(m.k3_model(rows, off, [1, 1, 3], [2, 2, -1])[:, :9], rows[:, :9])


def test_dedup_model_by_hand():
    # size 0.5: voxels (0,0,0) (0,0,0) | (-1,0,0) (0,0,0) -- -0.25 floors to -1, it does not truncate to 0
    rows = rows_of([[0.1, 0.1, 0.1], [0.4, 0.2, 0.3], [-0.25, 0.1, 0.1], [0.3, 0.3, 0.3]])
    off = np.array([0, 2, 2, 4])
    frames, new_off = m.dedup_model(rows, off, 0, 3, 0.5)
    assert [f[:, 3].tolist() for f in frames] == [[0.0], [], [2.0]] and new_off.tolist() == [0, 1, 1, 2]
    # from slot 1 on: the copy in slot 0 does not count, leading empty frames stay at lo
    frames, new_off = m.dedup_model(rows, off, 1, 3, 0.5)
    assert [f[:, 3].tolist() for f in frames] == [[], [2.0, 3.0]] and new_off.tolist() == [0, 2, 2, 4]
    # all in one voxel, trailing frames become empty; boundaries at the old end move to the new end
    off = np.array([0, 1, 3, 4, 4])
    frames, new_off = m.dedup_model(rows_of([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]]), off, 0, 4, 8.0)
    assert [len(f) for f in frames] == [1, 0, 0, 0] and new_off.tolist() == [0, 1, 1, 1, 1]
    # the key's range: -2^20 - 1 and -2^20 share the lower boundary voxel, 2^20 - 1, 2^20 and +inf the upper one
    e = 2.0 ** 20
    assert m.voxels([[-e - 1, -e, -e + 1], [e - 2, e - 1, e], [np.inf, -np.inf, 0.5]], 1.0).tolist() == \
        [[0, 0, 1], [2 * e - 2, 2 * e - 1, 2 * e - 1], [2 * e - 1, 0, e]]


def test_hash_restatement_on_known_values():
    """The finaliser is MurmurHash3's fmix64, whose published test values are fmix64(1) and fmix64(2)."""
    h = m.voxel_hash(np.array([0, 1, 2], dtype=np.uint64))
    assert [int(v) for v in h] == [0, 0xb456bcfc34c2cb2c, 0x3abf2a20650683e7]
    assert int(m.voxel_key([[1, 2, 3]])[0]) == (1 << 63) | (1 << 42) | (2 << 21) | 3


# ---- the conditions of the scenes ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', m.K2_SCENES)
def test_k2_windows(orc, name):
    sc = m.k2_scene(name)
    rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
    lo, hi = off[sc['slot_begin']], off[sc['slot_end']]
    assert lo > 0 and hi < off[-1]                              # guards on both sides
    changed = np.any(m.k2_model(rows, off, sc['slot_begin'], sc['slot_end'], sc['Ts'], orc) != rows, axis=1)
    if name in m.K2_UNCHANGED:
        assert not changed.any()
    else:
        assert changed[lo:hi].all() and not changed[:lo].any() and not changed[hi:].any() and hi > lo
    if name.startswith('lo'):
        assert (lo % 2, hi - lo) == (int(name[2]), int(name.split('_n')[1]))
    if name == 'second_trip':
        assert lo % 2 == 1 and hi - lo == m.K2_TRIP + 7


def test_k2_parities_and_columns():
    seen = set()
    for name in m.K2_SCENES:
        sc = m.k2_scene(name)
        off = m.offsets(sc['frames'])
        lo, hi = off[sc['slot_begin']], off[sc['slot_end']]
        if hi > lo:
            seen.add((int(lo % 2), int(hi % 2)))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    r = m.frame(np.random.default_rng(0), 4000)
    assert np.isfinite(r).all() and np.array_equal(r[:, 3].astype(np.float32).astype(np.float64), r[:, 3])
    assert r[:, 4:8].min() == 0 and r[:, 4:8].max() == 255 and set(r[:, 8]) == set(range(-1, 7)) and 0 < r[:, 9].mean() < 1
    Ts = m.transforms(np.random.default_rng(0), 34)
    assert all(np.any(Ts[a, :3] != Ts[b, :3], axis=1).all() for a in range(34) for b in range(a))


@pytest.mark.parametrize('n_pairs', m.K3_PAIR_COUNTS)
def test_k3_scenes_mark_some_and_not_all(n_pairs):
    sc = m.k3_scene(n_pairs)
    rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
    got = m.k3_model(rows, off, sc['slots'], sc['idxs'])
    assert len(sc['slots']) == n_pairs and all(s >= m.K3_HEAD for s in sc['slots'])
    new = (got[:, 9] == 1) & (rows[:, 9] != 1)
    if n_pairs == 0:
        assert not new.any()
        return
    named = np.zeros(len(rows), bool)
    for s in sc['slots']:
        named[off[s]:off[s + 1]] = True
    assert new.any() and not new[~named].any() and (got[named, 9] != 1).any()
    assert ((rows[:, 9] == 1) <= (got[:, 9] == 1)).all() and (rows[named, 9] == 1).any()    # already dynamic stays dynamic
    if n_pairs >= 32:
        assert len(set(zip(sc['slots'], sc['idxs']))) < n_pairs and -1 in sc['idxs']       # repeated pairs, the unlabelled
        assert any(off[s] == off[s + 1] for s in sc['slots'])                               # a pair on an empty frame
        assert len({i for s, i in zip(sc['slots'], sc['idxs']) if s == 3}) == 2              # two instances on one slot
        assert new[off[3] + m.K3_ROW:off[4]].any()                                           # beyond the threads of a row


@pytest.mark.parametrize('name', m.DEDUP_SCENES)
def test_dedup_scenes(name):
    sc = m.dedup_scene(name)
    rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
    sb, se = sc['slot_begin'], sc['slot_end']
    lo, hi = off[sb], off[se]
    frames, new_off = m.dedup_model(rows, off, sb, se, sc['size'])
    kept, total = sum(len(f) for f in frames), hi - lo
    assert sb > 0 and lo % 2 == 1 and se == len(sc['frames']) and new_off[se] == lo + kept
    assert np.array_equal(new_off[:sb + 1], off[:sb + 1]) and np.all(np.diff(new_off) >= 0)
    if name in m.DEDUP_KEEPS_ALL:
        assert kept == total and np.array_equal(new_off, off)
    else:
        assert 0 < kept < total
    if total:                                                   # the guard holds copies of window points
        assert np.array_equal(rows[:min(5, total)], rows[lo:lo + min(5, total)])
    if name.startswith('n'):
        assert total == (1025 if name == 'no_duplicates' else int(name[1:]))
    if name == 'tile_edges':
        assert (off[sb:] - lo).tolist() == [0, 1023, 1024, 1025, 2048, 2049]
    if name == 'one_voxel':
        assert [len(f) for f in frames] == [1, 0, 0, 0, 0]
    if name == 'empty_runs':
        assert [len(f) > 0 for f in frames] == [False, False, True, False, False, False, True, False, False]
    if name == 'clamp':
        # per axis the first point at each end of the range stays, the four others fall into the two boundary voxels
        assert frames[0][:, 3].tolist() == rows[lo + np.array([0, 2, 6]), 3].tolist()
        assert np.array_equal(frames[1][:3], rows[lo + np.array([8, 12, 14])])
        assert (~np.isfinite(rows[lo:hi, :3])).sum() == 6


@pytest.mark.parametrize('name', ['collide_1024', 'collide_4096'])
def test_collision_scenes_home_every_voxel_at_the_last_slot(name):
    """Under the restated key and hash.  (Should the kernel's hash change, this fails and says that the scenes have lost their
    property; the device test stays a valid test of the result.)"""
    sc = m.dedup_scene(name)
    rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
    w = rows[off[sc['slot_begin']]:off[sc['slot_end']], :3]
    cap = m.table_slots(sc['max_points'])
    assert cap == int(name.split('_')[1]) and len(w) <= sc['max_points']
    assert np.all(m.home_slot(w, sc['size'], cap) == cap - 1)
    assert len(np.unique(m.voxels(w, sc['size']), axis=0)) >= (230 if cap == 1024 else 320)


# ---- the scenes discriminate: wrong variants of the models -----------------------------------------------------------
def k2_variants(orc):
    def head_skipped(rows, lo, hi, Ts):
        return m.apply_chain(rows, lo + (lo % 2 if hi > lo else 0), hi, Ts, orc)

    def tail_skipped(rows, lo, hi, Ts):
        return m.apply_chain(rows, lo, hi - (hi % 2 if hi > lo else 0), Ts, orc)

    return {'scalar head skipped': head_skipped, 'scalar tail skipped': tail_skipped,
            'first 16 transforms only': lambda rows, lo, hi, Ts: m.apply_chain(rows, lo, hi, Ts[:m.K2_CHAIN], orc),
            'reverse order': lambda rows, lo, hi, Ts: m.apply_chain(rows, lo, hi, Ts[::-1], orc),
            'one trip of the stride loop': lambda rows, lo, hi, Ts: m.apply_chain(rows, lo, min(hi, lo + m.K2_TRIP), Ts, orc),
            'frame before slot_begin too': None}


def test_k2_scenes_discriminate(orc):
    variants = k2_variants(orc)
    caught = {k: [] for k in variants}
    for name in m.K2_SCENES:
        sc = m.k2_scene(name)
        rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
        sb, se, Ts = sc['slot_begin'], sc['slot_end'], sc['Ts']
        right = m.k2_model(rows, off, sb, se, Ts, orc)
        for k, f in variants.items():
            wrong = f(rows, off[sb], off[se], Ts) if f else m.apply_chain(rows, off[sb - 1], max(off[se], off[sb - 1]), Ts, orc)
            if not m.same_bits(wrong, right):
                caught[k].append(name)
    print(caught)
    assert all(caught.values()), caught
    assert caught['one trip of the stride loop'] == ['second_trip'] and 'nT17' in caught['first 16 transforms only']


def test_k2_tail_scenes_discriminate(orc):
    def variant(rows, off, first, n, Ts, owes=lambda i: i + 1, t_end=None, f_end=None, p_end=None):
        out = rows
        for i in range(n if f_end is None else min(n, f_end)):
            lo, hi = off[first + i], off[first + i + 1]
            out = m.apply_chain(out, lo, hi if p_end is None else min(hi, lo + p_end), Ts[owes(i):t_end], orc)
        return out
    variants = {'frame i takes Ts[i:]': dict(owes=lambda i: i), 'transforms from 17 on dropped': dict(t_end=m.K2_CHAIN + 1),
                'frames from 16 on untouched': dict(f_end=m.K2_CHAIN), 'first 8192 points of a frame only': dict(p_end=m.TAIL_ROW)}
    caught = {k: [] for k in variants}
    for n in m.TAIL_FRAMES:
        sc = m.k2_tail_scene(n)
        rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
        right = m.k2_tail_model(rows, off, sc['first_slot'], n, sc['Ts'], orc)
        assert m.same_bits(variant(rows, off, sc['first_slot'], n, sc['Ts']), right)           # (the variant's own defaults are right)
        assert np.array_equal(right[:off[2]], rows[:off[2]]) and np.array_equal(right[off[2 + n]:], rows[off[2 + n]:])
        assert (n < 2) == m.same_bits(right, rows)
        for k, kw in variants.items():
            if not m.same_bits(variant(rows, off, sc['first_slot'], n, sc['Ts'], **kw), right):
                caught[k].append(n)
    print(caught)
    assert all(caught.values()), caught
    assert caught['transforms from 17 on dropped'] == [18, 33, 34] and caught['frames from 16 on untouched'] == [18, 33, 34]


def test_k3_scenes_discriminate():
    def beyond_the_row(rows, off, slots, idxs):
        out = rows.copy()
        for s, i in zip(slots, idxs):
            seg = out[off[s]:min(off[s + 1], off[s] + m.K3_ROW)]
            seg[seg[:, 8] == i, 9] = 1
        return out
    variants = {'first 32 pairs only': lambda r, o, s, i: m.k3_model(r, o, s[:m.K3_PAIRS], i[:m.K3_PAIRS]),
                'idx -1 ignored': lambda r, o, s, i: m.k3_model(r, o, [a for a, b in zip(s, i) if b != -1], [b for b in i if b != -1]),
                'first 16384 points of a frame only': beyond_the_row,
                'slot relative to the first live slot': lambda r, o, s, i: m.k3_model(r, o, [min(a + m.K3_HEAD, len(o) - 2) for a in s], i)}
    caught = {k: [] for k in variants}
    for n in m.K3_PAIR_COUNTS:
        sc = m.k3_scene(n)
        rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
        right = m.k3_model(rows, off, sc['slots'], sc['idxs'])
        for k, f in variants.items():
            if not m.same_bits(f(rows, off, sc['slots'], sc['idxs']), right):
                caught[k].append(n)
    print(caught)
    assert all(caught.values()), caught
    assert caught['first 32 pairs only'] == [33, 65]


def test_dedup_scenes_discriminate():
    def keep_by(vox, off, sb, se, how):
        lo = off[sb]
        if how == 'last':
            return m.first_of_each(vox[::-1])[::-1]
        cuts = off[sb:se + 1] - lo if how == 'frame' else np.append(np.arange(0, len(vox), m.TILE), len(vox))
        keep = np.zeros(len(vox), bool)
        for a, b in zip(cuts[:-1], cuts[1:]):
            keep[a:b] = m.first_of_each(vox[a:b])
        return keep

    def variant(rows, off, sb, se, size, how='first', empties_move=True, **kw):
        vox = m.voxels(rows[off[sb]:off[se], :3], size, **kw)
        keep = m.first_of_each(vox) if how == 'first' else keep_by(vox, off, sb, se, how)
        frames, new_off = m.compacted(rows, off, sb, se, keep)
        if not empties_move:                                    # the boundaries of trailing empty frames stay where they were
            stay = np.flatnonzero(off[sb + 1:se] >= off[se]) + sb + 1
            new_off[stay] = off[stay]
        return frames, new_off
    variants = {'last occurrence kept': dict(how='last'), 'per frame': dict(how='frame'), 'per 1024-point tile': dict(how='tile'),
                'no clamp': dict(clamp=False), 'trunc for floor': dict(rnd=np.trunc), 'rint for floor': dict(rnd=np.rint),
                'boundaries of empty frames not moved': dict(empties_move=False)}
    caught = {k: [] for k in variants}
    for name in m.DEDUP_SCENES:
        sc = m.dedup_scene(name)
        rows, off = m.all_rows(sc['frames']), m.offsets(sc['frames'])
        args = (rows, off, sc['slot_begin'], sc['slot_end'], sc['size'])
        right = m.dedup_model(*args)
        same = lambda a, b: m.same_bits(m.all_rows(a[0]), m.all_rows(b[0])) and np.array_equal(a[1], b[1])      # noqa: E731
        assert same(variant(*args), right)
        for k, kw in variants.items():
            if not same(variant(*args, **kw), right):
                caught[k].append(name)
    print(caught)
    assert all(caught.values()), caught
    assert 'clamp' in caught['no clamp'] and 'frame_copies' in caught['per frame'] and 'tile_edges' in caught['per 1024-point tile']
