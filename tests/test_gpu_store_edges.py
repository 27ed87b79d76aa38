"""The kernels that maintain the point store in place (csrc/pca_accum.hip) at their edges: K2 (k2_retransform: the 16-byte body
over even-aligned pairs with its scalar head and tail, the grid-stride loop, the 16-transform passes), its batch tail
(k2_retransform_tail: the rows of a pass), K3 (k3_mark_dynamic: the 32-pair passes) and the voxel de-duplication (dedup_insert,
dedup_compact<256>, dedup_offsets: table, in-place compaction, rewrite of frame_off), against the models of
tests/store_edges_common.py -- whose own checks, the conditions on the scenes and the wrong variants the scenes tell apart are
tests/test_store_edges_models.py.  Every comparison is exact: K2 and its tail are bit-equal to the C oracle, K3 and the
de-duplication are integer and selection logic.

Every case loads its scene into a store that is larger than its content, fills the slack of the seven arrays and the unused
tail of frame_off with sentinels, and compares the WHOLE arrays and frame_off after the call with what the model says: the
guard frames, the columns a kernel does not own, the slack and frame_off must keep their bits.  The de-duplication may change
the old window [lo, old hi) and frame_off[slot_begin + 1 .. slot_end], nothing else; what it leaves between the new and the old
end of the window is not specified."""
import ctypes as C

import numpy as np
import pytest

import store_edges_common as m

pytestmark = pytest.mark.gpu

ARRAYS = ('x', 'y', 'z', 'intensity', 'rgbs', 'inst', 'dyn')
SENTINEL = dict(x=-12345.678, y=7.25e11, z=-3.5e-7, intensity=-77.5, rgbs=0x5a5a5a5a, inst=-99, dyn=0xa5, frame_off=-7777)


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


class Loaded:
    """A scene in a DeviceStore with slack and sentinels; `before` is the snapshot the call's result is compared with."""

    def __init__(self, frames, evict=0, slack=37, spare_slots=3):
        import torch
        from pca_amd.device_store import DeviceStore
        assert torch.cuda.is_available(), 'GPU tests need the MI355X'
        self.torch = torch
        self.frames = frames
        self.rows, self.off = m.all_rows(frames), m.offsets(frames)
        self.total = len(self.rows)
        self.st = st = DeviceStore(capacity=self.total + slack, max_frames=len(frames) + spare_slots)
        assert st.load_rows(frames) is None
        for name, t in zip(ARRAYS, st._arrays()):
            t[self.total:] = SENTINEL[name]
        st.frame_off[len(frames) + 1:] = SENTINEL['frame_off']
        st.evict(evict)
        self.ctx, self.lib = st.ctx, st.ctx.lib
        self.ctx.status()                                        # (synchronises; the case starts with a clear status word)
        self.before = self.snapshot()
        want = m.soa(self.rows)
        assert all(m.same_bits(self.before[k][:self.total], want[k]) for k in ARRAYS)          # the store holds the scene
        assert all(len(self.before[k]) == self.total + slack for k in ARRAYS)

    def snapshot(self):
        self.torch.cuda.synchronize()
        snap = {k: t.cpu().numpy() for k, t in zip(ARRAYS, self.st._arrays())}
        snap['rgbs'] = snap['rgbs'].view(np.uint32)
        snap['frame_off'] = self.st.frame_off.cpu().numpy()
        return snap

    def expected(self, rows=None, off=None):
        """`before` with the scene's rows and offsets replaced by the model's."""
        exp = {k: v.copy() for k, v in self.before.items()}
        if rows is not None:
            for k, v in m.soa(rows).items():
                exp[k][:self.total] = v
        if off is not None:
            exp['frame_off'][:len(off)] = off
        return exp

    def call(self, fn, *args):
        """A C entry point (ctx, store, frame_off, ..., stream); returns its code."""
        return fn(self.ctx.h, C.byref(self.st.c_store()), self.st.frame_off.data_ptr(), *args, self.ctx.stream())

    def check(self, exp, clean=True):
        after = self.snapshot()
        for k in ARRAYS + ('frame_off', ):
            assert m.same_bits(after[k], exp[k]), (k, np.flatnonzero(after[k] != exp[k])[:8])
        if clean:
            self.st.check_status()
        return after


def c_transforms(Ts):
    from pca_amd import _lib
    Ts = np.asarray(Ts, dtype=np.float64).reshape(-1, 16)
    return _lib.f64_array(Ts, Ts.size) if len(Ts) else _lib.f64_array(np.zeros(16), 16)     # (n_T = 0 still wants a pointer)


# ---- K2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', m.K2_SCENES)
def test_k2_windows_parities_chains_and_the_second_trip(orc, name):
    sc = m.k2_scene(name)
    L = Loaded(sc['frames'])
    sb, se, Ts = sc['slot_begin'], sc['slot_end'], sc['Ts']
    assert L.call(L.lib.pca_retransform, sb, se, c_transforms(Ts), len(Ts)) == 0, L.lib.pca_last_error(L.ctx.h)
    want = m.k2_model(L.rows, L.off, sb, se, Ts, orc)
    assert (name in m.K2_UNCHANGED) == m.same_bits(want, L.rows)
    L.check(L.expected(rows=want))


# ---- K2 tail -------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_frames', m.TAIL_FRAMES)
def test_k2_tail_rows_of_every_pass(orc, n_frames):
    """first_slot = 2 with guard frames on both sides; a distinct transform per frame: one too many or too few changes bits."""
    sc = m.k2_tail_scene(n_frames)
    L = Loaded(sc['frames'])
    assert L.call(L.lib.pca_retransform_batch_tail, sc['first_slot'], n_frames, c_transforms(sc['Ts'])) == 0, L.lib.pca_last_error(L.ctx.h)
    L.check(L.expected(rows=m.k2_tail_model(L.rows, L.off, sc['first_slot'], n_frames, sc['Ts'], orc)))


def test_k2_tail_through_retransform_batch_with_frames_stored_before(orc):
    """DeviceStore.retransform_batch after an evict: the live frames before the batch take every transform (K2), the batch's
    frames their tails; the evicted frame and the slack keep their bits."""
    sc = m.k2_tail_scene(18)
    rng = np.random.default_rng(7)
    batch = sc['frames'][2:-1]
    L = Loaded([m.frame(rng, n) for n in (9, 301, 0, 78)] + batch, evict=1)
    L.st.retransform_batch(sc['Ts'], len(batch))
    want = m.k2_model(L.rows, L.off, 1, 4, sc['Ts'], orc)
    L.check(L.expected(rows=m.k2_tail_model(want, L.off, 4, len(batch), sc['Ts'], orc)))


def test_k2_tail_refuses_more_frames_than_a_launch_has_rows():
    L = Loaded(m.k2_tail_scene(2)['frames'])
    assert L.call(L.lib.pca_retransform_batch_tail, 2, 65536, c_transforms([])) == -1
    L.check(L.expected())
    assert L.call(L.lib.pca_retransform_batch_tail, 2, -1, c_transforms([])) == -1
    L.check(L.expected())


# ---- K3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_pairs', m.K3_PAIR_COUNTS)
def test_k3_pair_passes_long_frames_and_absolute_slots(n_pairs):
    """After evict(1) the slots are absolute (first live slot = 1); repeated pairs, two instances on one slot, idx = -1, a pair
    on an empty frame, frames beyond the threads of a row; points that are dynamic already stay dynamic."""
    sc = m.k3_scene(n_pairs)
    L = Loaded(sc['frames'], evict=m.K3_HEAD)
    slots, idxs = (C.c_int32 * max(n_pairs, 1))(*sc['slots']), (C.c_int32 * max(n_pairs, 1))(*sc['idxs'])
    assert L.call(L.lib.pca_mark_dynamic, slots if n_pairs else None, idxs if n_pairs else None, n_pairs) == 0, L.lib.pca_last_error(L.ctx.h)
    want = m.k3_model(L.rows, L.off, sc['slots'], sc['idxs'])
    after = L.check(L.expected(rows=want))
    assert (n_pairs == 0) == np.array_equal(after['dyn'], L.before['dyn'])


# ---- voxel de-duplication ------------------------------------------------------------------------
def dedup(L, slot_begin, slot_end, size, max_points, shift=0, short=0):
    """pca_voxel_dedup with a workspace of the call's own, `shift` bytes past its allocation's start, `short` bytes less than
    pca_voxel_dedup_workspace_bytes asks for; returns the code."""
    need = int(L.lib.pca_voxel_dedup_workspace_bytes(max_points, slot_end - slot_begin))
    ws = L.torch.full((need + 256, ), 0xee, dtype=L.torch.uint8, device=L.st.device)
    assert ws.data_ptr() % 256 == 0
    rc = L.call(L.lib.pca_voxel_dedup, slot_begin, slot_end, float(size), int(max_points), ws.data_ptr() + shift, need - short)
    L.torch.cuda.synchronize()
    return rc


def check_dedup(L, before, lo, old_hi, kept_frames, new_off, clean=True):
    """The kept rows lie in [lo, new hi) frame by frame, frame_off is the model's, everything outside [lo, old hi) has the bits
    of `before`; [new hi, old hi) is left to the kernel."""
    after = L.snapshot()
    kept = m.soa(m.all_rows(kept_frames))
    new_hi = lo + len(kept['x'])
    exp_off = before['frame_off'].copy()
    exp_off[:len(new_off)] = new_off
    assert np.array_equal(after['frame_off'], exp_off), (after['frame_off'][:len(new_off) + 2], new_off)
    for k in ARRAYS:
        assert m.same_bits(after[k][:lo], before[k][:lo]), (k, 'before the window')
        assert m.same_bits(after[k][old_hi:], before[k][old_hi:]), (k, 'behind the window')
        assert m.same_bits(after[k][lo:new_hi], kept[k]), (k, 'kept points')
    if clean:
        L.st.check_status()
    return after


@pytest.mark.parametrize('name', m.DEDUP_SCENES)
def test_dedup_scenes_match_the_model(name):
    """Windows of 0, 1, 1023, 1024, 1025 and 2049 points, frame boundaries on, before and behind the 1024-point tile, runs of
    empty frames, one voxel, no duplicates, copied frames, probe chains through the table's last slot, the key's range: always
    from slot 1 on at an odd lo, the guard frame holding copies of window points."""
    sc = m.dedup_scene(name)
    sb, se = sc['slot_begin'], sc['slot_end']
    L = Loaded(sc['frames'], evict=sb)
    lo, hi = int(L.off[sb]), int(L.off[se])
    frames, new_off = m.dedup_model(L.rows, L.off, sb, se, sc['size'])
    assert dedup(L, sb, se, sc['size'], sc['max_points'] or max(hi - lo, 1)) == 0, L.lib.pca_last_error(L.ctx.h)
    after = check_dedup(L, L.before, lo, hi, frames, new_off)
    if name in m.DEDUP_KEEPS_ALL:
        assert all(m.same_bits(after[k], L.before[k]) for k in ARRAYS + ('frame_off', ))
    got = L.st.frame_rows()                                      # ... and as the store's own view of its live frames
    assert len(got) == len(frames) and all(np.array_equal(a, b) for a, b in zip(got, frames))


def test_dedup_workspace_that_is_not_256_byte_aligned():
    sc = m.dedup_scene('tile_edges')
    sb, se = sc['slot_begin'], sc['slot_end']
    L = Loaded(sc['frames'], evict=sb)
    lo, hi = int(L.off[sb]), int(L.off[se])
    assert dedup(L, sb, se, sc['size'], hi - lo, shift=8) == 0, L.lib.pca_last_error(L.ctx.h)
    check_dedup(L, L.before, lo, hi, *m.dedup_model(L.rows, L.off, sb, se, sc['size']))


def test_dedup_again_with_the_same_and_with_a_larger_size():
    """DeviceStore.voxel_dedup three times: the second call, same size, changes nothing at all; the third, four times the size,
    gives the model applied to the first call's result."""
    sc = m.dedup_scene('frame_copies')
    sb, se, size = sc['slot_begin'], sc['slot_end'], sc['size']
    L = Loaded(sc['frames'], evict=sb)
    lo, hi = int(L.off[sb]), int(L.off[se])
    frames1, off1 = m.dedup_model(L.rows, L.off, sb, se, size)
    L.st.voxel_dedup(size)
    first = check_dedup(L, L.before, lo, hi, frames1, off1)
    L.st.voxel_dedup(size)
    second = L.snapshot()
    assert all(m.same_bits(second[k], first[k]) for k in ARRAYS + ('frame_off', ))
    rows1 = m.all_rows(L.frames[:sb] + frames1)
    frames2, off2 = m.dedup_model(rows1, off1, sb, se, 4 * size)
    assert 0 < sum(len(f) for f in frames2) < sum(len(f) for f in frames1)
    L.st.voxel_dedup(4 * size)
    check_dedup(L, second, lo, int(off1[se]), frames2, off2)


def test_append_after_a_dedup_lands_at_the_new_end(orc):
    sc = m.dedup_scene('empty_runs')
    sb, se = sc['slot_begin'], sc['slot_end']
    L = Loaded(sc['frames'], evict=sb)
    frames, new_off = m.dedup_model(L.rows, L.off, sb, se, sc['size'])
    L.st.voxel_dedup(sc['size'])
    rng = np.random.default_rng(3)
    n, ncam, H, W = 20, 2, 8, 12
    pc = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-2, 4, n), rng.integers(0, 256, n).astype(float),
                   rng.uniform(1.01, W - 1.01, n), rng.uniform(1.01, H - 1.01, n), rng.integers(-1, 5, n).astype(float)], 1)
    cam = rng.integers(0, ncam, n)
    imgs, sems = rng.integers(0, 256, (ncam, H, W, 3), dtype=np.uint8), rng.integers(0, 19, (ncam, H, W)).astype(np.uint8)
    Tw = m.transforms(rng, 1)[0]
    x_ptr = L.st.x.data_ptr()
    L.st.append_nusc(*(L.torch.from_numpy(a).cuda() for a in (pc, cam, imgs, sems)), Tw, [])
    ost = orc.Store(64)
    assert orc.nusc_sample_filter_transform(ost, pc, cam, imgs, sems, Tw, []) == n
    assert L.st.x.data_ptr() == x_ptr                            # (the store had room: nothing was moved)
    assert L.st.offsets().tolist() == new_off[sb:se + 1].tolist() + [int(new_off[se]) + n]
    assert np.array_equal(L.st.rows(), np.concatenate([m.all_rows(frames), ost.rows()]))
    after, lo, hi = L.snapshot(), int(L.off[sb]), int(L.off[se])
    assert int(new_off[se]) + n <= hi                            # (the new frame lies inside the old window)
    assert all(m.same_bits(after[k][:lo], L.before[k][:lo]) and m.same_bits(after[k][hi:], L.before[k][hi:]) for k in ARRAYS)
    assert np.array_equal(after['frame_off'][se + 2:], L.before['frame_off'][se + 2:])
    L.st.check_status()


def test_dedup_window_above_max_points_reports_the_overflow():
    """Nothing is asserted inside the old window; outside it, and in frame_off outside [slot_begin + 1, slot_end], no bit moves."""
    sc = m.dedup_scene('tile_edges')
    sb, se = sc['slot_begin'], sc['slot_end']
    L = Loaded(sc['frames'], evict=sb)
    lo, hi = int(L.off[sb]), int(L.off[se])
    assert dedup(L, sb, se, sc['size'], 1500) == 0, L.lib.pca_last_error(L.ctx.h)
    after = L.snapshot()
    for k in ARRAYS:
        assert m.same_bits(after[k][:lo], L.before[k][:lo]) and m.same_bits(after[k][hi:], L.before[k][hi:]), k
    assert np.array_equal(after['frame_off'][:sb + 1], L.before['frame_off'][:sb + 1])
    assert np.array_equal(after['frame_off'][se + 1:], L.before['frame_off'][se + 1:])
    with pytest.raises(RuntimeError, match='overflow'):
        L.st.check_status()


@pytest.mark.parametrize('what', ['size 0', 'negative size', 'NaN size', 'workspace one byte short'])
def test_dedup_refusals_write_nothing(what):
    sc = m.dedup_scene('n1025')
    sb, se = sc['slot_begin'], sc['slot_end']
    L = Loaded(sc['frames'], evict=sb)
    size = {'size 0': 0.0, 'negative size': -1.0, 'NaN size': float('nan')}.get(what, sc['size'])
    assert dedup(L, sb, se, size, 1025, short=1 if what.startswith('workspace') else 0) == -1
    assert L.lib.pca_last_error(L.ctx.h)
    L.check(L.expected())
