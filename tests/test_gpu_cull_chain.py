"""The frame-culling chain against the oracle, link by link (a mistake anywhere in it does not crash: it silently leaves points
out of a BEV).  K1 leaves a per-frame f32 box in pca_store.frame_box; DeviceStore reads it back and keeps _then / _box /
_has_cone / _moved; pca_bev_view_hint turns that into a slot range in the context (pca_bev_bin_range); level 1 of the raster then
reads frame_off[bin_first] .. frame_off[bin_end] only.

  C  K1's boxes against min / max of the ORACLE's kept rows, per form of K1, slot row by slot row.
  B  pca_bev_bin_range at the kernel level against the oracle's raster of the sub-window; what level 1 was launched with is read
     through pca_debug_bev_level1.
  A  the shipped KITTI launch structure (deferred K1, view hints, owed chains, slides, a camera change, per-point labels) against
     orc.bev on the oracle's own store, raster by raster.
No test here compares one HIP path with another as its proof."""
import ctypes as C
import gc

import numpy as np
import pytest

import cull_chain_common as cc
import k1_edges_common as kc
from test_gpu_dropin import BEV_KITTI, KITTI_FILTERS, SEM_IDXS
from test_gpu_k1_edges import dev_frame, oracle_rows
from test_gpu_kernels import CAM_TO_VELO, DYNOBJ, _tilting_transform, assert_planes_match, cu, dev_store

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def level1(ctx):
    """(G, Gk, bin_first, bin_end) of the context's last raster (pca_debug_bev_level1)."""
    out = (C.c_int * 4)()
    assert ctx.lib.pca_debug_bev_level1(ctx.h, out) == 0
    return tuple(out)


# =========================================================================================================== C: K1's frame boxes
def boxes(st, first, n):
    """Rows [first, first + n) of st.frame_box, raw (u32) and decoded (f32 [n, 6]).  Reads the tensor only: no library call that
    would run a noted K1."""
    raw = np.ascontiguousarray(st.frame_box[first:first + n].cpu().numpy().view(np.uint32))
    dec = np.full((n, 6), np.nan, np.float32)
    st.ctx.lib.pca_f32_box_decode(raw.ctypes.data_as(C.c_void_p), n, dec.ctypes.data_as(C.c_void_p))
    return raw, dec


def check_boxes(st, wants, name, first=None):
    """The box rows of the frames whose oracle rows are `wants` (slots from `first`, default the store's head) against the
    expected boxes, bit for bit; a frame of which nothing is kept decodes to lo > hi; every other row of the table is zero."""
    first = st.head if first is None else first
    raw, dec = boxes(st, first, len(wants))
    for f, rows in enumerate(wants):
        want = cc.box_of_rows(rows)
        if want is None:
            assert not raw[f].any() and (dec[f, 0::2] > dec[f, 1::2]).all(), (name, f)
        else:
            assert np.array_equal(dec[f].view(np.uint32), want.view(np.uint32)), (name, f, dec[f], want)
            assert (dec[f] == want).all() or np.isnan(want).any(), (name, f)
    table = st.frame_box.cpu().numpy()
    assert not table[:first].any() and not table[first + len(wants):].any(), name
    assert table.shape[0] > first + len(wants)                      # (there are such rows)


def synthetic_want(orc, name):
    """The oracle's rows of a synthetic frame: computed once, shared, never written to."""
    key = ('syn', name)
    from test_gpu_k1_edges import _want
    if key not in _want:
        pts, P, sem_gt = cc.synthetic_frame(name)
        img, sem = cc.synthetic_images(name)
        ost = orc.Store(len(pts))
        orc.kitti_project_sample_filter(ost, pts, P, None if sem_gt is not None else img, None if sem_gt is not None else sem, sem_gt,
                                        cc.SYN_H, cc.SYN_W, KITTI_FILTERS)
        rows = ost.rows()
        rows.setflags(write=False)
        _want[key] = rows
    return _want[key]


def synthetic_dev(T, name):
    pts, P, sem_gt = cc.synthetic_frame(name)
    if sem_gt is not None:
        return dict(pts=cu(T, pts), sem_gt=cu(T, sem_gt)), P, 1, 1
    img, sem = cc.synthetic_images(name)
    return dict(pts=cu(T, pts), rgb=cu(T, img), sem=cu(T, sem)), P, cc.SYN_H, cc.SYN_W


def test_the_synthetic_frames_are_what_their_names_say(orc):
    n = {name: len(synthetic_want(orc, name)) for name in cc.SYNTHETIC}
    assert n['none_kept'] == 0 and n['one_kept'] == 1 and n['all_negative'] > 1000 and n['zeros_denormals'] > 1000 and n['huge'] > 1000
    assert (synthetic_want(orc, 'all_negative')[:, :3] < 0).all()
    z = synthetic_want(orc, 'zeros_denormals')[:, :3].astype(np.float32)
    assert np.signbit(z[:, 2]).all() and (np.abs(z) < 1.2e-38).all() and (z[:, 0] == np.float32(1e-45)).any()
    assert (np.abs(synthetic_want(orc, 'huge')[:, 2]) > 1e35).sum() > 1000


@pytest.mark.parametrize('sample_mode', ['nearest', 'bilinear'])
@pytest.mark.parametrize('name', kc.CASES)
def test_box_fused_one_frame_of_several_tiles(T, orc, name, sample_mode):
    """FUSED, one frame of 14 tiles of 1024 points, the last one partial (507): per lane, per wave, through LDS, then the global
    atomic maximum -- in a slot behind the head (first_slot = 1), nearest and bilinear sampling."""
    fr = kc.frame(name)
    want = oracle_rows(orc, name, bilinear=sample_mode == 'bilinear')
    st = dev_store(capacity=2 * len(fr.pts), max_frames=4)
    f = dev_frame(T, fr)
    st.append_kitti([f], fr.P, fr.H, fr.W, fr.filters, sample_mode=sample_mode)
    st.append_kitti([f], fr.P, fr.H, fr.W, fr.filters, sample_mode=sample_mode)
    st.check_status()
    assert st.sizes().tolist() == [len(want)] * 2
    check_boxes(st, [want, want], (name, sample_mode))


@pytest.mark.parametrize('name', cc.SYNTHETIC)
def test_box_fused_synthetic_frames(T, orc, name):
    """Nothing kept (the row stays zero: lo > hi), one kept point (lo = hi), all-negative coordinates, -0.0 and denormals among
    the kept points (bit for bit: -0.0 is below +0.0), coordinates of 1e35 that the reference keeps."""
    f, P, H, W = synthetic_dev(T, name)
    want = synthetic_want(orc, name)
    st = dev_store(capacity=4096, max_frames=4)
    st.append_kitti([f], P, H, W, KITTI_FILTERS)
    st.check_status()
    assert np.array_equal(st.rows().view(np.uint64), want.view(np.uint64))
    check_boxes(st, [want], name)


@pytest.mark.parametrize('name', kc.CASES)
def test_box_fused_ragged_batch_every_frame_in_its_own_row(T, orc, name):
    """The composition of test_k1_edges_ragged_batch (empty, head, one point, tail, one full tile) in ONE call behind a frame
    stored before (first_slot = 1): every frame's box in its OWN slot row -- first_slot + its index in the batch --, the empty
    frame's row and the rows of the slots never written all zero."""
    fr = kc.frame(name)
    fam = fr.of('u_hi')
    fam = fam[fam >= 700]
    cut = int(fam[len(fam) // 2])
    kept = np.intersect1d(fr.of('ladder_e36'), kc.fixture(name)['kept'])
    pieces = {'empty': fr.pts[:0], 'one': fr.pts[kept[:1]], 'head': fr.pts[:cut], 'tail': fr.pts[cut:], 'tile': fr.pts[1000:1000 + 1024]}
    order = ['empty', 'head', 'one', 'tail', 'tile']
    wants = [oracle_rows(orc, name, pieces[k], key='tile1024' if k == 'tile' else k) for k in order]
    assert [len(w) for w in wants[:3:2]] == [0, 1]
    st = dev_store(capacity=3 * len(fr.pts), max_frames=8)
    st.append_kitti([dev_frame(T, fr, pieces['one'])], fr.P, fr.H, fr.W, fr.filters)
    st.append_kitti([dev_frame(T, fr, pieces[k]) for k in order], fr.P, fr.H, fr.W, fr.filters)
    st.check_status()
    wants = [wants[2]] + wants
    assert st.sizes().tolist() == [len(w) for w in wants]
    check_boxes(st, wants, name)


@pytest.mark.parametrize('name', kc.CASES)
def test_box_fused_per_point_labels(T, orc, name):
    """use_gt_sem: no projection and no cull, so inf and NaN are kept -- the box is then the extreme of the encoding's order (a
    NaN bound: pca_host_view_hull takes a number that is not finite as proof of nothing)."""
    fr = kc.frame(name)
    sem_gt = np.random.default_rng(fr.seed + 1).integers(0, 19, len(fr.pts)).astype(np.uint8)
    want = oracle_rows(orc, name, sem_gt=sem_gt)
    st = dev_store(capacity=len(fr.pts), max_frames=4)
    st.append_kitti([dict(pts=cu(T, fr.pts), sem_gt=cu(T, sem_gt))], fr.P, 1, 1, fr.filters)
    st.check_status()
    assert st.sizes().tolist() == [len(want)] and np.isnan(want[:, :3]).any()
    check_boxes(st, [want], name)


@pytest.mark.parametrize('name', kc.CASES + ('syn:none_kept', 'syn:one_kept', 'syn:all_negative', 'syn:huge'))
def test_box_of_a_k1_riding_in_the_raster(T, orc, name):
    """pca_k1_defer: append_kitti_obs only notes the frame's K1 -- its row is still zero --, the raster that follows runs it as
    its first workgroups (1024 x 4 tiles) and the row is the box of the oracle's kept rows; in slot 1, behind a frame stored
    before, whose row does not change."""
    from pca_amd import _lib
    from pca_amd.device_store import make_bev_params
    if name.startswith('syn:'):
        f, P, H, W = synthetic_dev(T, name[4:])
        want, n = synthetic_want(orc, name[4:]), len(cc.synthetic_frame(name[4:])[0])
    else:
        fr = kc.frame(name)
        f, P, H, W, want, n = dev_frame(T, fr), fr.P, fr.H, fr.W, oracle_rows(orc, name), len(fr.pts)
    st = dev_store(capacity=2 * n, max_frames=4)
    st.append_kitti([f], P, H, W, KITTI_FILTERS)
    prm = make_bev_params((0., 0., 0.), np.eye(3), 0., 0., 40., 64, None, 20., 20., 0.5, 0, DYNOBJ, False)
    st.set_defer_k1(True)
    try:
        o = _lib.PcaKittiObs()
        o.pts, o.rgb, o.sem, o.sem_gt, o.n, o.host_mask = f['pts'].data_ptr(), f['rgb'].data_ptr(), f['sem'].data_ptr(), None, n, 0
        st.ctx.profile(True)
        st.append_kitti_obs(o, P, H, W, KITTI_FILTERS, keep=f)
        before = st.frame_box.cpu().numpy().copy()
        st.bev(1, prm)
        launches = st.ctx.profile_read()['kitti_project_sample_filter'][1]
        st.ctx.profile(False)
        grid = level1(st.ctx)
    finally:
        st.set_defer_k1(False)
    assert not before[1:].any()                               # noted, not run: still zero
    assert launches == 0 and grid[1] == -(-n // 4096)         # (no K1 launch since profiling began: it rode, as that many tiles)
    st.check_status()
    assert st.sizes().tolist() == [len(want)] * 2
    check_boxes(st, [want, want], name)


@pytest.mark.parametrize('form', ['one_frame', 'batch'])
def test_box_rows_stay_zero_in_the_split_form(T, orc, monkeypatch, form):
    """PCA_K1_MODE=split writes no box: the rows stay zero and decode as unknown (such a frame always counts as visible).
    DeviceStore._poll_boxes relies on exactly that; whoever fills them later has to fill them right."""
    monkeypatch.setenv('PCA_K1_MODE', 'split')
    fr = kc.frame('axis')
    want = oracle_rows(orc, 'axis')
    k = 1 if form == 'one_frame' else 3
    st = dev_store(capacity=k * len(fr.pts), max_frames=4)
    st.append_kitti([dev_frame(T, fr)] * k, fr.P, fr.H, fr.W, fr.filters)
    st.check_status()
    assert st.sizes().tolist() == [len(want)] * k and len(want) > 1000
    raw, dec = boxes(st, 0, st.frame_box.shape[0])
    assert not raw.any() and (dec[:, 0::2] > dec[:, 1::2]).all()


# ====================================================================================================== B: pca_bev_bin_range
VIEW, PX, INTS, SPLIT = 32., 64, (1., 30., 0.12), 3
_frames, _planes = {}, {}


def window(key='small'):
    if key not in _frames:
        fr = cc.window_frames() if key == 'small' else cc.window_frames(8, 37300, 75, seed=7)      # ('one_round': 300 500 points)
        for r in fr:
            r.setflags(write=False)
        _frames[key] = fr
    return _frames[key]


def bev_args(px=PX):
    return ((0.25, -0.125, 0.0625), np.eye(3), 0., 0., VIEW, px, None, *INTS, 0, DYNOBJ, True)


def oracle_window(orc, frames, lo, hi, split, px=PX, key=None):
    """orc.bev on the rows of frames [lo, hi) only, 'present' = those before `split`: computed once per key, never written to."""
    k = (key, lo, hi, split, px)
    if key is None or k not in _planes:
        sub = list(frames[lo:hi]) if hi > lo else []
        rows = np.concatenate(sub) if sub else np.zeros((0, 10))
        n_present = int(sum(len(r) for r in frames[lo:min(max(split, lo), hi)]))
        ref = orc.bev(orc.Store.from_rows(rows, intensity_div255=True), n_present, orc.make_bev_params(*bev_args(px)))
        for v in ref.values():
            v.setflags(write=False)
        if key is None:
            return ref
        _planes[k] = ref
    return _planes[k]


def loaded_store(frames, **kw):
    st = dev_store(capacity=sum(len(r) for r in frames) + kw.pop('room', 0), max_frames=kw.pop('max_frames', 16), intensity_div255=True)
    assert st.load_rows(list(frames)) is None
    st.cull = False                                           # view_hint leaves the context alone: the range below is the only one
    return st


def ranged_bev(st, f, e, split, prm, **kw):
    """pca_bev_bin_range(head + f, head + e) directly in front of st.bev; returns the planes and what level 1 was launched with."""
    ctx = st.ctx
    assert ctx.lib.pca_bev_bin_range(ctx.h, st.head + f, st.head + e) == 0
    p16, p64 = st.bev(split, prm, want_f64=True, **kw)
    grid = level1(ctx)
    st.check_status()
    return p16.cpu().numpy(), p64.cpu().numpy(), grid


RANGES = [(0, 8), (2, 6), (0, 3), (3, 8), (4, 6), (1, 2), (5, 5), (-3, 20), (6, 2)]


@pytest.mark.parametrize('f,e', RANGES)
def test_bin_range_rasters_the_sub_window(T, orc, f, e):
    """Every frame lies inside the view, so honouring the range visibly changes the planes: full window, a range that straddles
    the present / future split, present only, future only, the split before the range (w.sp < w.lo: everything is future), the
    split behind it (everything is present), an empty range (the planes of an empty window), a range clipped to the window, and
    one that pca_bev_bin_range marks invalid (end before begin: the full window)."""
    from pca_amd.device_store import make_bev_params
    frames = window()
    st = loaded_store(frames)
    lo, hi = (0, 8) if e < f else (max(f, 0), max(min(e, 8), max(f, 0)))
    p16, p64, grid = ranged_bev(st, f, e, SPLIT, make_bev_params(*bev_args()))
    assert grid[1:] == (0, st.head + lo, st.head + hi), grid
    ref = oracle_window(orc, frames, lo, hi, SPLIT, key='small')
    if (lo, hi) != (0, 8):
        full = oracle_window(orc, frames, 0, 8, SPLIT, key='small')['planes']
        assert not np.array_equal(full[14:21], ref['planes'][14:21])          # (the range matters)
    assert_planes_match(p16, p64, ref, f'range {f}..{e}')


def test_bin_range_is_clipped_to_the_rasterised_frames_and_good_for_one_call(T, orc):
    """first_frame = 1, last_frame = 7 with the range (0, 8): clipped to the rasterised frames.  The range is good for ONE call:
    the next raster without one sees the full window."""
    from pca_amd.device_store import make_bev_params
    frames = window()
    st = loaded_store(frames)
    prm = make_bev_params(*bev_args())
    p16, p64, grid = ranged_bev(st, 0, 8, SPLIT, prm, first_frame=1, last_frame=7)
    assert grid[2:] == (1, 7)
    assert_planes_match(p16, p64, oracle_window(orc, frames, 1, 7, SPLIT, key='small'), 'clipped to 1..7')
    p16, p64, grid = ranged_bev(st, 2, 6, SPLIT, prm)
    assert grid[2:] == (2, 6)
    assert_planes_match(p16, p64, oracle_window(orc, frames, 2, 6, SPLIT, key='small'), 'range 2..6')
    p16, p64 = st.bev(SPLIT, prm, want_f64=True)
    assert level1(st.ctx)[2:] == (0, 8)
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), oracle_window(orc, frames, 0, 8, SPLIT, key='small'), 'after a ranged call')


def test_bev_many_ignores_a_bin_range_and_forgets_it(T, orc):
    """A range set before bev_many (pca_bev_generate_many) is for a single raster: both jobs see their whole windows, and the
    single raster after it sees no range either."""
    from pca_amd.device_store import make_bev_params
    from test_gpu_bev_edges import assert_f16_matches_oracle
    frames = window()
    st = loaded_store(frames)
    prm = make_bev_params(*bev_args())
    assert st.ctx.lib.pca_bev_bin_range(st.ctx.h, st.head + 2, st.head + 6) == 0
    out = T.empty((2, 21, PX, PX), dtype=T.float16, device='cuda')
    st.bev_many([(SPLIT, prm, 0, None), (SPLIT, prm, 1, 7)], out)
    st.check_status()
    out = out.cpu().numpy()
    assert_f16_matches_oracle(out[0], oracle_window(orc, frames, 0, 8, SPLIT, key='small'), 'job 0')
    assert_f16_matches_oracle(out[1], oracle_window(orc, frames, 1, 7, SPLIT, key='small'), 'job 1')
    p16, p64 = st.bev(SPLIT, prm, want_f64=True)
    assert level1(st.ctx)[2:] == (0, 8)
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), oracle_window(orc, frames, 0, 8, SPLIT, key='small'), 'after bev_many')


def owed_frames(orc, frames, Ts, ends):
    """The frames after transforms Ts, transform k owed by frames [0, ends[k]) (the oracle's K2, one pass per transform)."""
    out = []
    for f, rows in enumerate(frames):
        ost = orc.Store.from_rows(rows, intensity_div255=True)
        for Tm, end in zip(Ts, ends):
            if f < end:
                orc.retransform(ost, Tm)
        out.append(ost.rows())
    return out


def owe(st, Ts, ends):
    for Tm, end in zip(Ts, ends):
        st.retransform(Tm, defer=True)
        st._pending[-1] = (st._pending[-1][0], st.head + end)     # frames from `end` on came after it


@pytest.mark.parametrize('ends', [(8, ), (8, 8), (1, 4, 8)])
def test_bin_range_with_owed_transforms_that_stay_owed(T, orc, ends):
    """One, two and three owed transforms that change z, not written back, with the range (2, 6): the planes are the oracle's of
    the TRANSFORMED sub-window.  The slot ends lie outside the range -- beyond its end (8), and, in the chain of three, before its
    begin (frame 0 alone owes the oldest: pend_hi below w.lo) and inside it (4).  Afterwards the stored coordinates are
    unchanged and the chain is still owed."""
    from pca_amd.device_store import make_bev_params
    frames = window()
    st = loaded_store(frames)
    st.CHAIN_K = 4
    Ts = [_tilting_transform(s) for s in range(len(ends))]
    owe(st, Ts, ends)
    p16, p64, grid = ranged_bev(st, 2, 6, SPLIT, make_bev_params(*bev_args()))
    assert grid[1:] == (0, 2, 6)
    moved = owed_frames(orc, frames, Ts, ends)
    assert not np.array_equal(moved[3][:, 2], frames[3][:, 2])
    assert_planes_match(p16, p64, oracle_window(orc, moved, 2, 6, SPLIT), f'owed {ends}')
    assert len(st._pending) == len(ends)
    stored = np.stack([t[:st.ub_tail].cpu().numpy() for t in (st.x, st.y, st.z)], 1)
    assert np.array_equal(stored, np.concatenate(frames)[:, :3])
    assert np.array_equal(st.rows(), np.concatenate(moved))  # (and K2 then applies what is owed: the oracle's rows)


@pytest.mark.parametrize('ends', [(8, 8, 8, 8), (1, 4, 6, 8)])
def test_a_raster_that_writes_back_ignores_the_range(T, orc, ends):
    """The fourth owed transform makes the raster write back.  A frame left out could not receive what it owes, so with the range
    (2, 6) set the call bins the FULL window (bev_decide_bin_range): full-window planes, and afterwards every frame's stored rows
    -- 0, 1, 6 and 7 included -- are the eagerly re-transformed ones."""
    from pca_amd.device_store import make_bev_params
    frames = window()
    st = loaded_store(frames)
    st.CHAIN_K = 4
    Ts = [_tilting_transform(s) for s in range(4)]
    owe(st, Ts, ends)
    p16, p64, grid = ranged_bev(st, 2, 6, SPLIT, make_bev_params(*bev_args()))
    assert st._pending == []
    moved = owed_frames(orc, frames, Ts, ends)
    assert_planes_match(p16, p64, oracle_window(orc, moved, 0, 8, SPLIT), f'write-back {ends}')
    stored = np.stack([t[:st.ub_tail].cpu().numpy() for t in (st.x, st.y, st.z)], 1)      # (read directly: nothing is owed any more)
    want = np.concatenate(moved)
    off = np.concatenate([[0], np.cumsum([len(r) for r in frames])])
    for f in range(8):
        assert np.array_equal(stored[off[f]:off[f + 1]], want[off[f]:off[f + 1], :3]), f
    assert np.array_equal(st.rows(), want)
    assert grid[1:] == (0, 0, 8), grid                        # (and level 1 was launched over the whole window)
    p16, p64, grid = ranged_bev(st, 2, 6, SPLIT, make_bev_params(*bev_args()))           # and the range counts again
    assert grid[1:] == (0, 2, 6)
    assert_planes_match(p16, p64, oracle_window(orc, moved, 2, 6, SPLIT), 'after the write-back')


@pytest.mark.parametrize('f,e', [(2, 6), (5, 5)])
@pytest.mark.parametrize('route', ['memory_path', 'intensity64', 'banded'])
def test_bin_range_on_the_other_routes(T, orc, monkeypatch, route, f, e):
    """The range on the routes that share level 1's window but differ in how they walk it: the memory path of pass B (one
    workgroup, PCA_BEV_G=1: the 13 300 points of frames 2..5 exceed the 12 288 of the registers), f64 intensities (24-byte
    records, no register path) and a banded grid (px = 1032: the range applies to every band)."""
    from pca_amd.device_store import make_bev_params
    frames = window()
    assert sum(len(r) for r in frames[2:6]) > 12288
    if route == 'memory_path':
        monkeypatch.setenv('PCA_BEV_G', '1')
    px = 1032 if route == 'banded' else PX
    st = loaded_store(frames)
    kw = {}
    if route == 'intensity64':                               # the very values the store holds, through the side channel
        kw['intensity64'] = T.from_numpy(np.ascontiguousarray(np.concatenate(frames)[:, 3])).cuda()
    p16, p64, grid = ranged_bev(st, f, e, SPLIT, make_bev_params(*bev_args(px)), **kw)
    assert grid[1:] == (0, f, e) and (route != 'memory_path' or grid[0] == 1)
    assert_planes_match(p16, p64, oracle_window(orc, frames, f, e, SPLIT, px=px, key='small'), f'{route} {f}..{e}')


P_CULL = np.array([[130.0, 0, 160.0, 0], [0, 130.0, 48.0, 0], [0, 0, 1, 0]]) @ np.linalg.inv(CAM_TO_VELO)
H_CULL, W_CULL = 96, 320


def test_a_riding_k1_is_binned_whatever_the_range_says(T, orc):
    """THE CONTRACT: the frame whose K1 rides in the raster is binned from K1's registers, not from the store, so a bin range that
    excludes the newest slot does not exclude it (window_end clips only the store's part of the window).  Range (2, 6) of a
    window of 9 whose ninth frame rides and lies inside the view: the planes are those of frames 2..5 PLUS the newest.  The view
    hull never leaves a visible frame out, so nothing the product computes depends on this -- but a caller of pca_bev_bin_range
    must know it."""
    from pca_amd import _lib
    from pca_amd.device_store import make_bev_params
    frames = window()
    rng = np.random.default_rng(31)
    n = 9000
    pc = np.stack([rng.uniform(0.5, 15, n), rng.uniform(-12, 12, n), rng.uniform(-2, 3, n), rng.integers(0, 256, n)], 1).astype(np.float32)
    img = rng.integers(0, 256, (H_CULL, W_CULL, 3), dtype=np.uint8)
    sem = rng.integers(0, 19, (H_CULL, W_CULL)).astype(np.uint8)
    ost = orc.Store(n, intensity_div255=True)
    orc.kitti_project_sample_filter(ost, pc, P_CULL, img, sem, None, H_CULL, W_CULL, KITTI_FILTERS)
    newest = ost.rows()
    assert len(newest) > 1000
    st = loaded_store(frames, room=n)
    f = dict(pts=cu(T, pc), rgb=cu(T, img), sem=cu(T, sem))
    st.set_defer_k1(True)
    try:
        o = _lib.PcaKittiObs()
        o.pts, o.rgb, o.sem, o.sem_gt, o.n, o.host_mask = f['pts'].data_ptr(), f['rgb'].data_ptr(), f['sem'].data_ptr(), None, n, 0
        st.append_kitti_obs(o, P_CULL, H_CULL, W_CULL, KITTI_FILTERS, keep=f)
        assert st.n_frames == 9 and st.head == 0
        p16, p64, grid = ranged_bev(st, 2, 6, SPLIT, make_bev_params(*bev_args()))
    finally:
        st.set_defer_k1(False)
    assert grid[1:] == (-(-n // 4096), 2, 6), grid            # it rode, and the store's part was cut to the range
    ref = oracle_window(orc, list(frames[2:6]) + [newest], 0, 5, 1)
    assert_planes_match(p16, p64, ref, 'riding K1 + range')
    assert np.array_equal(st.rows(8), newest)


def test_one_round_launch_sized_by_a_stale_point_count(T, orc, monkeypatch):
    """With a bin range level 1 is launched as ONE round of workgroups (G = the device's compute units) when the previous ranged
    call binned few points; the count comes from the device and only sizes the launch.  300 000 points in 8 frames under
    PCA_BEV_CHUNK=1024 (G = 293 > 256 without it): the first ranged call primes the count, the second is sized by it, the third
    bins a range of six times as many points with a launch sized by the second's count.  All three are the sub-window's oracle."""
    from pca_amd.device_store import make_bev_params
    monkeypatch.setenv('PCA_BEV_CHUNK', '1024')
    frames = window('one_round')
    n_cu = T.cuda.get_device_properties(0).multi_processor_count
    assert 256 <= n_cu < sum(len(r) for r in frames) // 1024 <= 512
    st = loaded_store(frames)
    prm = make_bev_params(*bev_args())
    grids = []
    for f, e in ((2, 3), (2, 3), (1, 7)):
        p16, p64, grid = ranged_bev(st, f, e, SPLIT, prm)
        grids.append(grid)
        assert grid[1:] == (0, f, e)
        assert_planes_match(p16, p64, oracle_window(orc, frames, f, e, SPLIT, key='one_round'), f'one round {f}..{e}')
    assert grids[1][0] == n_cu and grids[2][0] == n_cu, grids
    p16, p64 = st.bev(SPLIT, prm, want_f64=True)             # without a range: the grid of the whole window again
    assert level1(st.ctx)[0] == sum(len(r) for r in frames) // 1024 + 1
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), oracle_window(orc, frames, 0, 8, SPLIT, key='one_round'), 'no range')


# ============================================================================ A: the shipped launch structure, raster by raster
N_CULL = 6000


def T_of(k):
    """~1 m steps on a curve that turns left, then right, with a little tilt (test_frames_that_cannot_reach_the_view_...)."""
    from pca_amd import host_logic as hl
    yaw = 0.03 * np.sin(k / 9.0) + 0.01
    pitch = 0.004 * np.cos(k / 5.0)
    Rp = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
    Tm = np.eye(4)
    Tm[:3, :3] = Rp @ hl.rotation_matrix_3d(yaw)
    Tm[:3, 3] = [-(0.8 + 0.4 * ((k * 7) % 5) / 5.0), 0.02 * np.sin(k), 0.003]
    return Tm


@pytest.mark.parametrize('scenario', ['camera', 'labels', 'mixed'])
def test_shipped_kitti_launch_structure_step_by_step_against_the_oracle(T, orc, monkeypatch, scenario):
    """The KITTI drop-in with its defaults -- K1 noted by integrate() and riding in the raster, rasters told which frames cannot
    reach the view, fast calls -- on a stream where frames really are culled: a 24 m view inside a 60 m horizon on a winding,
    tilting path, boxes read back every second frame, a store small enough to slide, a raster on two steps of three (owed chains
    of 1..4 transforms).  150 steps; EVERY raster's 21 planes and three polylines against orc.bev / the numpy polyline code on
    the oracle's own store and track; stored rows, poses and evictions at the end.
      camera  the camera's class map (cone + boxes), host and device point arrays in turn
      labels  per-point labels (no cone: boxes only)
      mixed   a 20-frame integrate_many warm-up (frames without a `then`: always visible), another camera at step 60 (the frames
              before it lose their cone), per-point labels from step 100 (frames with and without a cone in one window)
    and the proof that the mechanisms engaged (hints taken, every chain length, a write-back while a hint was available and the
    full window binned by it, boxes landed, a slide, K1 riding)."""
    import sem_pc_accum
    from kitti360_sem_pc_accum import Kitti360SemanticPointCloudAccumulator
    from pca_amd import host_logic as hl
    from pca_amd.device_store import DeviceStore, make_bev_params
    H, W, N = H_CULL, W_CULL, N_CULL
    P1 = P_CULL
    P2 = np.array([[95.0, 0, 160.0, 0], [0, 95.0, 48.0, 0], [0, 0, 1, 0]]) @ np.linalg.inv(CAM_TO_VELO)
    rng = np.random.default_rng(12)
    monkeypatch.setattr(DeviceStore, 'BOX_EVERY', 2)

    def frame():
        pc = np.stack([rng.uniform(-25, 25, N), rng.uniform(-25, 25, N), rng.uniform(-2, 3, N), rng.uniform(0, 1, N)], 1).astype(np.float32)
        return pc, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 19, (H, W)).astype(np.uint8)
    frames = [frame() for _ in range(5)]
    by_id = {id(f[1]): f[2] for f in frames}

    class Resident:
        def pred(self, rgb):
            return by_id[id(rgb)][None, None]
    monkeypatch.setattr(sem_pc_accum, 'SemSegONNX', lambda path: Resident())
    horizon, view, px = 60., 24, 64
    use_gt = scenario == 'labels'
    calib = {'h_velo_cam': None, 'p_cam_frame': None, 'p_velo_frame': P1}
    gc.collect()                                              # (a dying store of an earlier test would run the context's noted K1)
    acc = Kitti360SemanticPointCloudAccumulator(horizon, calib, 1e3, 'resident', KITTI_FILTERS, SEM_IDXS, use_gt,
                                                dict(BEV_KITTI, view_size=view, pixel_size=px))
    acc._store_args = dict(capacity=1 << 19, max_frames=48)
    assert acc._defer_k1 and acc._fast and acc.store.cull     # the defaults
    warm = 20 if scenario == 'mixed' else 0
    Ts = [T_of(k) for k in range(warm + 150)]
    it = iter(Ts)
    acc.pose_provider = lambda pc: next(it)
    store, ctx = acc.store, acc.store.ctx

    ost, track = orc.Store(1 << 20), hl.PoseTrack()
    state = dict(sizes=[], lo=0, P=P1, gt=use_gt)

    def labels_of(k):
        return (np.arange(N)[:, None] * 7 + k) % 19

    def oracle_step(k):
        pc, img, sem = frames[k % 5]
        if len(track):
            track.apply_transform(Ts[k])
            orc.retransform(ost, Ts[k], state['lo'], ost.n)
        if state['gt']:
            m = orc.kitti_project_sample_filter(ost, pc, state['P'], None, None, labels_of(k).astype(np.uint8), H, W, KITTI_FILTERS)
        else:
            m = orc.kitti_project_sample_filter(ost, pc, state['P'], img, sem, None, H, W, KITTI_FILTERS)
        state['sizes'].append(m)
        track.append([0., 0., 0.])
        ev = 0
        if len(track) > 1:
            ev = track.evict_beyond(horizon, track.push_segment())
            state['lo'] += int(np.sum(state['sizes'][:ev]))
            state['sizes'] = state['sizes'][ev:]
        return ev

    removed_dev, removed_orc = [], []
    if warm:
        removed_dev += acc.integrate_many([[(frames[k % 5][1], frames[k % 5][0], None)] for k in range(warm)])
        removed_orc += [oracle_step(k) for k in range(warm)]
    chains, rode, rasters, heads, slides = set(), [], 0, [store.head], 0
    hinted_ranges, write_back_with_hint = 0, 0
    first, last = C.c_int(0), C.c_int(0)
    for k in range(warm, warm + 150):
        if scenario == 'mixed' and k == warm + 60:
            acc.P_velo_frame = state['P'] = P2
        if scenario == 'mixed' and k == warm + 100:
            acc.use_gt_sem = state['gt'] = True
        pc, img, sem = frames[k % 5]
        pts = pc if k % 2 else T.from_numpy(pc).cuda()
        removed_dev.append(acc.integrate([(img, pts, labels_of(k) if state['gt'] else None)]))
        removed_orc.append(oracle_step(k))
        if store.head < heads[-1]:                            # the window slid to the front: head went back to 0 inside integrate(),
            assert store.head == removed_dev[-1]              # and the step's eviction then advanced it from there
            slides += 1
        heads.append(store.head)
        d = track.incr()
        if not (len(d) > 3 and d[-1] > 22.0 and k % 3 != 2):  # (a step without a raster now and then: longer owed chains)
            continue
        pidx = min(max(int(((d - (d[-1] - 20.0)) > 0).argmax()), 1), len(d) - 2)       # the pose ~20 m of path behind the newest
        poses = np.array(track.poses)
        origin = poses[pidx]
        R = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:pidx] - origin))
        args = (origin, R, 0., 0., view, px, None, 20., 20., 0.5, 0, [13, 14, 15, 17], False)
        n_owed, n = len(store._pending), store.n_frames
        assert n == len(track)
        chains.add(n_owed)
        # what the hull says for this raster, from the store's own tables (the hint the call is about to be offered)
        a = store.head
        cone = store._cone[2] if (store._cone is not None and store._n_nocone == 0) else None
        dprm = make_bev_params(*args)
        assert ctx.lib.pca_host_view_hull(n, store._then_addr + 96 * a, store._box_addr + 24 * a, cone, store._moved.ctypes.data,
                                          C.addressof(dprm), C.byref(first), C.byref(last)) == 0
        narrower = not (first.value == 0 and last.value == n - 1)
        hints_before = store.hints_taken
        ctx.profile(True)                                     # (a K1 launch counted from here on is this step's K1 NOT riding)
        bev = acc.generate_bev(pidx, 1, gen_future=True)[0]
        assert len(bev.keys()) >= 18                          # (the copy has landed: 15 plane entries and the polylines)
        k1_launches = ctx.profile_read()['kitti_project_sample_filter'][1]
        ctx.profile(False)
        grid = level1(ctx)
        # rode: no K1 launch of its own and its two tiles led level 1's grid (camera frames and per-point labels alike)
        rode.append(k1_launches == 0 and grid[1] == -(-N // 4096))
        rasters += 1
        if n_owed >= store.CHAIN_K:                           # this raster wrote back: the full window, whatever the hull said
            assert grid[2:] == (a, a + n) and store.hints_taken == hints_before and store._pending == []
            write_back_with_hint += narrower
        elif narrower:
            assert store.hints_taken == hints_before + 1
            assert grid[2:] == (a + max(first.value, 0), a + last.value + 1), (k, grid, first.value, last.value)
            hinted_ranges += 1
        else:
            assert grid[2:] == (a, a + n) and store.hints_taken == hints_before
        sub = orc.Store(1)
        lo = state['lo']
        for name in ('x', 'y', 'z', 'intensity', 'rgbs', 'inst', 'dyn'):
            setattr(sub, name, getattr(ost, name)[lo:ost.n])
        sub.n = sub.cap = ost.n - lo
        F = orc.bev(sub, int(np.sum(state['sizes'][:pidx])), orc.make_bev_params(*args))['f16']
        for s, name in enumerate(('present', 'future', 'full')):
            for key, pl in (('road', 0), ('dynamic', 5), ('elevation', 6)):
                assert np.array_equal(bev[f'{key}_{name}'].view(np.uint16), F[7 * s + pl].view(np.uint16)), (k, key, name)
            assert np.array_equal(bev[f'rgb_{name}'].view(np.uint16), F[7 * s + 2:7 * s + 5].view(np.uint16)), (k, name)
            di = np.abs(bev[f'intensity_{name}'].view(np.uint16).astype(int) - F[7 * s + 1].view(np.uint16).astype(int))
            assert di.max() <= 1 and (di != 0).mean() < 1e-3, (k, name)
        rel = poses - origin
        for name, part in (('present', rel[:pidx]), ('future', rel[pidx:]), ('full', rel)):
            want = hl.transform_traj(part.copy(), R, 0., 0., view, px)
            assert len(bev[f'trajs_{name}']) == 1 and np.array_equal(bev[f'trajs_{name}'][0], want), (k, name)
    # ---- the end state ----
    assert removed_dev == removed_orc and sum(removed_dev) >= 30
    assert np.array_equal(np.concatenate(acc.sem_pcs), ost.rows(state['lo']))
    assert np.array_equal(np.array(acc.poses), np.array(track.poses))
    store.check_status()
    # ---- the mechanisms engaged ----
    print(f'engaged [{scenario}]: rasters {rasters}, hints {store.hints_taken}, hinted ranges {hinted_ranges}, chains {sorted(chains)}, '
          f'write-backs with a hint {write_back_with_hint}, boxes seen {int((store._box[:, 0] <= store._box[:, 1]).sum())}, '
          f'slides {slides}, K1 rode in {np.mean(rode):.2f} of the rasters, evicted {sum(removed_dev)}')
    assert rasters > 60
    assert store.hints_taken >= 8 and hinted_ranges >= 8, (store.hints_taken, hinted_ranges)
    assert chains >= {1, 2, 3, 4}, chains
    assert write_back_with_hint >= 1
    assert (store._box[:, 0] <= store._box[:, 1]).any()       # a box read-back landed
    assert slides >= 1 and max(heads) > 0, heads
    assert np.mean(rode) > 0.5, np.mean(rode)                 # K1 rode along in most steps that rasterise
    store.set_defer_k1(False)
