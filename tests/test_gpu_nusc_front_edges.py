"""The NuScenes front end on the device at its edges: K0n (k0n_project), both forms of K1n (k1n_nusc; k1n_front_batch +
k1n_append_batch), the strict bilinear sampler (sample_bilinear) and the image normaliser (image_to_nchw_f32), through the C
ABI, against the reference's recorded outputs (tests/golden/nusc_front_edges.npz), the models of
tests/nusc_front_edges_common.py and the C oracle -- whose own checks, the conditions on the scenes and the wrong rules the
scenes tell apart are tests/test_nusc_front_edges_golden.py.  Every comparison is exact.

Every output buffer is larger than its content and the slack holds a sentinel; K1n appends into a store that already holds
guard frames (tests/test_gpu_store_edges.py: Loaded), behind which the slack and the unused tail of frame_off hold sentinels
too.  WHOLE arrays are compared, slack included, and the status word is read after every call.

One exemption: the sign of a NaN that the arithmetic itself produced (0 x inf, inf - inf, 0 / 0) is not held -- gfx950 clears
it, x86 sets it, and such values never reach the store.  There isnan is compared, and bits everywhere else."""
import ctypes as C

import numpy as np
import pytest

import nusc_front_edges_common as ec
import store_edges_common as m
from test_gpu_store_edges import Loaded

pytestmark = pytest.mark.gpu

UV_OUT, OVERFLOW = 2, 1                          # PCA_STATUS_UV_OUT_OF_IMAGE, PCA_STATUS_STORE_OVERFLOW
SLACK = 67
SENT_F64, SENT_I64, SENT_F32 = -12345.678, -987654321, np.float32(-77.25)


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def ctx(T):
    from pca_amd import _lib
    c = _lib.Context.get()
    c.status()
    return c


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope='module')
def fx(golden):
    return golden('nusc_front_edges')


def cu(T, a):
    a = np.array(a, order='C')                               # (a copy: the scenes' arrays are read-only)
    return T.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()     # (an empty array still gets an address)


def out_buf(T, n, sentinel, dtype):
    return T.full((n + SLACK, ), sentinel, dtype=dtype, device='cuda')


def f64s(a):
    from pca_amd import _lib
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return _lib.f64_array(a, a.size)


def with_slack(a, sentinel):
    a = np.ascontiguousarray(a).ravel()
    return np.concatenate([a, np.full(SLACK, sentinel, a.dtype)])


def sel_of(fx, name):
    return ec.sel_from(fx, name)


# ---- K0n ----------------------------------------------------------------------------------------
def run_k0n(T, ctx, pc, r, n=None, ncam=None):
    """pca_nusc_project_cams on the first n points with the first ncam cameras: (code, ego, uv, cam_idx, status), the arrays
    flat and with their slack."""
    n = len(pc) if n is None else n
    ncam = len(r['wh']) if ncam is None else ncam
    pc_d = cu(T, pc[:max(n, 0)])
    ego, uv, cam = out_buf(T, 3 * n, SENT_F64, T.float64), out_buf(T, 2 * n, SENT_F64, T.float64), out_buf(T, n, SENT_I64, T.int64)
    pad = lambda a, k: np.concatenate([np.asarray(a, dtype=np.float64).ravel(), np.zeros(max(9, ncam) * k)])      # (room for any ncam the call names)
    rc = ctx.lib.pca_nusc_project_cams(ctx.h, pc_d.data_ptr(), n, f64s(r['ego_from_lidar']), f64s(r['glob_from_ego']),
                                       f64s(pad(r['cam_from_glob'], 16)), f64s(pad(r['K'], 9)), f64s(pad(r['wh'], 2)), ncam,
                                       ego.data_ptr(), uv.data_ptr(), cam.data_ptr(), ctx.stream())
    status = ctx.status()
    return rc, ego.cpu().numpy(), uv.cpu().numpy(), cam.cpu().numpy(), status


def check_k0n(got, want, n):
    """got = run_k0n's result, want = (ego, uv, cam_idx) of all points: the first n, then the sentinels."""
    rc, ego, uv, cam, status = got
    assert rc == 0 and status == 0
    w_ego, w_uv, w_cam = with_slack(want[0][:n], SENT_F64), with_slack(want[1][:n], SENT_F64), with_slack(want[2][:n].astype(np.int64), SENT_I64)
    assert ec.same_bits_or_nan(ego, w_ego), np.flatnonzero(ego != w_ego)[:8] // 3
    assert ec.same_bits(ego[np.isfinite(w_ego)], w_ego[np.isfinite(w_ego)])
    assert ec.same_bits(uv, w_uv), np.flatnonzero(uv != w_uv)[:8] // 2
    assert np.array_equal(cam, w_cam), np.flatnonzero(cam != w_cam)[:8]


@pytest.mark.parametrize('name', ec.RIGS)
def test_k0n_every_rig_against_the_reference(T, ctx, fx, name):
    """The 200 nearest points on either side of u = 1, u = w - 1, v = 1, v = h - 1 and cz = 1e-3 of every camera, frusta that
    overlap in twos and threes, points behind a camera whose quotient lies inside, NaN / inf / zeros / denormals / 1e300, and on
    'axis' the exact hits."""
    sc = ec.k0n_scene(name, sel_of(fx, name))
    p = 'k0n_%s_' % name
    want = (fx[p + 'pc_in_ego'], fx[p + 'uv'], fx[p + 'cam_idx'])
    check_k0n(run_k0n(T, ctx, sc['pc'], sc['rig']), want, len(sc['pc']))


@pytest.mark.parametrize('ncam', [0, 1, 8])
def test_k0n_camera_counts_up_to_the_limit(T, ctx, fx, ncam):
    sc = ec.k0n_scene('nusc', sel_of(fx, 'nusc'))
    r = ec.sub_rig(ec.rig('eight'), ncam)
    want = ec.k0n_model_rig(sc['pc'], r)
    if ncam == 0:                                            # ego written, uv 0, cam_idx -1
        assert not want[1].any() and np.all(want[2] == -1) and np.isfinite(want[0]).sum() > 3 * 13000
    else:
        assert np.count_nonzero(want[2] == ncam - 1) > 100
    check_k0n(run_k0n(T, ctx, sc['pc'], r), want, len(sc['pc']))


@pytest.mark.parametrize('ncam', [9, -1])
def test_k0n_refuses_a_camera_count_out_of_range_and_touches_nothing(T, ctx, fx, ncam):
    sc = ec.k0n_scene('axis', sel_of(fx, 'axis'))
    rc, ego, uv, cam, status = run_k0n(T, ctx, sc['pc'], sc['rig'], n=300, ncam=ncam)
    assert rc == -1 and status == 0 and ctx.lib.pca_last_error(ctx.h)
    assert np.all(ego == SENT_F64) and np.all(uv == SENT_F64) and np.all(cam == SENT_I64)


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257])
def test_k0n_point_counts_around_a_workgroup(T, ctx, fx, n):
    """n = 0 returns 0 and touches nothing; the others write n points and leave the slack behind them alone ('axis': the
    first points are the family of u = 1, nearest first)."""
    sc = ec.k0n_scene('axis', sel_of(fx, 'axis'))
    want = (fx['k0n_axis_pc_in_ego'], fx['k0n_axis_uv'], fx['k0n_axis_cam_idx'])
    got = run_k0n(T, ctx, sc['pc'], sc['rig'], n=n)
    check_k0n(got, want, n)
    assert n > 0 or (np.all(got[1] == SENT_F64) and np.all(got[3] == SENT_I64))


def test_k0n_second_trip_of_the_grid_stride_loop(T, ctx, fx):
    """2048 x 256 + 1 points on 'mixed', the smallest frame whose last point is handled on a workgroup's second trip: families
    at both ends, the last point on the kept side of an edge."""
    sc = ec.k0n_second_trip_scene(sel_of(fx, 'mixed'))
    want = ec.k0n_model_rig(sc['pc'], sc['rig'])
    assert len(sc['pc']) == ec.K0N_TRIP + 1 and want[2][-1] == 2
    check_k0n(run_k0n(T, ctx, sc['pc'], sc['rig']), want, len(sc['pc']))


# ---- K1n ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev_stack(T):
    cache = {}

    def get(name, rgb='position'):
        if (name, rgb) not in cache:
            cache[name, rgb] = tuple(cu(T, a) for a in ec.stack(name, rgb))
        return cache[name, rgb]

    return get


class Appender:
    """A store with three guard frames (9, 0 and 30 rows), `room` free rows plus slack behind them and `slots` free slots:
    K1n appends from slot 3 on; `exp` follows what the store must hold."""

    def __init__(self, T, room, slots):
        rng = np.random.default_rng(5)
        self.T = T
        self.L = Loaded([m.frame(rng, 9), m.frame(rng, 0), m.frame(rng, 30)], slack=room + 37, spare_slots=slots + 2)
        self.exp = self.L.expected()
        self.slot, self.at = 3, self.L.total
        self.keep = []

    def c_store(self, capacity=None):
        from pca_amd import _lib
        st = _lib.PcaStore.from_buffer_copy(self.L.st.c_store())
        if capacity is not None:
            st.capacity = capacity
        return st

    def single(self, pc, cam, stack_d, shape, T4, filters, mode=0, capacity=None):
        from pca_amd import _lib
        L, (ncam, H, W) = self.L, shape
        pc_d, cam_d = cu(self.T, pc), cu(self.T, np.asarray(cam, dtype=np.int64))
        self.keep += [pc_d, cam_d]
        st = self.c_store(capacity)
        return L.lib.pca_nusc_sample_filter_transform_ex(L.ctx.h, pc_d.data_ptr(), cam_d.data_ptr(), len(pc), stack_d[0].data_ptr(),
                                                         stack_d[1].data_ptr(), ncam, H, W, f64s(T4), _lib.class_mask(filters), C.byref(st),
                                                         L.st.frame_off.data_ptr(), self.slot, mode, L.ctx.stream())

    def batch(self, frames, stack_d, shape, T4, filters, mode=0, capacity=None):
        """frames: (pc, cam) host pairs, or None for an empty frame (no points, no addresses)."""
        from pca_amd import _lib
        L, (ncam, H, W) = self.L, shape
        descs = (_lib.PcaNuscFrame * len(frames))()
        Tc = f64s(T4)
        dev = {}
        for k, f in enumerate(frames):
            if f is not None and id(f[0]) not in dev:
                dev[id(f[0])] = (cu(self.T, f[0]), cu(self.T, np.asarray(f[1], dtype=np.int64)))
            descs[k].pc, descs[k].cam_idx = (None, None) if f is None or not len(f[0]) else (d.data_ptr() for d in dev[id(f[0])])
            descs[k].imgs, descs[k].sems = stack_d[0].data_ptr(), stack_d[1].data_ptr()
            descs[k].n = 0 if f is None else len(f[0])
            descs[k].T = C.cast(Tc, C.POINTER(C.c_double))
        self.keep += [dev, Tc, descs]
        st = self.c_store(capacity)
        return L.lib.pca_nusc_sample_filter_transform_batch(L.ctx.h, descs, len(frames), ncam, H, W, _lib.class_mask(filters), C.byref(st),
                                                            L.st.frame_off.data_ptr(), self.slot, mode, L.ctx.stream())

    def expect(self, rows_list, capacity=None):
        """One (M,10) array per appended frame.  With `capacity`, rows behind it are not stored (frame_off counts them)."""
        for rows in rows_list:
            for k, v in ec.soa(rows).items():
                hi = min(self.at + len(v), len(self.exp[k]) if capacity is None else capacity)
                self.exp[k][self.at:hi] = v[:max(hi - self.at, 0)]
            self.at += len(rows)
            self.slot += 1
            self.exp['frame_off'][self.slot] = self.at

    def check(self, status=0):
        self.L.check(self.exp, clean=False)
        assert self.L.ctx.status() == status


def oracle_rows(orc, pc, cam, name, T4, filters, mode=0, rgb='position'):
    imgs, sems = ec.stack(name, rgb)
    st = orc.Store(max(len(pc), 1))
    orc.set_sample_mode(mode)
    try:
        orc.nusc_sample_filter_transform(st, pc, cam, imgs, sems, T4, filters)
    finally:
        orc.set_sample_mode(0)
    return st.rows()


@pytest.mark.parametrize('name', list(ec.K1N_STACKS))
def test_k1n_scenes_both_forms_against_the_reference(T, fx, dev_stack, name):
    """Nearest mode: one to three nextafter steps inside each bound of every camera, exact ties, the first legal and the last
    pixel, cam_idx -2^40 .. 2^40, a filtered class per mask word.  The single form at slot 3, then the batch form at first_slot
    4 with an empty frame between two copies of the scene."""
    sc, shape, rows = ec.k1n_scene(name), ec.K1N_STACKS[name], fx['k1n_%s_rows' % name]
    A = Appender(T, 3 * len(rows), 4)
    assert A.single(sc['pc'], sc['cam'], dev_stack(name), shape, sc['T'], sc['filters']) == 0
    A.expect([rows])
    A.check()
    f = (sc['pc'], sc['cam'])
    assert A.batch([f, None, f], dev_stack(name), shape, sc['T'], sc['filters']) == 0
    A.expect([rows, rows[:0], rows])
    A.check()


@pytest.mark.parametrize('name', list(ec.K1N_STACKS))
def test_k1n_bilinear_mode_both_forms_against_the_oracle(T, orc, dev_stack, name):
    """The opt-in mode on the same points over seeded colours: colours as the oracle restates them (one to three steps inside a
    bound the upper neighbour is column W - 1 / row H - 1, its weight all but 1), the class still the nearest pixel's."""
    sc, shape = ec.k1n_scene(name), ec.K1N_STACKS[name]
    rows = oracle_rows(orc, sc['pc'], sc['cam'], name, sc['T'], sc['filters'], mode=1, rgb='random')
    near = oracle_rows(orc, sc['pc'], sc['cam'], name, sc['T'], sc['filters'], mode=0, rgb='random')
    assert np.array_equal(rows[:, 7], near[:, 7]) and ec.same_bits(rows[:, :4], near[:, :4]) and not np.array_equal(rows[:, 4:7], near[:, 4:7])
    stack_d = dev_stack(name, 'random')
    A = Appender(T, 2 * len(rows), 3)
    assert A.single(sc['pc'], sc['cam'], stack_d, shape, sc['T'], sc['filters'], mode=1) == 0
    A.expect([rows])
    A.check()
    assert A.batch([(sc['pc'], sc['cam'])], stack_d, shape, sc['T'], sc['filters'], mode=1) == 0
    A.expect([rows])
    A.check()


@pytest.mark.parametrize('name', list(ec.K1N_STACKS))
@pytest.mark.parametrize('kind', ec.OFFENDERS)
def test_k1n_offending_frames_raise_and_drop_the_point_their_twins_raise_nothing(T, dev_stack, name, kind):
    """An assigned point with uv on a bound, one step outside it, NaN, +-inf or -0.0: PCA_STATUS_UV_OUT_OF_IMAGE, and exactly
    the model's rows of the other points are stored (the documented behaviour: the point is dropped).  The twin (cam_idx -1
    or ncam) stores the same rows and raises nothing.  Both forms; in the batch form the offender travels with its twin."""
    sc, shape = ec.k1n_scene(name), ec.K1N_STACKS[name]
    imgs, sems = ec.stack(name)
    bad, twin = ec.k1n_offender(name, kind), ec.k1n_offender(name, kind, twin=True)
    rows, asserts = ec.k1n_model(*bad, imgs, sems, sc['T'], sc['filters'])
    assert asserts
    A = Appender(T, 5 * len(rows), 6)
    args = (dev_stack(name), shape, sc['T'], sc['filters'])
    assert A.single(*bad, *args) == 0
    A.expect([rows])
    A.check(UV_OUT)
    assert A.single(*twin, *args) == 0
    A.expect([rows])
    A.check()
    assert A.batch([twin, bad], *args) == 0
    A.expect([rows, rows])
    A.check(UV_OUT)
    assert A.batch([twin], *args) == 0
    A.expect([rows])
    A.check()


@pytest.mark.parametrize('kind', ec.OFFENDERS)
def test_k1n_offending_frames_in_bilinear_mode(T, orc, dev_stack, kind):
    """The same on the 8 x 12 stack in the opt-in mode, over seeded colours: the bit is raised, the point dropped, and the
    other points' rows are the oracle's bilinear rows of the twin."""
    name, shape = 's8', ec.K1N_STACKS['s8']
    sc = ec.k1n_scene(name)
    bad, twin = ec.k1n_offender(name, kind), ec.k1n_offender(name, kind, twin=True)
    rows = oracle_rows(orc, *twin, name, sc['T'], sc['filters'], mode=1, rgb='random')
    near, asserts = ec.k1n_model(*bad, *ec.stack(name, 'random'), sc['T'], sc['filters'])
    assert asserts and np.array_equal(rows[:, 7], near[:, 7]) and not np.array_equal(rows[:, 4:7], near[:, 4:7])
    A = Appender(T, 4 * len(rows), 5)
    args = (dev_stack(name, 'random'), shape, sc['T'], sc['filters'])
    assert A.single(*bad, *args, mode=1) == 0
    A.expect([rows])
    A.check(UV_OUT)
    assert A.batch([twin, bad], *args, mode=1) == 0
    A.expect([rows, rows])
    A.check(UV_OUT)
    assert A.batch([twin], *args, mode=1) == 0
    A.expect([rows])
    A.check()


def test_k1n_single_form_draws_its_tiles_from_the_ticket(T, orc, dev_stack):
    """512 x CUs + 1 points: one tile more than the device has CUs, so the kernel draws its tiles from the ticket.  A second
    such call and a 513-point call follow on the same context: a ticket left non-zero or a stale look-back word would show."""
    cus = T.cuda.get_device_properties(0).multi_processor_count
    n = ec.K1N_TILE * cus + 1
    assert (n + ec.K1N_TILE - 1) // ec.K1N_TILE == cus + 1 > cus
    name, shape = 'nusc', ec.K1N_STACKS['nusc']
    filters = ec.k1n_scene(name)['filters']
    frames = [ec.k1n_random_frame(name, k, seed) for k, seed in ((n, 1), (n, 2), (513, 3))]
    rows = [oracle_rows(orc, pc, cam, name, ec.K1N_T, filters) for pc, cam in frames]
    assert all(0 < len(r) < len(f[0]) for r, f in zip(rows, frames))
    A = Appender(T, sum(len(r) for r in rows), 4)
    for f, r in zip(frames, rows):
        assert A.single(*f, dev_stack(name), shape, ec.K1N_T, filters) == 0
        A.expect([r])
        A.check()


@pytest.mark.parametrize('form', ['single', 'batch'])
def test_k1n_capacity_equal_to_the_kept_count_and_one_less(T, orc, dev_stack, form):
    """capacity == the rows the call stores: no status.  One less: PCA_STATUS_STORE_OVERFLOW, the rows below `capacity` are the
    oracle's and nothing behind it changed (the buffers themselves are larger); frame_off counts every kept row, the
    dropped one included (include/pca.h)."""
    name, shape = 's8', ec.K1N_STACKS['s8']
    filters = ec.k1n_scene(name)['filters']
    f = ec.k1n_random_frame(name, 1100, 9)                   # three tiles
    rows = oracle_rows(orc, *f, name, ec.K1N_T, filters)
    call = (lambda A, cap: A.single(*f, dev_stack(name), shape, ec.K1N_T, filters, capacity=cap)) if form == 'single' else \
        (lambda A, cap: A.batch([f], dev_stack(name), shape, ec.K1N_T, filters, capacity=cap))
    A = Appender(T, len(rows), 2)
    assert call(A, A.at + len(rows)) == 0
    A.expect([rows])
    A.check()
    A = Appender(T, len(rows), 2)
    cap = A.at + len(rows) - 1
    assert call(A, cap) == 0
    A.expect([rows], capacity=cap)
    A.check(OVERFLOW)


def cap_frames(n_frames_extra=0):
    """16 384 tiles exactly: a 513-point frame first (two tiles), the 's8' scene in the middle (one), a 1025-point frame last
    (three), empty frames (one tile each) everywhere else."""
    first, last = ec.k1n_random_frame('s8', 513, 21), ec.k1n_random_frame('s8', 1025, 22)
    sc = ec.k1n_scene('s8')
    n_empty = ec.K1N_MAX_BATCH_TILES - 6 + n_frames_extra
    frames = [first] + [None] * (n_empty // 2) + [(sc['pc'], sc['cam'])] + [None] * (n_empty - n_empty // 2) + [last]
    assert sum(max((len(f[0]) + ec.K1N_TILE - 1) // ec.K1N_TILE, 1) if f else 1 for f in frames) == ec.K1N_MAX_BATCH_TILES + n_frames_extra
    return frames


def test_k1n_batch_of_exactly_16384_tiles(T, orc, dev_stack):
    frames = cap_frames()
    filters = ec.k1n_scene('s8')['filters']
    empty = np.zeros((0, 10))
    rows = [empty if f is None else oracle_rows(orc, *f, 's8', ec.K1N_T, filters) for f in frames]
    assert all(len(rows[k]) > 0 for k in (0, len(frames) // 2, len(frames) - 1))
    A = Appender(T, sum(len(r) for r in rows), len(frames) + 1)
    assert A.batch(frames, dev_stack('s8'), ec.K1N_STACKS['s8'], ec.K1N_T, filters) == 0, A.L.lib.pca_last_error(A.L.ctx.h)
    A.expect(rows)
    A.check()


def test_k1n_batch_of_16385_tiles_is_refused_and_writes_nothing(T, dev_stack):
    frames = cap_frames(1)
    A = Appender(T, 2048, len(frames) + 1)
    assert A.batch(frames, dev_stack('s8'), ec.K1N_STACKS['s8'], ec.K1N_T, ec.k1n_scene('s8')['filters']) == -1
    assert b'batch too large' in A.L.lib.pca_last_error(A.L.ctx.h)
    A.check()


# ---- strict bilinear sampler ---------------------------------------------------------------------
def run_bilinear(T, ctx, fmap, uv, n):
    out = out_buf(T, n, SENT_F64, T.float64)
    map_d, uv_d = cu(T, fmap), cu(T, uv[:n])
    rc = ctx.lib.pca_sample_bilinear(ctx.h, map_d.data_ptr(), fmap.shape[0], fmap.shape[1], uv_d.data_ptr(), n, out.data_ptr(), ctx.stream())
    status = ctx.status()
    return rc, out.cpu().numpy(), status


@pytest.mark.parametrize('n', [0, 1, 256, 257])
def test_strict_bilinear_against_the_reference(T, ctx, fx, n):
    """Bit-equal where the reference is finite, NaN where it has NaN (an integer u or v: 0 / 0), coordinates one to three steps
    inside each bound included; n = 0 touches nothing."""
    fmap, uv = ec.bilinear_scene()
    rc, out, status = run_bilinear(T, ctx, fmap, uv, n)
    want = with_slack(fx['bil_out'][:n], SENT_F64)
    assert rc == 0 and status == 0
    assert ec.same_bits_or_nan(out, want), np.flatnonzero(out != want)[:8]
    assert n < 256 or np.isnan(want).sum() >= 9


@pytest.mark.parametrize('p,col,value', [(0, 0, 1.0), (100, 0, np.nextafter(ec.BIL_HW[1] - 1.0, 99.0)), (256, 1, ec.BIL_HW[0] - 1.0),
                                         (255, 1, np.nextafter(1.0, 0.0)), (64, 0, np.nan), (63, 1, np.inf), (1, 0, -np.inf), (200, 0, -0.0)])
def test_strict_bilinear_refuses_one_point_and_leaves_the_others(T, ctx, fx, p, col, value):
    fmap, uv = ec.bilinear_scene()
    uv = uv.copy()
    uv[p, col] = value
    rc, out, status = run_bilinear(T, ctx, fmap, uv, len(uv))
    want = with_slack(fx['bil_out'], SENT_F64)
    want[p] = 0.0
    assert rc == 0 and status == UV_OUT
    assert ec.same_bits_or_nan(out, want) and not np.signbit(out[p])


# ---- image normaliser ----------------------------------------------------------------------------
def run_nchw(T, ctx, img, mean, std):
    H, W = img.shape[:2]
    out = out_buf(T, 3 * H * W, float(SENT_F32), T.float32)
    img_d = cu(T, img)
    rc = ctx.lib.pca_image_to_nchw_f32(ctx.h, img_d.data_ptr(), H, W, (C.c_float * 3)(*mean), (C.c_float * 3)(*std), out.data_ptr(), ctx.stream())
    status = ctx.status()
    return rc, out.cpu().numpy(), status


@pytest.mark.parametrize('H,W,norm', [(16, 16, 'wrapper'), (16, 16, 'unit'), (1, 1, 'wrapper'), (1, 255, 'wrapper'), (1, 256, 'wrapper'),
                                      (1, 257, 'wrapper'), (7, 13, 'wrapper'), (17, 61681, 'wrapper'), (900, 1600, 'wrapper')])
def test_normaliser_every_byte_value_and_the_second_trip(T, ctx, H, W, norm):
    """16 x 16 holds every byte value in every channel; 1, 255, 256 and 257 pixels; an odd width; 17 x 61 681 = 4096 x 256 + 1
    pixels, the smallest image with a second trip of the loop, and a NuScenes image.  Bit-equal to ToTensor + Normalize in f32."""
    mean, std = (ec.MEAN, ec.STD) if norm == 'wrapper' else ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    img = ec.nchw_image(H, W)
    assert (H, W) != (17, 61681) or H * W == ec.NCHW_TRIP + 1
    rc, out, status = run_nchw(T, ctx, img, mean, std)
    want = with_slack(ec.nchw_model(img, mean, std), SENT_F32)
    assert rc == 0 and status == 0
    assert ec.same_bits(out, want), np.flatnonzero(out != want)[:8]
