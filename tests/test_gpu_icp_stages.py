"""Device ICP stage by stage (csrc/pca_icp.hip): the sorted grids, the normals, the partners, the sums of the last pass and the
step, each read out of the caller's workspace at the offsets of pca_debug_icp_layout after ONE pca_icp_register, against the
models of tests/icp_stage_common.py (whose own checks, and the conditions on the scenes, are tests/test_icp_stage_models.py).

What is exact: cells and their members, the slab ranges, the valid flag of a normal, the partner of every query inside the
coarse grid whose nearest target is closer than the cap (or than 4 m with the reference's 1e3), fitness and rmse as functions of
the sums.  What has a bound: a normal's angle (2^-22 + 2^-44 r_K^2 / (l1 - l0) rad; the model summed in reversed order and in
longdouble stays within 1.3e-8 of that bound, measured on the CPU), the sums (n_src 2^-52 x the sum of the absolute terms), the
step (64 cond(J^T J) 2^-52 max(1, |T|) per entry).  Measured on the MI355X (each test prints its figures before it asserts): the
normals use 0.18 of their bound at most (largest sine 4.3e-8), the sums 1e-4, the step 4.4e-6 (cond 165); no partner differs.
One changed line of the kernels at a time -- 29 neighbours, 5 coarse rings for the normals, the highest index among equal
distances inside a lane -- fails the normals' angle, the valid flag, and the partners of the duplicated targets.

What the kernel does with a query OUTSIDE the coarse grid (here: planted sources above 16 m) is pinned, not specified: it is
never searched; in the first pass it takes the target of its own index if that lies inside the grid within 4 m and the
threshold, afterwards it keeps that partner while it stays within the threshold.  The tests assert only that such a partner, if
any, is a target inside the grid and closer than the threshold.
"""
import ctypes as C

import numpy as np
import pytest

import icp_stage_common as m

pytestmark = pytest.mark.gpu


class Run:
    """One pca_icp_register with a workspace of the test's own; the regions are read at the accessor's offsets."""
    NAMES = ('start0', 'spts0', 'start1', 'spts1', 'normal', 'nn_prev', 'nn_cell', 'nn_slack', 'partial', 'zr_part', 'state', 'total',
             'st_zr', 'st_sums', 'nacc', 'cells')

    def __init__(self, src, tgt, max_corr_dist, init=None, max_iteration=30):
        import torch
        from pca_amd import _lib
        from pca_amd.icp import GpuIcp
        ctx = _lib.Context.get()
        self.n_src, self.n_tgt = len(src), len(tgt)
        s, t = GpuIcp.to_device(src), GpuIcp.to_device(tgt)
        need = ctx.lib.pca_icp_workspace_bytes(max(self.n_src, self.n_tgt))
        self.ws = torch.empty(int(need), dtype=torch.uint8, device=s.device)
        lay = (C.c_int64 * 16)()
        assert ctx.lib.pca_debug_icp_layout(self.n_src, self.n_tgt, lay) == 0
        self.at = dict(zip(self.NAMES, list(lay)))
        assert self.at['cells'] == m.NX * m.NY * m.NZ and self.at['nacc'] == 30
        self.base = (-self.ws.data_ptr()) % 256
        assert self.base + self.at['total'] <= need
        T = (C.c_double * 16)()
        fit, rmse, it = C.c_double(0), C.c_double(0), C.c_int(0)
        init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64)
        rc = ctx.lib.pca_icp_register(ctx.h, s.data_ptr(), self.n_src, t.data_ptr(), self.n_tgt, float(max_corr_dist),
                                      _lib.f64_array(init, 16), int(max_iteration), 1e-6, 1e-6, self.ws.data_ptr(), int(need), T,
                                      C.byref(fit), C.byref(rmse), C.byref(it), ctx.stream())
        assert rc == 0, ctx.lib.pca_last_error(ctx.h)
        torch.cuda.synchronize()
        assert ctx.status() == 0
        self.T = np.array(T[:]).reshape(4, 4)
        self.fitness, self.rmse, self.iterations = fit.value, rmse.value, it.value

    def read(self, name, count, dtype, skip=0):
        """count items of dtype from region `name`, `skip` items in."""
        size = np.dtype(dtype).itemsize
        lo = self.base + self.at[name] + skip * size
        return self.ws[lo:lo + count * size].cpu().numpy().view(dtype).copy()

    def slab_words(self):
        return [int(v) for v in self.read('state', 4, np.uint32, skip=2 * self.at['st_zr'])]

    def sums(self):
        return self.read('state', 30, np.float64, skip=self.at['st_sums'])

    def normals(self):
        return self.read('normal', 4 * self.n_tgt, np.float32).reshape(-1, 4)

    def partners(self):
        return self.read('nn_prev', self.n_src, np.int32).astype(np.int64)


def few_sources():
    return m._sweeps('sparse')[0][:64]


# ---- grids ----
def check_grids(run, tgt):
    zr = run.slab_words()
    for lv in (0, 1):
        g = m.grid_model(tgt, lv)
        assert (zr[2 * lv], zr[2 * lv + 1]) == g['slab'], (lv, zr, g['slab'])
        if g['n_in'] == 0:
            continue
        lo, hi = g['slab']
        start = run.read('start%d' % lv, (hi - lo) * m.SLAB + 1, np.uint32, skip=lo * m.SLAB).astype(np.int64)
        assert np.all(np.diff(start) >= 0) and start[-1] == g['n_in'], (lv, start[0], start[-1], g['n_in'])
        spts = run.read('spts%d' % lv, 4 * g['n_in'], np.uint32).reshape(-1, 4)
        dev_cell = np.searchsorted(start, np.arange(g['n_in']), side='right') - 1 + lo * m.SLAB
        dev_idx = spts[:, 3].view(np.int32).astype(np.int64)
        assert dev_idx.min() >= 0 and dev_idx.max() < len(tgt)
        order = np.lexsort((dev_idx, dev_cell))
        assert np.array_equal(dev_cell[order], g['cell']), lv           # every cell holds exactly the model's members ...
        assert np.array_equal(dev_idx[order], g['index']), lv
        assert np.array_equal(spts[:, :3], np.ascontiguousarray(tgt[dev_idx, :3]).view(np.uint32)), lv     # ... with the input's bits
    return zr


@pytest.mark.parametrize('n_tgt', [1, 255, 257, None])
def test_grids_hold_every_point_in_its_cell(n_tgt):
    """Borders (multiples of 0.25 / 0.5, +-0.0), the grids' faces (-128 inside, +128 outside, nextafter(128, 0), z = -16,
    nextafter(16, 0), the fine grid's +-64 / +-8), NaN and +-inf rows, 300 consecutive copies of one point, one cell over the
    rows 60..70, two cells in alternation; the first 1, 255, 257 rows and the whole cloud."""
    tgt = m.grid_scene()[:n_tgt]
    zr = check_grids(Run(few_sources(), tgt, 1e3, None, 1), tgt)
    if n_tgt == 1:
        assert zr == [0, 1, 0xffffffff, 0]                   # (-128, -128, -16): the coarse grid's first cell, outside the fine grid
    else:
        assert zr == [0, 64, 0, 64]                          # the faces are planted: every slab of both grids


def test_grids_with_empty_slabs_between_occupied_ones():
    tgt = m.two_slab_scene()
    zr = check_grids(Run(few_sources(), tgt, 1e3, None, 1), tgt)
    assert zr == [21, 43, 11, 53]


# ---- normals ----
_NORMALS = {}


def normals_case(name):
    if name not in _NORMALS:
        tgt = m.normals_scene(name)
        _NORMALS[name] = (tgt, m.normals_model(tgt))
    return _NORMALS[name]


@pytest.mark.parametrize('name', ['sparse', 'dense'])
def test_normals_against_the_box_model(name):
    """The valid flag exactly; the angle of every valid normal whose eigen-gap is not small (at most 2 % are) within the bound.
    Measured on the MI355X: see the figures printed before the assertions."""
    tgt, mod = normals_case(name)
    dev = Run(few_sources(), tgt, 1e3, None, 1).normals()
    assert np.array_equal(dev[:, 3] != 0, mod['valid'])
    assert np.all((dev[:, 3] == 0) | (dev[:, 3] == 1))
    assert np.array_equal(dev[~mod['valid'], :3], np.tile(np.float32([0, 0, 1]), ((~mod['valid']).sum(), 1)))
    gap = m.small_gap(mod['lam'])
    check = mod['valid'] & ~gap
    assert (mod['valid'] & gap).sum() <= 0.02 * len(tgt)
    dn = dev[:, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(dn[mod['valid']], axis=1) - 1.0).max() <= 2.0 ** -22
    sine = m.sine_between(dn[check], mod['normal'][check])
    bound = m.angle_bound(mod['kth'], mod['lam'])[check]
    print('normals', name, 'checked', int(check.sum()), 'of', len(tgt), 'max sine', sine.max(), 'max share of the bound', (sine / bound).max())
    worst = np.argmax(sine / bound)
    assert np.all(sine <= bound), (np.flatnonzero(check)[worst], sine[worst], bound[worst], int((sine > bound).sum()))


# ---- partners and sums ----
_RUNS = {}


def partner_run(cap, iters):
    """One registration per (threshold, iterations), shared by the partner and the accumulator test (read-only)."""
    if (cap, iters) not in _RUNS:
        src, tgt, info = m.partner_scene()
        run = Run(src, tgt, cap, None, iters)
        q = m.transform(run.T, src)
        _RUNS[(cap, iters)] = dict(run=run, q=q, mod=m.partners_model(q, tgt), nn=run.partners(), normal=run.normals(), sums=run.sums())
    return _RUNS[(cap, iters)]


def sure_partner(r, cap):
    """Queries whose partner the kernel must find: inside the coarse grid, nearest target closer than the cap (the search box
    holds every target within 4 m whatever the threshold)."""
    reach = min(cap, m.MATCH_REACH)
    return r['mod']['in_grid'] & (r['mod']['d2'] < reach * reach)


CASES = [(cap, iters) for cap in (3.9, 1e3) for iters in (1, 2, 30)]


@pytest.mark.parametrize('cap,iters', CASES)
def test_partners_are_the_nearest_targets(cap, iters):
    """nn_prev after the last pass against the exact nearest neighbour at the returned T.  With 30 iterations the late passes
    keep partners without a search.  Ties (targets duplicated at far-apart indices): the lowest index."""
    src, tgt, info = m.partner_scene()
    r = partner_run(cap, iters)
    run, mod, nn = r['run'], r['mod'], r['nn']
    assert run.iterations == iters if iters < 30 else run.iterations >= 3
    sure = sure_partner(r, cap)
    in_grid_t = m.cells(tgt[:, :3], 0)[0]
    assert nn.min() >= -1 and nn.max() < len(tgt)
    print('partners', cap, iters, 'iterations', run.iterations, 'sure', int(sure.sum()), 'tied', int((mod['ties'][sure] > 1).sum()),
          'differ', int((nn[sure] != mod['nearest'][sure]).sum()))
    assert (mod['ties'][sure] == 2).sum() >= 10 and (mod['ties'][sure] >= m.DUP_COPIES).sum() >= 3
    assert np.array_equal(nn[sure], mod['nearest'][sure]), np.flatnonzero(sure & (nn != mod['nearest']))[:10]
    # nearest target at the cap or beyond: no partner, or one inside the search box -- not nearer than the nearest, within the threshold
    rest = np.flatnonzero(mod['in_grid'] & ~sure)
    assert len(rest) > 10
    has = rest[nn[rest] >= 0]
    d2 = m.f64_dist2(tgt[nn[has], :3], r['q'][has])
    assert np.all(in_grid_t[nn[has]]) and np.all(d2 >= mod['d2'][has]) and np.all(d2 < cap * cap)
    if cap < m.MATCH_REACH:
        assert len(has) == 0
    # outside the grid (planted, counted): see the module's docstring
    out = np.flatnonzero(~mod['in_grid'])
    assert out.tolist() == info['high'].tolist() + [info['nan_row'], info['inf_row']]
    assert nn[info['nan_row']] == -1 and nn[info['inf_row']] == -1
    has = out[nn[out] >= 0]
    assert np.all(in_grid_t[nn[has]]) and np.all(m.f64_dist2(tgt[nn[has], :3], r['q'][has]) < cap * cap)


@pytest.mark.parametrize('cap,iters', CASES)
def test_sums_fitness_and_rmse_of_the_last_pass(cap, iters):
    """The 30 sums against the model's (model partners where the kernel must find them, the kernel's own elsewhere; the
    device's normals); fitness and rmse are functions of the sums, bit for bit; the NaN row counts in fitness's denominator."""
    src, tgt, info = m.partner_scene()
    r = partner_run(cap, iters)
    run, nn, dev = r['run'], r['nn'], r['sums']
    partner = np.where(sure_partner(r, cap), r['mod']['nearest'], nn)
    sums, mag = m.accumulators_model(r['q'], tgt, partner, r['normal'])
    tol = len(src) * 2.0 ** -52 * mag
    with np.errstate(divide='ignore', invalid='ignore'):
        print('sums', cap, iters, 'max share of the bound', np.nanmax(np.abs(dev - sums) / tol))
    assert dev[28] == sums[28] == (nn >= 0).sum() and 0 < dev[28] < len(src)
    assert np.all(np.abs(dev - sums) <= tol), np.flatnonzero(np.abs(dev - sums) > tol)
    assert run.fitness == dev[28] / len(src)
    assert run.rmse == np.sqrt(dev[27] / dev[28])


# ---- the step ----
def test_one_step_from_an_init_is_the_models_step():
    """max_iteration = 1 from a non-trivial init: the returned T is exp(x) init with x solved from the model's pass-0 system
    (model partners at init, the device's normals)."""
    src, tgt, init = m.step_scene()
    cap = 3.9                                                # below the box's reach: every partner is the model's
    run = Run(src, tgt, cap, init, 1)
    assert run.iterations == 1
    q0 = m.transform(init, src)
    mod = m.partners_model(q0, tgt)
    assert mod['in_grid'].all()
    partner = np.where(mod['d2'] < cap * cap, mod['nearest'], -1)
    sums, _ = m.accumulators_model(q0, tgt, partner, run.normals())
    A, b = m.system_of(sums)
    want = m.exp_step(np.linalg.solve(A, -b)) @ init
    tol = 64 * np.linalg.cond(A) * 2.0 ** -52 * np.maximum(1.0, np.abs(want))
    print('step: cond', np.linalg.cond(A), 'max share of the bound', (np.abs(run.T - want) / tol).max(), 'moved', np.abs(want - init).max())
    assert np.abs(want - init).max() > 1e-3                  # a real step
    assert np.all(np.abs(run.T - want) <= tol), (run.T - want)
    assert np.array_equal(run.T[3], [0, 0, 0, 1])


def test_a_horizontal_plane_returns_the_init():
    """A target of lattice points on one horizontal plane: every normal is (0, 0, 1) exactly, J^T J has three zero columns,
    the system is singular -- the init comes back bit for bit after no update, with the model's fitness."""
    src, tgt, init = m.plane_scene()
    cap = 0.25
    run = Run(src, tgt, cap, init, 30)
    nrm = run.normals()
    assert np.array_equal(nrm, np.tile(np.float32([0, 0, 1, 1]), (len(tgt), 1)))
    q = m.transform(init, src)
    mod = m.partners_model(q, tgt)
    partner = np.where(mod['in_grid'] & (mod['d2'] < cap * cap), mod['nearest'], -1)
    sums, _ = m.accumulators_model(q, tgt, partner, nrm)
    A, _ = m.system_of(sums)
    assert not A[:, 2:5].any() and A[0, 0] > 0 and A[5, 5] > 6
    assert 0.2 * len(src) < sums[28] < 0.9 * len(src)
    assert run.T.tobytes() == np.asarray(init, dtype=np.float64).tobytes()
    assert run.iterations == 0
    assert np.array_equal(run.partners(), partner)
    assert run.fitness == sums[28] / len(src)
