"""GPU: what the CORE entry points refuse, at the C ABI through ctypes -- K1 and the NuScenes front end, image and store
maintenance, the four rasters and the warp, the two session calls and their _v forms, the bin range and the view hint, the D2H
tickets and ICP -- and what a refused or diverted call leaves armed in the context for the next one.

1  test_refusals_launch_nothing_and_leave_the_outputs_alone, one case per entry point of core_refusals_common.TABLES: one small
   valid call is the fixture; every refused variant of it (one per host-side check of the entry point's source, each cited in
   the table as file:line, read before the case was written) returns -1 with its message, leaves every output buffer with its
   sentinel and the store's seven arrays and frame_off with their bits, and over the whole table no profiled kernel id counts a
   launch.  Then the valid call, on the same context, succeeds and equals the oracle (rasters, K1, K1n, K0n, K2: oracle/,
   bit-equal, intensity within the 1e-12 of test_gpu_kernels.assert_planes_match; dedup, warp and the normaliser: the numpy forms
   of their own tests), and the launch counts rise by exactly what that call launches: the fixture was valid, the refusals left
   the context usable, and the zero counts were not an idle profiler.  The sampler, the normaliser, the warp, the D2H copy
   and the output writer's kernels (the device codec, Adler-32, the preview sheets: in the tables so that every entry point that
   launches a kernel has one) are launched without a profiler id: their sentinels are their proof.
2  what stays armed: (a) a bin range across a refused pca_kitti_generate_bev_v and across a view hint that returns 0, (b) a
   deferred K1 that must be checked when it is noted, with the good path (a noted K1 survives a refused raster and rides in the
   next one) beside it -- tests/test_gpu_kernels.py::test_k1_defer_semantics_at_the_c_abi pins which calls run a noted K1, not
   that a refused raster leaves it noted --, (c) pca_icp_register's pass count beyond eight bits.

On the parent commit (read, not run):
  (a) test_a_refused_generate_bev_v_leaves_no_bin_range_armed: pca_kitti_generate_bev_v armed the hint's range (pca_session.hip:
      160-164 then), pca_kitti_generate_bev returned -1 at its own checks (:129, :131) before pca_bev_generate_chain took the range
      (pca_bev.hip:1892): the raster that follows reports bin (2, 6) instead of (0, 8) and its planes are the sub-window's.
      test_a_view_hint_that_returns_0_replaces_an_armed_range: pca_bev_view_hint returned 0 at pca_api.hip:203 without touching
      bin_valid: the same two assertions fail.
  (b) test_a_deferred_k1_is_checked_when_it_is_noted: pca_kitti_integrate only tested `plain` (pca_session.hip:86), noted the frame
      and stepped the track: rc is 0 (not -1), the track is one pose longer, evicted / path_length are overwritten.
  (c) test_icp_runs_every_pass_it_is_asked_for[300]: icp_news_pack(tag, ended, 256) -- the news of pass 255, an update like any
      other -- carried into the ended bit (pca_icp.hip:99 then): the host stopped launching and read the mirror, and
      `iterations == max_iter` fails with about 256 instead of 300.  max_iter = 254 never packs 256 and 255 packs it with its
      last, evaluating pass, which ends the run anyway: both pass there; 256 is cut one pass short (fitness and rmse are
      those of the pose before the last update), which a converged run hides within the bar.

Left out on purpose: every case that a failing device call alone could refuse, and everything that needs a stalled
stream -- the ICP poll time-out (IcpNews::wait_for) among them.  Of the 62 `ctx->err = ...` sites of the sources of the entry
points above, 58 are reached by a case; the 4 that are not are core_refusals_common.UNREACHED with their reasons (one behind a
failing hipEventRecord, one an invariant no argument reaches, one no int32 reaches, one behind device allocations for more
than 65535 frame descriptors)."""
import ctypes as C
import re

import numpy as np
import pytest

import core_refusals_common as cr
import store_edges_common as m
from test_gpu_kernels import assert_planes_match
from test_gpu_store_edges import Loaded, check_dedup

pytestmark = pytest.mark.gpu
SENT = 7


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def counts(lib, h):
    """{kernel id: launches} of a context since pca_profile_enable(1) (pca_profile_read; synchronises)."""
    from pca_amd import _lib
    names = (_lib.KERNEL_IDS + _lib.KERNEL_IDS_VOXEL + _lib.KERNEL_IDS_RAYS + _lib.KERNEL_IDS_RENDER + _lib.KERNEL_IDS_CARVE + _lib.KERNEL_IDS_INST
             + _lib.KERNEL_IDS_CAMERA + _lib.KERNEL_IDS_SSC + _lib.KERNEL_IDS_DIST + _lib.KERNEL_IDS_BOX)
    out = {}
    for k, name in enumerate(names):
        n = C.c_int64(-1)
        assert lib.pca_profile_read(h, k, None, C.byref(n)) == 0
        out[name] = n.value
    return out


def level1(ctx):
    out = (C.c_int * 4)()
    assert ctx.lib.pca_debug_bev_level1(ctx.h, out) == 0
    return tuple(out)


def f64s(a):
    from pca_amd import _lib
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return _lib.f64_array(a, a.size)


def pick(bad, name, default):
    return bad[name] if name in bad else default


def same_bits(a, b):
    return m.same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b))


def oracle_planes(orc, frames, lo, hi, split, args):
    """orc.bev of frames [lo, hi), 'present' = those before `split`."""
    sub = list(frames[lo:hi])
    rows = np.concatenate(sub) if sub else np.zeros((0, 10))
    n_present = int(sum(len(r) for r in frames[lo:min(max(split, lo), hi)]))
    return orc.bev(orc.Store.from_rows(rows, intensity_div255=bool(args[-1])), n_present, orc.make_bev_params(*args))


def f16_matches(p16, ref, name):
    """The fp16 half of assert_planes_match (p16: the planes' bits as uint16 [21, px, px])."""
    F = ref['f16'].view(np.uint16)
    for k in range(21):
        if k % 7 == 1:
            d = np.abs(p16[k].astype(int) - F[k].astype(int))
            assert d.max() <= 1 and (d != 0).mean() < 1e-3, (name, k)
        else:
            assert np.array_equal(p16[k], F[k]), (name, k)


BEV_RISE = {'bev_bin': 1, 'bev_cells': 1, 'bev_cells_heavy': (0, 1)}    # (the heavy kernel follows while one of the context's last 64 rasters saw a heavy tile)


class Fx:
    """One entry point's fixture: the valid call, its refused variants (call(**bad)), the outputs with their sentinels and, where
    the entry point takes one, the store (a test_gpu_store_edges.Loaded: slack and sentinels behind the scene)."""
    L = None

    def __init__(self, T, orc, symbol):
        from pca_amd import _lib
        self.T, self.orc, self.symbol, self._lib = T, orc, symbol, _lib
        self.ctx = _lib.Context.get()
        self.lib, self.h = self.ctx.lib, self.ctx.h
        self.fn = getattr(self.lib, symbol)
        self.outs, self.host = {}, {}
        self.setup()
        T.cuda.synchronize()

    def out(self, name, n, dtype):
        self.outs[name] = self.T.full((int(n), ), SENT, dtype=dtype, device='cuda')
        return self.outs[name]

    def cu(self, a):
        return self.T.from_numpy(np.ascontiguousarray(a)).cuda()

    def hh(self, bad):
        return None if bad.get('null_ctx') else self.h

    def store(self, bad):
        return pick(bad, 'store', C.byref(self.L.st.c_store()))

    def frame_off(self, bad):
        return pick(bad, 'frame_off', self.L.st.frame_off.data_ptr())

    def stream(self):
        return self.ctx.stream()

    def untouched(self, label):
        self.T.cuda.synchronize()
        for name, t in self.outs.items():
            assert bool((t == SENT).all()), (self.symbol, label, name)
        for name, (get, want) in self.host.items():
            assert get() == want, (self.symbol, label, name, get())
        if self.L is not None:
            self.L.check(self.L.expected())

    def close(self):
        pass


# ---------------------------------------------------------------------------------------------- K1 and the NuScenes front end
class FxK1(Fx):
    def setup(self):
        sc = self.sc = cr.kitti_scene()
        self.L = Loaded([], slack=300, spare_slots=8)
        self.pts = [self.cu(p) for p in sc['frames']]
        self.img, self.sem = self.cu(sc['img']), self.cu(sc['sem'])
        self.P, self.fm = f64s(sc['P']), self._lib.class_mask(cr.KITTI_FILTERS)

    def descs(self, change):
        d = (self._lib.PcaKittiFrame * 4)()
        for k, p in enumerate(self.pts):
            d[k].pts, d[k].rgb, d[k].sem, d[k].sem_gt, d[k].n = (p.data_ptr() if len(p) else None), self.img.data_ptr(), self.sem.data_ptr(), None, len(p)
        if change:
            setattr(d[change[0]], change[1], change[2])
        return d

    def call(self, **bad):
        args = [self.hh(bad), pick(bad, 'frames', self.descs(bad.get('frame'))), pick(bad, 'n_frames', 4), pick(bad, 'P', self.P),
                pick(bad, 'H', cr.H), pick(bad, 'W', cr.W), self.fm, self.store(bad), self.frame_off(bad), 0]
        if self.symbol.endswith('_ex'):
            args.append(pick(bad, 'sample_mode', 0))
        return self.fn(*args, self.stream())

    def valid(self):
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        sc, ost, off = self.sc, self.orc.Store(cr.N_POINTS), [0]
        for p in sc['frames']:
            off.append(off[-1] + self.orc.kitti_project_sample_filter(ost, p, sc['P'], sc['img'], sc['sem'], None, cr.H, cr.W, cr.KITTI_FILTERS))
        assert 0 < off[1] < 96 and off[3] == off[2]                      # the camera cut some points, the empty frame is empty
        exp = self.L.expected()
        for k, v in m.soa(ost.rows()).items():
            exp[k][:len(v)] = v
        exp['frame_off'][:5] = off
        self.L.check(exp)
        return {'kitti_project_sample_filter': 1}


class FxK1n(Fx):
    def setup(self):
        sc = self.sc = cr.nusc_scene()
        self.L = Loaded([], slack=300, spare_slots=8)
        self.dev = [(self.cu(pc), self.cu(cam), f64s(Tw)) for pc, cam, Tw in sc['frames']]
        self.imgs, self.sems = self.cu(sc['imgs']), self.cu(sc['sems'])
        self.fm = self._lib.class_mask(cr.NUSC_FILTERS)
        self.batch = self.symbol.endswith('_batch')

    def descs(self, change):
        d = (self._lib.PcaNuscFrame * 4)()
        for k, (pc, cam, Tw) in enumerate(self.dev):
            n = len(pc)
            d[k].pc, d[k].cam_idx, d[k].imgs, d[k].sems, d[k].n = (pc.data_ptr() if n else None), (cam.data_ptr() if n else None), self.imgs.data_ptr(), self.sems.data_ptr(), n
            d[k].T = C.cast(Tw, C.POINTER(C.c_double))
        if change:
            setattr(d[change[0]], change[1], change[2])
        return d

    def call(self, **bad):
        geo = [pick(bad, 'ncam', cr.NCAM), pick(bad, 'H', cr.H), pick(bad, 'W', cr.W)]
        if self.batch:
            return self.fn(self.hh(bad), pick(bad, 'frames', self.descs(bad.get('frame'))), pick(bad, 'n_frames', 4), *geo, self.fm,
                           self.store(bad), self.frame_off(bad), 0, pick(bad, 'sample_mode', 0), self.stream())
        pc, cam, Tw = self.dev[3]
        args = [self.hh(bad), pick(bad, 'pc', pc.data_ptr()), pick(bad, 'cam_idx', cam.data_ptr()), pick(bad, 'n', len(pc)),
                pick(bad, 'imgs', self.imgs.data_ptr()), pick(bad, 'sems', self.sems.data_ptr()), *geo, pick(bad, 'T', Tw), self.fm,
                self.store(bad), self.frame_off(bad), 0]
        if self.symbol.endswith('_ex'):
            args.append(pick(bad, 'sample_mode', 0))
        return self.fn(*args, self.stream())

    def valid(self):
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        sc, ost, off = self.sc, self.orc.Store(cr.N_POINTS), [0]
        for pc, cam, Tw in (sc['frames'] if self.batch else sc['frames'][3:]):
            off.append(off[-1] + self.orc.nusc_sample_filter_transform(ost, pc, cam, sc['imgs'], sc['sems'], Tw, cr.NUSC_FILTERS))
        assert 0 < off[-1] < cr.N_POINTS
        exp = self.L.expected()
        for k, v in m.soa(ost.rows()).items():
            exp[k][:len(v)] = v
        exp['frame_off'][:len(off)] = off
        self.L.check(exp)
        return {'nusc_sample_filter_transform': 1}


class FxK0n(Fx):
    def setup(self):
        sc = self.sc = cr.k0n_scene()
        self.pc = self.cu(sc['pc'])
        self.mats = {k: f64s(sc[k]) for k in ('ego_from_lidar', 'glob_from_ego', 'cam_from_glob', 'K', 'wh')}
        n = len(sc['pc'])
        self.out('ego', 3 * n, self.T.float64), self.out('uv', 2 * n, self.T.float64), self.out('cam', n, self.T.int64)

    def call(self, **bad):
        mt = {k: pick(bad, k, v) for k, v in self.mats.items()}
        return self.fn(self.hh(bad), pick(bad, 'pc', self.pc.data_ptr()), len(self.sc['pc']), mt['ego_from_lidar'], mt['glob_from_ego'],
                       mt['cam_from_glob'], mt['K'], mt['wh'], pick(bad, 'ncam', cr.NCAM), pick(bad, 'out_ego', self.outs['ego'].data_ptr()),
                       pick(bad, 'out_uv', self.outs['uv'].data_ptr()), pick(bad, 'out_cam', self.outs['cam'].data_ptr()), self.stream())

    def valid(self):
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        sc = self.sc
        ego, uv, cam = self.orc.nusc_project_cams(sc['pc'], sc['ego_from_lidar'], sc['glob_from_ego'], sc['cam_from_glob'], sc['K'], sc['wh'])
        assert set(cam.tolist()) == {-1, 0, 1}                           # both cameras take points, some points are taken by none
        assert same_bits(self.outs['ego'].cpu().numpy(), ego.ravel()) and same_bits(self.outs['uv'].cpu().numpy(), uv.ravel())
        assert np.array_equal(self.outs['cam'].cpu().numpy(), cam)
        assert self.ctx.status() == 0
        return {'nusc_project_cams': 1}


class FxBilinear(Fx):
    def setup(self):
        sc = self.sc = cr.bilinear_scene()
        self.map, self.uv = self.cu(sc['map']), self.cu(sc['uv'])
        self.out('out', len(sc['uv']), self.T.float64)

    def call(self, **bad):
        return self.fn(self.hh(bad), pick(bad, 'map', self.map.data_ptr()), pick(bad, 'H', cr.H), pick(bad, 'W', cr.W),
                       pick(bad, 'uv', self.uv.data_ptr()), pick(bad, 'n', len(self.sc['uv'])), pick(bad, 'out', self.outs['out'].data_ptr()), self.stream())

    def valid(self):
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        assert same_bits(self.outs['out'].cpu().numpy(), self.orc.sample_bilinear(self.sc['map'], self.sc['uv']))
        assert self.ctx.status() == 0
        return {}


class FxNchw(Fx):
    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def setup(self):
        import nusc_front_edges_common as ec
        self.ec, self.img_h = ec, ec.nchw_image(cr.H, cr.W)
        self.img = self.cu(self.img_h)
        self.mean, self.std = (C.c_float * 3)(*self.MEAN), (C.c_float * 3)(*self.STD)
        self.out('out', 3 * cr.H * cr.W, self.T.float32)

    def call(self, **bad):
        return self.fn(self.hh(bad), pick(bad, 'rgb', self.img.data_ptr()), pick(bad, 'H', cr.H), pick(bad, 'W', cr.W), pick(bad, 'mean', self.mean),
                       pick(bad, 'std', self.std), pick(bad, 'out', self.outs['out'].data_ptr()), self.stream())

    def valid(self):
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        assert same_bits(self.outs['out'].cpu().numpy(), self.ec.nchw_model(self.img_h, self.MEAN, self.STD).ravel())
        return {}


# ---------------------------------------------------------------------------------------------- store maintenance
class FxStore(Fx):
    def setup(self):
        rng = np.random.default_rng(11)
        self.L = Loaded([m.frame(rng, n) for n in cr.FRAME_SIZES])
        self.Ts = m.transforms(rng, 4)
        self.cTs = f64s(self.Ts)
        self.slots, self.idxs = [0, 3, 2, 0], [0, 1, 3, -1]
        self.cslots, self.cidxs = (C.c_int32 * 4)(*self.slots), (C.c_int32 * 4)(*self.idxs)
        self.need = int(self.lib.pca_voxel_dedup_workspace_bytes(cr.N_POINTS, 4))
        if self.symbol == 'pca_voxel_dedup':
            self.ws = self.out('workspace', self.need + 256, self.T.uint8)

    def call(self, **bad):
        head = [self.hh(bad), self.store(bad), self.frame_off(bad)]
        if self.symbol == 'pca_retransform':
            return self.fn(*head, pick(bad, 'slot_begin', 0), pick(bad, 'slot_end', 4), pick(bad, 'Ts', self.cTs), pick(bad, 'n_T', 3), self.stream())
        if self.symbol == 'pca_retransform_batch_tail':
            return self.fn(*head, 0, pick(bad, 'n_frames', 4), pick(bad, 'Ts', self.cTs), self.stream())
        if self.symbol == 'pca_mark_dynamic':
            return self.fn(*head, pick(bad, 'slots', self.cslots), pick(bad, 'inst_idx', self.cidxs), pick(bad, 'n_pairs', 4), self.stream())
        return self.fn(*head, pick(bad, 'slot_begin', 0), pick(bad, 'slot_end', 4), pick(bad, 'voxel_size', 25.0), pick(bad, 'max_points', cr.N_POINTS),
                       pick(bad, 'workspace', self.ws.data_ptr()), self.need - bad.get('short', 0), self.stream())

    def valid(self):
        L = self.L
        self.outs.clear()                                            # (the workspace is scratch from here on)
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        if self.symbol == 'pca_retransform':
            L.check(L.expected(rows=m.k2_model(L.rows, L.off, 0, 4, self.Ts[:3], self.orc)))
            return {'retransform': 1}
        if self.symbol == 'pca_retransform_batch_tail':
            L.check(L.expected(rows=m.k2_tail_model(L.rows, L.off, 0, 4, self.Ts, self.orc)))
            return {'retransform': 1}
        if self.symbol == 'pca_mark_dynamic':
            want = m.k3_model(L.rows, L.off, self.slots, self.idxs)
            assert not np.array_equal(want[:, 9], L.rows[:, 9])
            L.check(L.expected(rows=want))
            return {'mark_dynamic': 1}
        kept, new_off = m.dedup_model(L.rows, L.off, 0, 4, 25.0)
        assert 1 < int(new_off[4]) < cr.N_POINTS                         # some points share a voxel
        check_dedup(L, L.before, 0, int(L.off[4]), kept, new_off)
        return {'voxel_dedup': 3}


# ---------------------------------------------------------------------------------------------- rasters and warp
class FxBev(Fx):
    """pca_bev_generate, _ex and _chain; with the hint and the bin range in front of the chain form (FxHint)."""
    PX = cr.PX

    def setup(self):
        from pca_amd.device_store import make_bev_params
        self.frames = cr.store_frames()
        self.L = Loaded(self.frames)
        self.args = cr.bev_args(self.PX)
        self.prm = make_bev_params(*self.args)
        self.need = int(self.lib.pca_bev_workspace_bytes(cr.N_POINTS, self.PX))
        cells = self.PX * self.PX
        self.out('workspace', self.need + 256, self.T.uint8)
        self.out('planes', 21 * cells, self.T.float64), self.out('planes_f16', 21 * cells, self.T.int16), self.out('extra', 9 * cells, self.T.float64)
        self.bufs = dict(self.outs)
        self.eye, self.two = f64s(np.eye(4)), f64s(np.stack([np.eye(4)] * 2))
        self.form = self.symbol if self.symbol.startswith('pca_bev_generate') else 'pca_bev_generate_chain'

    def prm_of(self, bad):
        if 'prm' in bad:
            return bad['prm']
        p = self._lib.PcaBevParams.from_buffer_copy(self.prm)
        if 'px' in bad:
            p.px = bad['px']
        if 'R' in bad:
            p.R[bad['R'][0]] = bad['R'][1]
        return C.byref(p)

    def raster(self, **bad):
        fn = getattr(self.lib, self.form)
        head = [self.hh(bad), self.store(bad), None, self.frame_off(bad), pick(bad, 'slot_begin', 0), pick(bad, 'slot_split', cr.SPLIT), 4,
                pick(bad, 'max_points', cr.N_POINTS), self.prm_of(bad)]
        if self.form == 'pca_bev_generate_chain':
            ends = (C.c_int * 4)(*bad.get('ends', (2, 4)), 4, 4)
            owed = [pick(bad, 'pending_Ts', self.two), pick(bad, 'pending_slot_ends', ends), pick(bad, 'n_pending', 0), 0]
        else:
            owed = [self.eye if bad.get('pending_T') else None, bad.get('pending_slot_end', 0)]
        tail = [pick(bad, 'workspace', self.bufs['workspace'].data_ptr()), self.need - bad.get('short', 0),
                pick(bad, 'planes', self.bufs['planes'].data_ptr()), pick(bad, 'planes_f16', self.bufs['planes_f16'].data_ptr())]
        if self.form != 'pca_bev_generate':
            tail.append(self.bufs['extra'].data_ptr())
        return fn(*head, *owed, *tail, self.stream())

    call = raster

    def release(self):
        """The outputs stop being sentinels: the valid call writes them."""
        self.outs.clear()
        self.p64, self.p16 = self.bufs['planes'], self.bufs['planes_f16']

    def planes_equal(self, lo, hi, name):
        p16 = self.p16.cpu().numpy().view(np.float16).reshape(21, self.PX, self.PX)
        p64 = self.p64.cpu().numpy().reshape(21, self.PX, self.PX)
        assert_planes_match(p16, p64, oracle_planes(self.orc, self.frames, lo, hi, cr.SPLIT, self.args), name)
        assert p64[14:21].any()
        self.L.check(self.L.expected())

    def valid(self):
        self.release()
        assert self.raster() == 0, self.lib.pca_last_error(self.h)
        assert level1(self.ctx)[1:] == (0, 0, 4)
        self.planes_equal(0, 4, self.symbol)
        return dict(BEV_RISE)


class FxHint(FxBev):
    """pca_bev_view_hint and pca_bev_bin_range: refused, they arm nothing and touch nothing; served, the raster behind them
    bins slots 1 .. 3 and equals the oracle's raster of those frames."""
    def call(self, **bad):
        if self.symbol == 'pca_bev_bin_range':
            return self.fn(self.hh(bad), 1, 4)
        then, box, now = self.tables = cr.hint_tables(visible=(1, 2, 3))
        return self.fn(self.hh(bad), 0, pick(bad, 'F', 4), pick(bad, 'then', then.ctypes.data), box.ctypes.data, None, pick(bad, 'now', now.ctypes.data),
                       pick(bad, 'prm', C.addressof(self.prm)))

    def valid(self):
        self.release()
        assert self.call() == (0 if self.symbol == 'pca_bev_bin_range' else 1)
        assert self.raster() == 0, self.lib.pca_last_error(self.h)
        assert level1(self.ctx)[1:] == (0, 1, 4)
        full = oracle_planes(self.orc, self.frames, 0, 4, cr.SPLIT, self.args)['planes']
        assert not np.array_equal(full, oracle_planes(self.orc, self.frames, 1, 4, cr.SPLIT, self.args)['planes'])   # (the range matters)
        self.planes_equal(1, 4, self.symbol)
        return dict(BEV_RISE)


class FxMany(Fx):
    JOBS = ((0, cr.SPLIT, 4), (1, cr.SPLIT, 4))

    def setup(self):
        from pca_amd.device_store import make_bev_params
        self.frames = cr.store_frames()
        self.L = Loaded(self.frames)
        self.args = cr.bev_args()
        self.prm = make_bev_params(*self.args)
        per = (int(self.lib.pca_bev_workspace_bytes(cr.N_POINTS, cr.PX)) + 255) & ~255
        self.need = per * len(self.JOBS) + 256
        cells = cr.PX * cr.PX
        self.out('workspace', self.need + 256, self.T.uint8)
        for k in range(len(self.JOBS)):
            self.out('planes%d' % k, 21 * cells, self.T.float64), self.out('planes_f16_%d' % k, 21 * cells, self.T.int16)
        self.bufs = dict(self.outs)

    def jobs(self, change):
        cj = (self._lib.PcaBevJob * len(self.JOBS))()
        for k, (b, s, e) in enumerate(self.JOBS):
            cj[k].slot_begin, cj[k].slot_split, cj[k].slot_end = b, s, e
            C.memmove(C.addressof(cj[k].prm), C.addressof(self.prm), C.sizeof(self._lib.PcaBevParams))
            cj[k].planes, cj[k].planes_f16 = self.bufs['planes%d' % k].data_ptr(), self.bufs['planes_f16_%d' % k].data_ptr()
        if change:
            k, what, v = change
            if what == 'px':
                cj[k].prm.px = v
            elif what == 'R':
                cj[k].prm.R[v[0]] = v[1]
            elif what == 'planes':
                cj[k].planes = cj[k].planes_f16 = None
            else:
                setattr(cj[k], what, v)
        return cj

    def call(self, **bad):
        ws_bytes = (1 << 62) if 'max_points' in bad else self.need - bad.get('short', 0)
        return self.fn(self.hh(bad), self.store(bad), None, self.frame_off(bad), pick(bad, 'jobs', self.jobs(bad.get('job'))), pick(bad, 'n_jobs', len(self.JOBS)),
                       pick(bad, 'max_points', cr.N_POINTS), self.bufs['workspace'].data_ptr(), ws_bytes, self.stream())

    def valid(self):
        self.outs.clear()
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        for k, (b, s, e) in enumerate(self.JOBS):
            p16 = self.bufs['planes_f16_%d' % k].cpu().numpy().view(np.float16).reshape(21, cr.PX, cr.PX)
            p64 = self.bufs['planes%d' % k].cpu().numpy().reshape(21, cr.PX, cr.PX)
            assert_planes_match(p16, p64, oracle_planes(self.orc, self.frames, b, e, s, self.args), 'job %d' % k)
        self.L.check(self.L.expected())
        return {'bev_unit': 1}


class FxWarp(Fx):
    def setup(self):
        from pca_amd import host_logic as hl
        self.hl = hl
        self.planes_h = np.random.default_rng(4).random((3, cr.PX, cr.PX))
        self.planes = self.cu(self.planes_h.astype(np.float16))
        self.coef = list(hl.cal_warp_params(6.3, cr.PX // 2, cr.PX - 1)) + list(hl.cal_warp_params(9.8, cr.PX // 2, cr.PX - 1))
        self.out('out', 3 * cr.PX * cr.PX, self.T.int16)

    def call(self, **bad):
        coef = [float(c) for c in self.coef]
        if 'coef' in bad:
            coef[bad['coef'][0]] = bad['coef'][1]
        out = self.planes.data_ptr() if bad.get('same') else pick(bad, 'out', self.outs['out'].data_ptr())
        return self.fn(self.hh(bad), pick(bad, 'planes', self.planes.data_ptr()), out, pick(bad, 'n_planes', 3), pick(bad, 'px', cr.PX), *coef, self.stream())

    def valid(self):
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        want = self.hl.warp_dense_probmaps(self.planes_h, *self.coef).astype(np.float16)
        got = self.outs['out'].cpu().numpy().view(np.uint16).reshape(3, cr.PX, cr.PX)
        assert np.array_equal(got, want.view(np.uint16)) and not np.array_equal(want, self.planes_h.astype(np.float16))
        return {}


# ---------------------------------------------------------------------------------------------- session, tickets, ICP
def c_track(poses):
    """A pca_host_track holding `poses` (the C pose track of pca_amd.host_logic)."""
    from pca_amd import host_logic as hl
    cls = hl._bind_c_track()
    assert cls is hl.CPoseTrack
    t = cls()
    t.poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    return t


def line_poses(n):
    return np.stack([np.linspace(-3.0, 3.0, n), 0.3 * np.sin(np.arange(n)), np.zeros(n)], 1)


class FxIntegrate(Fx):
    def setup(self):
        sc = self.sc = cr.kitti_scene()
        self.frames = cr.store_frames()[:3]
        self.L = Loaded(self.frames, slack=100, spare_slots=4)
        self.pts, self.img, self.sem = self.cu(sc['frames'][3]), self.cu(sc['img']), self.cu(sc['sem'])
        self.P, self.fm = f64s(sc['P']), self._lib.class_mask(cr.KITTI_FILTERS)
        self.track = c_track(line_poses(3))
        self.step = np.eye(4)
        self.step[0, 3] = -0.5
        self.cstep = f64s(self.step)
        self.evicted, self.path = C.c_int64(SENT), C.c_double(SENT)
        self.block = self._lib.PcaKittiIntegrateArgs()
        self.v = self.symbol.endswith('_v')
        self.host['track length'] = (lambda: len(self.track), 3)
        if self.v:
            self.host['evicted'], self.host['path_length'] = (lambda: self.block.evicted, SENT), (lambda: self.block.path_length, float(SENT))
        else:
            self.host['evicted'], self.host['path_length'] = (lambda: self.evicted.value, SENT), (lambda: self.path.value, float(SENT))
        assert self.lib.pca_k1_defer(self.h, 0) == 0

    def obs(self, bad):
        o = self._lib.PcaKittiObs()
        o.pts, o.rgb, o.sem = pick(bad, 'pts', self.pts.data_ptr()), pick(bad, 'rgb', self.img.data_ptr()), pick(bad, 'sem', self.sem.data_ptr())
        o.sem_gt, o.n, o.host_mask = None, pick(bad, 'n', len(self.pts)), 0
        return o

    def call(self, **bad):
        o = self.keep = self.obs(bad)
        st = self.L.st.c_store()
        a = dict(obs=pick(bad, 'obs', C.byref(o)), P=pick(bad, 'P', self.P), H=pick(bad, 'H', cr.H), W=pick(bad, 'W', cr.W),
                 filter_mask=pick(bad, 'filter_mask', self.fm), store=pick(bad, 'store', C.byref(st)), frame_off=self.frame_off(bad), slot=3,
                 sample_mode=pick(bad, 'sample_mode', 0), track=self.track._h, T_new_prev=pick(bad, 'T_new_prev', self.cstep), horizon=1e9)
        if not self.v:
            return self.fn(self.hh(bad), a['obs'], a['P'], a['H'], a['W'], a['filter_mask'], a['store'], a['frame_off'], a['slot'], a['sample_mode'],
                           a['track'], a['T_new_prev'], a['horizon'], pick(bad, 'evicted', C.byref(self.evicted)),
                           pick(bad, 'path_length', C.byref(self.path)), self.stream())
        b = self.block
        for k, v in a.items():
            setattr(b, k, v if isinstance(v, (int, float)) or v is None else C.cast(v, C.c_void_p))
        b.evicted, b.path_length, b.stream = SENT, float(SENT), self.ctx.stream_int()
        return self.fn(self.hh(bad), pick(bad, 'block', C.addressof(b)))

    def valid(self):
        self.host.clear()
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        return self.appended()

    def appended(self):
        """The frame stands in slot 3 as the oracle has it, the track has taken its step."""
        sc = self.sc
        ost = self.orc.Store(64)
        k = self.orc.kitti_project_sample_filter(ost, sc['frames'][3], sc['P'], sc['img'], sc['sem'], None, cr.H, cr.W, cr.KITTI_FILTERS)
        assert 0 < k < 33
        exp, n0 = self.L.expected(), self.L.total
        for name, v in m.soa(ost.rows()).items():
            exp[name][n0:n0 + k] = v
        exp['frame_off'][4] = n0 + k
        self.L.check(exp)
        want = np.concatenate([line_poses(3) + [-0.5, 0, 0], np.zeros((1, 3))])
        assert len(self.track) == 4 and np.allclose(self.track.as_array(), want, rtol=0, atol=1e-12)
        assert (self.block.evicted if self.v else self.evicted.value) == 0
        return {'kitti_project_sample_filter': 1}


class FxNoted(FxIntegrate):
    """pca_k1_defer, pca_k1_flush and pca_status: refused, they run nothing; served, they run the K1 that a pca_kitti_integrate
    under pca_k1_defer(1) has noted -- the frame then stands in the store as the oracle has it."""
    def setup(self):
        FxIntegrate.setup(self)
        self.v, self.fn = False, self.lib.pca_kitti_integrate
        self.host = {k: v for k, v in self.host.items() if k == 'track length'}
        self.word = C.c_uint32(SENT)

    def call(self, **bad):
        run = getattr(self.lib, self.symbol)
        if self.symbol == 'pca_status':
            return run(self.hh(bad), self.stream(), pick(bad, 'status_out', C.byref(self.word)))
        return run(self.hh(bad), 0) if self.symbol == 'pca_k1_defer' else run(self.hh(bad))

    def valid(self):
        assert self.lib.pca_k1_defer(self.h, 1) == 0
        try:
            assert FxIntegrate.call(self) == 0, self.lib.pca_last_error(self.h)
            assert not any(counts(self.lib, self.h).values())            # noted: nothing has run
            assert self.call() == 0, self.lib.pca_last_error(self.h)
            assert self.symbol != 'pca_status' or self.word.value == 0
        finally:
            assert self.lib.pca_k1_defer(self.h, 0) == 0
        return self.appended()


class FxGenerate(Fx):
    def setup(self):
        from pca_amd.device_store import make_bev_params
        self.frames = cr.store_frames()
        self.L = Loaded(self.frames)
        self.args = cr.bev_args()
        self.prm = make_bev_params(*self.args)
        self.need = int(self.lib.pca_bev_workspace_bytes(cr.N_POINTS, cr.PX))
        self.out('workspace', self.need + 256, self.T.uint8), self.out('planes_f16', 21 * cr.PX * cr.PX, self.T.int16)
        self.bufs = dict(self.outs)
        self.track = c_track(line_poses(4))
        self.rows, self.start, self.n_rows = np.full(2 * 3 * 3, float(SENT)), np.full(4, SENT, np.int32), C.c_int32(SENT)
        self.block = self._lib.PcaKittiGenerateBevArgs()
        self.v = self.symbol.endswith('_v')
        self.host['traj_rows'] = (lambda: bool((self.rows == SENT).all()), True)
        self.host['traj_start'] = (lambda: bool((self.start == SENT).all()), True)
        self.host['n_rows'] = (lambda: self.block.n_rows if self.v else self.n_rows.value, SENT)
        self.tables = cr.hint_tables(visible=(0, 1, 2, 3))

    def call(self, **bad):
        p = self._lib.PcaBevParams.from_buffer_copy(self.prm)
        if 'px' in bad:
            p.px = bad['px']
        if 'R' in bad:
            p.R[bad['R'][0]] = bad['R'][1]
        self.keep = (p, self.L.st.c_store())
        a = dict(store=pick(bad, 'store', C.byref(self.keep[1])), frame_off=self.frame_off(bad), slot_begin=pick(bad, 'slot_begin', 0),
                 slot_split=pick(bad, 'slot_split', cr.SPLIT), slot_end=4, max_points=cr.N_POINTS, prm=pick(bad, 'prm', C.byref(p)), pending_Ts=None,
                 pending_slot_ends=None, n_pending=pick(bad, 'n_pending', 0), write_back=0, workspace=pick(bad, 'workspace', self.bufs['workspace'].data_ptr()),
                 workspace_bytes=self.need - bad.get('short', 0), planes_f16=pick(bad, 'planes_f16', self.bufs['planes_f16'].data_ptr()), host_planes=None,
                 track=pick(bad, 'track', self.track._h), traj_rows=pick(bad, 'traj_rows', self.rows.ctypes.data),
                 traj_start=pick(bad, 'traj_start', self.start.ctypes.data))
        if not self.v:
            return self.fn(self.hh(bad), *a.values(), pick(bad, 'n_rows', C.byref(self.n_rows)), self.stream())
        b = self.block
        for k, v in a.items():
            setattr(b, k, v if isinstance(v, int) or v is None else C.cast(v, C.c_void_p))
        then, box, now = self.tables
        b.n_rows, b.stream, b.hint_slot0, b.hint_F = SENT, self.ctx.stream_int(), 0, 4
        b.hint_then, b.hint_box, b.hint_cone, b.hint_now = pick(bad, 'hint_then', then.ctypes.data), box.ctypes.data, None, pick(bad, 'hint_now', now.ctypes.data)
        return self.fn(self.hh(bad), pick(bad, 'block', C.addressof(b)))

    def valid(self):
        self.outs.clear(), self.host.clear()
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        assert level1(self.ctx)[1:] == (0, 0, 4) and (not self.v or self.block.hinted == 0)
        p16 = self.bufs['planes_f16'].cpu().numpy().view(np.uint16).reshape(21, cr.PX, cr.PX)
        f16_matches(p16, oracle_planes(self.orc, self.frames, 0, 4, cr.SPLIT, self.args), self.symbol)
        self.L.check(self.L.expected())
        # the polylines: pca_host_ego_to_grid on poses - origin (host code, pinned by tests/test_host_logic.py)
        rel = np.ascontiguousarray(line_poses(4) - np.asarray(self.args[0]))
        rows, start = np.zeros(18), np.zeros(4, np.int32)
        R = np.eye(3)
        n = self.lib.pca_host_ego_to_grid(rel.ctypes.data, 4, R.ctypes.data, 0., 0., cr.VIEW, cr.PX, rows.ctypes.data, start.ctypes.data)
        assert n >= 3 and (self.block.n_rows if self.v else self.n_rows.value) == n
        assert np.array_equal(self.rows[:3 * n], rows[:3 * n]) and np.array_equal(self.start, start)
        return dict(BEV_RISE)


class FxD2H(Fx):
    """pca_host_d2h_async on the shared context; pca_host_d2h_wait on a private one, whose tickets are known."""
    def setup(self):
        self.data = np.arange(64, dtype=np.uint8) * 3 + 1
        self.dev = self.cu(self.data)
        self.pin = self.T.full((64, ), SENT, dtype=self.T.uint8).pin_memory()
        self.host['pinned'] = (lambda: bool((self.pin == SENT).all()), True)
        self.private = None
        if self.symbol == 'pca_host_d2h_wait':
            self.private = C.c_void_p()
            assert self.lib.pca_ctx_create(self.ctx.device_index, C.byref(self.private)) == 0
            self.h = self.private

    def call(self, **bad):
        if self.symbol == 'pca_host_d2h_wait':
            return self.fn(self.hh(bad), bad.get('ticket', 0) if bad else self.ticket)
        return self.fn(self.hh(bad), pick(bad, 'dev', self.dev.data_ptr()), pick(bad, 'pinned', self.pin.data_ptr()), pick(bad, 'bytes', 64), self.stream())

    def valid(self):
        self.host.clear()
        self.ticket = self.lib.pca_host_d2h_async(self.h, self.dev.data_ptr(), self.pin.data_ptr(), 64, self.stream())
        assert 0 <= self.ticket <= 63 and (self.private is None or self.ticket == 0), self.lib.pca_last_error(self.h)
        assert self.lib.pca_host_d2h_wait(self.h, self.ticket) == 0
        assert np.array_equal(self.pin.numpy(), self.data)
        return {}

    def close(self):
        if self.private is not None:
            self.lib.pca_ctx_destroy(self.private)


class FxWriter(Fx):
    """pca_deflate_chunks, its dynamic form and pca_adler32_chunks: four chunks of 96, 1, 0 and 33 bytes of one source."""
    ROWS = ((3, 96), (100, 1), (50, 0), (120, 33))

    def setup(self):
        from pca_amd.writer import DEFLATE_CHUNK_DTYPE
        rng = np.random.default_rng(8)
        self.src_h = np.repeat(rng.integers(0, 256, 40, dtype=np.uint8), 4)       # (runs: something to match)
        self.src = self.cu(self.src_h)
        self.table = self.cu(np.array([(o, n, 0) for o, n in self.ROWS], dtype=DEFLATE_CHUNK_DTYPE).view(np.uint8).copy())
        self.adler = self.symbol == 'pca_adler32_chunks'
        n = len(self.ROWS)
        if self.adler:
            self.out('out', n + 4, self.T.int32)
        else:
            self.cap = sum((9 * b + 7) // 8 + 16 for _, b in self.ROWS)
            self.out('out', self.cap + 64, self.T.uint8), self.out('sizes', n, self.T.int32), self.out('crcs', n, self.T.int32)
            self.out('workspace', int(self.lib.pca_deflate_workspace_bytes(n)) + 256, self.T.uint8)
        self.bufs = dict(self.outs)

    def call(self, **bad):
        head = [self.hh(bad), pick(bad, 'src', self.src.data_ptr()), pick(bad, 'table', self.table.data_ptr()), pick(bad, 'n_chunks', len(self.ROWS)),
                pick(bad, 'out', self.bufs['out'].data_ptr())]
        if not self.adler:
            head += [pick(bad, 'sizes', self.bufs['sizes'].data_ptr()), pick(bad, 'crcs', self.bufs['crcs'].data_ptr()),
                     pick(bad, 'workspace', self.bufs['workspace'].data_ptr())]
        return self.fn(*head, self.stream())

    def valid(self):
        import zlib
        self.outs.clear()
        ticket = self.call()
        assert ticket >= 0, self.lib.pca_last_error(self.h)
        assert self.lib.pca_host_d2h_wait(self.h, ticket) == 0
        raw = self.src_h.tobytes()
        if self.adler:
            got = self.bufs['out'].cpu().numpy().view(np.uint32)
            assert [int(v) for v in got[:4]] == [zlib.adler32(raw[o:o + n]) for o, n in self.ROWS] and (got[4:] == SENT).all()
            return {}
        sizes, crcs = self.bufs['sizes'].cpu().numpy().view(np.uint32), self.bufs['crcs'].cpu().numpy().view(np.uint32)
        out = self.bufs['out'].cpu().numpy()
        offs = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
        assert offs[-1] <= self.cap and (out[offs[-1]:] == SENT).all()
        for c, (o, n) in enumerate(self.ROWS):
            assert zlib.decompressobj(-15).decompress(out[offs[c]:offs[c + 1]].tobytes()) == raw[o:o + n], c
            assert crcs[c] == zlib.crc32(raw[o:o + n]), c
        d = zlib.decompressobj(-15)
        assert d.decompress(out[:offs[-1]].tobytes() + b'\x03\x00') == b''.join(raw[o:o + n] for o, n in self.ROWS) and d.eof
        return {}


class FxPreview(Fx):
    """pca_preview_sheets: one sample of the crafted block of tests/preview_common.py at px = 16, filter type 1."""
    def setup(self):
        import preview_common as pc
        from pca_amd.preview import panel_ranges, polyline_tables
        self.pc = pc
        planes, trajs = pc.crafted_block(cr.PX, 1)
        self.lut_h = pc.model_lut()
        self.sheet = pc.model_sheet(planes[0], trajs[0], self.lut_h)
        verts, lines = polyline_tables(trajs, cr.PX)
        assert len(verts) and len(lines)
        self.n_verts, self.n_lines = len(verts), len(lines)
        self.planes, self.verts, self.lines = self.cu(planes), self.cu(verts.reshape(-1).copy()), self.cu(lines.view(np.uint8).copy())
        self.lut = self.cu(self.lut_h)
        self.ranges = panel_ranges(pc.ELEV_RANGE)
        self.sb = pc.stream_bytes(cr.PX)
        self.out('out', self.sb + 64, self.T.uint8), self.out('workspace', int(self.lib.pca_preview_workspace_bytes(1, cr.PX)) + 256, self.T.uint8)
        self.bufs = dict(self.outs)

    def call(self, **bad):
        return self.fn(self.hh(bad), pick(bad, 'planes', self.planes.data_ptr()), pick(bad, 'k', 1), pick(bad, 'px', cr.PX), pick(bad, 'verts', self.verts.data_ptr()),
                       pick(bad, 'n_verts', self.n_verts), pick(bad, 'polylines', self.lines.data_ptr()), pick(bad, 'n_polylines', self.n_lines),
                       pick(bad, 'lut', self.lut.data_ptr()), pick(bad, 'ranges', self.ranges.ctypes.data), pick(bad, 'filter', 1),
                       pick(bad, 'out', self.bufs['out'].data_ptr()), pick(bad, 'workspace', self.bufs['workspace'].data_ptr()), self.stream())

    def valid(self):
        self.outs.clear()
        ticket = self.call()
        assert ticket >= 0, self.lib.pca_last_error(self.h)
        assert self.lib.pca_host_d2h_wait(self.h, ticket) == 0
        out = self.bufs['out'].cpu().numpy()
        assert out[:self.sb].tobytes() == self.pc.filter_rows(self.sheet, 1) and (out[self.sb:] == SENT).all()
        return {}


def icp_pair():
    """The third scene family of test_gpu_icp.test_icp_matches_kdtree_model (32 beams, 900 azimuths, 30 m; 0.9 m apart), each
    sweep cut to 300 points (core_refusals_common.icp_cut); cast once, shared, read-only."""
    if not _ICP:
        import test_gpu_icp as ti
        for name, args in (('a', (0.0, 0.0, 0.0, 5)), ('b', (0.9, 0.03, 0.008, 6))):
            pts = cr.icp_cut(ti.sweep(*args, n_beams=32, n_az=900, max_range=30.0))
            pts.setflags(write=False)
            _ICP[name] = pts
    return _ICP['a'], _ICP['b']


_ICP, _ICP_MODEL = {}, {}
ICP_TOL = 1e-2               # the bar test_gpu_icp.test_icp_matches_kdtree_model holds this scene family to


def icp_model(max_iter):
    """test_gpu_icp.icp_model run for exactly max_iter updates (rel = 0: no convergence test ends it), once per max_iter: T, rmse,
    updates taken, and the fitness of its final pose under the device's 4 m correspondence cap."""
    if max_iter not in _ICP_MODEL:
        import test_gpu_icp as ti
        from scipy.spatial import cKDTree
        a, b = icp_pair()
        Tm, rmse, it = ti.icp_model(a, b, max_iter=max_iter, rel=0.0)
        d, _ = cKDTree(b[:, :3].astype(np.float64)).query(a[:, :3].astype(np.float64) @ Tm[:3, :3].T + Tm[:3, 3])
        _ICP_MODEL[max_iter] = (Tm, rmse, it, float((d < 4.0).mean()))
    return _ICP_MODEL[max_iter]


def icp_close(T_out, fitness, rmse, iterations, max_iter):
    import test_gpu_icp as ti
    Tm, rmse_m, it_m, fit_m = icp_model(max_iter)
    Td = np.array(list(T_out)).reshape(4, 4)
    print('icp max_iter %d: |dt| %.3e, rot %.3e deg, |d rmse| %.3e, |d fitness| %.3e, iterations %d' % (
        max_iter, np.linalg.norm(Td[:3, 3] - Tm[:3, 3]), ti.rot_err_deg(Td[:3, :3] @ Tm[:3, :3].T), abs(rmse - rmse_m), abs(fitness - fit_m), iterations))
    assert it_m == max_iter and iterations == max_iter, (iterations, it_m, max_iter)
    assert np.linalg.norm(Td[:3, 3] - Tm[:3, 3]) < ICP_TOL
    assert ti.rot_err_deg(Td[:3, :3] @ Tm[:3, :3].T) < 60 * ICP_TOL
    assert abs(rmse - rmse_m) < ICP_TOL and abs(fitness - fit_m) < ICP_TOL
    assert np.array_equal(Td[3], [0, 0, 0, 1])


class FxIcp(Fx):
    ITER = 5

    def setup(self):
        a, b = icp_pair()
        self.src, self.tgt = self.cu(a), self.cu(b)
        self.need = int(self.lib.pca_icp_workspace_bytes(cr.ICP_N))
        self.out('workspace', self.need + 256, self.T.uint8)
        self.bufs = dict(self.outs)
        self.T_out, self.fit, self.rmse, self.it = (C.c_double * 16)(*[SENT] * 16), C.c_double(SENT), C.c_double(SENT), C.c_int(SENT)
        self.host['results'] = (lambda: list(self.T_out) + [self.fit.value, self.rmse.value, self.it.value], [float(SENT)] * 18 + [SENT])
        self.eye = f64s(np.eye(4))

    def call(self, **bad):
        return self.fn(self.hh(bad), pick(bad, 'src', self.src.data_ptr()), pick(bad, 'n_src', cr.ICP_N), pick(bad, 'tgt', self.tgt.data_ptr()),
                       pick(bad, 'n_tgt', cr.ICP_N), 1e3, self.eye, pick(bad, 'max_iter', self.ITER), 0.0, 0.0,
                       pick(bad, 'workspace', self.bufs['workspace'].data_ptr()), self.need - bad.get('short', 0), pick(bad, 'T_out', self.T_out),
                       C.byref(self.fit), C.byref(self.rmse), C.byref(self.it), self.stream())

    def valid(self):
        self.outs.clear(), self.host.clear()
        assert self.call() == 0, self.lib.pca_last_error(self.h)
        icp_close(self.T_out, self.fit.value, self.rmse.value, self.it.value, self.ITER)
        assert self.ctx.status() == 0
        return {'icp': 5 + 2 * (self.ITER + 1)}                          # the target's five kernels, then match + solve per pass; one pass more than updates


FIXTURES = {
    'pca_kitti_project_sample_filter': FxK1, 'pca_kitti_project_sample_filter_ex': FxK1,
    'pca_nusc_sample_filter_transform': FxK1n, 'pca_nusc_sample_filter_transform_ex': FxK1n, 'pca_nusc_sample_filter_transform_batch': FxK1n,
    'pca_nusc_project_cams': FxK0n, 'pca_sample_bilinear': FxBilinear, 'pca_image_to_nchw_f32': FxNchw,
    'pca_retransform': FxStore, 'pca_retransform_batch_tail': FxStore, 'pca_mark_dynamic': FxStore, 'pca_voxel_dedup': FxStore,
    'pca_bev_generate': FxBev, 'pca_bev_generate_ex': FxBev, 'pca_bev_generate_chain': FxBev, 'pca_bev_generate_many': FxMany, 'pca_bev_warp': FxWarp,
    'pca_kitti_integrate': FxIntegrate, 'pca_kitti_integrate_v': FxIntegrate, 'pca_kitti_generate_bev': FxGenerate, 'pca_kitti_generate_bev_v': FxGenerate,
    'pca_k1_defer': FxNoted, 'pca_k1_flush': FxNoted, 'pca_status': FxNoted, 'pca_bev_view_hint': FxHint, 'pca_bev_bin_range': FxHint,
    'pca_deflate_chunks': FxWriter, 'pca_deflate_chunks_dyn': FxWriter, 'pca_adler32_chunks': FxWriter, 'pca_preview_sheets': FxPreview,
    'pca_host_d2h_async': FxD2H, 'pca_host_d2h_wait': FxD2H, 'pca_icp_register': FxIcp,
}


def test_every_table_has_its_fixture():
    assert sorted(FIXTURES) == sorted(cr.TABLES)


# =============================================================================================================== 1: the tables
@pytest.mark.parametrize('symbol', sorted(cr.TABLES))
def test_refusals_launch_nothing_and_leave_the_outputs_alone(T, orc, symbol):
    fx = FIXTURES[symbol](T, orc, symbol)
    lib = fx.lib
    try:
        assert lib.pca_profile_enable(fx.h, 1) == 0
        for label, bad, msg in cr.TABLES[symbol]:
            rc = fx.call(**bad)
            err = lib.pca_last_error(None if bad.get('null_ctx') else fx.h).decode()
            assert rc == -1 and re.match(msg, err), (symbol, label, rc, err)
            fx.untouched(label)
        launched = counts(lib, fx.h)
        assert not any(launched.values()), (symbol, {k: v for k, v in launched.items() if v})
        rise = fx.valid()
        launched = counts(lib, fx.h)
        for name, n in launched.items():
            want = rise.get(name, 0)
            assert n in want if isinstance(want, tuple) else n == want, (symbol, name, n, want)
    finally:
        lib.pca_profile_enable(fx.h, 0)
        fx.close()


# ==================================================================================================== 2 (a): the bin range
def hint_tables8(visible):
    then = np.tile(np.eye(4)[:3].reshape(12), (8, 1))
    for f in range(8):
        if f not in visible:
            then[f, 3] = 1000.0
    box = np.tile(np.array([-16, 16, -16, 16, -1, 2], np.float32), (8, 1))
    return np.ascontiguousarray(then), np.ascontiguousarray(box), np.ascontiguousarray(np.eye(4)[:3].reshape(12))


class Window8:
    """The window of tests/test_gpu_cull_chain.py (8 frames of about 3000 points, every one inside the view) in a store, and the
    whole-window raster at the C ABI."""
    def __init__(self, T, orc):
        import test_gpu_cull_chain as tc
        from pca_amd.device_store import make_bev_params
        self.T, self.tc = T, tc
        self.frames = tc.window()
        self.st = st = tc.loaded_store(self.frames)
        self.ctx, self.lib, self.h = st.ctx, st.ctx.lib, st.ctx.h
        self.prm = make_bev_params(*tc.bev_args())
        self.n = sum(len(r) for r in self.frames)
        self.need = int(self.lib.pca_bev_workspace_bytes(self.n, tc.PX))
        self.ws = T.empty(self.need + 256, dtype=T.uint8, device='cuda')
        self.p64 = T.full((21, tc.PX, tc.PX), SENT, dtype=T.float64, device='cuda')
        self.p16 = T.full((21, tc.PX, tc.PX), SENT, dtype=T.int16, device='cuda')
        self.cstore = st.c_store()
        self.full = tc.oracle_window(orc, self.frames, 0, 8, tc.SPLIT, key='small')
        self.sub = tc.oracle_window(orc, self.frames, 2, 6, tc.SPLIT, key='small')
        assert not np.array_equal(self.full['planes'], self.sub['planes'])               # (a range left armed would show)
        assert not np.array_equal(self.full['f16'].view(np.uint16), self.sub['f16'].view(np.uint16))

    def raster_is_the_whole_window(self, name):
        st, tc = self.st, self.tc
        rc = self.lib.pca_bev_generate_chain(self.h, C.byref(self.cstore), None, st.frame_off.data_ptr(), st.head, st.head + tc.SPLIT, st.head + 8, self.n,
                                             C.byref(self.prm), None, None, 0, 0, self.ws.data_ptr(), self.need, self.p64.data_ptr(), self.p16.data_ptr(), None,
                                             self.ctx.stream())
        assert rc == 0, self.lib.pca_last_error(self.h)
        grid = level1(self.ctx)
        st.check_status()
        assert grid[2:] == (st.head, st.head + 8), (name, grid)
        assert_planes_match(self.p16.cpu().numpy().view(np.float16), self.p64.cpu().numpy(), self.full, name)


@pytest.mark.parametrize('how', ['a pose track one frame short', 'planes_f16 NULL'])
def test_a_refused_generate_bev_v_leaves_no_bin_range_armed(T, orc, how):
    """pca_kitti_generate_bev_v arms the hint's range (frames 2 .. 5 of 8) and is then refused by pca_kitti_generate_bev's own
    checks, before any raster could take the range: the plain raster that follows bins the whole window."""
    from pca_amd import _lib
    w = Window8(T, orc)
    then, box, now = hint_tables8(visible=(2, 3, 4, 5))
    track = c_track(line_poses(7 if how.startswith('a pose') else 8))
    rows, start = np.zeros(2 * 7 * 3), np.zeros(8, np.int32)
    b = _lib.PcaKittiGenerateBevArgs()
    b.store, b.frame_off = C.cast(C.pointer(w.cstore), C.c_void_p), w.st.frame_off.data_ptr()
    b.slot_begin, b.slot_split, b.slot_end, b.max_points = w.st.head, w.st.head + w.tc.SPLIT, w.st.head + 8, w.n
    b.prm, b.n_pending, b.write_back = C.addressof(w.prm), 0, 0
    b.workspace, b.workspace_bytes = w.ws.data_ptr(), w.need
    b.planes_f16 = None if how == 'planes_f16 NULL' else w.p16.data_ptr()
    b.host_planes, b.track, b.traj_rows, b.traj_start, b.stream = None, track._h, rows.ctypes.data, start.ctypes.data, w.ctx.stream_int()
    b.hint_slot0, b.hint_F, b.hint_then, b.hint_box, b.hint_cone, b.hint_now = w.st.head, 8, then.ctypes.data, box.ctypes.data, None, now.ctypes.data
    assert w.lib.pca_kitti_generate_bev_v(w.h, C.addressof(b)) == -1
    assert b.hinted == 1 and w.lib.pca_last_error(w.h).startswith(b'kitti_generate_bev: ')      # the hint DID narrow; the session call refused
    assert bool((w.p16 == SENT).all())
    w.raster_is_the_whole_window(how)


def test_a_view_hint_that_returns_0_replaces_an_armed_range(T, orc):
    """pca_bev_bin_range(head + 2, head + 6), then a hint that finds every frame in reach of the view (0): nothing stays armed."""
    w = Window8(T, orc)
    then, box, now = hint_tables8(visible=range(8))
    assert w.lib.pca_bev_bin_range(w.h, w.st.head + 2, w.st.head + 6) == 0
    assert w.lib.pca_bev_view_hint(w.h, w.st.head, 8, then.ctypes.data, box.ctypes.data, None, now.ctypes.data, C.addressof(w.prm)) == 0
    w.raster_is_the_whole_window('hint 0')


# ==================================================================================================== 2 (b): the deferred K1
BAD_FRAMES = {'points without pts': (dict(pts=None), r'k1: bad frame'), 'H -1': (dict(H=-1), 'k1: H and W must not be negative'),
              'W -1': (dict(W=-1), 'k1: H and W must not be negative'), 'H = W = -2': (dict(H=-2, W=-2), 'k1: H and W must not be negative'),
              'H W 3 >= 2^31': (dict(H=cr.HW_TOO_LARGE[0], W=cr.HW_TOO_LARGE[1]), 'k1: image too large')}


@pytest.mark.parametrize('what', sorted(BAD_FRAMES))
def test_a_deferred_k1_is_checked_when_it_is_noted(T, what):
    """pca_k1_defer(1) on a PRIVATE context, one refused pca_kitti_integrate, then pca_ctx_destroy at once, whatever the call
    answered: pca_ctx_destroy does not run a noted K1 (pca_api.hip: it frees and deletes), so a frame that was noted unchecked
    shows as a failed assertion below and never as a launch.  No path of this test launches anything."""
    from pca_amd import _lib
    lib = _lib.Context.get().lib
    bad, msg = BAD_FRAMES[what]
    sc = cr.kitti_scene()
    cu = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()
    pts, img, sem = cu(sc['frames'][3]), cu(sc['img']), cu(sc['sem'])
    x = T.zeros(64, dtype=T.float64, device='cuda')
    f32, i32, u8 = T.zeros(64, dtype=T.float32, device='cuda'), T.zeros(64, dtype=T.int32, device='cuda'), T.zeros(64, dtype=T.uint8, device='cuda')
    frame_off = T.zeros(4, dtype=T.int64, device='cuda')
    store = _lib.PcaStore(x.data_ptr(), x.data_ptr(), x.data_ptr(), f32.data_ptr(), i32.data_ptr(), i32.data_ptr(), u8.data_ptr(), 64, None)
    track = c_track(line_poses(3))
    o = _lib.PcaKittiObs()
    o.pts, o.rgb, o.sem, o.sem_gt, o.n, o.host_mask = pick(bad, 'pts', pts.data_ptr()), img.data_ptr(), sem.data_ptr(), None, len(pts), 0
    evicted, path = C.c_int64(SENT), C.c_double(SENT)
    T.cuda.synchronize()
    h = C.c_void_p()
    assert lib.pca_ctx_create(T.cuda.current_device(), C.byref(h)) == 0
    try:
        armed = lib.pca_k1_defer(h, 1)
        rc = lib.pca_kitti_integrate(h, C.byref(o), f64s(sc['P']), pick(bad, 'H', cr.H), pick(bad, 'W', cr.W), _lib.class_mask(cr.KITTI_FILTERS),
                                     C.byref(store), frame_off.data_ptr(), 0, 0, track._h, f64s(np.eye(4)), 1e9, C.byref(evicted), C.byref(path), None)
        err = lib.pca_last_error(h).decode()
    finally:
        lib.pca_ctx_destroy(h)
    assert armed == 0 and rc == -1 and re.match(msg, err), (what, rc, err)
    assert len(track) == 3 and evicted.value == SENT and path.value == SENT


def test_a_noted_k1_survives_a_refused_raster_and_rides_in_the_next(T, orc):
    """The good path, on the shared context: a valid frame is noted (no K1 launch), a raster of its window is refused (workspace
    one byte short), the same raster with the whole workspace takes the K1 along (Gk > 0, still no K1 launch of its own): planes
    and appended rows are the oracle's."""
    from pca_amd import _lib
    fx = FxIntegrate(T, orc, 'pca_kitti_integrate')
    lib, h, L = fx.lib, fx.h, fx.L
    sc = fx.sc
    ost = orc.Store(64)
    k = orc.kitti_project_sample_filter(ost, sc['frames'][3], sc['P'], sc['img'], sc['sem'], None, cr.H, cr.W, cr.KITTI_FILTERS)
    frames = fx.frames + [ost.rows()]
    args = cr.bev_args()
    from pca_amd.device_store import make_bev_params
    prm = make_bev_params(*args)
    n_max = L.total + 33
    need = int(lib.pca_bev_workspace_bytes(n_max, cr.PX))
    ws = T.full((need + 256, ), SENT, dtype=T.uint8, device='cuda')
    p64 = T.full((21, cr.PX, cr.PX), SENT, dtype=T.float64, device='cuda')
    p16 = T.full((21, cr.PX, cr.PX), SENT, dtype=T.int16, device='cuda')
    cstore = L.st.c_store()

    def raster(ws_bytes):
        return lib.pca_bev_generate_chain(h, C.byref(cstore), None, L.st.frame_off.data_ptr(), 0, cr.SPLIT, 4, n_max, C.byref(prm), None, None, 0, 0,
                                          ws.data_ptr(), ws_bytes, p64.data_ptr(), p16.data_ptr(), None, fx.stream())
    assert lib.pca_k1_defer(h, 1) == 0
    try:
        assert lib.pca_profile_enable(h, 1) == 0
        assert fx.call() == 0, lib.pca_last_error(h)                      # noted
        assert raster(need - 1) == -1 and lib.pca_last_error(h) == b'bev: workspace too small'
        T.cuda.synchronize()
        assert bool((p64 == SENT).all()) and bool((p16 == SENT).all()) and bool((ws == SENT).all())
        assert raster(need) == 0, lib.pca_last_error(h)
        grid = level1(fx.ctx)
        launched = counts(lib, h)
    finally:
        lib.pca_profile_enable(h, 0)
        assert lib.pca_k1_defer(h, 0) == 0
    assert grid[1] == 1 and grid[2:] == (0, 4), grid                      # the 33 points rode as one tile
    assert launched['kitti_project_sample_filter'] == 0 and launched['bev_bin'] == 1 and launched['bev_cells'] == 1, launched
    assert_planes_match(p16.cpu().numpy().view(np.float16), p64.cpu().numpy(), oracle_planes(orc, frames, 0, 4, cr.SPLIT, args), 'riding K1')
    exp, n0 = L.expected(), L.total
    for name, v in m.soa(ost.rows()).items():
        exp[name][n0:n0 + k] = v
    exp['frame_off'][4] = n0 + k
    L.check(exp)
    assert len(fx.track) == 4


# ==================================================================================================== 2 (c): ICP's pass count
@pytest.mark.parametrize('max_iter', [254, 255, 256, 300])
def test_icp_runs_every_pass_it_is_asked_for(T, orc, max_iter):
    """rel_fitness = rel_rmse = 0.0: `fabs(..) < 0` never ends a run, so the registration takes exactly max_iter updates -- across
    the 8 bits the pass count used to have -- and lands where the k-d-tree model lands after as many."""
    fx = FxIcp(T, orc, 'pca_icp_register')
    assert fx.call(max_iter=max_iter) == 0, fx.lib.pca_last_error(fx.h)
    icp_close(fx.T_out, fx.fit.value, fx.rmse.value, fx.it.value, max_iter)
    assert fx.ctx.status() == 0


def test_icp_refuses_more_passes_than_the_news_word_counts(T, orc):
    fx = FxIcp(T, orc, 'pca_icp_register')
    lib = fx.lib
    try:
        assert lib.pca_profile_enable(fx.h, 1) == 0
        assert fx.call(max_iter=cr.ICP_MAX_ITER + 1) == -1 and lib.pca_last_error(fx.h) == b'icp: max_iter must not exceed 32766'
        fx.untouched('max_iter')
        assert counts(lib, fx.h)['icp'] == 0
    finally:
        lib.pca_profile_enable(fx.h, 0)
