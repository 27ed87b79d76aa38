"""Device-resident point store: the HBM replacement of the reference's ``self.sem_pcs`` list.

Layout (include/pca.h): structure-of-arrays, frames are contiguous segments, the segment boundaries
``frame_off`` live on the device so that integrate() never reads a count back.  The host only tracks
UPPER bounds of the append position (every input point kept) for capacity planning; exact counts are
fetched lazily (``sizes()``) when somebody asks for rows.

Slots: frame k of the live window occupies slot ``head + k``; eviction advances ``head``; when slots or
capacity run out the live window is moved to the front (rare, amortised).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import PcaBevParams, PcaKittiFrame, PcaStore

# PCA_BEV_CULL=0: no raster is told which frames cannot reach its view (A/B -- results are identical)
CULL = os.environ.get('PCA_BEV_CULL', '1') != '0'


class DeviceStore:
    """The accumulated points in HBM (SoA) with the host-side bookkeeping of slots and owed re-transforms.
    NOTE: the coordinate tensors x / y / z lag behind by the re-transforms in `_pending` (up to CHAIN_MAX of them);
    every method of this class that reads coordinates applies them first.  Code that reads the tensors directly calls
    `flush_pending()` before."""
    CHAIN_MAX = 4            # owed re-transforms at most (PCA_BEV_MAX_CHAIN of the C ABI)
    CHAIN_K = int(os.environ.get('PCA_BEV_CHAIN', '4'))   # the rasteriser writes them back when this many are owed

    def __init__(self, capacity=1 << 24, max_frames=4096, device=None, intensity_div255=False):
        self.ctx = _lib.Context.get(device)
        self.device = torch.device('cuda', self.ctx.device_index)
        self.intensity_div255 = bool(intensity_div255)
        self.max_frames = int(max_frames)
        self._alloc(int(capacity))
        self.frame_off = torch.zeros(self.max_frames + 1, dtype=torch.int64, device=self.device)
        self._moved = np.eye(4)  # product of every transform applied to all live frames so far (newest on the left)
        self.cull = CULL         # tell the rasters which slots can reach their view (view_hint)
        self.hints_taken = 0     # rasters of this store that were told to leave frames out
        self._alloc_frame_tables(self.max_frames)
        self.head = 0            # first live slot
        self.tail = 0            # one past the last live slot
        self.ub_tail = 0         # upper bound of frame_off[tail]
        self.lb_head = 0         # lower bound of frame_off[head] (exact after a sync)
        self._ub = []            # per live frame: upper bound of its size (its input point count)
        self._ub_sum = 0         # sum(self._ub), kept incrementally
        self._pending = []       # [(T 16 doubles, end slot)], oldest first: re-transforms owed to slots [head, end slot)
        self._k1_cache = None
        self._k1_src = None      # (P object, filters object, their values) of the last append_kitti_obs
        self._ia = None          # argument block of pca_kitti_integrate_v, kept between calls
        self._ws = None
        self._ws_many = None
        self._ws_points, self._ws_px = 0, 0
        # scratch of bev_class_planes, of bev_elev_partition and of bev_voxel_labels, each its own (a main raster may have sized
        # _ws differently): name -> [buffer, the points it is sized for, px], see _side_workspace
        self._ws_side = {}
        self._render_keys = {}           # (H, W) -> the z-buffer's keys (render_camera)
        self._dedup_ws = None
        self._dist_ws = None              # pca_voxel_distance's scratch, grown to the largest volume seen
        self._match_ws = None             # pca_voxel_instance_match's scratch, grown to the largest call seen
        self._obs_out = None
        self._k1_noted = None    # what the K1 noted by the last append_kitti_obs still reads (device tensors), or None
        self._pend_T = (C.c_double * (16 * self.CHAIN_MAX))()      # the owed chain as the C calls take it
        self._pend_T_np = np.frombuffer(self._pend_T, dtype=np.float64)
        self._pend_ends = (C.c_int * self.CHAIN_MAX)()

    # ---- memory ----------------------------------------------------------------------------
    def _alloc(self, cap):
        d = self.device
        self.capacity = cap
        self._cstore = None
        self.x = torch.empty(cap, dtype=torch.float64, device=d)
        self.y = torch.empty(cap, dtype=torch.float64, device=d)
        self.z = torch.empty(cap, dtype=torch.float64, device=d)
        self.intensity = torch.empty(cap, dtype=torch.float32, device=d)
        self.rgbs = torch.empty(cap, dtype=torch.int32, device=d)     # bit pattern of the u32
        self.inst = torch.empty(cap, dtype=torch.int32, device=d)
        self.dyn = torch.empty(cap, dtype=torch.uint8, device=d)

    def _arrays(self):
        return (self.x, self.y, self.z, self.intensity, self.rgbs, self.inst, self.dyn)

    # ---- where the frames are (for pca_host_view_hull: include/pca.h) --------------------------
    BOX_EVERY = 16           # the frames' boxes are read back every so many append_kitti_obs (asynchronously; the frames that
                             # need their box are the OLD ones behind the view -- the new ones ahead of it are out by their cone)

    def _alloc_frame_tables(self, max_frames, keep=None):
        """Per slot: the box K1 leaves on the device (frame_box), what the host has seen of it (_box: lo > hi = not seen), the
        store's `moved` matrix when the frame was created (_then; NaN = unknown: the frame always counts as visible) and
        whether K1's camera test applied to it (_has_cone).  keep = (first, n): those rows move to the front."""
        n1 = max_frames + 1
        box = torch.zeros((n1, 6), dtype=torch.int32, device=self.device)
        then = np.full((n1, 12), np.nan)
        seen = np.tile(np.array([1, -1] * 3, dtype=np.float32), (n1, 1))
        cone = np.zeros(n1, dtype=bool)
        if keep is not None:
            a, n = keep
            box[:n] = self.frame_box[a:a + n]
            then[:n], seen[:n], cone[:n] = self._then[a:a + n], self._box[a:a + n], self._has_cone[a:a + n]
        self.frame_box, self._then, self._box, self._has_cone = box, then, seen, cone
        self._then_addr, self._box_addr = then.ctypes.data, seen.ctypes.data
        self._box_pin = None     # pinned landing block of the read-backs
        self._box_copy = None    # (event, first slot, slots) of the read-back in flight
        self._since_box = 0
        self._cone = None        # (key, 15 doubles) of the camera the live frames were taken with
        self._n_nocone = 0 if keep is None else int(np.count_nonzero(~cone[:keep[1]] & np.isfinite(then[:keep[1], 0])))   # noted frames without the camera test
        self._cstore = None

    def _note_moved(self, Ts):
        """Ts (k,16): transforms applied -- now or owed -- to EVERY live frame, in order."""
        for T in Ts:
            M = T.reshape(4, 4) @ self._moved
            M[3] = (0., 0., 0., 1.)                 # (the kernels apply rows 0..2 only: whatever a T's last row says, it is not applied)
            self._moved = M

    def _note_frame(self, slot, cone_key):
        """A frame K1 is about to put into `slot`, created under the current `moved`; cone_key: (P bytes, H, W) if K1's camera
        test applies to it, else None."""
        self._then[slot] = self._moved[:3].reshape(12)      # (its row of _box says "not seen": every slot is used once between slides)
        if cone_key is not None:
            if self._cone is None or self._cone[0] != cone_key:
                if self._cone is not None:                  # another camera: the frames taken with the old one lose their cone
                    self._has_cone[self.head:self.tail] = False
                    self._n_nocone = self.tail - self.head
                out = np.empty(15)
                Pm = np.frombuffer(cone_key[0], dtype=np.float64)
                self.ctx.lib.pca_host_camera_cone(Pm.ctypes.data, int(cone_key[1]), int(cone_key[2]), out.ctypes.data)
                self._cone = (cone_key, out, out.ctypes.data)
            self._has_cone[slot] = True
        else:
            self._n_nocone += 1
        self._since_box += 1
        self._poll_boxes()
        if self._since_box >= self.BOX_EVERY and self._box_copy is None:
            n = self.tail - self.head
            if n > 0:
                if self._box_pin is None or self._box_pin.shape[0] < self.frame_box.shape[0]:
                    self._box_pin = torch.empty(tuple(self.frame_box.shape), dtype=torch.int32, pin_memory=True)
                self._box_pin[:n].copy_(self.frame_box[self.head:self.tail], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._box_copy = (ev, self.head, n)
                self._since_box = 0

    def _poll_boxes(self):
        """Takes in a finished read-back: the rows K1 had filled by then (a row of zeros stays unknown)."""
        if self._box_copy is None or not self._box_copy[0].query():
            return
        _, first, n = self._box_copy
        self._box_copy = None
        rows = self._box_pin[:n].numpy()
        dec = np.empty((n, 6), dtype=np.float32)
        self.ctx.lib.pca_f32_box_decode(rows.ctypes.data, n, dec.ctypes.data)
        known = dec[:, 0] <= dec[:, 1]
        tgt = self._box[first:first + n]
        tgt[known] = dec[known]

    def view_hint_into(self, args, first_frame, last_frame):
        """The arguments of pca_bev_view_hint for live frames [first_frame, last_frame) written into the hint_* fields of an
        argument block (pca_kitti_generate_bev_v); returns hint_F (0: no hint)."""
        n = last_frame - first_frame
        if not self.cull or n < 4:
            return 0
        a = self.head + first_frame
        args.hint_slot0 = a
        args.hint_then, args.hint_box = self._then_addr + 96 * a, self._box_addr + 24 * a
        args.hint_cone = self._cone[2] if (self._cone is not None and self._n_nocone == 0) else None
        args.hint_now = self._moved.ctypes.data
        return n

    def view_hint(self, prm, first_frame, last_frame, write_back):
        """Tells the context which slots of live frames [first_frame, last_frame) can reach the view of `prm` (pca_bev_view_hint)
        before a raster that writes nothing back.  Returns 1 if frames will be left out."""
        n = last_frame - first_frame
        if not self.cull or write_back or n < 4:
            return 0
        a = self.head + first_frame
        cone = self._cone[2] if (self._cone is not None and self._n_nocone == 0) else None
        return self._count_hint(self.ctx.lib.pca_bev_view_hint(self.ctx.h, a, n, self._then_addr + 96 * a, self._box_addr + 24 * a, cone,
                                              self._moved.ctypes.data, C.addressof(prm)))

    def _count_hint(self, r):
        self.hints_taken += 1 if r > 0 else 0
        return r

    def c_store(self):
        if self._cstore is None:
            self._cstore = PcaStore(self.x.data_ptr(), self.y.data_ptr(), self.z.data_ptr(), self.intensity.data_ptr(),
                                    self.rgbs.data_ptr(), self.inst.data_ptr(), self.dyn.data_ptr(), self.capacity,
                                    self.frame_box.data_ptr())
        return self._cstore

    @property
    def n_frames(self):
        return self.tail - self.head

    def set_defer_k1(self, on):
        """pca_k1_defer for this store's context: the K1 of append_kitti_obs is left for the raster that follows it (it rides in
        that raster's first kernel; see include/pca.h).  Every library call that touches a store runs a noted K1 first; the
        methods of this class that read the arrays with torch (offsets, rows, reserve, ...) call flush_k1() themselves.  Code
        that reads self.x ... self.frame_off directly must call flush_k1() first."""
        self.ctx.check(self.ctx.lib.pca_k1_defer(self.ctx.h, 1 if on else 0))
        self.ctx.k1_defer = bool(on)              # (the switch belongs to the context: every store on it sees it)
        if not on:
            self._k1_noted = None

    def flush_k1(self):
        if self._k1_noted is not None:
            self.ctx.check(self.ctx.lib.pca_k1_flush(self.ctx.h))
            self._k1_noted = None

    def __del__(self):
        # a K1 noted for THIS store must not outlive its arrays (the context would run it later, into memory that torch has
        # handed to someone else by then)
        try:
            if self._k1_noted is not None:
                self.flush_k1()
        except Exception:
            pass

    def offsets(self):
        """Exact segment boundaries of the live frames (host numpy int64, length n_frames+1).  Synchronises."""
        self.flush_k1()
        off = self.frame_off[self.head:self.tail + 1].cpu().numpy()
        self.lb_head = int(off[0])
        self.ub_tail = int(off[-1])
        self._ub = [int(v) for v in np.diff(off)]
        self._ub_sum = sum(self._ub)
        return off

    def sizes(self):
        return np.diff(self.offsets())

    def poll_status(self):
        """check_status() without the wait (the host-visible mirror of the status word); for every call."""
        self.ctx.poll_status()

    def check_status(self):
        self.ctx.check_status()

    def reserve(self, n_new, n_slots=1):
        """Make room for n_slots more frames holding at most n_new points in total."""
        if self.tail + n_slots <= self.max_frames and self.ub_tail + n_new <= self.capacity:
            return
        self.flush_pending()
        off = self.offsets()                       # synchronises: exact numbers
        a, b = int(off[0]), int(off[-1])
        live, nf = b - a, self.n_frames
        new_cap = self.capacity
        while live + n_new > new_cap:
            new_cap *= 2
        new_maxf = self.max_frames
        while nf + n_slots > new_maxf:
            new_maxf *= 2
        old = self._arrays()
        if new_cap != self.capacity:
            self._alloc(new_cap)
            for dst, src in zip(self._arrays(), old):
                dst[:live] = src[a:b]
        elif a > 0:                                # slide the live window to the front
            for t in old:
                t[:live] = t[a:b].clone()
        self.max_frames = new_maxf
        new_off = torch.zeros(new_maxf + 1, dtype=torch.int64, device=self.device)
        new_off[:nf + 1] = torch.from_numpy(off - a).to(self.device)
        self.frame_off = new_off
        cone = self._cone
        self._alloc_frame_tables(new_maxf, keep=(self.head, nf))   # the live frames keep their rows, every other slot starts empty
        self._cone = cone
        self.head, self.tail = 0, nf
        self.lb_head, self.ub_tail = 0, live

    def evict(self, k):
        k = int(k)
        if self._n_nocone and k:                   # (frames K1 noted without its camera test: the others have no `then` at all)
            sl = slice(self.head, self.head + k)
            self._n_nocone -= int(np.count_nonzero(~self._has_cone[sl] & np.isfinite(self._then[sl, 0])))
        self.head += k
        self._ub_sum -= sum(self._ub[:int(k)])
        del self._ub[:int(k)]

    def max_window_points(self):
        return max(self._ub_sum, 1)

    def clear(self):
        self.flush_k1()
        self.head = self.tail = 0
        self.ub_tail = self.lb_head = 0
        self._ub = []
        self._ub_sum = 0
        self._pending = []
        self.frame_off.zero_()
        self._alloc_frame_tables(self.max_frames)
        self._moved = np.eye(4)

    # ---- K1: KITTI ------------------------------------------------------------------------
    @staticmethod
    def kitti_descs(frames):
        """The C descriptors of a list of frame dicts (see append_kitti)."""
        descs = (PcaKittiFrame * len(frames))()
        for k, f in enumerate(frames):
            n = int(f['pts'].shape[0])
            assert f['pts'].dtype == torch.float32 and f['pts'].is_contiguous()
            descs[k].pts = f['pts'].data_ptr() if n else None
            descs[k].rgb = f['rgb'].data_ptr() if f.get('rgb') is not None else None
            descs[k].sem = f['sem'].data_ptr() if f.get('sem') is not None else None
            descs[k].sem_gt = f['sem_gt'].data_ptr() if f.get('sem_gt') is not None else None
            descs[k].n = n
        return descs

    def append_kitti(self, frames, P, H, W, filters, descs=None, sample_mode='nearest'):
        """frames: list of dicts {pts (n,4) f32 cuda, rgb (H,W,3) u8 cuda | None, sem (H,W) u8 cuda | None,
        sem_gt (n,) u8 cuda | None}.  One call appends all of them (stable order) as new slots.
        descs: kitti_descs(frames) built earlier (a caller that replays the same batch).
        sample_mode: 'nearest' (the reference) or 'bilinear' (opt-in: bilinear rgb, class of the nearest pixel)."""
        lib, ctx = self.ctx.lib, self.ctx
        n_in = sum(int(f['pts'].shape[0]) for f in frames)
        self.reserve(n_in, len(frames))
        if descs is None:
            descs = self.kitti_descs(frames)
        st = self.c_store()
        # keyed on VALUES (12 doubles + a short list): a calibration or filter list mutated in place is seen
        key = (np.asarray(P, dtype=np.float64).tobytes(), tuple(int(c) for c in (filters or ())))
        if self._k1_cache is None or self._k1_cache[0] != key:
            self._k1_cache = (key, _lib.f64_array(P, 12), _lib.class_mask(filters))
        Pc, fmask = self._k1_cache[1], self._k1_cache[2]
        ctx.check(lib.pca_kitti_project_sample_filter_ex(ctx.h, descs, len(frames), Pc, int(H), int(W),
                                                         fmask, C.byref(st), self.frame_off.data_ptr(), self.tail,
                                                         _lib.SAMPLE_MODES[sample_mode], ctx.stream()))
        self.tail += len(frames)
        self.ub_tail += n_in
        self._ub += [int(f['pts'].shape[0]) for f in frames]
        self._ub_sum += n_in

    def append_kitti_obs(self, obs, P, H, W, filters, sample_mode='nearest', track=None, T_new_prev=None, horizon=0., keep=None):
        """One observation through pca_kitti_integrate: `obs` is a _lib.PcaKittiObs whose pointers are device pointers or --
        where its host_mask says so -- host arrays (staged by the library: one pinned block, one H2D copy).  With `track` (a
        host_logic.CPoseTrack) the pose bookkeeping of the frame happens in the same call: returns (evicted frames, path
        length | None); without, (None, None) and the caller steps its own track.  The caller evicts.
        keep: the objects behind the struct's device pointers; with set_defer_k1 they are held until the noted K1 has run."""
        lib, ctx = self.ctx.lib, self.ctx
        n = int(obs.n)
        self.reserve(n, 1)
        # keyed on VALUES (a calibration or filter list mutated in place is seen); the same objects as last time take the short way
        src = self._k1_src
        if src is not None and src[0] is P and src[1] is filters and P.tobytes() == src[2] and tuple(filters or ()) == src[3]:
            key = self._k1_cache[0]
        else:
            key = (np.asarray(P, dtype=np.float64).tobytes(), tuple(int(c) for c in (filters or ())))
            ok = isinstance(P, np.ndarray) and P.dtype == np.float64 and all(type(c) is int for c in (filters or ()))
            self._k1_src = (P, filters, key[0], key[1]) if ok else None
        if self._k1_cache is None or self._k1_cache[0] != key:
            self._k1_cache = (key, _lib.f64_array(P, 12), _lib.class_mask(filters))
        Pc, fmask = self._k1_cache[1], self._k1_cache[2]
        st = self.c_store()
        th = getattr(track, '_h', None)
        # the call's arguments live in a block that is kept between calls (pca_kitti_integrate_v): what does not change from
        # frame to frame -- calibration, filter, store, track -- is written when it changes, the rest per call
        a = self._ia
        if a is None:
            a = self._ia = _lib.PcaKittiIntegrateArgs()
            self._ia_T = np.zeros(16)
            self._ia_T_addr = self._ia_T.ctypes.data
            self._ia_const = None
        const = (id(obs), id(Pc), int(H), int(W), id(st), id(self.frame_off), sample_mode, th, float(horizon))
        if const != self._ia_const:
            a.obs, a.P, a.H, a.W, a.filter_mask = C.addressof(obs), C.addressof(Pc), int(H), int(W), C.addressof(fmask)
            a.store, a.frame_off, a.sample_mode = C.addressof(st), self.frame_off.data_ptr(), _lib.SAMPLE_MODES[sample_mode]
            a.track, a.horizon = getattr(th, 'value', th), float(horizon)
            self._ia_const = const
            self._ia_keep = (obs, Pc, fmask, st, self.frame_off)     # (what the addresses point into)
        a.slot = self.tail
        if th is not None:
            self._ia_T[:] = np.asarray(T_new_prev, dtype=np.float64).reshape(16)
            a.T_new_prev = self._ia_T_addr
        else:
            a.T_new_prev = None
        a.stream = ctx.stream_int() or None
        ctx.check(lib.pca_kitti_integrate_v(ctx.h, C.addressof(a)))
        self._k1_noted = (keep, ) if getattr(ctx, 'k1_defer', False) else None      # (the K1 noted by the call before has run by now)
        self._note_frame(self.tail, (key[0], int(H), int(W)) if obs.sem_gt is None else None)
        self.tail += 1
        self.ub_tail += n
        self._ub.append(n)
        self._ub_sum += n
        if th is None:
            return None, None
        v = a.path_length
        return int(a.evicted), (None if v != v else np.float64(v))

    # ---- K1n: NuScenes --------------------------------------------------------------------
    def append_nusc(self, pc, cam_idx, imgs, sems, T, filters, sample_mode='nearest'):
        lib, ctx = self.ctx.lib, self.ctx
        n = int(pc.shape[0])
        self.reserve(n)
        ncam, H, W = sems.shape
        st = self.c_store()
        ctx.check(lib.pca_nusc_sample_filter_transform_ex(ctx.h, pc.data_ptr(), cam_idx.data_ptr(), n, imgs.data_ptr(),
                                                          sems.data_ptr(), int(ncam), int(H), int(W),
                                                          _lib.f64_array(T, 16), _lib.class_mask(filters),
                                                          C.byref(st), self.frame_off.data_ptr(), self.tail,
                                                          _lib.SAMPLE_MODES[sample_mode], ctx.stream()))
        self.tail += 1
        self.ub_tail += n
        self._ub.append(n)
        self._ub_sum += n

    def append_nusc_many(self, frames, filters, sample_mode='nearest'):
        """frames: list of dicts {pc (n,7) f64 cuda, cam_idx (n,) i64 cuda, imgs (ncam,H,W,3) u8 cuda, sems (ncam,H,W) u8
        cuda, T (4,4) T_ego_world}.  ONE front + one append launch for all of them (pca_nusc_sample_filter_transform_batch):
        the stored rows are those of len(frames) append_nusc calls in order."""
        lib, ctx = self.ctx.lib, self.ctx
        if not frames:
            return
        ncam, H, W = (int(v) for v in frames[0]['sems'].shape)
        max_tiles = 16384
        b0 = 0
        while b0 < len(frames):                               # the C call takes at most 16384 tiles of 512 points
            tiles, b1 = 0, b0
            while b1 < len(frames):
                t = max((int(frames[b1]['pc'].shape[0]) + 511) // 512, 1)
                if b1 > b0 and tiles + t > max_tiles:
                    break
                tiles += t
                b1 += 1
            part = frames[b0:b1]
            n_in = sum(int(f['pc'].shape[0]) for f in part)
            self.reserve(n_in, len(part))
            descs = (_lib.PcaNuscFrame * len(part))()
            keep = []
            for k, f in enumerate(part):
                assert f['pc'].dtype == torch.float64 and f['pc'].is_contiguous() and f['cam_idx'].dtype == torch.int64
                assert tuple(f['sems'].shape) == (ncam, H, W) and f['imgs'].is_contiguous() and f['sems'].is_contiguous()
                n = int(f['pc'].shape[0])
                Tc = _lib.f64_array(f['T'], 16)
                keep.append(Tc)
                descs[k].pc = f['pc'].data_ptr() if n else None
                descs[k].cam_idx = f['cam_idx'].data_ptr() if n else None
                descs[k].imgs, descs[k].sems = f['imgs'].data_ptr(), f['sems'].data_ptr()
                descs[k].n = n
                descs[k].T = C.cast(Tc, C.POINTER(C.c_double))
            st = self.c_store()
            ctx.check(lib.pca_nusc_sample_filter_transform_batch(ctx.h, descs, len(part), ncam, H, W, _lib.class_mask(filters),
                                                                 C.byref(st), self.frame_off.data_ptr(), self.tail,
                                                                 _lib.SAMPLE_MODES[sample_mode], ctx.stream()))
            self.tail += len(part)
            self.ub_tail += n_in
            self._ub += [int(f['pc'].shape[0]) for f in part]
            self._ub_sum += n_in
            b0 = b1

    # ---- K2 / K3 --------------------------------------------------------------------------
    def retransform(self, Ts, defer=False):
        """Applies the 4x4 transform(s) to every live point, in order (Ts: (4,4) or (k,4,4)).
        defer=True (single transform): the transform is only recorded; it is applied by the next consumer
        of the coordinates -- fused into the BEV rasteriser's first pass if that comes next (it reads every
        coordinate anyway), otherwise by a K2 launch (`flush_pending`).  Up to CHAIN_MAX transforms may be owed at a
        time: the rasteriser applies all of them to what it reads and writes the result back only every CHAIN_K-th time
        (the write-back is 24 B per stored point).  Results are bit-identical either way: one fma chain per transform."""
        if self.n_frames == 0:
            return
        Ts = np.ascontiguousarray(Ts, dtype=np.float64).reshape(-1, 16)
        self._note_moved(Ts)
        if defer and Ts.shape[0] == 1:
            if len(self._pending) >= self.CHAIN_MAX:
                self.flush_pending()
            self._pending.append((Ts[0].copy(), self.tail))
            return
        self.flush_pending()
        self._launch_retransform(Ts, self.head, self.tail)

    def _launch_retransform(self, Ts, begin_slot, end_slot):
        st = self.c_store()
        ctx = self.ctx
        ctx.check(ctx.lib.pca_retransform(ctx.h, C.byref(st), self.frame_off.data_ptr(), begin_slot, end_slot,
                                          _lib.f64_array(Ts, Ts.size), Ts.shape[0], ctx.stream()))

    def retransform_batch(self, Ts, n_new):
        """After append_kitti of `n_new` frames in one call: applies the per-frame transforms Ts (n_new,4,4) exactly as
        n_new successive integrate() steps would have -- frames stored before the batch get all of them, frame i of the
        batch gets Ts[i+1:] (nothing is ever transformed by its own frame's T)."""
        Ts = np.ascontiguousarray(Ts, dtype=np.float64).reshape(-1, 16)
        assert Ts.shape[0] == n_new
        self.flush_pending()
        self._note_moved(Ts)                      # (the batch's own frames have no `then`: they always count as visible)
        first_new = self.tail - n_new
        if first_new > self.head:
            st, ctx = self.c_store(), self.ctx
            ctx.check(ctx.lib.pca_retransform(ctx.h, C.byref(st), self.frame_off.data_ptr(), self.head, first_new,
                                              _lib.f64_array(Ts, Ts.size), Ts.shape[0], ctx.stream()))
        st, ctx = self.c_store(), self.ctx
        ctx.check(ctx.lib.pca_retransform_batch_tail(ctx.h, C.byref(st), self.frame_off.data_ptr(), first_new, n_new,
                                                     _lib.f64_array(Ts, Ts.size), ctx.stream()))

    def flush_pending(self):
        """Applies the owed transforms with K2: the slots between two consecutive end slots owe the same transforms (all
        the later ones), so every stored point is touched once."""
        pend, self._pending = self._pending, []
        begin = self.head
        for k, (_, end_slot) in enumerate(pend):
            if end_slot > begin:
                self._launch_retransform(np.stack([T for T, _ in pend[k:]]), begin, end_slot)
                begin = end_slot

    def mark_dynamic(self, pairs):
        """pairs: iterable of (frame index in the live window, instance index)."""
        pairs = list(pairs)
        if not pairs:
            return
        slots = (C.c_int32 * len(pairs))(*[self.head + int(f) for f, _ in pairs])
        insts = (C.c_int32 * len(pairs))(*[int(i) for _, i in pairs])
        st = self.c_store()
        ctx = self.ctx
        ctx.check(ctx.lib.pca_mark_dynamic(ctx.h, C.byref(st), self.frame_off.data_ptr(), slots, insts, len(pairs),
                                           ctx.stream()))

    def voxel_dedup(self, voxel_size):
        """Opt-in (no reference counterpart): of all live points in one voxel floor(xyz / voxel_size) only the first
        in store order (the oldest observation) stays; frames are compacted in place, order-preserving.
        Voxel indices are clamped to [-2^20, 2^20) per axis (+-2^20 * voxel_size metres): the points beyond that share the
        boundary voxel of their side, of which only the first stays."""
        if self.n_frames == 0:
            return
        self.flush_pending()
        ctx, lib = self.ctx, self.ctx.lib
        max_points = self.max_window_points()
        need = lib.pca_voxel_dedup_workspace_bytes(max_points, self.n_frames)
        if self._dedup_ws is None or self._dedup_ws.numel() < need:
            self._dedup_ws = torch.empty(int(need) + 256, dtype=torch.uint8, device=self.device)
        st = self.c_store()
        ctx.check(lib.pca_voxel_dedup(ctx.h, C.byref(st), self.frame_off.data_ptr(), self.head, self.tail,
                                      float(voxel_size), max_points, self._dedup_ws.data_ptr(),
                                      self._dedup_ws.numel(), ctx.stream()))

    # ---- BEV ------------------------------------------------------------------------------
    def bev(self, split_frame, prm, want_f64=False, intensity64=None, first_frame=0, last_frame=None, out16=None,
            extra=None):
        """Rasterises live frames [first_frame, last_frame) with 'present' = frames before split_frame.
        Returns (planes_f16 [21,px,px] cuda float16, planes_f64 or None).
        extra: optional cuda f64 [3, len(_lib.BEV_EXTRA_PLANES), px, px] receiving the opt-in extra reducers."""
        ctx, lib = self.ctx, self.ctx.lib
        last_frame = self.n_frames if last_frame is None else last_frame
        px = int(prm.px)
        max_points = self.bev_workspace(px)
        if out16 is not None:
            assert out16.dtype == torch.float16 and out16.is_contiguous() and tuple(out16.shape) == (21, px, px)
        p16 = out16 if out16 is not None else torch.empty((21, px, px), dtype=torch.float16, device=self.device)
        p64 = torch.empty((21, px, px), dtype=torch.float64, device=self.device) if want_f64 else None
        st = self.c_store()
        n_pend, pend_T, pend_ends, write_back = self.bev_pending(first_frame, last_frame)
        if extra is not None:
            assert extra.dtype == torch.float64 and extra.is_contiguous() \
                and tuple(extra.shape) == (3, len(_lib.BEV_EXTRA_PLANES), px, px)
        self.view_hint(prm, first_frame, last_frame, n_pend > 0 and write_back)     # (right in front of the call it is meant for)
        ctx.check(lib.pca_bev_generate_chain(ctx.h, C.byref(st), None if intensity64 is None else intensity64.data_ptr(),
                                             self.frame_off.data_ptr(), self.head + first_frame, self.head + split_frame,
                                             self.head + last_frame, max_points, C.byref(prm), pend_T, pend_ends, n_pend,
                                             write_back, self._ws.data_ptr(), self._ws.numel(),
                                             None if p64 is None else p64.data_ptr(), p16.data_ptr(),
                                             None if extra is None else extra.data_ptr(), ctx.stream()))
        self.bev_done(write_back)                  # only now: a failed call above leaves the owed re-transforms owed
        return p16, p64

    def bev_workspace(self, px):
        """Makes sure the raster's scratch fits the live window at `px`; returns the window's point bound (max_points)."""
        max_points = self.max_window_points()
        if self._ws is None or max_points > self._ws_points or px != self._ws_px:
            # sized with headroom so that a window growing frame by frame does not reallocate every call
            self._ws_points, self._ws_px = int(max_points * 1.25) + 1, px
            need = self.ctx.lib.pca_bev_workspace_bytes(self._ws_points, px)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(int(need) + 256, dtype=torch.uint8, device=self.device)
        return max_points

    def bev_pending(self, first_frame, last_frame):
        """The owed re-transforms as a raster over live frames [first_frame, last_frame) takes them (oldest first; they are
        written back only when CHAIN_K of them are owed): (n_pend, Ts, slot ends, write_back) for pca_bev_generate_chain.
        A raster that does not cover what they are owed to gets them flushed first (K2)."""
        if not self._pending:
            return 0, None, None, 1
        if first_frame != 0 or self._pending[-1][1] > self.head + last_frame:
            self.flush_pending()
            return 0, None, None, 1
        n_pend = 0
        for T, e in self._pending:
            if e > self.head:
                self._pend_T_np[16 * n_pend:16 * n_pend + 16] = T
                self._pend_ends[n_pend] = int(e)
                n_pend += 1
        if n_pend == 0:
            return 0, None, None, 0
        return n_pend, self._pend_T, self._pend_ends, (1 if n_pend >= self.CHAIN_K else 0)

    def _owed_read_only(self, first_frame, last_frame):
        """The owed re-transforms as a read-only pass over ANY live frames [first_frame, last_frame) can take them without a
        flush: a transform owed by the slots below e is owed by the window's slots below min(e, the window's end) -- the C
        calls refuse an end beyond the window and give a transform whose end lies at or below the window's first slot to no
        point.  (n_pend, Ts, slot ends, 0); nothing is written back and the chain stays owed."""
        n_pend, end = 0, self.head + last_frame
        for T, e in self._pending:
            if e > self.head:
                self._pend_T_np[16 * n_pend:16 * n_pend + 16] = T
                self._pend_ends[n_pend] = min(int(e), end)
                n_pend += 1
        return (n_pend, self._pend_T, self._pend_ends, 0) if n_pend else (0, None, None, 0)

    def bev_done(self, write_back):
        """After a raster call of this store has returned."""
        if self._pending and write_back:
            self._pending = []
        self._k1_noted = None                      # (a raster takes a noted K1 along or runs it first: nothing is noted any more)

    def _side_workspace(self, name, workspace_bytes, max_points, px):
        """The scratch of a side pass (bev_class_planes, bev_elev_partition, bev_voxel_labels, bev_voxel_carve, bev_voxel_instances), fit for
        max_points at `px`."""
        ws = self._ws_side.setdefault(name, [None, 0, 0])
        if ws[0] is None or max_points > ws[1] or px != ws[2]:
            # sized with headroom so that a window growing frame by frame does not reallocate every call
            ws[1], ws[2] = int(max_points * 1.25) + 1, px
        need = workspace_bytes(ws[1], px)              # (asked every call: PCA_BEV_CLASS_G / _ELEV_G / _VOXEL_G change it)
        if ws[0] is None or ws[0].numel() < need:
            ws[0] = torch.empty(int(need) + 256, dtype=torch.uint8, device=self.device)
        return ws[0]

    def _window_pass(self, prm, first_frame, last_frame, max_points=None, side=None, writes=False, keep_owed=False):
        """What every read-only pass over live frames [first_frame, last_frame) is called with (bev_class_planes,
        bev_elev_partition, bev_voxel_labels, bev_voxel_rays, bev_voxel_carve, bev_voxel_instances and render_camera, whose `prm`
        is its camera block; the next pass of the family starts here): last_frame's default, max_points' default (the window's own
        bound), the scratch for side = (name, pca_*_workspace_bytes) and -- `writes`: the caller stores afterwards, mark_dyn --
        the owed chain flushed.  Returns (last_frame, max_points, call); call(fn, own, outs, split_frame=None) is the C call
            fn(ctx, store, frame_off, slots, max_points, prm, *own, owed chain, [workspace], *outs' pointers, stream)
        with the owed chain taken read-only from bev_pending (which flushes it when the window does not cover what is owed;
        keep_owed: from _owed_read_only, which never flushes).
        The C call runs a noted K1 first: after it nothing is noted any more; a refused call raises and leaves it noted."""
        if writes:
            self.flush_pending()
        last_frame = self.n_frames if last_frame is None else last_frame
        max_points = self.max_window_points() if max_points is None else max(int(max_points), 1)
        ws = None if side is None else self._side_workspace(*side, max_points, int(prm.px))

        def call(fn, own, outs, split_frame=None):
            ctx = self.ctx
            n_pend, pend_T, pend_ends, _ = (self._owed_read_only if keep_owed else self.bev_pending)(first_frame, last_frame)
            slots = [self.head + f for f in (first_frame, split_frame, last_frame) if f is not None]
            st = self.c_store()
            ctx.check(fn(ctx.h, C.byref(st), self.frame_off.data_ptr(), *slots, max_points, C.byref(prm), *own, pend_T, pend_ends,
                         n_pend, *(() if ws is None else (ws.data_ptr(), ws.numel())),
                         *(None if t is None else t.data_ptr() for t in outs), ctx.stream()))
            self._k1_noted = None
        return last_frame, max_points, call

    def _window_extent(self, first_frame, last_frame, max_points, per_point):
        """(first point, per_point[:exact length, cut at max_points]) of live frames [first_frame, last_frame): one synchronising read-back."""
        lo, hi = self.frame_off[[self.head + first_frame, self.head + last_frame]].tolist()
        return lo, per_point[:min(hi - lo, max_points)]

    def _mark_dyn(self, lo, flags):
        self.dyn[lo + torch.nonzero(flags == 1).squeeze(1)] = 1

    def bev_class_planes(self, split_frame, prm, groups, first_frame=0, last_frame=None, want_counts=False):
        """Planes of any semantic class groups over live frames [first_frame, last_frame), 'present' = frames before
        split_frame (pca_bev_class_planes: one counts-only pass for all groups).  groups: a list of class-index lists (1..16
        of them, they may overlap).  Returns (prob_f16, prob_f64, counts | None) as cuda tensors: [3, len(groups), px, px]
        float16 / float64 and -- want_counts -- [3, len(groups) + 1, px, px] int32 holding the u32 counts per group, the last
        slot every static point; set order {present, future, full}.  The store is not written: owed re-transforms are applied
        to what the call reads and stay owed."""
        lib = self.ctx.lib
        px, ng = int(prm.px), len(groups)
        cg = (_lib.PcaClassGroup * max(ng, 1))()
        for k, g in enumerate(groups):
            cg[k].mask[:] = list(_lib.class_mask(g))
        _, _, call = self._window_pass(prm, first_frame, last_frame, side=('class', lib.pca_bev_class_workspace_bytes))
        shape = (3, max(ng, 1), max(px, 1), max(px, 1))
        p16 = torch.empty(shape, dtype=torch.float16, device=self.device)
        p64 = torch.empty(shape, dtype=torch.float64, device=self.device)
        cnt = torch.empty((3, shape[1] + 1) + shape[2:], dtype=torch.int32, device=self.device) if want_counts else None
        call(lib.pca_bev_class_planes, (cg, ng), (p64, p16, cnt), split_frame=split_frame)
        return p16, p64, cnt

    def bev_elev_partition(self, prm, elev_thresh, first_frame=0, last_frame=None, include_dyn=False, mark_dyn=False,
                           max_points=None):
        """Live frames [first_frame, last_frame) partitioned by height above the cell minimum (pca_bev_elev_partition; the
        reference's static_obj_partitioning_by_elev, sem_bev.py:556-591, in the frame of `prm`): a point is ELEVATED if its z
        in the BEV frame lies more than elev_thresh (it may be negative) above the minimum z of its cell.  include_dyn=False:
        points with dyn == 1 take no part (the static partition of generate_bev); True: every point does.
        Returns a dict of cuda tensors: 'elev' float64 (px, px), the cell minimum (0 where nothing was seen), image rows;
        'observed' bool (px, px); 'flags' uint8, one per point of the window in store order (0 kept, 1 elevated, 255 not in
        view); 'counts' int64 [3] = points in view, elevated, not elevated.  (The length of 'flags' is the window's exact
        point count: one offset is read back, the call synchronises.)
        The store is not written: owed re-transforms are applied to what the call reads and stay owed -- unless mark_dyn=True,
        the only path that alters the store: the elevated points get dyn = 1 (owed re-transforms are flushed first).  The
        mark is made in THIS view's cells and persists: every later raster, of any view, treats these points as dynamic.
        max_points: the bound at which the window is cut (default: the live window's own bound)."""
        lib = self.ctx.lib
        last_frame, max_points, call = self._window_pass(prm, first_frame, last_frame, max_points, writes=mark_dyn,
                                                         side=('elev', lib.pca_bev_elev_workspace_bytes))
        side = max(int(prm.px), 1)
        elev = torch.empty((side, side), dtype=torch.float64, device=self.device)
        obs = torch.empty((side, side), dtype=torch.uint8, device=self.device)
        flags = torch.empty(max_points, dtype=torch.uint8, device=self.device)
        counts = torch.empty(3, dtype=torch.int64, device=self.device)
        call(lib.pca_bev_elev_partition, (float(elev_thresh), 1 if include_dyn else 0), (elev, obs, flags, counts))
        lo, flags = self._window_extent(first_frame, last_frame, max_points, flags)
        if mark_dyn:
            self._mark_dyn(lo, flags)
        return {'elev': elev, 'observed': obs.bool(), 'flags': flags, 'counts': counts}

    def bev_voxel_labels(self, prm, z_lo, z_step, nz, label_of, n_labels, first_frame=0, last_frame=None, include_dyn=False,
                         max_points=None, keep_owed=False):
        """Live frames [first_frame, last_frame) voxelised into semantic occupancy labels (pca_bev_voxel_labels): the grid of
        `prm` with nz height bins of z_step metres from z_lo (z in the BEV frame; outside the range a point is dropped, not
        clamped), a majority vote per voxel.  label_of: 256 entries, class -> label below n_labels, 255 = the class takes
        no part.  include_dyn=False: points with dyn == 1 take no part.
        Returns a dict of cuda tensors, each [nz, px, px], image rows: 'labels' uint8, the smallest label among the most
        frequent ones (255: an empty voxel -- free or unseen is not decided here: bev_voxel_rays); 'counts' and 'top'
        int32 holding the u32 numbers of labelled points and of points of the winning label.
        The store is not written: owed re-transforms are applied to what the call reads and stay owed.
        max_points: the bound at which the window is cut (default: the live window's own bound).  keep_owed: a window that
        does not cover what is owed (it starts behind frame 0 or ends before the newest owing frame) has the owed
        re-transforms flushed first by default; True leaves the store alone there too."""
        lib = self.ctx.lib
        px = int(prm.px)
        table = np.ascontiguousarray(label_of, dtype=np.uint8)
        if table.shape != (256, ):
            raise ValueError('label_of must hold 256 entries')
        _, _, call = self._window_pass(prm, first_frame, last_frame, max_points, side=('voxel', lib.pca_bev_voxel_workspace_bytes),
                                       keep_owed=keep_owed)
        shape = (max(int(nz), 1), max(px, 1), max(px, 1))
        labels = torch.empty(shape, dtype=torch.uint8, device=self.device)
        counts = torch.empty(shape, dtype=torch.int32, device=self.device)
        top = torch.empty(shape, dtype=torch.int32, device=self.device)
        call(lib.pca_bev_voxel_labels, (float(z_lo), float(z_step), int(nz), table.ctypes.data, int(n_labels),
                                        1 if include_dyn else 0), (labels, counts, top))
        return {'labels': labels, 'counts': counts, 'top': top}

    def bev_voxel_rays(self, prm, z_lo, z_step, nz, origins, first_frame=0, last_frame=None, include_dyn=False,
                       max_points=None):
        """One lidar ray per stored point of the live frames [first_frame, last_frame), cast through the voxel grid of
        bev_voxel_labels (pca_bev_voxel_rays): from the sensor position of the point's frame to the point.  origins:
        [frames, 3], a numpy array or a tensor, row i = the sensor position of frame first_frame + i in the store's current
        coordinates (the pose track: it owes nothing); uploaded as f64.  The crop, the height filter and the class play no
        part; include_dyn=False: points with dyn == 1 cast no ray.
        Returns a dict of cuda tensors: 'seen' uint8 [nz, px, px], image rows, 1 = at least one ray passed through the voxel
        (the end voxel of a ray is not marked by that ray); 'stats' int64 [4]: points considered, rays cast, rays dropped
        for a coordinate that is not finite (or beyond 2^30), rays dropped for more than 16 384 voxel steps.
        The store is not written: owed re-transforms are applied to what the call reads and stay owed.
        max_points: the bound at which the window is cut (default: the live window's own bound)."""
        last_frame, max_points, call = self._window_pass(prm, first_frame, last_frame, max_points)
        px = int(prm.px)
        org = self._origins_of(origins, last_frame - first_frame)
        shape = (max(int(nz), 1), max(px, 1), max(px, 1))
        seen = torch.empty(shape, dtype=torch.uint8, device=self.device)
        stats = torch.empty(4, dtype=torch.int64, device=self.device)
        call(self.ctx.lib.pca_bev_voxel_rays, (float(z_lo), float(z_step), int(nz), 1 if include_dyn else 0, org.data_ptr()),
             (seen, stats))
        return {'seen': seen, 'stats': stats}

    def _origins_of(self, origins, n_frames):
        """origins [n_frames, 3] (numpy or tensor) as an f64 device tensor; a valid pointer even for no frame."""
        if isinstance(origins, torch.Tensor):
            org = origins.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            org = torch.from_numpy(np.ascontiguousarray(origins, dtype=np.float64)).to(self.device)
        if org.dim() != 2 or org.shape[1] != 3 or org.shape[0] != n_frames:
            raise ValueError('origins must be [frames, 3], one row per frame of the range')
        if org.shape[0] == 0:
            org = torch.zeros((1, 3), dtype=torch.float64, device=self.device)     # (never read)
        return org

    def bev_voxel_carve(self, prm, z_lo, z_step, nz, origins, classes, end_margin=1, min_cross=2, ratio=1.0, first_frame=0,
                        last_frame=None, include_dyn=False, mark_dyn=False, max_points=None):
        """Free-space carving by ray hit / miss over the live frames [first_frame, last_frame) (pca_bev_voxel_carve): the
        rays of bev_voxel_rays (same grid, same origins, same drop rules), counted.  Per voxel, 'hits' = the rays that end in
        it and 'cross' = the rays that pass through it at a step more than end_margin steps before their own end -- counted
        only for CANDIDATE voxels, those in which a point of `classes` (a list of class indices: the classes that can move)
        ends; 0 elsewhere.  A candidate point is FLAGGED iff cross >= min_cross and cross >= ratio * hits in its voxel: beams
        of other moments went straight through where it was seen, so it belonged to something that moved.  The rays of a
        point's own frame count like any other: end_margin keeps a surface from carving itself, ratio keeps a surface that is
        hit as often as it is crossed.  include_dyn=False: points with dyn == 1 take no part.
        The defaults (1, 2, 1.0) are this project's choice, checked on a synthetic scene only (tests/test_voxel_carve_model.py:
        a car that leaves is flagged whole, a parked one not at all); no real-data number exists.
        Returns a dict of cuda tensors: 'hits' and 'cross' int32 [nz, px, px] holding the u32 counts, image rows; 'flags'
        uint8, one per point of the window in store order (1 flagged, 0 candidate kept, 255 everything else; the window's
        exact length: one offset is read back, the call synchronises); 'stats' int64 [6]: points that take part, rays cast,
        dropped not finite, dropped too long, candidate points, flagged points.
        The store is not written: owed re-transforms are applied to what the call reads and stay owed -- unless mark_dyn=True,
        the only path that alters the store: the flagged points get dyn = 1, for good (owed re-transforms are flushed first).
        max_points: the bound at which the window is cut (default: the live window's own bound)."""
        lib = self.ctx.lib
        if not 0 <= int(min_cross) < 1 << 32 or not -(1 << 31) <= int(end_margin) < 1 << 31:
            raise ValueError('min_cross must fit an unsigned, end_margin a signed 32-bit integer')
        nz = int(nz)
        last_frame, max_points, call = self._window_pass(
            prm, first_frame, last_frame, max_points, writes=mark_dyn,
            side=('carve', lambda m, px: lib.pca_bev_carve_workspace_bytes(m, px, nz)))
        org = self._origins_of(origins, last_frame - first_frame)
        only = _lib.PcaClassGroup()
        only.mask[:] = list(_lib.class_mask(classes))
        px = int(prm.px)
        shape = (max(nz, 1), max(px, 1), max(px, 1))
        hits = torch.empty(shape, dtype=torch.int32, device=self.device)
        cross = torch.empty(shape, dtype=torch.int32, device=self.device)
        flags = torch.empty(max_points, dtype=torch.uint8, device=self.device)
        stats = torch.empty(6, dtype=torch.int64, device=self.device)
        call(lib.pca_bev_voxel_carve, (float(z_lo), float(z_step), nz, 1 if include_dyn else 0, org.data_ptr(), only,
                                       int(end_margin), int(min_cross), float(ratio)), (hits, cross, flags, stats))
        lo, flags = self._window_extent(first_frame, last_frame, max_points, flags)
        if mark_dyn:
            self._mark_dyn(lo, flags)
        return {'hits': hits, 'cross': cross, 'flags': flags, 'stats': stats}

    def bev_voxel_instances(self, prm, z_lo, z_step, nz, label_of, n_labels, min_points=1, connectivity=26, min_voxels=1,
                            max_instances=4096, dyn='static', first_frame=0, last_frame=None, max_points=None):
        """The object voxels of the live frames [first_frame, last_frame) clustered into instances (pca_bev_voxel_instances):
        connected components of the voxels of bev_voxel_labels' grid that hold at least min_points kept points (same
        geometry, same label_of / n_labels: the counts that are thresholded are bev_voxel_labels' counts).  dyn: 'static' --
        points with dyn == 1 take no part; 'all' -- every point; 'dynamic' -- ONLY points with dyn == 1 (the movers after
        bev_voxel_carve(mark_dyn=True), or of a NuScenes window).  connectivity 6 or 26 on (k, row, col), nothing wraps.  A
        component survives with at least min_voxels voxels; the n survivors are numbered 0 .. n - 1 by their smallest place,
        so the numbering does not depend on the order of the points.
        Returns a dict of cuda tensors: 'inst' int32 [nz, px, px], the voxel's instance or -1; 'ids' int32, one per point of
        the window in store order, the instance of a kept point's voxel or -1 (the window's exact length: one offset is read
        back, the call synchronises); 'table' int32 [max_instances, 9] holding the u32 columns root place, voxels, kept
        points, col_min, col_max, row_min, row_max, k_min, k_max (rows from n on are zero; host_logic.instance_boxes turns
        them into metres); 'label_counts' int32 [max_instances, n_labels]; 'top_label' uint8 [max_instances], the most
        frequent label of the instance, the smallest on a tie, 255 for an empty row; 'stats' int64 [6]: kept points,
        foreground voxels, components, surviving components (n), kept points with an instance, voxels of the largest
        surviving component.  'inst' and 'ids' are not capped by max_instances; the two tables are.
        The store is not written: owed re-transforms are applied to what the call reads and stay owed.
        max_points: the bound at which the window is cut (default: the live window's own bound)."""
        lib = self.ctx.lib
        if dyn not in _lib.DYN_MODES:
            raise ValueError("dyn must be 'static', 'all' or 'dynamic'")
        label_table = np.ascontiguousarray(label_of, dtype=np.uint8)
        if label_table.shape != (256, ):
            raise ValueError('label_of must hold 256 entries')
        args = [int(a) for a in (nz, n_labels, min_points, connectivity, min_voxels, max_instances)]
        if any(not -(1 << 31) <= a < 1 << 31 for a in args):
            raise ValueError('nz, n_labels, min_points, connectivity, min_voxels and max_instances must fit 32 bits')
        nz, n_labels, min_points, connectivity, min_voxels, max_instances = args
        last_frame, max_points, call = self._window_pass(
            prm, first_frame, last_frame, max_points,
            side=('inst', lambda m, px: lib.pca_bev_instances_workspace_bytes(m, px, nz, max_instances)))
        px = int(prm.px)
        rows = min(max(max_instances, 1), 65536)           # (a value outside 1..65536 is refused by the call)
        inst = torch.empty((max(nz, 1), max(px, 1), max(px, 1)), dtype=torch.int32, device=self.device)
        ids = torch.empty(max_points, dtype=torch.int32, device=self.device)
        table = torch.empty((rows, _lib.BEV_INST_COLS), dtype=torch.int32, device=self.device)
        label_counts = torch.empty((rows, min(max(n_labels, 1), 32)), dtype=torch.int32, device=self.device)
        stats = torch.empty(6, dtype=torch.int64, device=self.device)
        call(lib.pca_bev_voxel_instances, (float(z_lo), float(z_step), nz, label_table.ctypes.data, n_labels, _lib.DYN_MODES[dyn],
                                           min_points, connectivity, min_voxels, max_instances),
             (inst, ids, table, label_counts, stats))
        _, ids = self._window_extent(first_frame, last_frame, max_points, ids)
        # the first maximum is the smallest label of a tie
        top_label = torch.where(label_counts.sum(dim=1) > 0, label_counts.argmax(dim=1), 255).to(torch.uint8)
        return {'inst': inst, 'ids': ids, 'table': table, 'label_counts': label_counts, 'top_label': top_label, 'stats': stats}

    def bev_instance_boxes(self, prm, ids, n_rows, cos_sin, criterion='area', edge_dist=0.2, extents=False, near=False,
                           first_frame=0, last_frame=None, max_points=None):
        """Oriented metric boxes around the instances of the live frames [first_frame, last_frame) (pca_bev_instance_boxes).
        ids: a cuda int32 tensor, one per point of the window in store order -- bev_voxel_instances' 'ids' for the same window
        and the same `prm`, or any other grouping: a point takes part iff 0 <= ids[p] < n_rows.  cos_sin: f64 [n_angles, 2],
        the directions to search (host_logic.fit_angles).  Per row and direction the rectangle around the row's points is
        taken in the view frame of `prm` (of which origin, R, dx and dy are read); criterion 'area' chooses the direction of
        the smallest rectangle, 'edge' the one with the most points within edge_dist metres of the rectangle's sides (of
        equal counts the smaller rectangle) -- ties go to the first direction of the table.
        Returns a dict of cuda tensors: 'fit' float64 [n_rows, 8] = lo1, hi1, lo2, hi2 along the chosen direction and across
        it, z lo, z hi, the rectangle's area, the direction's index (seven NaNs and -1 for a row without a point); 'fit_n'
        int32 [n_rows, 2] holding the u32 point count and the near count of the chosen direction (0 unless 'edge' or
        near=True); 'boxes' float64 [n_rows, 7] = cx, cy, cz, length, width, height, yaw in the view frame (length >= width,
        yaw in [0, pi); NaN for a row without a point; host_logic.oriented_boxes is its host form and adds the corners);
        'stats' int64 [4]: points that take part, points with ids >= n_rows (skipped), rows with a point, points of the
        largest row; extents=True: 'extents' float64 [n_rows, n_angles, 4]; near=True: 'near' int32 [n_rows, n_angles].
        Only extremes and integer counts are taken: the same points in any order give the same bits.  (The length of `ids` is
        checked against the window: one offset is read back, the call synchronises -- or, while a K1 is still noted, against
        the window's upper bound, without a read.)
        The store is not written: owed re-transforms are applied to what the call reads and stay owed.
        max_points: the bound at which the window is cut (default: the live window's own bound)."""
        lib = self.ctx.lib
        if criterion not in _lib.BOX_CRITERIA:
            raise ValueError("criterion must be 'area' or 'edge'")
        table = np.ascontiguousarray(cos_sin, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 2:
            raise ValueError('cos_sin must be [n_angles, 2]')
        n_rows, n_angles = int(n_rows), int(table.shape[0])
        if not -(1 << 31) <= n_rows < 1 << 31:
            raise ValueError('n_rows must fit 32 bits')
        if not (isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and ids.is_cuda and ids.dim() == 1 and ids.is_contiguous()):
            raise ValueError('ids must be a contiguous 1-d cuda int32 tensor')
        rows, angles = min(max(n_rows, 1), 65536), min(max(n_angles, 1), 256)     # (values outside are refused by the call)
        last_frame, max_points, call = self._window_pass(
            prm, first_frame, last_frame, max_points,
            side=('boxes', lambda m, px: lib.pca_bev_instance_boxes_workspace_bytes(m, rows, angles)))
        if self._k1_noted is not None:                     # (the newest frame's length is not known before its K1 has run)
            lo, hi = 0, self.max_window_points()
        else:
            lo, hi = self.frame_off[[self.head + first_frame, self.head + last_frame]].tolist()
        if ids.numel() < min(hi - lo, max_points):
            raise ValueError('ids must hold one entry per point of the window')
        if ids.numel() == 0:
            ids = torch.zeros(1, dtype=torch.int32, device=self.device)           # (never read)
        fit = torch.empty((rows, 8), dtype=torch.float64, device=self.device)
        fit_n = torch.empty((rows, 2), dtype=torch.int32, device=self.device)
        ext = torch.empty((rows, angles, 4), dtype=torch.float64, device=self.device) if extents else None
        nr = torch.empty((rows, angles), dtype=torch.int32, device=self.device) if near else None
        stats = torch.empty(4, dtype=torch.int64, device=self.device)
        call(lib.pca_bev_instance_boxes, (ids.data_ptr(), n_rows, table.ctypes.data, n_angles, _lib.BOX_CRITERIA[criterion],
                                          float(edge_dist)), (fit, fit_n, ext, nr, stats))
        out = {'fit': fit, 'fit_n': fit_n, 'boxes': self._boxes_of(fit, table), 'stats': stats}
        if extents:
            out['extents'] = ext
        if near:
            out['near'] = nr
        return out

    def _boxes_of(self, fit, table):
        """host_logic.oriented_boxes' boxes on the device: a few torch ops on `fit` and the uploaded table (cos, sin, atan2)."""
        tab = torch.from_numpy(np.concatenate([table, np.arctan2(table[:, 1], table[:, 0])[:, None]], axis=1)).to(self.device)
        t = fit[:, 7].to(torch.int64)
        ok = t >= 0
        row = tab[torch.where(ok, t, 0)]
        nan = torch.full_like(fit[:, 0], float('nan'))
        c, s, theta = (torch.where(ok, row[:, k], nan) for k in range(3))
        lo1, hi1, lo2, hi2, zlo, zhi = (fit[:, k] for k in range(6))
        m1, m2 = 0.5 * (lo1 + hi1), 0.5 * (lo2 + hi2)
        d1, d2 = hi1 - lo1, hi2 - lo2
        swap = d2 > d1
        yaw = torch.remainder(torch.where(swap, theta + 0.5 * math.pi, theta), math.pi)
        yaw = torch.where(yaw >= math.pi, torch.zeros_like(yaw), yaw)
        return torch.stack([c * m1 - s * m2, s * m1 + c * m2, 0.5 * (zlo + zhi), torch.where(swap, d2, d1),
                            torch.where(swap, d1, d2), zhi - zlo, yaw], dim=1)

    def render_camera(self, cam, first_frame=0, last_frame=None, classes=None, max_points=None):
        """The stored points of the live frames [first_frame, last_frame) rendered into a pinhole camera with a z-buffer
        (pca_render_camera).  cam: _lib.make_camera(P, width, height, radius, include_dyn, depth_range), P 3x4 from the
        store's current coordinates to the image, as p_velo_frame.  A point is projected as K1 projects (the reference's
        velo2frame + velo2img on the stored f64 coordinates) and dropped if it falls outside the image or the open depth
        range, if include_dyn is off and dyn == 1, or if `classes` (a list of class indices; None: every class) does not
        hold its class.  A kept point competes for the pixels of its square footprint of half side cam.radius, clipped to
        the image; a pixel goes to the smallest depth rounded to float32 and, of equal depths, to the smallest index in
        the window, so the result does not depend on the order in which points arrive.
        Returns a dict of cuda tensors: 'depth' float32 [H, W] (0 where no point); 'index' int64 [H, W], the winner's index
        relative to the window's first point (-1 where none); 'rgb' uint8 [H, W, 3] and 'sem' uint8 [H, W], the winner's
        colour and class (0 and 255 where none); 'stats' int64 [3]: points considered, points kept, pixels covered.
        The store is not written: owed re-transforms are applied to what the call reads and stay owed.
        max_points: the bound at which the window is cut (default: the live window's own bound)."""
        _, _, call = self._window_pass(cam, first_frame, last_frame, max_points)
        H, W = max(int(cam.height), 1), max(int(cam.width), 1)
        only = None
        if classes is not None:
            only = _lib.PcaClassGroup()
            only.mask[:] = list(_lib.class_mask(classes))
        shape = (H, W) if H * W <= 1 << 24 else (1, 1)      # (a larger image is refused by the call: nothing to allocate for it)
        keys = self._render_keys.get(shape)
        if keys is None:
            keys = self._render_keys[shape] = torch.empty(shape, dtype=torch.int64, device=self.device)
        depth = torch.empty(shape, dtype=torch.float32, device=self.device)
        index = torch.empty(shape, dtype=torch.int64, device=self.device)
        rgb = torch.empty(shape + (3, ), dtype=torch.uint8, device=self.device)
        sem = torch.empty(shape, dtype=torch.uint8, device=self.device)
        stats = torch.empty(3, dtype=torch.int64, device=self.device)
        call(self.ctx.lib.pca_render_camera, (only, ), (keys, depth, index, rgb, sem, stats))
        return {'depth': depth, 'index': index, 'rgb': rgb, 'sem': sem, 'stats': stats}

    def bev_voxel_camera(self, prm, z_lo, z_step, nz, labels, cams, stride=1, max_depth=None):
        """Camera rays cast through the voxel grid of bev_voxel_labels (pca_bev_voxel_camera): one ray per pixel of every
        camera, from the camera centre to camera depth max_depth (None: prm.view, the side of the grid); a ray marks the voxels it visits and stops at the first
        occupied one.  labels: uint8 [nz, px, px], a cuda tensor or a numpy array (uploaded), 255 = empty -- occupied is
        whatever it says.  cams: a list of (P, (W, H)), P 3x4 from the coordinates of `prm` (the store's) to the image, as
        render_camera takes it; inv(M) and the camera centre of P = [M | p4] are computed in numpy f64
        (_lib.make_ray_camera).  stride: every stride-th pixel casts a ray, through the middle of its stride x stride block.
        The cameras run one call each into the same 'visible' (the first clears it).  One pinhole per call, no lens
        distortion.
        Returns a dict of cuda tensors: 'visible' uint8 [nz, px, px], image rows, 1 = a ray of some camera reached the voxel
        (the voxel that stopped it included); 'hit' int32, 'depth' float32, 'label' uint8: lists with one [H // stride,
        W // stride] tensor per camera -- the place (k px + row) px + col of the first occupied voxel (-1: none), its camera
        depth (0: none) and its label (255: none); 'stats' int64 [cameras, 5]: rays, rays cast, dropped for a coordinate
        that is not finite (or beyond 2^30), dropped for more than 16 384 voxel steps, hits.
        Neither the store nor the owed re-transforms are read or written."""
        if not cams:
            raise ValueError('cams must hold at least one (P, (W, H))')
        px, nz = int(prm.px), int(nz)
        max_depth = float(prm.view) if max_depth is None else float(max_depth)
        shape = (max(nz, 1), max(px, 1), max(px, 1))
        if not isinstance(labels, torch.Tensor):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8))
        labels = labels.to(device=self.device).contiguous()
        if labels.dtype != torch.uint8 or tuple(labels.shape) != shape:
            raise ValueError('labels must be uint8 [nz, px, px]')
        ctx = self.ctx
        visible = torch.empty(shape, dtype=torch.uint8, device=self.device)
        stats = torch.empty((len(cams), 5), dtype=torch.int64, device=self.device)
        out = {'visible': visible, 'hit': [], 'depth': [], 'label': [], 'stats': stats}
        for n, (P, size) in enumerate(cams):
            cam = _lib.make_ray_camera(P, size[0], size[1], stride, max_depth, clear=n == 0)
            # (a size or stride the call refuses: nothing to allocate for it)
            ok = cam.stride >= 1 and cam.width >= cam.stride and cam.height >= cam.stride
            rays = (cam.height // cam.stride, cam.width // cam.stride) if ok else (1, 1)
            hit = torch.empty(rays, dtype=torch.int32, device=self.device)
            depth = torch.empty(rays, dtype=torch.float32, device=self.device)
            label = torch.empty(rays, dtype=torch.uint8, device=self.device)
            ctx.check(ctx.lib.pca_bev_voxel_camera(ctx.h, C.byref(prm), float(z_lo), float(z_step), nz, labels.data_ptr(),
                                                   C.byref(cam), visible.data_ptr(), hit.data_ptr(), depth.data_ptr(),
                                                   label.data_ptr(), stats[n].data_ptr(), ctx.stream()))
            out['hit'].append(hit)
            out['depth'].append(depth)
            out['label'].append(label)
        return out

    def _u8_volume(self, v, name, shape=None):
        """A uint8 [nz, px, px] volume on the device (numpy arrays and bool tensors are taken too), checked against `shape`."""
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.ascontiguousarray(v).astype(np.uint8, copy=False))
        v = v.to(device=self.device)
        if v.dtype == torch.bool:
            v = v.to(torch.uint8)
        v = v.contiguous()
        if v.dtype != torch.uint8 or v.dim() != 3 or v.shape[1] != v.shape[2] or (shape is not None and tuple(v.shape) != shape):
            raise ValueError(f'{name} must be uint8 [nz, px, px]' + ('' if shape is None else ', the shape of labels'))
        return v

    def voxel_pool(self, labels, seen, visible=None, scales=(2, 4, 8), occupied_fraction=(1, 20)):
        """The volumes of the occupancy chain pooled to coarser scales, all of them in one launch (pca_voxel_pool).  labels,
        seen, visible (optional): uint8 [nz, px, px], cuda tensors or numpy arrays (uploaded); a voxel is occupied where its
        label is below 32, else free where seen != 0, else unseen.  scales: any of 2, 4, 8, each dividing px and nz.  A
        coarse voxel is occupied iff it holds an occupied fine voxel and n_occ * den >= s^3 * num for occupied_fraction =
        (num, den) -- (1, 20) is SemanticKITTI-SSC's rule -- and takes the smallest label among its most frequent ones (a
        vote of voxels, taken over the fine voxels at every scale); else it is free iff more of its fine voxels are free
        than unseen.  Returns {s: {'labels', 'state'[, 'visible']}}, cuda uint8 [nz/s, px/s, px/s]: labels 255 = not
        occupied, state 2 / 1 / 0 = occupied / free / unseen, visible 1 = some fine voxel was visible.
        Neither the store nor the owed re-transforms are read or written."""
        labels = self._u8_volume(labels, 'labels')
        shape = tuple(labels.shape)
        seen = self._u8_volume(seen, 'seen', shape)
        visible = None if visible is None else self._u8_volume(visible, 'visible', shape)
        nz, px = shape[0], shape[1]
        scales = [int(s) for s in scales]
        out = {}
        levels = (_lib.PcaVoxelPoolLevel * max(len(scales), 1))()
        for lv, s in zip(levels, scales):
            # (a scale the call refuses: nothing to allocate for it)
            coarse = (nz // s, px // s, px // s) if s > 0 and nz >= s and px >= s else (1, 1, 1)
            vol = {k: torch.empty(coarse, dtype=torch.uint8, device=self.device)
                   for k in ('labels', 'state') + (('visible', ) if visible is not None else ())}
            lv.scale, lv.labels, lv.state = s, vol['labels'].data_ptr(), vol['state'].data_ptr()
            lv.visible = vol['visible'].data_ptr() if visible is not None else None
            out[s] = vol
        ctx = self.ctx
        ctx.check(ctx.lib.pca_voxel_pool(ctx.h, px, nz, labels.data_ptr(), seen.data_ptr(),
                                         None if visible is None else visible.data_ptr(), int(occupied_fraction[0]),
                                         int(occupied_fraction[1]), levels, len(scales), ctx.stream()))
        return out

    def voxel_pack(self, labels, seen=None, visible=None, input_occ=None, label_map=None, empty_value=0):
        """The file payloads of one level, fine or pooled, in SemanticKITTI-SSC's form (pca_voxel_pack): voxel (i, j, k) of
        the [nz, px, px] volumes -- at [k, px - 1 - j, i] -- goes to place (i px + j) nz + k.  Returns cuda tensors: 'label'
        uint16 [px px nz], label_map[l] for an occupied voxel and empty_value elsewhere (label_map: 32 entries; None: l + 1,
        because label 0 is a class here and 0 means empty in the file); and, one per input that was given, 'invalid' (from
        seen: 1 = neither occupied nor seen), 'occluded' (from visible: 1 = not visible) and 'bin' (from input_occ: 1 = set)
        as uint8 [ceil(px px nz / 8)], exactly np.packbits of the bits in place order.  .cpu().numpy().tobytes() of each is
        the content of the file.  numpy inputs are uploaded."""
        labels = self._u8_volume(labels, 'labels')
        shape = tuple(labels.shape)
        seen, visible, input_occ = (None if v is None else self._u8_volume(v, n, shape)
                                    for v, n in ((seen, 'seen'), (visible, 'visible'), (input_occ, 'input_occ')))
        nz, px = shape[0], shape[1]
        table = np.arange(1, 33, dtype=np.uint16) if label_map is None else np.ascontiguousarray(label_map, dtype=np.uint16)
        if table.shape != (32, ):
            raise ValueError('label_map must hold 32 entries')
        n = px * px * nz
        out = {'label': torch.empty(n, dtype=torch.uint16, device=self.device)}
        for key, v in (('invalid', seen), ('occluded', visible), ('bin', input_occ)):
            if v is not None:
                out[key] = torch.empty((n + 7) // 8, dtype=torch.uint8, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
        ctx = self.ctx
        ctx.check(ctx.lib.pca_voxel_pack(ctx.h, px, nz, labels.data_ptr(), ptr(seen), ptr(visible), ptr(input_occ),
                                         table.ctypes.data, int(empty_value) & 0xffff, out['label'].data_ptr(),
                                         ptr(out.get('invalid')), ptr(out.get('occluded')), ptr(out.get('bin')), ctx.stream()))
        return out

    def voxel_distance(self, labels, seen=None, site_labels=None, weights=(1, 1), max_dist2=None, fill_dist2=None, fill_free=False,
                       tsdf=None):
        """The exact distance transform of a label volume (pca_voxel_distance): how far every voxel is from the nearest site,
        which site that is, and what is made of it.  labels, seen (optional): uint8 [nz, px, px], cuda tensors or numpy arrays
        (uploaded).  A voxel is a site where its label is below 32 and in site_labels (an iterable of labels; None: every
        label).  The squared distance between two places is weights[0] (drow^2 + dcol^2) + weights[1] dk^2, in integers
        (pca_amd.host_logic.voxel_metric gives the weights of a grid in metres); of equally near sites the one with the
        smallest place (k px + row) px + col wins.  max_dist2: sites further than that do not exist (None: unbounded).
        Returns a dict of cuda tensors [nz, px, px]: 'dist2' int32 (-1: no site), 'nearest' int32 (the site's place, -1),
        'nearest_label' uint8 (255); with fill_dist2, 'filled' uint8: the own label where there is one, else the nearest
        site's label where it lies within fill_dist2 and the voxel is unseen (seen == 0; every empty voxel with fill_free
        or without `seen`), else 255; with tsdf = (unit, trunc, flip), 'tsdf' float32: min(sqrt(dist2) unit, trunc) / trunc
        (1 without a site), 1 - that if flip, negative where the voxel is empty and unseen.
        Neither the store nor the owed re-transforms are read or written."""
        labels = self._u8_volume(labels, 'labels')
        shape = tuple(labels.shape)
        seen = None if seen is None else self._u8_volume(seen, 'seen', shape)
        nz, px = shape[0], shape[1]
        ctx = self.ctx
        need = int(ctx.lib.pca_voxel_distance_workspace_bytes(px, nz))
        if need > 0 and (self._dist_ws is None or self._dist_ws.numel() < need):
            self._dist_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws = self._dist_ws
        group = None
        if site_labels is not None:
            group = _lib.PcaClassGroup()
            group.mask[:] = list(_lib.class_mask(site_labels))
        out = {'dist2': torch.empty(shape, dtype=torch.int32, device=self.device),
               'nearest': torch.empty(shape, dtype=torch.int32, device=self.device),
               'nearest_label': torch.empty(shape, dtype=torch.uint8, device=self.device)}
        if fill_dist2 is not None:
            out['filled'] = torch.empty(shape, dtype=torch.uint8, device=self.device)
        unit, trunc, flip = (0., 0., False) if tsdf is None else tsdf
        if tsdf is not None:
            out['tsdf'] = torch.empty(shape, dtype=torch.float32, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
        ctx.check(ctx.lib.pca_voxel_distance(ctx.h, px, nz, labels.data_ptr(), ptr(seen), None if group is None else C.byref(group),
                                             int(weights[0]), int(weights[1]), -1 if max_dist2 is None else int(max_dist2),
                                             -1 if fill_dist2 is None else int(fill_dist2), 1 if fill_free else 0, float(unit),
                                             float(trunc), 1 if flip else 0, ptr(ws), 0 if ws is None else ws.numel(),
                                             out['dist2'].data_ptr(), out['nearest'].data_ptr(), out['nearest_label'].data_ptr(),
                                             ptr(out.get('filled')), ptr(out.get('tsdf')), ctx.stream()))
        return out

    def _i32_volume(self, v, name, shape=None):
        """An int32 [nz, px, px] volume on the device (numpy arrays are uploaded), checked against `shape`."""
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.array(v, dtype=np.int32))          # (a copy: the caller's array may be read-only)
        v = v.to(device=self.device).contiguous()
        if v.dtype != torch.int32 or v.dim() != 3 or v.shape[1] != v.shape[2] or (shape is not None and tuple(v.shape) != shape):
            raise ValueError(f'{name} must be int32 [nz, px, px]' + ('' if shape is None else ', the shape of prev_inst'))
        return v

    def voxel_instance_match(self, prev_inst, n_prev, cur_inst, n_cur, index_map, prev_track=None, counter=None, min_overlap=1,
                             min_iou=0.0, cap_pairs=None, ids=None):
        """The instances of one sample matched to those of the sample before it (pca_voxel_instance_match): ids that hold over
        a sequence.  prev_inst, cur_inst: int32 [nz, px, px] instance volumes of one shape, -1 = no instance (what
        bev_voxel_instances returns as 'inst'; cuda tensors or numpy arrays, uploaded); n_prev, n_cur: their rows -- a voxel
        whose id is not in [0, rows) takes no part and is counted.  index_map: f64 3 x 4, from the continuous index (col, row,
        k) of a cur voxel centre to that in prev (host_logic.voxel_index_map).  C(a, b) counts the voxels of cur instance b
        whose centre lands in prev instance a; b matches a iff each is the other's best partner (largest C, smallest id among
        equal ones), C >= min_overlap and C >= min_iou (vox_prev[a] + vox_cur[b] - C).  prev_track: int32 [n_prev], the tracks
        of prev's rows (None: a row is its own track); counter: a cuda int32 [1] tensor holding the next unused track number,
        read and moved on ON THE DEVICE (None: a fresh one holding 0) -- pass both from call to call and a sequence chains.
        ids: int32 per-point instance ids of cur (bev_voxel_instances' 'ids').
        Returns a dict of cuda tensors: 'cur_track' int32 [n_cur] (the matched row's track, a new number for an unmatched row
        with a voxel, -1 for a row without one); 'match' int32 [n_cur] (the prev row or -1); 'cur_info' int32 [n_cur, 4]
        holding u32 vox_cur, in_view, C at the best prev row, that row + 1; 'prev_info' int32 [n_prev, 4]: vox_prev, C at the
        best cur row, that row + 1, the matched row + 1; 'track_vol' int32 [nz, px, px]; 'track_ids' (with ids); 'pairs' int32
        [n, 3] = a, b, C, compacted and sorted by (b, a) on the device; 'stats' int64 [10] (pca.h) and 'counter'.
        cap_pairs: the slots of the pair table, a power of two (None: the next one >= 4 max(n_prev, n_cur)); if an increment
        found no slot the call raises a RuntimeError -- stats is read back for that, the call synchronises.
        min_overlap=1 and min_iou=0 are this project's choice, checked on synthetic scenes only.
        Neither the store nor the owed re-transforms are read or written."""
        prev_inst = self._i32_volume(prev_inst, 'prev_inst')
        shape = tuple(prev_inst.shape)
        cur_inst = self._i32_volume(cur_inst, 'cur_inst', shape)
        nz, px = shape[0], shape[1]
        n_prev, n_cur = int(n_prev), int(n_cur)
        M = np.ascontiguousarray(index_map, dtype=np.float64)
        if M.shape != (3, 4):
            raise ValueError('index_map must be 3 x 4')
        if cap_pairs is None:
            cap_pairs = 16
            while cap_pairs < 4 * max(n_prev, n_cur, 1) and cap_pairs < 1 << 22:
                cap_pairs *= 2
        cap_pairs = int(cap_pairs)

        def i32_vector(t, name, n=None):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor):
                t = torch.from_numpy(np.array(t, dtype=np.int32))
            t = t.to(device=self.device).contiguous()
            if t.dtype != torch.int32 or t.dim() != 1 or (n is not None and t.numel() != n):
                raise ValueError(f'{name} must be int32 [{"n" if n is None else n}]')
            return t
        prev_track = i32_vector(prev_track, 'prev_track', max(n_prev, 0))
        ids = i32_vector(ids, 'ids')
        if counter is None:
            counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        if not (isinstance(counter, torch.Tensor) and counter.dtype == torch.int32 and counter.is_cuda and counter.numel() == 1):
            raise ValueError('counter must be a cuda int32 tensor of one element')
        ctx = self.ctx
        need = int(ctx.lib.pca_voxel_instance_match_workspace_bytes(n_prev, n_cur, cap_pairs))
        if need > 0 and (self._match_ws is None or self._match_ws.numel() < need):
            self._match_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        ws = self._match_ws
        rows_c, rows_p = min(max(n_cur, 1), 65536), min(max(n_prev, 1), 65536)   # (values outside are refused by the call)
        slots = cap_pairs if need > 0 else 1
        i32 = dict(dtype=torch.int32, device=self.device)
        out = {'cur_track': torch.empty(rows_c, **i32), 'match': torch.empty(rows_c, **i32),
               'cur_info': torch.empty((rows_c, 4), **i32), 'prev_info': torch.empty((rows_p, 4), **i32),
               'track_vol': torch.empty(shape, **i32)}
        if ids is not None:
            out['track_ids'] = torch.empty(ids.numel(), **i32)
        pairs = torch.empty((slots, 3), **i32)
        stats = torch.empty(10, dtype=torch.int64, device=self.device)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()       # noqa: E731
        ctx.check(ctx.lib.pca_voxel_instance_match(
            ctx.h, px, nz, prev_inst.data_ptr(), n_prev, cur_inst.data_ptr(), n_cur, M.ctypes.data, int(min_overlap), float(min_iou),
            cap_pairs, ptr(prev_track), counter.data_ptr(), ptr(ids), 0 if ids is None else ids.numel(), ptr(ws),
            0 if ws is None else ws.numel(), out['cur_track'].data_ptr(), out['match'].data_ptr(), out['cur_info'].data_ptr(),
            out['prev_info'].data_ptr(), out['track_vol'].data_ptr(), ptr(out.get('track_ids')), pairs.data_ptr(), stats.data_ptr(),
            ctx.stream()))
        dropped = int(stats[4].item())                     # the one read-back
        if dropped:
            raise RuntimeError(f'pca: voxel instance match: {dropped} increments found no slot in the pair table of {cap_pairs} '
                               f'(raise cap_pairs)')
        used = pairs[pairs[:, 0] != -1]
        order = torch.argsort(used[:, 1].to(torch.int64) * 65536 + used[:, 0].to(torch.int64))
        out.update(pairs=used[order], stats=stats, counter=counter)
        return out

    def bev_many(self, jobs, out16):
        """jobs: [(split_frame, prm, first_frame, last_frame | None)]; out16: cuda float16 [len(jobs),21,px,px].  All rasters
        in ONE launch of each kernel (pca_bev_generate_many): equal to len(jobs) bev() calls.  Owed transforms are applied
        first (K2)."""
        ctx, lib = self.ctx, self.ctx.lib
        n = len(jobs)
        if n == 0:
            return out16
        self.flush_pending()
        px = int(jobs[0][1].px)
        assert out16.dtype == torch.float16 and out16.is_contiguous() and tuple(out16.shape) == (n, 21, px, px)
        max_points = self.max_window_points()
        per = (int(lib.pca_bev_workspace_bytes(max_points, px)) + 255) & ~255
        need = per * n + 512
        if self._ws_many is None or self._ws_many.numel() < need:
            self._ws_many = torch.empty(int(need * 1.25), dtype=torch.uint8, device=self.device)
        cj = (_lib.PcaBevJob * n)()
        plane_bytes = 21 * px * px * 2
        for k, (split, prm, first, last) in enumerate(jobs):
            last = self.n_frames if last is None else last
            cj[k].slot_begin, cj[k].slot_split, cj[k].slot_end = self.head + first, self.head + split, self.head + last
            C.memmove(C.addressof(cj[k].prm), C.addressof(prm), C.sizeof(PcaBevParams))
            cj[k].planes = None
            cj[k].planes_f16 = out16.data_ptr() + k * plane_bytes
        st = self.c_store()
        ctx.check(lib.pca_bev_generate_many(ctx.h, C.byref(st), None, self.frame_off.data_ptr(), cj, n, max_points,
                                            self._ws_many.data_ptr(), self._ws_many.numel(), ctx.stream()))
        return out16

    # ---- host views (synchronise) -----------------------------------------------------------
    def rows(self, frame=None):
        """(M,10) f64 rows exactly as the reference keeps them in sem_pcs (one frame, or all live points)."""
        self.flush_pending()
        off = self.offsets()
        lo, hi = (int(off[0]), int(off[-1])) if frame is None else (int(off[frame]), int(off[frame + 1]))
        out = np.empty((hi - lo, 10))
        out[:, 0] = self.x[lo:hi].cpu().numpy()
        out[:, 1] = self.y[lo:hi].cpu().numpy()
        out[:, 2] = self.z[lo:hi].cpu().numpy()
        i = self.intensity[lo:hi].cpu().numpy().astype(np.float64)
        out[:, 3] = i / 255. if self.intensity_div255 else i
        r = self.rgbs[lo:hi].cpu().numpy().view(np.uint32)
        out[:, 4], out[:, 5], out[:, 6], out[:, 7] = r & 255, (r >> 8) & 255, (r >> 16) & 255, r >> 24
        out[:, 8] = self.inst[lo:hi].cpu().numpy()
        out[:, 9] = self.dyn[lo:hi].cpu().numpy()
        return out

    def frame_rows(self):
        off = self.offsets()
        allrows = self.rows()
        base = int(off[0])
        return [allrows[int(off[k]) - base:int(off[k + 1]) - base] for k in range(self.n_frames)]

    def load_rows(self, rows_list, intensity64_out=None):
        """Replaces the content by host (M,10) f64 arrays, one frame each.  Returns a cuda f64 intensity
        tensor if column 3 is not representable in the store's f32(+/255) encoding, else None."""
        self.clear()
        total = int(sum(r.shape[0] for r in rows_list))
        if total > self.capacity or len(rows_list) > self.max_frames:
            self.max_frames = max(self.max_frames, len(rows_list))
            self._alloc(max(total, 1))
            self.frame_off = torch.zeros(self.max_frames + 1, dtype=torch.int64, device=self.device)
            self._alloc_frame_tables(self.max_frames)
        rows = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 10) for r in rows_list]) if rows_list \
            else np.zeros((0, 10))
        c = rows[:, 4:8]
        if rows.size and not (np.all(c == np.floor(c)) and c.min() >= 0 and c.max() <= 255):
            raise NotImplementedError('rgb / semantic columns must hold integers 0..255')
        if rows.size and not np.all(rows[:, 8] == np.floor(rows[:, 8])):
            raise NotImplementedError('instance column must hold integers')
        d = self.device
        self.x[:total] = torch.from_numpy(np.ascontiguousarray(rows[:, 0])).to(d)
        self.y[:total] = torch.from_numpy(np.ascontiguousarray(rows[:, 1])).to(d)
        self.z[:total] = torch.from_numpy(np.ascontiguousarray(rows[:, 2])).to(d)
        inten = rows[:, 3]
        raw = np.rint(inten * 255.) if self.intensity_div255 else inten
        raw32 = raw.astype(np.float32)
        back = raw32.astype(np.float64) / 255. if self.intensity_div255 else raw32.astype(np.float64)
        i64 = None
        if not np.array_equal(back, inten) or (inten.size and (inten.min() < 0 or np.signbit(inten).any())):
            i64 = torch.from_numpy(np.ascontiguousarray(inten)).to(d)
        self.intensity[:total] = torch.from_numpy(raw32).to(d)
        cu = c.astype(np.uint32)
        packed = (cu[:, 0] | (cu[:, 1] << 8) | (cu[:, 2] << 16) | (cu[:, 3] << 24)).astype(np.uint32)
        self.rgbs[:total] = torch.from_numpy(packed.view(np.int32)).to(d)
        self.inst[:total] = torch.from_numpy(rows[:, 8].astype(np.int32)).to(d)
        self.dyn[:total] = torch.from_numpy((rows[:, 9] == 1).astype(np.uint8)).to(d)
        off = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows_list])]).astype(np.int64)
        self.frame_off[:off.size] = torch.from_numpy(off).to(d)
        self.head, self.tail = 0, len(rows_list)
        self.lb_head, self.ub_tail = 0, total
        self._ub = [int(r.shape[0]) for r in rows_list]
        self._ub_sum = sum(self._ub)
        return i64


def make_bev_params(origin, R, dx, dy, view, px, height_filter, int_scaler, int_sep_scaler, int_mid_threshold,
                    road_class, dynobj_classes, intensity_div255, rgb_fill=0.):
    prm = PcaBevParams()
    prm.origin[:] = [float(v) for v in origin]
    prm.R[:] = [float(v) for v in np.asarray(R, dtype=np.float64).ravel()]
    prm.dx, prm.dy, prm.view = float(dx), float(dy), float(view)
    prm.height_filter = float('nan') if height_filter is None else float(height_filter)
    prm.int_scaler = float(int_scaler)
    prm.int_sep_scaler = float(int_sep_scaler)
    prm.int_mid_threshold = float(int_mid_threshold)
    prm.rgb_fill = float(rgb_fill)
    prm.px = int(px)
    prm.road_class = int(road_class)
    prm.dynobj_mask[:] = list(_lib.class_mask(dynobj_classes))
    prm.intensity_div255 = int(bool(intensity_div255))
    return prm
