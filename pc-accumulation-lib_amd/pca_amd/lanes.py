"""The ground-truth lane centrelines of a map on the device (csrc/pca_lanes.hip, include/pca.h: pca_lanes_*).

The reference keeps the lanes of the whole city map as a list of (k,3) arrays and, for EVERY BEV sample, shifts, rotates,
clips and grids each of them on the host, to throw nearly all of the results away (bev_generator.py:101-109).  Here the map
is packed and uploaded once (`DeviceLanes`); a sample -- or S samples at once -- is one launch set over all edges, and only
the rows of the lanes that reach the view come back.  No host work is done per lane of the map.
"""
import ctypes as C
import threading
from collections.abc import Sequence

import numpy as np


class PcaLaneView(C.Structure):
    _fields_ = [('origin', C.c_double * 3), ('R', C.c_double * 9), ('dx', C.c_double), ('dy', C.c_double),
                ('view', C.c_double), ('px', C.c_int32), ('reserved', C.c_int32)]


class LaneView:
    """One sample's frame: lane - origin, rotated by rot_mat, shifted by (dx, dy), clipped to `view` metres, `px` cells."""

    __slots__ = ('origin', 'rot_mat', 'dx', 'dy', 'view', 'px')

    def __init__(self, origin, rot_mat, dx, dy, view, px):
        self.origin = np.asarray(origin, dtype=np.float64).reshape(3)
        self.rot_mat = np.asarray(rot_mat, dtype=np.float64).reshape(9)
        self.dx, self.dy, self.view, self.px = float(dx), float(dy), float(view), int(px)


class LaneHandle:
    """What an accumulator puts under trajs['gt_lanes'] in place of L shifted copies: the lane set and the sample's origin."""

    __slots__ = ('lanes', 'origin')

    def __init__(self, lanes, origin):
        self.lanes = lanes
        self.origin = np.array(origin, dtype=np.float64)

    def as_list(self):
        """The reference's list: every lane minus the origin (host arrays)."""
        return [lane - self.origin for lane in self.lanes.as_list()]


class _Batch:
    """The device results of one pca_lanes_to_grid call -- [n_rows | row_lane | rows] of S samples in ONE block -- and their
    way to the host: at once (a blocking copy), or through pca_host_d2h_async into pinned memory, waited for on first use."""

    def __init__(self, lanes, views, cap, asynchronous, ctx=None):
        import torch
        ctx, S = ctx or lanes.ctx, len(views)
        self.lanes, self.views, self.cap, self.S, self.asynchronous = lanes, views, int(cap), S, bool(asynchronous)
        self.off_lane = (8 * S + 255) & ~255
        self.off_rows = (self.off_lane + 4 * S * self.cap + 255) & ~255
        total = self.off_rows + 24 * S * self.cap
        dev = torch.empty(total, dtype=torch.uint8, device=lanes.device)
        ws_bytes = ctx.lib.pca_lanes_workspace_bytes(lanes.n_vertices, S, self.cap)
        if ws_bytes < 0:
            raise ValueError('lanes: too many vertices or samples for one call')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=lanes.device)
        arr = (PcaLaneView * S)()
        for k, v in enumerate(views):
            arr[k].origin[:] = v.origin.tolist()
            arr[k].R[:] = v.rot_mat.tolist()
            arr[k].dx, arr[k].dy, arr[k].view, arr[k].px = v.dx, v.dy, v.view, v.px
        p = dev.data_ptr()
        ctx.check(ctx.lib.pca_lanes_to_grid(ctx.h, lanes.xyz.data_ptr(), lanes.vertex_lane.data_ptr(), lanes.start.data_ptr(),
                                            lanes.n_vertices, lanes.n_lanes, arr, S, self.cap, p + self.off_rows,
                                            p + self.off_lane, p, ws.data_ptr(), ctx.stream()))
        self.host = None
        self.event = None
        if asynchronous:
            from bev_generator.sem_bev import _PendingCopy
            host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            ticket = ctx.lib.pca_host_d2h_async(ctx.h, p, host.data_ptr(), total, ctx.stream())
            if ticket < 0:
                ctx.check(ticket)
            self.event = _PendingCopy(ctx, ticket, (dev, ws, host))
            self._host_t = host
        else:
            self._host_t = dev.cpu()
            ctx.poll_status()

    def arrays(self):
        """(n_rows [S] i64, row_lane [S, cap] i32, rows [S, cap, 3] f64) on the host (waits for the copy the first time)."""
        if self.host is None:
            if self.event is not None:
                self.event.synchronize()
                self.event = None
            b = self._host_t.numpy()
            S, cap = self.S, self.cap
            self.host = (b[:8 * S].view(np.int64), b[self.off_lane:self.off_lane + 4 * S * cap].view(np.int32).reshape(S, cap),
                         b[self.off_rows:self.off_rows + 24 * S * cap].view(np.float64).reshape(S, cap, 3))
        return self.host


def _split_rows(rows, row_lane):
    """rows of one sample -> the reference's list: one (k,3) array per surviving lane, in map order (own copies)."""
    if rows.shape[0] == 0:
        return []
    cuts = np.flatnonzero(row_lane[1:] != row_lane[:-1]) + 1
    return [np.array(part) for part in np.split(rows, cuts)]


class PendingLanes(Sequence):
    """The clipped lanes of ONE sample, possibly still on their way from the device.  `resolve()` returns the list the
    reference's generate() leaves under 'gt_lanes' (non-empty lanes only, map order, (k,3) f64 each); `resolved` tells
    whether that has happened, `PendingLanes.n_resolved` counts how often it has, over all objects.  Read as a sequence
    (len, index, iteration) it resolves itself; a LazyBev sample replaces it by the plain list when it fills in."""

    n_resolved = 0

    def __init__(self):
        self._batch = None
        self._index = 0
        self._then = []
        self._value = None
        self.resolved = False
        self.reruns = 0

    def _bind(self, batch, index):
        self._batch, self._index = batch, index

    def then(self, fn):
        """fn(list) -> list, applied when the lanes are decoded (the warp augmentation of the few lanes left)."""
        if self.resolved:
            self._value = fn(self._value)
        else:
            self._then.append(fn)
        return self

    def __len__(self):
        return len(self.resolve())

    def __getitem__(self, i):
        return self.resolve()[i]

    def __reduce__(self):                        # pickles as the plain list the reference writes
        return (list, (self.resolve(), ))

    def resolve(self):
        if not self.resolved:
            b, k = self._batch, self._index
            n_rows, row_lane, rows = b.arrays()
            n = int(n_rows[k])
            if n > b.cap:
                # more rows than the block had room for: this sample once more, alone, with room for exactly its rows
                self.reruns += 1
                b.lanes.note_rows(n)
                again = b.lanes.rerun(b.views[k], n, b.asynchronous)
                n_rows, row_lane, rows = again.arrays()
                k = 0
                assert int(n_rows[0]) == n
            else:
                b.lanes.note_rows(n)
            value = _split_rows(rows[k, :n], row_lane[k, :n])
            for fn in self._then:
                value = fn(value)
            self._value, self._then, self._batch = value, [], None
            self.resolved = True
            PendingLanes.n_resolved += 1
        return self._value


class DeviceLanes:
    """A list of (k,3) lane polylines packed into one device array (k may be 0 or 1: such a lane has no edge)."""

    DEFAULT_CAP_ROWS = 16384         # rows per sample the first calls make room for (28 bytes each); grows with what is seen

    def __init__(self, lanes, device=None):
        import torch

        from . import _lib
        self.ctx = _lib.Context.get(device)
        self.device = torch.device('cuda', self.ctx.device_index)
        arrays = [np.asarray(lane, dtype=np.float64).reshape(-1, 3) for lane in lanes]
        counts = np.array([a.shape[0] for a in arrays], dtype=np.int64)
        self.n_lanes = len(arrays)
        self.n_vertices = int(counts.sum())
        if self.n_vertices >= 1 << 30:
            raise ValueError('lanes: at most 2^30 vertices')
        start = np.zeros(self.n_lanes + 1, dtype=np.int32)
        np.cumsum(counts, out=start[1:])
        self._start_host = start
        xyz = np.concatenate(arrays) if self.n_vertices else np.zeros((0, 3))
        vertex_lane = np.repeat(np.arange(self.n_lanes, dtype=np.int32), counts)
        self.xyz = torch.from_numpy(np.ascontiguousarray(xyz)).to(self.device)
        self.vertex_lane = torch.from_numpy(vertex_lane).to(self.device)
        self.start = torch.from_numpy(start).to(self.device)
        self.has_edges = bool((counts >= 2).any())
        self._cap_hint = self.DEFAULT_CAP_ROWS
        self.launches = 0                # to_grid calls that reached the device (the re-run of an overflowing sample not counted)

    def __len__(self):
        return self.n_lanes

    def transform(self, T):
        """Every vertex p <- (T [p; 1])[:3], in place on the device (the first frame's global -> world transform)."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        assert T.shape == (4, 4), f"{T.shape} is not (4, 4)"
        if self.n_vertices:
            self.ctx.check(self.ctx.lib.pca_lanes_transform(self.ctx.h, self.xyz.data_ptr(), self.n_vertices, T.ctypes.data,
                                                            self.ctx.stream()))
        return self

    def as_list(self):
        """Host copies, one (k,3) f64 array per lane (the reference's gt_lane_poses)."""
        xyz = self.xyz.cpu().numpy()
        s = self._start_host
        return [xyz[s[i]:s[i + 1]].copy() for i in range(self.n_lanes)]

    _rerun_lock = threading.Lock()
    _rerun_ctx = {}

    def rerun(self, view, n, other_thread):
        """One sample again with room for n rows, results on the host.  A sample that was delivered asynchronously may be
        decoded on ANY thread (the background writer's): such a run takes a context of its own, one caller at a time, and
        shares no pinned block or status word with the call sequence of the accumulator's thread.  The vertices it reads
        were final before the copy that has just been waited for."""
        if not other_thread:
            return _Batch(self, [view], n, asynchronous=False)
        from . import _lib
        with DeviceLanes._rerun_lock:
            ctx = DeviceLanes._rerun_ctx.get(self.ctx.device_index)
            if ctx is None:
                ctx = DeviceLanes._rerun_ctx[self.ctx.device_index] = _lib.Context(self.ctx.device_index)
            return _Batch(self, [view], n, asynchronous=False, ctx=ctx)

    def note_rows(self, n):
        """Room for later calls: a quarter more than the largest sample seen."""
        if n + n // 4 > self._cap_hint:
            self._cap_hint = n + n // 4

    def to_grid(self, views, cap_rows=None, asynchronous=False, into=None):
        """One pca_lanes_to_grid call for all the `views` (LaneView).  Returns one PendingLanes per view (`into`: objects
        handed out earlier, to be bound to this call).  asynchronous=False: the rows are on the host when this returns;
        True: they leave through pca_host_d2h_async and are waited for when the first of them is resolved."""
        views = list(views)
        out = list(into) if into is not None else [PendingLanes() for _ in views]
        assert len(out) == len(views)
        if not views:
            return out
        if not self.has_edges:                       # nothing can be emitted: no launch
            for p in out:
                p._value, p.resolved = [], True
                for fn in p._then:
                    p._value = fn(p._value)
                p._then = []
            return out
        cap = self._cap_hint if cap_rows is None else int(cap_rows)
        if cap < 0:
            raise ValueError('cap_rows must not be negative')
        self.launches += 1
        batch = _Batch(self, views, cap, asynchronous)
        for k, p in enumerate(out):
            p._bind(batch, k)
        return out
