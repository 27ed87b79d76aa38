"""Semantic BEV generator -- drop-in for the reference's ``bev_generator.sem_bev.SemBEVGenerator``.

All 21 planes (7 per point set) come out of one device launch sequence (csrc/pca_bev.hip), the optional warp
augmentation included (pca_bev_warp); this class only frames the problem (heading, augmentation), handles the
trajectory polylines on the host and packs the reference's output dict (README.md:60-99 of the reference: keys,
shapes, float16).
"""
import numpy as np

from .bev_generator import PLANES, SETS, BEVGenerator, WindowPart


class _PendingCopy:
    """A device -> host copy in flight (pca_host_d2h_async).  Holds the device tensor until the copy has been waited for, so
    that its memory is not handed to another tensor while the side stream may still read it."""

    __slots__ = ('ctx', 'ticket', 'keep')

    def __init__(self, ctx, ticket, keep):
        self.ctx, self.ticket, self.keep = ctx, ticket, keep

    def synchronize(self):
        if self.keep is not None:
            self.ctx.check(self.ctx.lib.pca_host_d2h_wait(self.ctx.h, self.ticket))
            self.keep = None
            # every kernel behind this copy has finished: what they raised is visible in the status mirror.  A sample made
            # from dropped points or an invalid compaction must not reach its consumer silently (the reference fails
            # synchronously: sem_bev.py:543-551, nuscenes_utils.py:191-195)
            self.ctx.poll_status()

    def __del__(self):                       # a sample nobody looked at: its blocks go back only after the copy has landed
        try:
            if self.keep is not None:
                self.ctx.lib.pca_host_d2h_wait(self.ctx.h, self.ticket)
        except Exception:                    # noqa: BLE001  (interpreter shutdown)
            pass


def _writer():
    from pca_amd import writer
    return writer


def _preview():
    from pca_amd import preview
    return preview


class LazyBev(dict):
    """The reference's BEV dict whose plane arrays are still on their way from the device: the fp16 D2H copy was
    enqueued on a side stream into pinned memory; the first access waits for THAT copy only and fills the dict in.
    A consumer that hands the dict to a background writer (write_compressed_pickle does) never waits at all.
    The arrays are VIEWS of the pinned block the copy landed in (no second copy of the 2.75 MB sample: that was 0.12 ms
    of the unchanged driver's 0.5 ms step); the block returns to torch's pinned-memory cache when the last array dies.
    A program that keeps more than MAX_PINNED_LIVE samples alive gets ordinary (copied) arrays for the ones beyond."""

    MAX_PINNED_LIVE = 64
    _live = [0]

    def __init__(self, host, index, event, trajs, gt_lanes=None):
        super().__init__()
        self._pending = (host, index, event, trajs, gt_lanes)
        self._error = None
        # while the writer's device codec is selected (pca_amd.writer): (the device planes this sample is part of, its index), so that it
        # can still be compressed there after it -- or a sibling that shares the copy -- has been filled in; the writer
        # drops the reference once the compression has been waited for
        self._dev = None
        self._host_planes = None
        keep = getattr(event, 'keep', None)
        if keep and _writer().device_codec_selected():
            self._dev = (keep[0], index)
        # while PCA_VIZ=device (pca_amd.preview): a reference of its own for the preview sheet -- (the device planes, the
        # sample's index, the trajectories of every sample of the block or None) -- kept until the preview has been enqueued
        # or the sample dies, whatever the writer's codec does with `_dev`
        self._dev_preview = None
        if keep and _preview().selected():
            self._dev_preview = (keep[0], index, None)
        self._zero_copy = LazyBev._live[0] < LazyBev.MAX_PINNED_LIVE
        if self._zero_copy:
            import weakref
            LazyBev._live[0] += 1
            weakref.finalize(self, LazyBev._released)

    @staticmethod
    def _released():
        LazyBev._live[0] -= 1

    def _fill(self):
        if self._pending is not None:
            if self._error is not None:          # the copy's wait raised (a device error): every later access says so again,
                raise self._error                # instead of handing out an empty dict or a bare KeyError
            host, index, event, trajs, gt_lanes = self._pending
            try:
                event.synchronize()
            except Exception as e:               # noqa: BLE001
                self._error = e
                raise
            planes = host[index].numpy()
            if not self._zero_copy:
                planes = np.array(planes)
            if self._dev is not None:            # the device codec will write the DEVICE planes: no silent edits of the copy
                planes.flags.writeable = False
                self._host_planes = planes
            if gt_lanes is not None and not isinstance(gt_lanes, list):     # pca_amd.lanes.PendingLanes: decoded now
                gt_lanes = gt_lanes.resolve()
            dict.update(self, SemBEVGenerator.pack_bev(planes, trajs[0], trajs[1], trajs[2], gt_lanes))
            self._pending = None                 # only now: the sample is complete
        return self

    def __getitem__(self, k):
        return dict.__getitem__(self._fill(), k)

    def __contains__(self, k):
        return dict.__contains__(self._fill(), k)

    def __iter__(self):
        return dict.__iter__(self._fill())

    def __len__(self):
        return dict.__len__(self._fill())

    def keys(self):
        return dict.keys(self._fill())

    def items(self):
        return dict.items(self._fill())

    def values(self):
        return dict.values(self._fill())

    def get(self, k, default=None):
        return dict.get(self._fill(), k, default)

    def __reduce__(self):                         # pickles as the plain dict the reference writes
        return (dict, (dict(self._fill()), ))


class SemBEVGenerator(BEVGenerator):

    def __init__(self,
                 sem_idxs: dict,
                 view_size: int,
                 pixel_size: int,
                 max_trans_radius: float = 0.,
                 zoom_thresh: float = 0.,
                 do_warp: bool = False,
                 int_scaler: float = 1.,
                 int_sep_scaler: float = 1.,
                 int_mid_threshold: float = 0.5,
                 height_filter=None,
                 rgb_fill: int = 0):
        super().__init__(view_size, pixel_size, max_trans_radius, zoom_thresh, do_warp, int_scaler, int_sep_scaler,
                         int_mid_threshold, height_filter)
        self.sem_idxs = sem_idxs     # semantic name -> class index ('road', 'car', 'truck', 'bus', 'motorcycle')
        self.dyn_idx = 9             # column of the dynamic flag
        self.rgb_fill = rgb_fill
        self._frame = None
        # extension (off while empty): extra class planes in every sample, plane name -> list of sem_idxs names or integer
        # classes, e.g. {'sidewalk': [1], 'vehicle': ['car', 'truck', 'bus', 'motorcycle']} -> keys '<name>_<set>'
        self.sem_planes = {}

    # ------------------------------------------------------------------------------------------
    def generate_bev_device(self, pc_present, pc_future, pc_full, want_f64=False, out16=None):
        """Device tensors only: (planes_f16, planes_f64|None), [21,px,px].  Used by the sharded runner and
        the benchmark, where BEVs stay in HBM until they are gathered."""
        if self._frame is None:
            rot_mat, dx, dy, view = np.eye(3), 0., 0., float(self.view_size)
        else:
            rot_mat, dx, dy, view = self._frame
        return self.rasterise(pc_present, pc_future, pc_full, rot_mat, dx, dy, view, want_f64, out16=out16)

    def generate_bev(self, pc_present, pc_future, pc_full, trajs_present, trajs_future, trajs_full,
                     gt_lane_trajs=None):
        """Inputs are what ``generate`` hands over: device window parts or host arrays in BEV-frame metres
        (the rotation/crop/grid steps the reference runs before this call are part of the device pipeline)."""
        if not isinstance(pc_present, WindowPart) and self._frame is None:
            # called directly with the reference's pre-gridded rows: put every point at its cell centre
            pc_present, pc_future, pc_full = (self._grid_rows_to_metres(p) for p in (pc_present, pc_future, pc_full))
        device_only, self._device_only = self._device_only, False
        out16, self._out16 = self._out16, None
        names, groups = self._sem_plane_groups()
        frame = self._frame if self._frame is not None else (np.eye(3), 0., 0., float(self.view_size))
        p16, _ = self.generate_bev_device(pc_present, pc_future, pc_full, out16=None if self.do_warp else out16)
        self._frame = None
        # the class planes come after the 21 planes, in the same frame
        c16 = self.class_planes_device(pc_present, pc_future, pc_full, groups, *frame)[0] if names else None
        if getattr(pc_present, 'window', None) is not None and pc_present.window.future_is_present:
            p16[7:14] = p16[0:7]             # generate_bev(present_idx=None, gen_future=True): every set is the window
            if c16 is not None:
                c16[1] = c16[0]
                c16[2] = c16[0]
        if self.do_warp:
            # polynomial warp augmentation: planes on the device (pca_bev_warp), trajectory vertices on the host
            px = self.pixel_size
            i_mid = j_mid = int(px / 2)
            i_warp, j_warp = self.get_random_warp_params(0.15, 0.30, px, px)
            a_1, a_2 = self.cal_warp_params(i_warp, i_mid, px - 1)
            b_1, b_2 = self.cal_warp_params(j_warp, j_mid, px - 1)
            p16 = self.warp_planes_device(p16, a_1, a_2, b_1, b_2, out16)
            if c16 is not None:
                c16 = self.warp_planes_device(c16.view(-1, px, px), a_1, a_2, b_1, b_2).view(3, len(names), px, px)
            args = (a_1, a_2, b_1, b_2, i_mid, j_mid, i_warp, j_warp)
            trajs_present = self.warp_trajs(trajs_present, *args)
            trajs_future = self.warp_trajs(trajs_future, *args)
            trajs_full = self.warp_trajs(trajs_full, *args)
            if isinstance(gt_lane_trajs, list):
                gt_lane_trajs = self.warp_trajs(gt_lane_trajs, *args)
            elif gt_lane_trajs is not None:          # pending device lanes: warped when they are decoded (few are left)
                gt_lane_trajs.then(lambda lanes, args=args: self.warp_trajs(lanes, *args))
        if device_only:
            out = {'planes_f16': p16, 'trajs_present': trajs_present, 'trajs_future': trajs_future,
                   'trajs_full': trajs_full}
            if gt_lane_trajs is not None:
                out['gt_lanes'] = gt_lane_trajs
            if c16 is not None:
                out['sem_planes_f16'], out['sem_plane_names'] = c16, names
            return out
        bev = self.pack_bev(p16.cpu().numpy(), trajs_present, trajs_future, trajs_full, gt_lane_trajs)
        if c16 is not None:
            c = c16.cpu().numpy()
            for s, set_name in enumerate(SETS):
                for k, name in enumerate(names):
                    bev[f'{name}_{set_name}'] = c[s, k]
        return bev

    # ---- class planes (extension: pca_bev_class_planes) --------------------------------------------
    RESERVED_PLANE_NAMES = ('road', 'intensity', 'rgb', 'dynamic', 'elevation', 'trajs')

    def _classes_of(self, sem_clss):
        """sem_idxs names (an unknown one raises KeyError, as the reference's lookup does) or integer classes -> integers."""
        return [self.sem_idxs[c] if isinstance(c, str) else int(c) for c in sem_clss]

    def _sem_plane_groups(self):
        """(plane names, class-index lists) of `sem_planes`."""
        planes = getattr(self, 'sem_planes', None) or {}
        for name in planes:
            if name in self.RESERVED_PLANE_NAMES:
                raise ValueError(f"sem_planes: '{name}' is the name of one of the sample's own planes")
        return list(planes), [self._classes_of(v) for v in planes.values()]

    # ---- one point set, one read-only pass: what class_planes_device, elev_partition_device, voxel_labels_device,
    #      voxel_rays_device, voxel_carve_device and voxel_instances_device share (a new pass of this family plugs in here and in DeviceStore._window_pass) ----
    def _pass_params(self, pc, rot_mat, dx, dy, aug_view_size):
        """pca_bev_params of a pass over `pc`: a WindowPart brings its window's origin, host rows are in BEV-frame metres."""
        if isinstance(pc, WindowPart):
            return self._raster_params(pc.window.origin, rot_mat, dx, dy, aug_view_size, pc.window.store.intensity_div255)
        return self._raster_params(np.zeros(3), rot_mat, dx, dy, aug_view_size, False)

    def _one_set_pass(self, pc, key, rot_mat, dx, dy, aug_view_size, per_frame=False):
        """(store, prm, frame range) a pass over one point set is called with: the window's store and the part's frames, or
        -- host rows: one array, per_frame: a list of arrays -- the temporary store `key` loaded with them, all of it."""
        prm = self._pass_params(pc, rot_mat, dx, dy, aug_view_size)
        if isinstance(pc, WindowPart):
            lo, hi = pc.frames()
            return pc.window.store, prm, dict(first_frame=lo, last_frame=hi)
        st = self._tmp_store(key)
        st.load_rows(pc if per_frame else [pc])
        return st, prm, {}

    @staticmethod
    def _voxel_grid(z_range, nz):
        """(z_lo, z_step, nz) of nz height bins over z_range = (lo, hi); nz <= 0 gives a NaN step, which the C call refuses."""
        lo, hi, nz = float(z_range[0]), float(z_range[1]), int(nz)
        return lo, ((hi - lo) / nz if nz > 0 else float('nan')), nz

    def class_planes_device(self, pc_present, pc_future, pc_full, groups, rot_mat, dx, dy, aug_view_size, want_counts=False):
        """(prob_f16, prob_f64, counts | None), cuda [3, len(groups) (+ 1), px, px]: the planes of the class groups over the
        static points of the three sets, in the frame the 21 planes are rasterised in (DeviceStore.bev_class_planes)."""
        prm = self._pass_params(pc_present, rot_mat, dx, dy, aug_view_size)
        if isinstance(pc_present, WindowPart):
            w = pc_present.window
            return w.store.bev_class_planes(w.split, prm, groups, first_frame=w.first, last_frame=w.last,
                                            want_counts=want_counts)
        # host arrays go through the temporary stores, as in rasterise: 'full' is an input of its own
        st = self._tmp_store('pf')
        st.load_rows([pc_present, pc_future])
        a = st.bev_class_planes(1, prm, groups, want_counts=want_counts)
        st2 = self._tmp_store('full')
        st2.load_rows([pc_full])
        b = st2.bev_class_planes(1, prm, groups, want_counts=want_counts)
        for x, y in zip(a, b):
            if x is not None:
                x[2] = y[0]
        return a

    def _class_counts_from_grid_rows(self, pc, groups):
        """Pre-gridded rows (columns 0, 1 = cell indices) -> (prob f64 [len(groups), px, px], counts [len(groups) + 1, px,
        px]) of ALL the rows: no static partition, no height filter -- these helpers reduce whatever rows they are given."""
        rows = np.array(pc, dtype=np.float64)
        px = self.pixel_size
        rows[:, 0:2] = np.where(rows[:, 0:2] == px, px - 1, rows[:, 0:2])   # (np.histogram2d: the last bin is closed on the right)
        rows = self._grid_rows_to_metres(rows)
        rows[:, 9] = 0
        hf, self.height_filter = self.height_filter, None
        try:
            empty = np.zeros((0, 10))
            _, p64, cnt = self.class_planes_device(rows, empty, empty, groups, np.eye(3), 0., 0., float(self.view_size),
                                                   want_counts=True)
        finally:
            self.height_filter = hf
        return p64[0].cpu().numpy(), cnt[0].cpu().numpy().view(np.uint32)

    def gen_sem_probmap(self, pc: np.array, sem_clss: list):
        """Dirichlet expectation of the classes `sem_clss` (sem_idxs names; integer classes are taken too) per cell of
        pre-gridded rows: f64 (px, px), image rows, as bev_generator.py:373-394 of the reference returns it."""
        return self._class_counts_from_grid_rows(pc, [self._classes_of(sem_clss)])[0][0]

    def gen_gridmap_count_map(self, pc: np.array, weights: np.array = None) -> np.array:
        """Points per cell of pre-gridded rows, f64 (px, px), image rows (bev_generator.py:438-455 of the reference).  With
        `weights` the sums are a host np.bincount over the same cell indices: not a hot path -- the reference itself uses
        it for per-class intensity sums only, which this drop-in gets from the rasteriser."""
        px = self.pixel_size
        if weights is None:
            return self._class_counts_from_grid_rows(pc, [[]])[1][1].astype(np.float64)
        pc = np.asarray(pc)
        i, j = np.floor(pc[:, 0]).astype(np.int64), np.floor(pc[:, 1]).astype(np.int64)
        i[pc[:, 0] == px] = px - 1                   # (np.histogram2d: the last bin is closed on the right)
        j[pc[:, 1] == px] = px - 1
        ok = (i >= 0) & (i < px) & (j >= 0) & (j < px)
        flat = np.bincount((px - 1 - j[ok]) * px + i[ok], weights=np.asarray(weights, dtype=np.float64)[ok],
                           minlength=px * px)
        return flat.reshape(px, px)

    # ---- partition by height above the cell minimum (extension: pca_bev_elev_partition) ------------
    def elev_partition_device(self, pc, rot_mat, dx, dy, aug_view_size, elev_thresh, include_dyn=False, mark_dyn=False):
        """One point set partitioned by height above its cells' minimum z, in the frame the 21 planes are rasterised in
        (DeviceStore.bev_elev_partition: the dict of cuda tensors 'elev', 'observed', 'flags', 'counts').  pc: a WindowPart
        (flags in the order of the part's frames in the store) or host rows in BEV-frame metres (flags in row order).
        mark_dyn applies to a WindowPart only: the elevated points of the device window get dyn = 1, for good."""
        if mark_dyn and not isinstance(pc, WindowPart):
            raise ValueError('mark_dyn needs a device window: host rows are not written')
        st, prm, frames = self._one_set_pass(pc, 'elev', rot_mat, dx, dy, aug_view_size)
        return st.bev_elev_partition(prm, elev_thresh, include_dyn=include_dyn, mark_dyn=mark_dyn, **frames)

    # ---- semantic occupancy labels (extension: pca_bev_voxel_labels) -------------------------------
    @staticmethod
    def voxel_label_table(classes=None):
        """(label_of uint8 [256], n_labels) of `classes`: a list of class-index lists, list i becomes label i (a class named
        in two lists is a ValueError); None: label = class for the classes 0 .. 31.  Every other class is ignored (255)."""
        table = np.full(256, 255, dtype=np.uint8)
        if classes is None:
            table[:32] = np.arange(32)
            return table, 32
        if not 1 <= len(classes) <= 32:
            raise ValueError('classes: 1 to 32 lists of classes')
        for label, group in enumerate(classes):
            for c in group:
                c = int(c)
                if not 0 <= c <= 255:
                    raise ValueError(f'classes: {c} is not a class byte')
                if table[c] != 255:
                    raise ValueError(f'classes: class {c} is named in two lists')
                table[c] = label
        return table, len(classes)

    def voxel_labels_device(self, pc, rot_mat, dx, dy, aug_view_size, z_range, nz, classes=None, include_dyn=False, keep_owed=False):
        """One point set voxelised into semantic occupancy labels, in the frame the 21 planes are rasterised in, with nz
        height bins over z_range = (lo, hi) metres of that frame (DeviceStore.bev_voxel_labels: the dict of cuda tensors
        'labels', 'counts', 'top', each [nz, px, px]).  pc: a WindowPart or host rows in BEV-frame metres.  classes: see
        voxel_label_table (sem_idxs names are taken too).  keep_owed: see DeviceStore.bev_voxel_labels."""
        grid = self._voxel_grid(z_range, nz)
        if classes is not None:
            classes = [self._classes_of(g) for g in classes]
        table, n_labels = self.voxel_label_table(classes)
        st, prm, frames = self._one_set_pass(pc, 'voxel', rot_mat, dx, dy, aug_view_size)
        return st.bev_voxel_labels(prm, *grid, table, n_labels, include_dyn=include_dyn, keep_owed=keep_owed, **frames)

    # ---- rays through the voxel grid: free against unseen (extension: pca_bev_voxel_rays) ------------
    def voxel_rays_device(self, pc, origins, rot_mat, dx, dy, aug_view_size, z_range, nz, include_dyn=False):
        """One lidar ray per point, from the sensor position of the point's frame to the point, cast through the grid of
        voxel_labels_device (same frame, same z_range and nz): DeviceStore.bev_voxel_rays' dict of cuda tensors 'seen'
        (uint8 [nz, px, px], 1 = a ray passed through) and 'stats' (int64 [4]).  pc: a WindowPart, with `origins`
        [frames, 3] the sensor positions of exactly that part's frames in the store's coordinates; or a list of per-frame
        host row arrays in BEV-frame metres, with one origin each in the same frame."""
        grid = self._voxel_grid(z_range, nz)
        if isinstance(pc, np.ndarray):
            raise ValueError('voxel_rays_device: host rows come as a list of per-frame arrays, one origin each')
        if not isinstance(pc, WindowPart):
            pc = [np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in pc]
        st, prm, frames = self._one_set_pass(pc, 'rays', rot_mat, dx, dy, aug_view_size, per_frame=True)
        return st.bev_voxel_rays(prm, *grid, origins, include_dyn=include_dyn, **frames)

    # ---- camera rays through the voxel grid: visible against occluded (extension: pca_bev_voxel_camera) ------------
    def voxel_camera_device(self, pc, labels, cams, rot_mat, dx, dy, aug_view_size, z_range, nz, stride=1, max_depth=None):
        """One ray per pixel of every camera of `cams`, cast through the grid of voxel_labels_device (same frame, same
        z_range and nz) until the first voxel that `labels` (uint8 [nz, px, px], 255 = empty; a cuda tensor or a numpy
        array) calls occupied: DeviceStore.bev_voxel_camera's dict of cuda tensors 'visible' (uint8 [nz, px, px]), the
        per-camera lists 'hit', 'depth', 'label' and 'stats' (int64 [cameras, 5]).  cams: a list of (P 3x4, (W, H)).  pc
        names the frame the cameras live in and is not read: a WindowPart -- P from the store's coordinates to the image --
        or None -- P from BEV-frame metres to the image.  max_depth: the camera depth at which a ray ends; None:
        aug_view_size, the side of the grid.  One pinhole per call, no lens distortion."""
        grid = self._voxel_grid(z_range, nz)
        if pc is not None and not isinstance(pc, WindowPart):
            raise ValueError('voxel_camera_device: pc is a WindowPart or None (the rays read labels, not points)')
        prm = self._pass_params(pc, rot_mat, dx, dy, aug_view_size)
        st = pc.window.store if isinstance(pc, WindowPart) else self._tmp_store('camera')
        return st.bev_voxel_camera(prm, *grid, labels, cams, stride=stride, max_depth=max_depth)

    # ---- coarser scales and SSC file payloads of the volumes (extension: pca_voxel_pool, pca_voxel_pack) ------------
    def voxel_pyramid_device(self, labels, seen, visible=None, input_occ=None, scales=(1, 2, 4, 8), label_map=None, empty_value=0,
                             occupied_fraction=(1, 20)):
        """The volumes of voxel_labels_device / voxel_rays_device / voxel_camera_device (uint8 [nz, px, px], cuda tensors or
        numpy arrays) as the scales SemanticKITTI-SSC ships, with each level's file payloads: ONE pool call for the scales
        above 1 (DeviceStore.voxel_pool; every scale is decided from the fine voxels), then one pack call per level
        (DeviceStore.voxel_pack).  Returns {'levels': {s: volumes}, 'packed': {s: payloads}}: level 1 holds the inputs and
        their 'state' (2 occupied, 1 free, 0 unseen) and is packed into 'label', 'invalid' and, where `visible` / `input_occ`
        were given, 'occluded' / 'bin'; the pooled levels hold 'labels', 'state' (and 'visible') and are packed into 'label'
        and 'invalid' only -- the benchmark ships no coarse .occluded / .bin.  label_map, empty_value: see voxel_pack."""
        import torch
        st = self._tmp_store('ssc')
        labels = st._u8_volume(labels, 'labels')
        shape = tuple(labels.shape)
        seen = st._u8_volume(seen, 'seen', shape)
        visible = None if visible is None else st._u8_volume(visible, 'visible', shape)
        input_occ = None if input_occ is None else st._u8_volume(input_occ, 'input_occ', shape)
        scales = [int(s) for s in scales]
        levels, packed = {}, {}
        pooled = st.voxel_pool(labels, seen, visible, [s for s in scales if s != 1], occupied_fraction) if scales != [1] else {}
        for s in scales:
            if s == 1:
                occ = labels < 32
                state = torch.where(occ, 2, (seen != 0).to(torch.int32)).to(torch.uint8)
                levels[1] = {'labels': labels, 'seen': seen, 'state': state}
                levels[1].update({} if visible is None else {'visible': visible})
                levels[1].update({} if input_occ is None else {'input_occ': input_occ})
                packed[1] = st.voxel_pack(labels, seen, visible, input_occ, label_map, empty_value)
            else:
                levels[s] = pooled[s]
                # (a pooled level's state is 0 exactly where it is neither occupied nor free: its `seen` for the packer)
                packed[s] = st.voxel_pack(pooled[s]['labels'], pooled[s]['state'], label_map=label_map, empty_value=empty_value)
        return {'levels': levels, 'packed': packed}

    # ---- distance to the nearest labelled voxel: fill, TSDF (extension: pca_voxel_distance) ------------
    def voxel_distance_device(self, labels, seen, view, z_range, nz, sites=None, metric='metres', max_dist=None, fill_dist=None,
                              fill_free=False, tsdf_trunc=None, flip=True):
        """The exact distance transform of the volumes of voxel_labels_device / voxel_rays_device (uint8 [nz, px, px], cuda
        tensors or numpy arrays; seen may be None) on the grid of side `view` metres with nz height bins over z_range:
        DeviceStore.voxel_distance's dict of cuda tensors 'dist2', 'nearest', 'nearest_label' (, 'filled' with fill_dist,
        'tsdf' with tsdf_trunc) plus 'weights' = (w_xy, w_z) and 'unit': sqrt(dist2) * unit is the distance.
        metric='metres': the weights of pca_amd.host_logic.voxel_metric for this grid's cell and bin, unit in metres, and
        max_dist / fill_dist / tsdf_trunc in metres; 'voxel': weights (1, 1), unit 1, and they count voxels.  A distance d
        becomes the integer bound floor((d / unit)^2).  sites: the labels that make a site (None: every label).  flip: the
        flipped TSDF, 1 at a surface and 0 at tsdf_trunc and beyond."""
        import math

        from pca_amd import host_logic as hl
        st = self._tmp_store('ssc')
        labels = st._u8_volume(labels, 'labels')
        px = int(labels.shape[1])
        if metric == 'metres':
            lo, step, _ = self._voxel_grid(z_range, nz)
            w_xy, w_z, unit = hl.voxel_metric(float(view) / px, step, px=px, nz=int(labels.shape[0]))
        elif metric == 'voxel':
            w_xy, w_z, unit = 1, 1, 1.
        else:
            raise ValueError("metric must be 'metres' or 'voxel'")

        def bound(d):
            return None if d is None else int(min(math.floor((float(d) / unit) ** 2), 2 ** 31 - 1))
        out = st.voxel_distance(labels, seen, site_labels=sites, weights=(w_xy, w_z), max_dist2=bound(max_dist),
                                fill_dist2=bound(fill_dist), fill_free=fill_free,
                                tsdf=None if tsdf_trunc is None else (unit, float(tsdf_trunc), flip))
        out['weights'], out['unit'] = (w_xy, w_z), unit
        return out

    # ---- free-space carving: points that beams saw through are dynamic (extension: pca_bev_voxel_carve) ------------
    def dynamic_classes(self):
        """The classes that can move: sem_idxs' car, truck, bus and motorcycle (those the dynamic plane is made of)."""
        return [self.sem_idxs[k] for k in ('car', 'truck', 'bus', 'motorcycle') if k in self.sem_idxs]

    def voxel_carve_device(self, pc, origins, rot_mat, dx, dy, aug_view_size, z_range, nz, classes=None, end_margin=1,
                           min_cross=2, ratio=1.0, include_dyn=False, mark_dyn=False):
        """The rays of voxel_rays_device (same point sets, same origins, same grid), counted: DeviceStore.bev_voxel_carve's
        dict of cuda tensors 'hits', 'cross' (int32 [nz, px, px]), 'flags' (uint8, one per point: 1 = a point of `classes`
        whose voxel the beams went through, 0 = one they did not, 255 everything else) and 'stats' (int64 [6]).  classes:
        class indices or sem_idxs names; None: dynamic_classes().  The defaults of end_margin, min_cross and ratio are this
        project's choice, checked on a synthetic scene only; no real-data number exists.
        mark_dyn applies to a WindowPart only: the flagged points of the device window get dyn = 1, for good."""
        grid = self._voxel_grid(z_range, nz)
        if isinstance(pc, np.ndarray):
            raise ValueError('voxel_carve_device: host rows come as a list of per-frame arrays, one origin each')
        if mark_dyn and not isinstance(pc, WindowPart):
            raise ValueError('mark_dyn needs a device window: host rows are not written')
        if not isinstance(pc, WindowPart):
            pc = [np.asarray(f, dtype=np.float64).reshape(-1, 10) for f in pc]
        classes = self.dynamic_classes() if classes is None else self._classes_of(classes)
        st, prm, frames = self._one_set_pass(pc, 'carve', rot_mat, dx, dy, aug_view_size, per_frame=True)
        return st.bev_voxel_carve(prm, *grid, origins, classes, end_margin=end_margin, min_cross=min_cross, ratio=ratio,
                                  include_dyn=include_dyn, mark_dyn=mark_dyn, **frames)

    # ---- object voxels clustered into instances (extension: pca_bev_voxel_instances) ------------
    def voxel_instances_device(self, pc, rot_mat, dx, dy, aug_view_size, z_range, nz, classes=None, min_points=1,
                               connectivity=26, min_voxels=1, max_instances=4096, dyn='static'):
        """One point set clustered into instances on the grid of voxel_labels_device (same frame, same z_range and nz):
        DeviceStore.bev_voxel_instances' dict of cuda tensors 'inst', 'ids', 'table', 'label_counts', 'top_label', 'stats'.
        pc: a WindowPart ('ids' in the order of the part's frames in the store) or host rows in BEV-frame metres ('ids' in
        row order).  classes: a list of class lists as voxel_labels_device takes them, list i becomes label i (sem_idxs
        names are taken too) and every other class takes no part; None: dynamic_classes(), one label each."""
        grid = self._voxel_grid(z_range, nz)
        classes = [[c] for c in self.dynamic_classes()] if classes is None else [self._classes_of(g) for g in classes]
        table, n_labels = self.voxel_label_table(classes)
        st, prm, frames = self._one_set_pass(pc, 'inst', rot_mat, dx, dy, aug_view_size)
        return st.bev_voxel_instances(prm, *grid, table, n_labels, min_points=min_points, connectivity=connectivity,
                                      min_voxels=min_voxels, max_instances=max_instances, dyn=dyn, **frames)

    # ---- oriented metric boxes around those instances (extension: pca_bev_instance_boxes) ------------
    def instance_boxes_device(self, pc, ids, n_rows, rot_mat, dx, dy, aug_view_size, n_angles=90, criterion='area', edge_dist=0.2,
                              cos_sin=None, extents=False, near=False):
        """The oriented boxes of the instances `ids` names in one point set, in the frame voxel_instances_device clusters in
        (same pc, rot_mat, dx, dy and aug_view_size): DeviceStore.bev_instance_boxes' dict of cuda tensors 'fit', 'fit_n',
        'boxes', 'stats' (, 'extents', 'near').  ids: voxel_instances_device's 'ids' for the same pc (a cuda int32 tensor, one
        per point); n_rows: the rows of the result, that call's max_instances.  The directions searched are
        host_logic.fit_angles(n_angles), a quarter turn in n_angles steps, or the caller's own cos_sin [n, 2]."""
        from pca_amd.host_logic import fit_angles
        table = fit_angles(n_angles) if cos_sin is None else cos_sin
        st, prm, frames = self._one_set_pass(pc, 'inst', rot_mat, dx, dy, aug_view_size)
        return st.bev_instance_boxes(prm, ids, n_rows, table, criterion=criterion, edge_dist=edge_dist, extents=extents, near=near,
                                     **frames)

    # ---- those instances matched to the previous sample's: stable ids (extension: pca_voxel_instance_match) ------------
    def voxel_instance_match_device(self, prev, cur, T_cur_from_prev, prev_track=None, counter=None, min_overlap=1, min_iou=0.0,
                                    cap_pairs=None, ids=None):
        """The instances of the sample `cur` matched to those of the sample `prev`, each a record (inst, rows, geom): the
        int32 [nz, px, px] instance volume voxel_instances_device returns as 'inst', the rows it is numbered over (that
        call's max_instances) and geom = (origin xyz, R 3 x 3, dx, dy, view, px, z_lo, z_step), where its grid lies in the
        store's coordinates at its moment (pca_amd.tracks.grid_geom).  T_cur_from_prev: f64 4 x 4, the rigid map the stored
        points underwent between the two moments (store_frame() now times the inverse of store_frame() then).  The index
        map is pca_amd.host_logic.voxel_index_map's; everything else is DeviceStore.voxel_instance_match's, whose dict of
        cuda tensors is returned.  Two samples of different px or nz raise a ValueError: such grids are out of scope."""
        from pca_amd import host_logic as hl
        (prev_inst, n_prev, prev_geom), (cur_inst, n_cur, cur_geom) = prev, cur
        if tuple(prev_inst.shape) != tuple(cur_inst.shape) or int(prev_geom[5]) != int(cur_geom[5]) or \
                int(cur_geom[5]) != int(cur_inst.shape[1]):
            raise ValueError('voxel_instance_match_device: the two samples must share px and nz')
        M = hl.voxel_index_map(prev_geom, cur_geom, T_cur_from_prev)
        return self._tmp_store('ssc').voxel_instance_match(prev_inst, n_prev, cur_inst, n_cur, M, prev_track=prev_track,
                                                           counter=counter, min_overlap=min_overlap, min_iou=min_iou,
                                                           cap_pairs=cap_pairs, ids=ids)

    def static_obj_partitioning_by_elev(self, pc: np.array, elev_thresh: float):
        """The reference's method (sem_bev.py:556-591).  pc: pre-gridded rows (columns 0, 1 = cell indices, 2 = z, 8 = the
        partition column).  Builds the minimum-z map of ALL the rows (no static partition, no height filter: the method
        reduces whatever rows it is given), sets column 8 of every row whose z lies more than elev_thresh above its cell's
        minimum to 1 IN PLACE and returns (pc_static, pc_dynamic, elevmap, elevmap_obs_mask): the rows whose column 8 is 0,
        those whose column 8 is 1 (a row whose column 8 was already >= 2 and is not elevated lands in neither), the f64
        (px, px) minimum map in image rows and its bool mask.  Minimum and flags come from the device
        (pca_bev_elev_partition); the bookkeeping runs on the caller's own f64 rows.
        What differs from the reference, at inputs of measure zero: a cell index equal to px is clamped to px - 1 (the
        reference raises an IndexError for column 0 and wraps to the last image row for column 1); where a pre-gridded z of
        -0.0 ties with +0.0 for a cell's minimum, the map holds +0.0 (in the reference it holds whichever came first);
        a row whose z is not finite, or whose cell lies outside the grid, takes no part and keeps its column 8."""
        px = self.pixel_size
        n = int(pc.shape[0])
        rows = np.zeros((n, 10))
        ij = np.asarray(pc[:, 0:2], dtype=np.float64)
        rows[:, 0:2] = np.where(ij == px, px - 1, ij)
        rows[:, 2] = pc[:, 2]
        rows = self._grid_rows_to_metres(rows)
        hf, self.height_filter = self.height_filter, None
        try:
            out = self.elev_partition_device(rows, np.eye(3), 0., 0., float(self.view_size), elev_thresh, include_dyn=True)
        finally:
            self.height_filter = hf
        elevated = out['flags'].cpu().numpy() == 1
        pc[elevated, 8] = 1
        pc_static = pc[pc[:, 8] == 0]
        pc_dynamic = pc[pc[:, 8] == 1]
        return pc_static, pc_dynamic, out['elev'].cpu().numpy(), out['observed'].cpu().numpy()

    def to_host_async(self, planes, results):
        """planes: cuda float16 [k,21,px,px] holding the k device_only results `results` (generate(..., device_only=True,
        out=planes[i])).  ONE device->host copy of all k samples is enqueued on a side stream into pinned memory; returns
        k LazyBev dicts at once (bev_num > 1: the k augmented rasters run back to back, no host round trip between)."""
        import torch
        from pca_amd import _lib
        ctx = _lib.Context.get(planes.device)
        # a fresh pinned block per call: torch's caching host allocator hands back a block whose arrays have all died, so in
        # steady state this allocates nothing.  The copy itself is ONE library call (pca_host_d2h_async: a side stream of
        # the context behind the current stream's work, a completion event named by a ticket) -- the same in torch (stream
        # context, wait_stream, copy_, Event, record_stream) was 0.04 ms per sample.
        host = torch.empty(tuple(planes.shape), dtype=torch.float16, pin_memory=True)
        ticket = ctx.lib.pca_host_d2h_async(ctx.h, planes.data_ptr(), host.data_ptr(), planes.numel() * planes.element_size(),
                                            ctx.stream())
        if ticket < 0:
            ctx.check(ticket)
        assert planes.is_contiguous()
        event = _PendingCopy(ctx, ticket, (planes, host))
        bevs = [LazyBev(host, i, event, (r['trajs_present'], r['trajs_future'], r['trajs_full']), r.get('gt_lanes'))
                for i, r in enumerate(results)]
        block = [b._pending[3] for b in bevs]
        for b in bevs:
            if b._dev_preview is not None:   # one sheet job renders the block: it needs every sample's trajectories
                b._dev_preview = b._dev_preview[:2] + (block, )
        return bevs

    @staticmethod
    def warp_planes_device(p16, a_1, a_2, b_1, b_2, out16=None):
        """cuda float16 [n,px,px] -> warped copy (bev_generator.py:482-525 of the reference as one gather kernel)."""
        import torch
        from pca_amd import _lib
        ctx = _lib.Context.get()
        out = out16 if out16 is not None else torch.empty_like(p16)
        assert p16.is_contiguous() and out.is_contiguous() and out.shape == p16.shape and out.dtype == torch.float16
        ctx.check(ctx.lib.pca_bev_warp(ctx.h, p16.data_ptr(), out.data_ptr(), int(p16.shape[0]), int(p16.shape[1]),
                                       float(a_1), float(a_2), float(b_1), float(b_2), ctx.stream()))
        return out

    @staticmethod
    def pack_bev(planes, trajs_present, trajs_future, trajs_full, gt_lane_trajs=None):
        """planes: float16 [21,px,px] set-major -> the reference's dict."""
        bev = {}
        trajs = {'present': trajs_present, 'future': trajs_future, 'full': trajs_full}
        for s, name in enumerate(SETS):
            p = planes[7 * s:7 * s + 7]
            bev[f'road_{name}'] = p[0]
            bev[f'trajs_{name}'] = trajs[name]
            bev[f'intensity_{name}'] = p[1]
            bev[f'rgb_{name}'] = p[2:5]
            bev[f'dynamic_{name}'] = p[5]
            bev[f'elevation_{name}'] = p[6]
        if gt_lane_trajs is not None:
            bev['gt_lanes'] = gt_lane_trajs
        return bev

    # ------------------------------------------------------------------------------------------
    def _grid_rows_to_metres(self, rows):
        rows = np.array(rows, dtype=np.float64)
        px, view = self.pixel_size, float(self.view_size)
        rows[:, 0:2] = (rows[:, 0:2] + 0.5 - 0.5 * px) * view / px
        return rows

    def _planes_from_grid_rows(self, pc):
        rows = self._grid_rows_to_metres(pc)
        rows[:, 9] = 0                       # these helpers reduce whatever rows they are given
        hf, self.height_filter = self.height_filter, None
        try:
            empty = np.zeros((0, 10))
            _, p64 = self.rasterise(rows, empty, empty, np.eye(3), 0., 0., float(self.view_size), want_f64=True)
        finally:
            self.height_filter = hf
        return p64[:7].cpu().numpy()

    def get_elevation_map(self, pc: np.array):
        """pc: pre-gridded rows (columns 0,1 = cell indices).  Returns (min-z map, observed mask)."""
        p = self._planes_from_grid_rows(pc)
        mask = np.zeros((self.pixel_size, self.pixel_size), dtype=bool)
        ij = np.asarray(pc)[:, :2].astype(int)
        mask[self.pixel_size - 1 - ij[:, 1], ij[:, 0]] = True
        return p[6], mask

    def get_rgb_maps(self, pc: np.array):
        """Per-cell channel medians (0..255 scale) of pre-gridded rows; empty cells hold rgb_fill."""
        p = self._planes_from_grid_rows(pc)
        return p[2] * 255., p[3] * 255., p[4] * 255.

    def road_marking_transform(self, intensity_map, int_scaler, int_sep_scaler, int_mid_threshold):
        out = int_scaler * self.sigmoid(int_sep_scaler * (intensity_map - int_mid_threshold))
        out[out > 1.] = 1.
        return out

    @staticmethod
    def sigmoid(z):
        return 1 / (1 + np.exp(-z))

    # ------------------------------------------------------------------------------------------
    def viz_bev(self, bev, file_path, rgbs=[], semsegs=[]):
        """Writes a PNG overview of one BEV sample (plot layout is not part of the parity contract).
        PCA_VIZ=device: the sample's preview sheet, rendered and compressed on the device and written by the shared
        background writer (pca_amd.preview: 3 x 5 panels and the trajectories; `rgbs`, `semsegs`, gt_lanes and extra
        sem_planes are not drawn); PCA_ASYNC_WRITE=0 waits for the file.  Default (PCA_VIZ=matplotlib): the figure below."""
        if _preview().selected():
            import os
            w = _writer().shared_writer()
            w.submit_preview(bev, file_path)
            if os.environ.get('PCA_ASYNC_WRITE', '1') == '0':
                _writer().flush_shared()
            return
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        sets = [s for s in SETS if f'road_{s}' in bev]
        cols = ('road', 'intensity', 'rgb', 'dynamic', 'elevation')
        n_img = len(rgbs)
        rows = len(sets) + (1 if n_img else 0)
        fig, axes = plt.subplots(rows, max(len(cols), n_img, 1), figsize=(3 * max(len(cols), n_img, 1), 3 * rows),
                                 squeeze=False)
        for ax in axes.ravel():
            ax.axis('off')
        for r, s in enumerate(sets):
            for c, key in enumerate(cols):
                img = np.asarray(bev[f'{key}_{s}'], dtype=np.float32)
                ax = axes[r][c]
                if key == 'rgb':
                    ax.imshow(np.clip(np.transpose(img, (1, 2, 0)), 0, 1))
                else:
                    ax.imshow(img, vmin=None if key == 'elevation' else 0, vmax=None if key == 'elevation' else 1)
                ax.set_title(f'{key}_{s}', fontsize=8)
                if key == 'road':
                    H = self.pixel_size
                    for t in bev.get(f'trajs_{s}', []):
                        t = np.asarray(t)
                        if t.shape[0]:
                            ax.plot(t[:, 0], H - 1 - t[:, 1], 'r-', linewidth=1)
        for k in range(n_img):
            axes[rows - 1][k].imshow(np.asarray(rgbs[k]))
        fig.tight_layout()
        fig.savefig(file_path)
        plt.close(fig)
