"""Semantic point-cloud accumulator base class -- drop-in for the reference's
``sem_pc_accum.SemanticPointCloudAccumulator`` (same constructor, attributes and method names).

State that the reference keeps as Python lists of (M,10) f64 numpy arrays (``self.sem_pcs``) lives in a
device-resident structure-of-arrays store (pca_amd.device_store.DeviceStore); ``sem_pcs`` is still
readable (it materialises host copies on access).  Poses, segment distances, images stay host lists
exactly like the reference.  There is no CPU fallback: constructing an accumulator without a visible
MI355X raises.
"""
import gzip
import os
import pickle

import numpy as np

from bev_generator.bev_generator import DeviceWindow
from bev_generator.rgb_bev import RGBBEVGenerator  # noqa: F401  (import surface of the reference module)
from bev_generator.sem_bev import SemBEVGenerator
from pca_amd import host_logic as hl


class SemanticPointCloudAccumulator:

    def __init__(self, horizon_dist: float, icp_threshold: float, semseg_onnx_path: str, semseg_filters: list,
                 sem_idxs: dict, use_gt_sem: bool, bev_params: dict):
        self.semseg_model = None
        if use_gt_sem is False:
            self.semseg_model = SemSegONNX(semseg_onnx_path)
        self.semseg_filters = semseg_filters
        self.sem_idxs = sem_idxs
        self.use_gt_sem = use_gt_sem
        self.icp_threshold = icp_threshold
        self.icp_trans_init = np.eye(4)
        self.T_prev_origin = np.eye(4)
        self.pcd_prev = None
        self.horizon_dist = horizon_dist

        self._track = hl.PoseTrack()     # poses (N) and seg_dists (N-1)
        self.rgbs = []
        self.semsegs = []
        self._store = None               # created on first use (needs the GPU)
        # the rigid map the stored points have undergone since construction (store_frame): bookkeeping only
        self._store_frame = np.eye(4)
        self._store_args = {}
        # opt-in voxel de-duplication of the accumulation buffer (extension, off by default: the reference only
        # evicts whole frames).  Set the attribute, or PCA_VOXEL_DEDUP=<voxel size in m> [PCA_VOXEL_DEDUP_EVERY=<k>].
        env = os.environ.get('PCA_VOXEL_DEDUP')
        self.voxel_dedup = float(env) if env else None
        self.voxel_dedup_every = int(os.environ.get('PCA_VOXEL_DEDUP_EVERY', '1'))
        self._integrated = 0
        self._aug_worker0 = 0            # number of the first augmentation "worker" of a generate_bev call (see _run_bev)
        # opt-in sample mode of the projection kernels (extension, default = the reference's nearest pixel):
        # 'bilinear' mixes r, g, b of the four neighbours (PCA_SAMPLE_MODE=bilinear), the class stays the nearest pixel's
        self.sample_mode = os.environ.get('PCA_SAMPLE_MODE', 'nearest')

        self.sem_bev_generator = None
        if bev_params['type'] == 'sem':
            self.sem_bev_generator = SemBEVGenerator(
                self.sem_idxs, bev_params['view_size'], bev_params['pixel_size'], bev_params['max_trans_radius'],
                bev_params['zoom_thresh'], bev_params['do_warp'], bev_params['int_scaler'],
                bev_params['int_sep_scaler'], bev_params['int_mid_threshold'], bev_params['height_filter'])
            # extension: extra class planes per sample (SemBEVGenerator.sem_planes); the key is optional
            self.sem_bev_generator.sem_planes = dict(bev_params.get('sem_planes') or {})
        elif bev_params['type'] == 'rgb':
            raise NotImplementedError('Needs refactoring')

    # ---- state views -------------------------------------------------------------------------
    @property
    def store(self):
        if self._store is None:
            from pca_amd.device_store import DeviceStore
            self._store = DeviceStore(**self._store_args)
        return self._store

    @property
    def poses(self):
        """List of [x,y,z] of the live frames (a copy: mutate through the accumulator, not this list)."""
        return self._track.poses

    @poses.setter
    def poses(self, value):
        self._track.poses = value

    @property
    def seg_dists(self):
        return self._track.seg_dists

    @seg_dists.setter
    def seg_dists(self, value):
        self._track.seg_dists = value

    @property
    def sem_pcs(self):
        """Host copies of the stored frames: list of (M,10) f64 arrays [x,y,z,i,r,g,b,sem,inst,dyn]."""
        if self._store is None:
            return []
        return self._store.frame_rows()

    # ---- integrate (platform specific) ---------------------------------------------------------
    def integrate(self, observations: list):
        raise NotImplementedError()

    def obs2sem_vec_space(self, rgb, pc, sem_gt=None) -> tuple:
        raise NotImplementedError()

    def _after_integrate(self):
        self._integrated += 1
        # errors of kernels that have finished (an overflowing store, a timed-out compaction, ...) surface on the next call
        # at the latest; the read is a few words of mapped host memory, no stream operation
        self.store.poll_status()
        if self.voxel_dedup and self._integrated % max(self.voxel_dedup_every, 1) == 0:
            self.store.voxel_dedup(self.voxel_dedup)

    def update_poses(self, T_new_prev):
        self._track.apply_transform(T_new_prev)

    def update_sem_pcs(self, T_new_prev):
        """Every stored point p <- T_new_prev p, in place on the device (K2; deferred so that a BEV that
        follows immediately applies it in its first pass -- same roundings, one read of the store less)."""
        T_new_prev = np.asarray(T_new_prev, dtype=np.float64)
        self._note_store_motion(T_new_prev)
        self.store.retransform(T_new_prev, defer=True)

    def _note_store_motion(self, T_new_prev):
        """The stored points are re-expressed by T_new_prev (p <- T_new_prev p): store_frame() follows."""
        self._store_frame = np.asarray(T_new_prev, dtype=np.float64).reshape(4, 4) @ self._store_frame

    def store_frame(self):
        """Extension (no reference counterpart): the product, f64 4 x 4, of every rigid map the stored points have been
        re-expressed by since construction, newest on the left (a copy; the identity for a class that never re-expresses its
        store, as NuScenes).  Two moments' values give the map the stored points underwent between them: T_cur_from_prev =
        F_cur inv(F_prev), what pca_amd.host_logic.voxel_index_map and track_instances need.  Bookkeeping only."""
        return self._store_frame.copy()

    def remove_observations(self):
        """Appends the newest path segment and evicts frames beyond the memory horizon."""
        path_length = self._track.push_segment()
        idx = self._track.evict_beyond(self.horizon_dist, path_length)
        if idx:
            self.store.evict(idx)
            self.rgbs = self.rgbs[idx:]
            self.semsegs = self.semsegs[idx:]
        return idx, path_length

    # ---- small host helpers --------------------------------------------------------------------
    @staticmethod
    def comp_incr_path_dist(seg_dists: list):
        return hl.incremental_path_dists(seg_dists)

    def get_segment_dists(self) -> list:
        return self._track.seg_array().tolist()

    def get_incremental_path_dists(self) -> np.array:
        return self._track.incr()

    def get_pose(self, idx: int = None) -> np.array:
        return self._track.as_array() if idx is None else self._track.pose(idx)

    def get_rgb(self, idx: int = None) -> list:
        return self.rgbs if idx is None else [self.rgbs[idx]]

    def get_semseg(self, idx: int = None) -> list:
        return self.semsegs if idx is None else [self.semsegs[idx]]

    @staticmethod
    def dist(pose_0: np.array, pose_1: np.array):
        return hl.pose_dist(pose_0, pose_1)

    @staticmethod
    def write_compressed_pickle(obj, filename, write_dir):
        """gzip(pickle(obj)) -> write_dir/filename.gz, the reference's container (sem_pc_accum.py:280-294).  A BEV sample
        whose planes are still in flight (LazyBev) goes to the process-wide background writer (pca_amd.writer: device wait,
        pickling and compression off the driver's thread; flushed at exit); PCA_ASYNC_WRITE=0 keeps it synchronous."""
        from bev_generator.sem_bev import LazyBev
        if isinstance(obj, LazyBev) and os.environ.get('PCA_ASYNC_WRITE', '1') != '0':
            from pca_amd.writer import shared_writer
            shared_writer().submit(obj, filename, write_dir)
            return
        path = os.path.join(write_dir, f"{filename}.gz")
        blob = pickle.dumps(obj)
        try:
            with gzip.open(path, "wb") as f:
                f.write(blob)
        except IOError as error:
            print(error)

    @staticmethod
    def read_compressed_pickle(path):
        from pca_amd import writer
        writer.flush_shared()                 # samples handed to the background writer are on disk before anything is read
        try:
            with gzip.open(path, "rb") as f:
                return pickle.loads(f.read())
        except IOError as error:
            print(error)

    @staticmethod
    def pc2pcd(pc):
        import open3d as o3d
        pcd = o3d.geometry.PointCloud()
        pcd.points = o3d.utility.Vector3dVector(pc[:, :3])
        pcd.estimate_normals()
        return pcd

    # ---- projection helpers of the reference's public surface (device-backed) ---------------------
    def _k1_rows(self, pc_velo, rgb, sem, P_velo_frame, filters):
        import torch
        from pca_amd.device_store import DeviceStore
        H, W = sem.shape[:2]
        tmp = DeviceStore(capacity=max(pc_velo.shape[0], 1), max_frames=2)
        dev = tmp.device
        frame = dict(pts=torch.from_numpy(np.ascontiguousarray(pc_velo, dtype=np.float32)).to(dev),
                     rgb=torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(dev),
                     sem=torch.from_numpy(np.ascontiguousarray(sem, dtype=np.uint8)).to(dev))
        tmp.append_kitti([frame], P_velo_frame, H, W, filters)
        return tmp.rows(0)

    def filter_semseg_pc(self, pc):
        keep = ~np.isin(pc[:, -1], list(self.semseg_filters))
        return pc[keep]

    def gen_semantic_pc(self, pc_velo, semantic_map, P_velo_frame):
        """(M, 4+K) rows [x,y,z,i, map channels] of the points that project inside the map."""
        semantic_map = np.asarray(semantic_map)
        K = semantic_map.shape[2]
        if K == 3:
            rows = self._k1_rows(pc_velo, semantic_map, np.zeros(semantic_map.shape[:2], np.uint8), P_velo_frame, [])
            return rows[:, :7]
        if K == 1:
            rgb0 = np.zeros(semantic_map.shape[:2] + (3, ), np.uint8)
            rows = self._k1_rows(pc_velo, rgb0, semantic_map[..., 0], P_velo_frame, [])
            return np.concatenate([rows[:, :4], rows[:, 7:8]], axis=1)
        raise NotImplementedError('semantic_map must have 1 or 3 layers')

    @staticmethod
    def velo2frame(pc_velo, P_velo_frame):
        """(N,3) velodyne -> (N,3) homogeneous image-frame coordinates (host helper, numpy)."""
        homo = np.concatenate((pc_velo, np.ones((pc_velo.shape[0], 1))), axis=1)
        return np.matmul(P_velo_frame, homo.T).T

    def velo2img(self, pc_velo, P_velo_frame, img_h, img_w, max_depth=np.inf):
        """(N,4) velodyne rows -> (M,6) rows [x, y, z, i, u, v] of the points that project inside the image (host
        helper for direct callers, the reference's expressions: sem_pc_accum.py:367-402; integrate() runs K1)."""
        frame = self.velo2frame(pc_velo[:, :3], P_velo_frame)
        depth = frame[:, 2]
        depth[depth == 0] = -1e-6
        u = np.round(frame[:, 0] / np.abs(depth)).astype(int)
        v = np.round(frame[:, 1] / np.abs(depth)).astype(int)
        inside = (u >= 0) & (u < img_w) & (v >= 0) & (v < img_h) & (depth > 0) & (depth < max_depth)
        return np.concatenate([pc_velo, u[:, None], v[:, None]], axis=1)[inside]

    def viz_sem_vec_space(self):
        """Open3D window with every stored point (host copy of the device store) and the ego path."""
        self.viz_sem_pc(np.concatenate(self.sem_pcs, axis=0), self.poses)

    @staticmethod
    def viz_sem_pc(sem_pc: np.array, poses: list = []):
        """sem_pc: (N,>=7) rows [x, y, z, intensity, r, g, b, ...]; poses: list of [x, y, z].  Needs open3d."""
        import open3d as o3d
        cloud = o3d.geometry.PointCloud()
        cloud.points = o3d.utility.Vector3dVector(sem_pc[:, :3])
        cloud.colors = o3d.utility.Vector3dVector(np.asarray(sem_pc[:, 4:7], dtype=np.float64) / 255.)
        frame = o3d.geometry.TriangleMesh.create_coordinate_frame(size=1, origin=poses[0] if len(poses) else [0, 0, 0])
        path = o3d.geometry.LineSet(points=o3d.utility.Vector3dVector(poses),
                                    lines=o3d.utility.Vector2iVector([[k, k + 1] for k in range(len(poses) - 1)]))
        path.colors = o3d.utility.Vector3dVector([[1, 0, 0]] * max(len(poses) - 1, 0))
        o3d.visualization.draw_geometries([frame, path, cloud])

    # ---- BEV -------------------------------------------------------------------------------------
    def viz_bev(self, bev, file_path, rgbs: list = [], semsegs: list = []):
        self.sem_bev_generator.viz_bev(bev, file_path, rgbs, semsegs)

    def generate_bev(self, present_idx: int = None, bev_num: int = 1, gen_future: bool = False):
        raise NotImplementedError()

    def _window_inputs(self, present_idx, gen_future, other_trajs=None, gt_lanes=None):
        """The reference's (pcs, trajs) dicts for one BEV sample, with device window handles in place of
        the concatenated host arrays (kitti360_sem_pc_accum.py:180-228 / nuscenes_oracle_...py:521-595)."""
        poses = self._track.as_array()
        origin = poses[-1].copy() if present_idx is None else poses[present_idx].copy()
        split = self.store.n_frames if present_idx is None else \
            (present_idx if present_idx >= 0 else self.store.n_frames + present_idx)
        if split <= 0:
            raise ValueError('need at least one array to concatenate')     # np.concatenate([]) in the reference
        all_sets = present_idx is None and gen_future        # the reference slices [:None] and [None:]: everything
        win = DeviceWindow(self.store, split, origin, future_is_present=all_sets)
        pcs = {'pc_present': win.part('present')}
        rel = poses - origin
        trajs = {'ego_traj_present': rel[:present_idx]}
        others = other_trajs if other_trajs is not None else ([], [], [])
        trajs['other_trajs_present'] = [np.concatenate([t]) - origin for t in others[0]]
        if gt_lanes is not None:
            if isinstance(gt_lanes, list):
                trajs['gt_lanes'] = [lane - origin for lane in gt_lanes]
            else:                                    # a device lane set: a handle, not L shifted copies
                from pca_amd.lanes import LaneHandle
                trajs['gt_lanes'] = LaneHandle(gt_lanes, origin)
        if gen_future:
            if split >= self.store.n_frames and not all_sets:
                raise ValueError('need at least one array to concatenate')
            pcs['pc_future'] = win.part('future')
            pcs['pc_full'] = win.part('full')
            trajs['ego_traj_future'] = rel[present_idx:]
            trajs['ego_traj_full'] = rel
            if not all_sets:
                trajs['_ego_split'] = split
            trajs['other_trajs_future'] = [np.concatenate([t]) - origin for t in others[1]]
            trajs['other_trajs_full'] = [np.concatenate([t]) - origin for t in others[2]]
        else:
            for k in ('pc_future', 'pc_full'):
                pcs[k] = None
            for k in ('ego_traj_future', 'other_trajs_future', 'ego_traj_full', 'other_trajs_full'):
                trajs[k] = None
        return pcs, trajs

    def _run_bev(self, pcs, trajs, bev_num):
        """bev_num samples of one window.  The reference forks a multiprocessing.Pool for bev_num > 1 (pickling the window
        per worker, kitti360_sem_pc_accum.py:236-241); here the bev_num rasters are enqueued back to back on the device
        into one [bev_num,21,px,px] tensor and leave it in ONE asynchronous copy: the returned dicts (LazyBev) fill in on
        first access.  Each raster has its own random augmentation, drawn as generate_rand_aug draws it: sample k reseeds
        as the reference's k-th Pool worker would (pid + k in place of the worker's own pid), so the samples of one
        window differ although they are drawn in one process within the same second."""
        import torch
        from bev_generator.bev_generator import WindowPart
        gen = self.sem_bev_generator
        if self._store is not None:
            self._store.poll_status()
        if not isinstance(pcs['pc_present'], WindowPart) or os.environ.get('PCA_SYNC_BEV') or getattr(gen, 'sem_planes', None):
            return [gen.generate_multiproc((pcs, self._copy_trajs(trajs)), worker=self._aug_worker0 + k)
                    for k in range(bev_num)]
        px = gen.pixel_size
        planes = torch.empty((bev_num, 21, px, px), dtype=torch.float16, device=self.store.device)
        with gen.raster_batch():                  # bev_num > 1: ONE launch of each kernel for all the samples
            results = [gen.generate_multiproc((pcs, self._copy_trajs(trajs)), device_only=True, out=planes[k],
                                              worker=self._aug_worker0 + k) for k in range(bev_num)]
        return gen.to_host_async(planes, results)

    def _window_inputs_for(self, present_idx, gen_future):
        """(pcs, trajs) of one sample as generate_bev builds them (overridden where other agents' trajectories exist)."""
        return self._window_inputs(present_idx, gen_future)

    def _unaugmented_part(self, present_idx, part):
        """(pc, rot_mat, view) of `part` ('present' | 'future' | 'full') of the sample generate_bev(present_idx, 1, True) would
        make, un-augmented: heading from the last two present poses, no shift, zoom 1."""
        if part not in ('present', 'future', 'full'):
            raise ValueError("part must be 'present', 'future' or 'full'")
        self.store.poll_status()
        pcs, trajs = self._window_inputs_for(present_idx, True)
        rot_mat = hl.rotation_matrix_3d(hl.heading_rot_ang(trajs['ego_traj_present']))
        return pcs['pc_' + part], rot_mat, 1. * self.sem_bev_generator.view_size

    def partition_by_elev(self, present_idx, elev_thresh, part='full', mark_dyn=False):
        """Extension (the reference's static_obj_partitioning_by_elev, sem_bev.py:556-591, on the device window): the points
        of `part` ('present' | 'future' | 'full') of the sample generate_bev(present_idx, 1, True) would make, partitioned by
        height above the minimum z of their cell, in that sample's un-augmented frame (heading from the last two present
        poses, no shift, zoom 1) and over its static partition (dyn != 1).  Returns DeviceStore.bev_elev_partition's dict of
        cuda tensors; 'elev' of part='present' is the f64 elevation plane of that sample.  What KITTI needs, where no
        instance labels exist and dyn is 0 everywhere: mark_dyn=True sets dyn = 1 for the elevated points, in the store,
        for good -- they then stay out of the medians, the elevation and the intensity planes of every later sample."""
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        return self.sem_bev_generator.elev_partition_device(pc, rot_mat, 0., 0., view, elev_thresh, include_dyn=False,
                                                            mark_dyn=mark_dyn)

    def voxel_labels(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, include_dyn=False):
        """Extension (no reference counterpart): semantic occupancy labels of `part` ('present' | 'future' | 'full') of the
        sample generate_bev(present_idx, 1, True) would make, in that sample's un-augmented frame (heading from the last
        two present poses, no shift, zoom 1): the sample's grid with nz height bins over z_range metres, a majority vote
        over the labelled points of every voxel.  classes: a list of class lists, list i becomes label i; None: label =
        class for the classes 0 .. 31.  Returns DeviceStore.bev_voxel_labels' dict of cuda tensors 'labels', 'counts',
        'top', each [nz, px, px]; labels 255 = no point in the voxel (free or unseen is not decided here: voxel_occupancy).
        Nothing is written: the store, the owed re-transforms and every later sample stay as they are."""
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        return self.sem_bev_generator.voxel_labels_device(pc, rot_mat, 0., 0., view, z_range, nz, classes=classes,
                                                          include_dyn=include_dyn)

    def voxel_occupancy(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, include_dyn=False,
                        origins=None):
        """Extension (no reference counterpart): voxel_labels of `part` plus what the lidar rays tell about its empty voxels,
        in the same un-augmented frame.  One ray per stored point of the part, from the sensor position of the point's frame
        to the point (DeviceStore.bev_voxel_rays).  origins: [frames of the part, 3] sensor positions in the store's
        coordinates; None: the pose-track rows of the part's frames (a caller whose sensor does not sit at the pose passes
        its own, e.g. NuScenes with the lidar above the ego origin).  One origin per stored frame -- the merged sweeps of a
        NuScenes sample share their key frame's -- and no per-beam minimum or maximum range.
        Returns cuda tensors: 'labels', 'counts', 'top' as voxel_labels gives them; 'seen' uint8 [nz, px, px], 'stats'
        int64 [4]; 'state' uint8 [nz, px, px]: 2 = occupied (counts > 0), else 1 = free (a ray passed through), else
        0 = unseen (what semantic-scene-completion training has to ignore).  Nothing is written to the store."""
        import torch
        gen = self.sem_bev_generator
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        if origins is None:
            lo, hi = pc.frames()
            origins = self._track.as_array()[lo:hi]
        out = gen.voxel_labels_device(pc, rot_mat, 0., 0., view, z_range, nz, classes=classes, include_dyn=include_dyn)
        out.update(gen.voxel_rays_device(pc, origins, rot_mat, 0., 0., view, z_range, nz, include_dyn=include_dyn))
        out['state'] = torch.where(out['counts'] != 0, 2, out['seen'].to(torch.int32)).to(torch.uint8)
        return out

    def voxel_visibility(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, include_dyn=False,
                         origins=None, cameras=None, stride=1, max_depth=None):
        """Extension (no reference counterpart): voxel_occupancy of `part` plus the voxels a camera can see -- the
        'mask_camera' of Occ3D beside its 'mask_lidar' (our 'seen'), the '.occluded' of SemanticKITTI-SSC beside '.invalid' --
        on the same grid, in the same un-augmented frame.  One ray per pixel of every camera (every stride-th pixel), from
        the camera centre to camera depth max_depth, through the voxels until the first occupied one; occupied means
        labels != 255, so the occupancy is whatever voxel_labels says under `classes` and include_dyn.
        cameras: a list of (P, (W, H)), P 3x4 from the STORE's coordinates to the image, as render_camera takes it; 'visible'
        is the union over them.  None: the dataset's own camera where the stored coordinates belong to one -- the KITTI class:
        p_velo_frame and the size of the last integrated image, that is the NEWEST frame's camera, which is the camera of the
        grid's own moment only for present_idx=None; the base class and NuScenes raise a ValueError.  max_depth: None: the
        generator's view_size -- the grid is view x view around the ego, so nothing in it lies deeper.  One pinhole per
        camera and no lens distortion.
        Returns voxel_occupancy's dict, unchanged, plus DeviceStore.bev_voxel_camera's: 'visible' uint8 [nz, px, px] (1 = a
        ray reached the voxel, the one that stopped it included); 'hit' int32, 'depth' float32, 'label' uint8, lists with one
        [H // stride, W // stride] tensor per camera (the first occupied voxel's place, camera depth and label; -1, 0 and 255
        where the ray hit nothing); 'camera_stats' int64 [cameras, 5] = rays, cast, dropped not finite, dropped too long,
        hits.  Nothing is written to the store."""
        gen = self.sem_bev_generator
        if cameras is None:
            P, size = self._render_defaults()
            if P is None or size is None:
                raise ValueError('voxel_visibility needs cameras: a list of (P 3x4 store coordinates -> image, (W, H))')
            cameras = [(P, size)]
        cameras = [(np.asarray(P, dtype=np.float64)[:3], size) for P, size in cameras]
        out = self.voxel_occupancy(present_idx, part=part, z_range=z_range, nz=nz, classes=classes, include_dyn=include_dyn,
                                   origins=origins)
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        cam = gen.voxel_camera_device(pc, out['labels'], cameras, rot_mat, 0., 0., view, z_range, nz, stride=stride,
                                      max_depth=1. * gen.view_size if max_depth is None else max_depth)
        out['camera_stats'] = cam.pop('stats')
        out.update(cam)
        return out

    def voxel_ssc_sample(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, include_dyn=False,
                         origins=None, cameras=None, stride=1, max_depth=None, scales=(1, 2, 4, 8), input_frames=1,
                         label_map=None, occluded=True):
        """Extension (no reference counterpart): one semantic-scene-completion sample in SemanticKITTI-SSC's form -- the
        volumes of voxel_visibility (occluded=True) or, for the classes without a default camera, of voxel_occupancy
        (occluded=False) of `part`, pooled to `scales` and packed into file payloads on the device
        (SemBEVGenerator.voxel_pyramid_device).  Returns that dict, unchanged, plus 'input_occ' uint8 [nz, px, px]: 1 where
        a voxel_labels pass over the last input_frames frames of the PRESENT part -- same frame, grid and classes -- found a
        point: the single-scan input the benchmark's .bin holds; 'levels': {s: volumes}, level 1 = 'labels', 'seen', 'state'
        (, 'visible'), 'input_occ', the pooled levels 'labels', 'state' (, 'visible'); 'packed': {s: payloads}, level 1 =
        'label', 'invalid' (, 'occluded'), 'bin', the pooled levels 'label' and 'invalid'.  label_map: 32 file values, None:
        label + 1 (0 is 'empty' in the files).  pca_amd.ssc.write_ssc_sample writes the files.
        voxel_ssc_sample_filled is the same sample with the pinholes of accumulated lidar closed first.
        Nothing is written to the store."""
        return self._voxel_ssc_sample(present_idx, None, part, z_range, nz, classes, include_dyn, origins, cameras, stride,
                                      max_depth, scales, input_frames, label_map, occluded)

    def voxel_ssc_sample_filled(self, present_idx, fill_dist, **sample):
        """Extension (no reference counterpart): voxel_ssc_sample(present_idx, **sample) with the pinholes of accumulated lidar
        closed.  Far road and wall surfaces are hit in every second or third voxel only, and the voxels between the hits are
        unseen -- a beam ends on a surface -- so they would land in .invalid.  fill_dist: a radius in metres; an unseen empty
        voxel within it of a labelled one takes that voxel's label, of equally near ones the label of the smallest place
        (SemBEVGenerator.voxel_distance_device, metric='metres'; a voxel a beam crossed stays free), and 'levels' and
        'packed' are made from these 'filled' labels instead of 'labels': a filled voxel is occupied, so it leaves .invalid
        by the pool's and the pack's own rule.  Returns voxel_ssc_sample's dict -- 'labels' is what it was -- plus 'filled'
        uint8, 'dist2' and 'nearest' int32 [nz, px, px].  fill_dist=None is voxel_ssc_sample itself.
        Nothing is written to the store."""
        import inspect
        bound = inspect.signature(self.voxel_ssc_sample).bind(present_idx, **sample)
        bound.apply_defaults()
        return self._voxel_ssc_sample(bound.arguments.pop('present_idx'), fill_dist, **bound.arguments)

    def _voxel_ssc_sample(self, present_idx, fill_dist, part, z_range, nz, classes, include_dyn, origins, cameras, stride, max_depth,
                          scales, input_frames, label_map, occluded):
        gen = self.sem_bev_generator
        if int(input_frames) < 1:
            raise ValueError('input_frames must be >= 1')
        if occluded:
            out = self.voxel_visibility(present_idx, part=part, z_range=z_range, nz=nz, classes=classes, include_dyn=include_dyn,
                                        origins=origins, cameras=cameras, stride=stride, max_depth=max_depth)
        else:
            out = self.voxel_occupancy(present_idx, part=part, z_range=z_range, nz=nz, classes=classes, include_dyn=include_dyn,
                                       origins=origins)
        out['input_occ'], view = self._input_scan_occ(present_idx, z_range, nz, classes, include_dyn, input_frames)
        labels = out['labels']
        if fill_dist is not None:
            d = gen.voxel_distance_device(labels, out['seen'], view, z_range, nz, metric='metres', max_dist=fill_dist,
                                          fill_dist=fill_dist)
            out.update({k: d[k] for k in ('filled', 'dist2', 'nearest')})
            labels = d['filled']
        out.update(gen.voxel_pyramid_device(labels, out['seen'], out.get('visible'), out['input_occ'], scales=scales,
                                            label_map=label_map))
        return out

    def _input_scan_occ(self, present_idx, z_range, nz, classes, include_dyn, input_frames):
        """('input_occ' uint8 [nz, px, px], view): 1 where a voxel_labels pass over the last input_frames frames of the
        PRESENT part of the sample found a point -- the single-scan input of voxel_ssc_sample and voxel_distance."""
        from bev_generator.bev_generator import DeviceWindow
        gen = self.sem_bev_generator
        pc, rot_mat, view = self._unaugmented_part(present_idx, 'present')
        lo, hi = pc.frames()
        w = pc.window
        scan = DeviceWindow(w.store, hi, w.origin, first=max(lo, hi - int(input_frames)), last=hi).part('full')
        # (keep_owed: the scan's window does not cover what the older frames owe, and this call writes nothing)
        one = gen.voxel_labels_device(scan, rot_mat, 0., 0., view, z_range, nz, classes=classes, include_dyn=include_dyn,
                                      keep_owed=True)
        return (one['counts'] != 0).to(one['labels'].dtype), view

    def voxel_distance(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, include_dyn=False, origins=None,
                       sites='labels', site_classes=None, input_frames=1, metric='metres', max_dist=None, fill_dist=None,
                       fill_free=False, tsdf_trunc=None, flip=True):
        """Extension (no reference counterpart): how far every voxel of voxel_occupancy's grid is from the nearest surface --
        the exact distance transform of `part`'s volumes, on the device (SemBEVGenerator.voxel_distance_device, whose options
        metric, max_dist, fill_dist, fill_free, tsdf_trunc and flip are passed on).  sites='labels': the distance is measured
        from the labelled voxels of the part, those of site_classes (labels, as `classes` numbers them; None: all);
        sites='input': from 'input_occ', the scan of the last input_frames frames that voxel_ssc_sample packs into .bin --
        the TSDF input encoding of SSCNet-style models; 'nearest_label' and 'filled' then speak of that scan's single label
        0.  Either way the sign of 'tsdf' and the voxels 'filled' may fill come from the part's own 'seen'.
        Returns voxel_occupancy's dict, unchanged, plus 'dist2', 'nearest', 'nearest_label' (, 'filled', 'tsdf'), 'weights',
        'unit' (, 'input_occ' with sites='input').  Nothing is written to the store."""
        import torch
        if sites not in ('labels', 'input'):
            raise ValueError("sites must be 'labels' or 'input'")
        gen = self.sem_bev_generator
        out = self.voxel_occupancy(present_idx, part=part, z_range=z_range, nz=nz, classes=classes, include_dyn=include_dyn,
                                   origins=origins)
        _, _, view = self._unaugmented_part(present_idx, part)
        if sites == 'input':
            if int(input_frames) < 1:
                raise ValueError('input_frames must be >= 1')
            out['input_occ'], _ = self._input_scan_occ(present_idx, z_range, nz, classes, include_dyn, input_frames)
            # (the scan as a label volume: 0 where it found a point, 255 elsewhere)
            source, site_classes = torch.where(out['input_occ'] != 0, 0, 255).to(torch.uint8), None
        else:
            source = out['labels']
        out.update(gen.voxel_distance_device(source, out['seen'], view, z_range, nz, sites=site_classes, metric=metric,
                                             max_dist=max_dist, fill_dist=fill_dist, fill_free=fill_free, tsdf_trunc=tsdf_trunc,
                                             flip=flip))
        return out

    def carve_dynamic(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, end_margin=1, min_cross=2,
                      ratio=1.0, origins=None, mark_dyn=False):
        """Extension (no reference counterpart): free-space carving by ray hit / miss over `part` ('present' | 'future' |
        'full') of the sample generate_bev(present_idx, 1, True) would make, in that sample's un-augmented frame, on the grid
        of voxel_occupancy.  A voxel in which a point of `classes` was seen at one moment, and which the beams of other
        frames later passed straight through, held a moving object: a point of `classes` is FLAGGED iff its voxel was crossed
        by at least min_cross rays, and by at least ratio times as many rays as ended in it; a ray's last end_margin steps
        before its own end voxel do not count, which keeps a surface from carving itself.  What KITTI needs, where no
        instance labels exist and dyn is 0 everywhere -- and, unlike partition_by_elev, it tells a parked car from a moving
        one and leaves poles and walls alone.
        classes: class indices or sem_idxs names; None: the generator's dynamic classes (car, truck, bus, motorcycle).
        origins: as voxel_occupancy takes them; None: the pose-track rows of the part's frames.  One origin per stored frame.
        The defaults (end_margin=1, min_cross=2, ratio=1.0) are this project's choice, checked only on a synthetic scene (a
        wall, a parked car and a car that leaves: tests/test_voxel_carve_model.py); no real-data number exists.
        Returns DeviceStore.bev_voxel_carve's dict of cuda tensors 'hits', 'cross', 'flags', 'stats'.  Points with dyn == 1
        take no part.  Nothing is written -- unless mark_dyn=True: the flagged points get dyn = 1 in the store, for good (owed
        re-transforms are flushed first), and stay out of the static planes of every later sample.  integrate() never calls
        this on its own."""
        gen = self.sem_bev_generator
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        if origins is None:
            lo, hi = pc.frames()
            origins = self._track.as_array()[lo:hi]
        return gen.voxel_carve_device(pc, origins, rot_mat, 0., 0., view, z_range, nz, classes=classes, end_margin=end_margin,
                                      min_cross=min_cross, ratio=ratio, include_dyn=False, mark_dyn=mark_dyn)

    def voxel_instances(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, min_points=1, connectivity=26,
                        min_voxels=1, max_instances=4096, dyn='static'):
        """Extension (no reference counterpart): which points form one object.  The points of `classes` in `part` ('present' |
        'future' | 'full') of the sample generate_bev(present_idx, 1, True) would make, clustered on the grid of voxel_labels
        in that sample's un-augmented frame: a voxel with at least min_points such points is foreground, foreground voxels
        that touch (connectivity 6: by a face; 26: by a face, an edge or a corner) form a component, a component of at least
        min_voxels voxels is an instance, and the instances are numbered by their smallest voxel index -- the same points in
        any order give the same numbers.  classes: a list of class lists, list i becomes label i; None: the generator's
        dynamic classes (car, truck, bus, motorcycle), one label each.  dyn: 'static' -- points with dyn == 1 take no part
        (the parked things); 'all'; 'dynamic' -- only points with dyn == 1 (the movers after carve_dynamic(mark_dyn=True), or
        of a NuScenes window).
        Returns DeviceStore.bev_voxel_instances' dict of cuda tensors: 'inst' [nz, px, px], 'ids' (one per point of the
        part), 'table' (voxel boxes and counts: pca_amd.host_logic.instance_boxes gives metres), 'label_counts', 'top_label',
        'stats'.  Nothing is written: the store, the owed re-transforms and every later sample stay as they are.
        integrate() never calls this on its own."""
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        return self.sem_bev_generator.voxel_instances_device(pc, rot_mat, 0., 0., view, z_range, nz, classes=classes,
                                                             min_points=min_points, connectivity=connectivity,
                                                             min_voxels=min_voxels, max_instances=max_instances, dyn=dyn)

    def instance_boxes(self, present_idx, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, min_points=1, connectivity=26,
                       min_voxels=1, max_instances=4096, dyn='static', n_angles=90, criterion='area', edge_dist=0.2, instances=None):
        """Extension (no reference counterpart): an oriented metric box around every instance of voxel_instances -- the box a
        detector is trained on or an object is tracked by, where the voxel box of a car parked at 30 degrees to the view is
        about twice its footprint.  Runs voxel_instances with the arguments up to dyn (or takes its dict as `instances`, made
        for the same present_idx and part), then, on the device, searches n_angles directions of a quarter turn for the
        rectangle around each instance's points: criterion 'area' takes the smallest rectangle, 'edge' the one with the most
        points within edge_dist metres of its sides (the search-based fit commonly used for lidar L-shapes: it keeps an L
        seen from two sides from being boxed diagonally).  Only extremes and integer counts are taken, so the same points in
        any order give the same bits.  n_angles=90 (one degree), criterion='area' and edge_dist=0.2 are this project's
        choices, checked on synthetic scenes only (tests/test_instance_boxes_model.py); no real-data number exists.
        Returns voxel_instances' dict plus 'fit' float64 [max_instances, 8], 'fit_n' int32 [max_instances, 2], 'boxes'
        float64 [max_instances, 7] = cx, cy, cz, length, width, height, yaw (length >= width, yaw in [0, pi); NaN rows from
        the number of instances on) and 'box_stats' int64 [4] (DeviceStore.bev_instance_boxes).  Boxes are in the sample's
        un-augmented view frame, the frame of pca_amd.host_logic.instance_boxes, whose voxel box holds each of them.
        Out of scope: boxes tilted out of the ground plane, tracking boxes across samples (track_instances(boxes=True) gives
        the instances ids that hold over a sequence and carries these boxes alongside), merging or splitting instances,
        the variance criterion (its float sums would depend on the order) and a KITTI label_2 / NuScenes writer.
        Nothing is written to the store.  integrate() never calls this on its own."""
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        if instances is None:
            instances = self.voxel_instances(present_idx, part=part, z_range=z_range, nz=nz, classes=classes, min_points=min_points,
                                             connectivity=connectivity, min_voxels=min_voxels, max_instances=max_instances, dyn=dyn)
        fit = self.sem_bev_generator.instance_boxes_device(pc, instances['ids'], int(instances['table'].shape[0]), rot_mat, 0., 0.,
                                                           view, n_angles=n_angles, criterion=criterion, edge_dist=edge_dist)
        out = dict(instances)
        out.update(fit=fit['fit'], fit_n=fit['fit_n'], boxes=fit['boxes'], box_stats=fit['stats'])
        return out

    def track_instances(self, present_idx, state=None, part='full', z_range=(-2.0, 4.4), nz=32, classes=None, min_points=1,
                        connectivity=26, min_voxels=1, max_instances=4096, dyn='static', min_overlap=1, min_iou=0.0, boxes=False,
                        n_angles=90, criterion='area', edge_dist=0.2):
        """Extension (no reference counterpart): instance ids that hold over a sequence of samples.  voxel_instances numbers a
        sample's instances by their smallest voxel place, which says nothing about the next sample; this runs voxel_instances
        with the arguments up to dyn (instance_boxes with boxes=True, which adds 'fit', 'fit_n', 'boxes' and 'box_stats') and
        then, on the device, matches the sample's instance volume against the previous sample's, carried in `state`
        (SemBEVGenerator.voxel_instance_match_device): the centre of every instance voxel is taken through the rigid map the
        store underwent since then (store_frame()) into the previous grid; an instance continues the track of the previous
        instance it overlaps most, if that one overlaps it most too and the overlap is at least min_overlap voxels and min_iou
        of the union; every other instance opens a new track.  state=None starts a sequence: every instance is new, from 0.
        Returns that dict plus 'track' int32 [max_instances] (per instance; -1 for a row without a voxel), 'track_vol' int32
        [nz, px, px], 'track_ids' int32 (one per point of the part, as 'ids'), 'match' int32 [max_instances] (the previous
        sample's row or -1), 'match_stats' int64 [10] (pca.h: pca_voxel_instance_match) and 'state', a pca_amd.tracks.TrackState
        to pass to the next call.  The track counter lives on the device and no count is read back, except the one word that
        says whether the pair table overflowed (a RuntimeError).
        min_overlap=1 and min_iou=0 are this project's choice, checked on synthetic scenes only
        (tests/test_voxel_tracks_model.py); no real-data number exists.
        Out of scope: motion models or prediction, re-identifying a track after a sample in which it was unmatched, merging
        or splitting instances (the larger overlap keeps the track, the rest are new), Hungarian or other globally optimal
        assignment, velocities, different px or nz between samples (a ValueError).
        Nothing is written to the store.  integrate() never calls this on its own."""
        import torch

        from pca_amd.tracks import TrackState, grid_geom
        gen = self.sem_bev_generator
        pc, rot_mat, view = self._unaugmented_part(present_idx, part)
        args = dict(part=part, z_range=z_range, nz=nz, classes=classes, min_points=min_points, connectivity=connectivity,
                    min_voxels=min_voxels, max_instances=max_instances, dyn=dyn)
        if boxes:
            out = dict(self.instance_boxes(present_idx, n_angles=n_angles, criterion=criterion, edge_dist=edge_dist, **args))
        else:
            out = dict(self.voxel_instances(present_idx, **args))
        inst, rows = out['inst'], int(out['table'].shape[0])
        z_lo, z_step, _ = gen._voxel_grid(z_range, nz)
        geom = grid_geom(pc.window.origin, rot_mat, 0., 0., view, gen.pixel_size, z_lo, z_step)
        frame = self.store_frame()
        if state is None:
            # (a sequence starts against a sample without instances: nothing matches, every instance is new)
            prev = (torch.full_like(inst, -1), 1, geom)
            prev_track, counter, T, samples = None, None, np.eye(4), 0
        else:
            prev, prev_track, counter, samples = state.record(), state.track, state.counter, state.samples
            T = frame @ np.linalg.inv(state.frame)
        m = gen.voxel_instance_match_device(prev, (inst, rows, geom), T, prev_track=prev_track, counter=counter,
                                            min_overlap=min_overlap, min_iou=min_iou, ids=out['ids'])
        out.update(track=m['cur_track'], track_vol=m['track_vol'], track_ids=m['track_ids'], match=m['match'],
                   match_stats=m['stats'],
                   state=TrackState(inst.clone(), rows, m['cur_track'], m['counter'], geom, frame, samples + 1))
        return out

    def _render_defaults(self):
        """(P, (W, H)) of render_camera where the dataset has one camera the stored coordinates belong to; (None, None) here."""
        return None, None

    def render_camera(self, P=None, size=None, frames=None, radius=0, depth_range=(0., np.inf), classes=None,
                      include_dyn=True):
        """Extension (the reference's velo2frame + velo2img, sem_pc_accum.py:347-402, over the whole accumulated cloud, with a
        z-buffer): the stored points of the live frames `frames` = (lo, hi) (default: all of them) rendered into a pinhole
        camera -- dense depth, colour and class targets for an image.  P: 3x4, from the STORE's coordinates to the image,
        as p_velo_frame; size = (W, H).  Both are required here: NuScenes stores world coordinates, so a camera with
        intrinsics K and pose T_world_from_cam has P = K [I|0] inv(T_world_from_cam); the KITTI class has defaults.
        A point outside the image or the open interval depth_range is dropped, so is one of a class outside `classes` (a list
        of class indices; None: every class) and, with include_dyn=False, one with dyn == 1.  A kept point competes for the
        pixels within `radius` (0..3) of its own, a square footprint clipped to the image: the splat keeps the background
        from showing through the gaps of a sparse foreground.  A pixel goes to the smallest depth rounded to float32, of
        equal depths to the point stored first.  One P per call and no lens distortion.
        Returns DeviceStore.render_camera's dict of cuda tensors: 'depth' float32 [H, W] (0: no point), 'index' int64 [H, W]
        (the winner's index among the points of `frames`, -1: none), 'rgb' uint8 [H, W, 3], 'sem' uint8 [H, W] (255: none),
        'stats' int64 [3] = points considered, kept, pixels covered.
        Nothing is written: the store, the owed re-transforms and every later sample stay as they are."""
        from pca_amd._lib import make_camera
        self.store.poll_status()
        dflt_P, dflt_size = self._render_defaults() if P is None or size is None else (None, None)
        P = dflt_P if P is None else P
        size = dflt_size if size is None else size
        if P is None or size is None:
            raise ValueError('render_camera needs P (3x4, store coordinates -> image) and size = (W, H)')
        lo, hi = (0, self.store.n_frames) if frames is None else frames
        if not 0 <= lo <= hi <= self.store.n_frames:
            raise ValueError('frames must be a range (lo, hi) of live frames')
        cam = make_camera(np.asarray(P, dtype=np.float64)[:3], size[0], size[1], radius, include_dyn, depth_range)
        return self.store.render_camera(cam, lo, hi, classes=classes)

    def generate_bev_many(self, present_idxs, gen_future: bool = True):
        """Extension (no reference counterpart): the samples generate_bev(idx, 1, gen_future)[0] would return for every idx of
        `present_idxs`, rasterised in ONE launch of each kernel (the store does not change between them: the driver's sweep
        over present_idx of a finished scene, run_nuscenes_bev_gen.py:245-271) and copied to the host in one asynchronous
        transfer.  Returns the list of dicts (LazyBev)."""
        import torch
        gen = self.sem_bev_generator
        present_idxs = list(present_idxs)
        if not present_idxs:
            return []
        self.store.poll_status()
        if getattr(gen, 'sem_planes', None):      # class planes: sample by sample, plain dicts (the path PCA_SYNC_BEV=1 takes in _run_bev)
            out = []
            for idx in present_idxs:
                pcs, trajs = self._window_inputs_for(idx, gen_future)
                out.append(gen.generate_multiproc((pcs, self._copy_trajs(trajs))))
            return out
        px = gen.pixel_size
        planes = torch.empty((len(present_idxs), 21, px, px), dtype=torch.float16, device=self.store.device)
        with gen.raster_batch():
            results = []
            for k, idx in enumerate(present_idxs):
                pcs, trajs = self._window_inputs_for(idx, gen_future)
                results.append(gen.generate_multiproc((pcs, self._copy_trajs(trajs)), device_only=True, out=planes[k]))
        return gen.to_host_async(planes, results)

    @staticmethod
    def _copy_trajs(trajs):
        out = {}
        lanes = trajs.get('gt_lanes')
        if lanes is not None and not isinstance(lanes, list):       # a pca_amd.lanes.LaneHandle passes through as it is
            trajs = dict(trajs)
            out['gt_lanes'] = trajs.pop('gt_lanes')
        for k, v in trajs.items():
            if isinstance(v, list):
                out[k] = [np.array(t) for t in v]
            elif v is None or isinstance(v, int):
                out[k] = v
            else:
                out[k] = np.array(v)
        return out


def SemSegONNX(path):
    """Late import so that GT-semantics runs never need onnxruntime."""
    from utils.onnx_utils import SemSegONNX as _S
    return _S(path)
