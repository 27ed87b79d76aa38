"""What the GPU tests of the read-only passes over a window of the store share (the class planes, the elevation partition,
the occupancy labels, the rays through the voxel grid): raster parameters, loaded stores, cached frames, an owed transform
noted by hand and the KITTI drop-in on the fake tree.  A plain module: no test, no fixture."""
import os

import numpy as np

import elev_partition_common as ec
from test_gpu_kernels import DYNOBJ, KITTI_FILTERS, SEM_IDXS, dev_store

INTS = (20., 20., 0.5)
BEV_KITTI = dict(type='sem', view_size=30, pixel_size=32, max_trans_radius=0., zoom_thresh=0., do_warp=False,
                 int_scaler=20., int_sep_scaler=20., int_mid_threshold=0.5, height_filter=None)


def params(origin, R, dx, dy, view, px, hf=None, dyn=DYNOBJ):
    """R: a 3x3 rotation, or the angle of one about z."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    R = hl.rotation_matrix_3d(R) if np.ndim(R) == 0 else R
    return make_bev_params(origin, R, dx, dy, view, px, hf, *INTS, 0, dyn, False)


def loaded(frames, capacity=1 << 15, max_frames=8):
    st = dev_store(capacity=capacity, max_frames=max_frames)
    assert st.load_rows(frames) is None
    return st


_frames = {}


def frames_of(seed, random_rows=ec.random_rows):
    """Three frames of 4 000 rows of `random_rows` within +-25 m, made once per seed and never changed."""
    if (random_rows, seed) not in _frames:
        rng = np.random.default_rng(seed)
        _frames[random_rows, seed] = [random_rows(rng, 4000, 25.) for _ in range(3)]
        for f in _frames[random_rows, seed]:
            f.setflags(write=False)
    return _frames[random_rows, seed]


def owe(st, Tm, n_frames):
    """Notes transform Tm as owed by the first n_frames frames of the store (what retransform(defer=True) notes when the
    store holds that many frames)."""
    st._pending.append((np.ascontiguousarray(Tm, dtype=np.float64).reshape(16).copy(), st.head + n_frames))


def kitti_tree(tmp_path, n_frames=10):
    from fake_kitti import SEQ, write_tree

    from datasets.kitti360_utils import get_camera_intrinsics, get_transf_matrices
    root = str(tmp_path / 'KITTI-360')
    if not os.path.isdir(root):
        write_tree(root, first_idx=0, n_frames=n_frames)
    _, h_velo_cam = get_transf_matrices(root)
    p_cam = get_camera_intrinsics(root)
    calib = {'h_velo_cam': h_velo_cam, 'p_cam_frame': p_cam, 'p_velo_frame': np.matmul(p_cam, h_velo_cam)}
    return root, SEQ, calib, np.load(os.path.join(root, 'T_new_prev.npy'))


def kitti_accumulator(tmp_path, bev_params, n_frames=10):
    from kitti360_sem_pc_accum import Kitti360SemanticPointCloudAccumulator
    from obs_dataloaders.kitti360_obs_dataloader import Kitti360Dataloader
    root, seq, calib, Ts = kitti_tree(tmp_path, n_frames)
    acc = Kitti360SemanticPointCloudAccumulator(50., calib, 1e3, 'none', KITTI_FILTERS, SEM_IDXS, True, bev_params)
    it = iter(Ts)
    acc.pose_provider = lambda pc: next(it)
    for observations in Kitti360Dataloader(root, 1, [seq], [0], [n_frames]):
        acc.integrate(observations)
    return acc
