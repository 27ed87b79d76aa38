"""Scenes and refusal tables of the core entry points (tests/test_gpu_core_refusals.py runs them on the device,
tests/test_refusal_coverage.py holds the C ABI to them).  CPU only, numpy only, deterministic.

TABLES[symbol] is the list of that entry point's refused calls: (label, bad, message).  `bad` names what the case changes in the
entry point's one valid call (the caller of the same name in test_gpu_core_refusals.py knows how), `message` is a regular
expression that pca_last_error has to match.  Every case stands next to the host-side check that refuses it, as file:line of
pc-accumulation-lib_amd/csrc/: the check was READ there before the case was written.  A case never reaches a kernel -- the
refusal comes before the call's first device call -- and no case here depends on a device call failing.

The scenes are the smallest with a ragged tail: a store of 4 frames of 96, 1, 0 and 33 points, px = 16, an 8 x 24 image,
two NuScenes cameras, ICP clouds of 300 points."""
import numpy as np

NAN = float('nan')
FRAME_SIZES = (96, 1, 0, 33)
N_POINTS = sum(FRAME_SIZES)
PX, VIEW, SPLIT = 16, 8.0, 2
H, W, NCAM = 8, 24, 2
ICP_N = 300
MAX_CAMS = 8                 # csrc/pca_accum.hip: MAX_CAMS
ICP_MAX_ITER = 32766         # include/pca.h: PCA_ICP_MAX_ITER
KITTI_FILTERS = [10, 11, 12, 16, 18, 255]
NUSC_FILTERS = [3, 70, 130, 199]
DYNOBJ = [13, 14, 15, 17]
INTS = (1., 30., 0.12)
P_CAM = np.array([[8., 0, 12, 0], [0, 8., 4, 0], [0, 0, 1, 0]])      # looks along +z, principal point in the middle of 8 x 24
HW_TOO_LARGE = (32768, 21846)                                        # 32768 * 21846 * 3 = 2 147 549 184 >= 2^31


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def store_frames(seed=77):
    """The store's 4 frames, (n,10) rows inside the 8 m view: f32-representable intensities, every column populated."""
    rng = np.random.default_rng(seed)
    out = []
    for n in FRAME_SIZES:
        r = np.zeros((n, 10))
        r[:, 0:2] = rng.uniform(-3.9, 3.9, (n, 2))
        r[:, 2] = rng.uniform(-1, 2, n)
        r[:, 3] = rng.integers(0, 256, n) / 256.0
        r[:, 4:7] = rng.integers(0, 256, (n, 3))
        r[:, 7] = rng.choice([0, 1, 2, 13], n, p=[0.6, 0.2, 0.15, 0.05])
        r[:, 8] = rng.integers(-1, 4, n)
        r[:, 9] = rng.random(n) < 0.1
        r.setflags(write=False)
        out.append(r)
    return out


def bev_args(px=PX):
    """The arguments of make_bev_params (device and oracle alike) of the one raster every raster case makes."""
    return ((0.25, -0.125, 0.0625), np.eye(3), 0., 0., VIEW, px, None, *INTS, 0, DYNOBJ, False)


def kitti_scene(seed=5):
    """K1: four frames of 96, 1, 0 and 33 points in front of an 8 x 24 camera, about a third of them outside the image."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    sem = rng.integers(0, 19, (H, W)).astype(np.uint8)
    frames = []
    for n in FRAME_SIZES:
        z = rng.uniform(2, 10, n)
        u, v = rng.uniform(-4, W + 4, n), rng.uniform(-2, H + 2, n)
        frames.append(np.stack([(u - 12) / 8 * z, (v - 4) / 8 * z, z, rng.integers(0, 256, n) / 256.0], 1).astype(np.float32).reshape(n, 4))
    return dict(frames=frames, img=img, sem=sem, P=P_CAM)


def nusc_scene(seed=41):
    """K1n: the four frames with two cameras of 8 x 24 pixels, a T per frame, camera indices -1 .. 1 and a few 7 (no camera)."""
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (NCAM, H, W, 3), dtype=np.uint8)
    sems = rng.integers(0, 200, (NCAM, H, W)).astype(np.uint8)
    frames = []
    for k, n in enumerate(FRAME_SIZES):
        pc = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-2, 4, n), rng.integers(0, 256, n).astype(float),
                       rng.uniform(1.01, W - 1.01, n), rng.uniform(1.01, H - 1.01, n), rng.integers(-1, 5, n).astype(float)], 1).reshape(n, 7)
        cam = rng.integers(-1, NCAM, n)
        if n > 8:
            cam[[3, n // 3]] = 7
        a = 0.02 * (k + 1)
        Tw = np.eye(4)
        Tw[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        Tw[:3, 3] = [1.5 * k, -0.3 * k, 0.02 * k]
        frames.append((pc, cam.astype(np.int64), Tw))
    return dict(frames=frames, imgs=imgs, sems=sems)


def k0n_scene(seed=9):
    """K0n: 33 lidar points around two cameras of 24 x 8 pixels that look along +x and -x of the ego frame."""
    rng = np.random.default_rng(seed)
    pc = np.stack([rng.uniform(-20, 20, 33), rng.uniform(-6, 6, 33), rng.uniform(-2, 2, 33)], 1)
    ego_from_lidar = np.eye(4)
    ego_from_lidar[:3, 3] = [0.9, 0.0, 1.8]
    glob_from_ego = np.eye(4)
    glob_from_ego[:2, :2] = [[np.cos(0.3), -np.sin(0.3)], [np.sin(0.3), np.cos(0.3)]]
    glob_from_ego[:3, 3] = [100., -40., 0.5]
    cams = []
    for sign in (1., -1.):
        ego_from_cam = np.eye(4)                             # camera axes: z forward, x right, y down
        ego_from_cam[:3, :3] = np.array([[0, 0, sign], [-sign, 0, 0], [0, -1, 0]], dtype=np.float64)
        ego_from_cam[:3, 3] = [sign * 1.5, 0., 1.6]
        cams.append(np.linalg.inv(glob_from_ego @ ego_from_cam))
    K = np.array([[[8., 0, 12], [0, 8., 4], [0, 0, 1]]] * NCAM)
    wh = np.array([[float(W), float(H)]] * NCAM)
    return dict(pc=pc, ego_from_lidar=ego_from_lidar, glob_from_ego=glob_from_ego, cam_from_glob=np.stack(cams), K=K, wh=wh)


def bilinear_scene(seed=3):
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(1.05, W - 1.05, 33), rng.uniform(1.05, H - 1.05, 33)], 1)
    return dict(map=rng.normal(size=(H, W)), uv=uv)


def hint_tables(visible):
    """then [4][12], box [4][6], now [12] of pca_bev_view_hint for the store's 4 frames: every frame's box is the view itself;
    `visible` = the frames whose `then` is the identity -- the others were created 1000 m away and miss the view."""
    then = np.tile(np.eye(4)[:3].reshape(12), (len(FRAME_SIZES), 1))
    for f in range(len(FRAME_SIZES)):
        if f not in visible:
            then[f, 3] = 1000.0
    box = np.tile(np.array([-4, 4, -4, 4, -1, 2], np.float32), (len(FRAME_SIZES), 1))
    return np.ascontiguousarray(then), np.ascontiguousarray(box), np.ascontiguousarray(np.eye(4)[:3].reshape(12))


def icp_cut(pts, n=ICP_N):
    """A sweep of tests/test_gpu_icp.py cut to n points: the patch 1 m < x < 6 m, 2.5 m < y < 7 m (ground, a parked car, the
    foot of a facade), thinned evenly.  Every 30-neighbourhood of the patch has a radius below 2.3 m and every nearest
    neighbour of the pair lies within 1.8 m (measured on the CPU): inside the device's search caps of 3 m and 4 m."""
    m = (pts[:, 0] > 1) & (pts[:, 0] < 6) & (pts[:, 1] > 2.5) & (pts[:, 1] < 7)
    q = pts[m]
    return np.ascontiguousarray(q[np.linspace(0, len(q) - 1, n).astype(int)])


# ---- the tables -------------------------------------------------------------------------------------------------------------
# (`null_ctx`: the entry point's own `if (!ctx) return -1`; pca_last_error(NULL) then says "null context": csrc/pca_api.hip:358)
K1_ARGS = r'k1: bad arguments'
_K1 = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_k1.hip:495 (_ex; the plain form forwards, :487)
    ('frames NULL', dict(frames=None), K1_ARGS),                                         # pca_k1.hip:349
    ('n_frames 0', dict(n_frames=0), K1_ARGS),                                           # pca_k1.hip:349
    ('store NULL', dict(store=None), K1_ARGS),                                           # pca_k1.hip:349
    ('frame_off NULL', dict(frame_off=None), K1_ARGS),                                   # pca_k1.hip:349
    ('P NULL', dict(P=None), K1_ARGS),                                                   # pca_k1.hip:349
    ('H -1', dict(H=-1), 'k1: H and W must not be negative'),                            # pca_k1.hip:350
    ('W -1', dict(W=-1), 'k1: H and W must not be negative'),                            # pca_k1.hip:350
    ('H = W = -2', dict(H=-2, W=-2), 'k1: H and W must not be negative'),                # pca_k1.hip:350 (H * W * 3 = 12 >= 4 looks plain)
    ('H W 3 >= 2^31', dict(H=HW_TOO_LARGE[0], W=HW_TOO_LARGE[1]), 'k1: image too large'),  # pca_k1.hip:351
    ('a frame with n -1', dict(frame=(3, 'n', -1)), r'k1: bad frame'),                   # pca_k1.hip:354
    ('points without pts', dict(frame=(0, 'pts', None)), r'k1: bad frame'),              # pca_k1.hip:354
    ('no rgb, no sem_gt', dict(frame=(0, 'rgb', None)), 'k1: frame needs rgb\\+sem or sem_gt'),   # pca_k1.hip:355
    ('no sem, no sem_gt', dict(frame=(3, 'sem', None)), 'k1: frame needs rgb\\+sem or sem_gt'),   # pca_k1.hip:355
    ('an image of no pixel', dict(H=0), 'k1: frame needs rgb\\+sem or sem_gt'),          # pca_k1.hip:355
]
_K1_EX = _K1 + [('unknown sample_mode', dict(sample_mode=2), 'k1: unknown sample_mode')]  # pca_k1.hip:348

K1N_ARGS, K1N_STACK = 'k1n: bad arguments', 'k1n: bad image stack'
_K1N = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:246
    ('ncam 0', dict(ncam=0), K1N_STACK),                                                 # pca_accum.hip:237
    ('H 0', dict(H=0), K1N_STACK),                                                       # pca_accum.hip:237
    ('W 0', dict(W=0), K1N_STACK),                                                       # pca_accum.hip:237
    ('a stack of 3 bytes', dict(ncam=1, H=1, W=1), K1N_STACK),                           # pca_accum.hip:237
    ('n -1', dict(n=-1), K1N_ARGS),                                                      # pca_accum.hip:249
    ('pc NULL', dict(pc=None), K1N_ARGS),                                                # pca_accum.hip:249
    ('cam_idx NULL', dict(cam_idx=None), K1N_ARGS),                                      # pca_accum.hip:249
    ('imgs NULL', dict(imgs=None), K1N_ARGS),                                            # pca_accum.hip:249
    ('sems NULL', dict(sems=None), K1N_ARGS),                                            # pca_accum.hip:249
    ('store NULL', dict(store=None), K1N_ARGS),                                          # pca_accum.hip:249
    ('frame_off NULL', dict(frame_off=None), K1N_ARGS),                                  # pca_accum.hip:249
    ('T NULL', dict(T=None), 'k1n: T must not be NULL'),                                 # pca_accum.hip:250 (added: T is read on the host)
]
_K1N_EX = _K1N + [('unknown sample_mode', dict(sample_mode=5), 'k1n: unknown sample_mode')]   # pca_accum.hip:236
K1N_FRAME = r'k1n: bad frame \(points, camera indices, image and class stacks, T\)'
_K1N_BATCH = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:539
    ('unknown sample_mode', dict(sample_mode=-1), 'k1n: unknown sample_mode'),           # pca_accum.hip:236
    ('ncam 0', dict(ncam=0), K1N_STACK),                                                 # pca_accum.hip:237
    ('H -3', dict(H=-3), K1N_STACK),                                                     # pca_accum.hip:237
    ('frames NULL', dict(frames=None), K1N_ARGS),                                        # pca_accum.hip:542
    ('n_frames 0', dict(n_frames=0), K1N_ARGS),                                          # pca_accum.hip:542
    ('store NULL', dict(store=None), K1N_ARGS),                                          # pca_accum.hip:542
    ('frame_off NULL', dict(frame_off=None), K1N_ARGS),                                  # pca_accum.hip:542
    ('a frame with n -1', dict(frame=(1, 'n', -1)), K1N_FRAME),                          # pca_accum.hip:473
    ('points without pc', dict(frame=(0, 'pc', None)), K1N_FRAME),                       # pca_accum.hip:473
    ('points without cam_idx', dict(frame=(3, 'cam_idx', None)), K1N_FRAME),             # pca_accum.hip:473
    ('the EMPTY frame without imgs', dict(frame=(2, 'imgs', None)), K1N_FRAME),          # pca_accum.hip:473
    ('a frame without sems', dict(frame=(1, 'sems', None)), K1N_FRAME),                  # pca_accum.hip:473
    ('a frame without T', dict(frame=(3, 'T', None)), K1N_FRAME),                        # pca_accum.hip:473
    # (16384 tiles in frame 0 alone, three more behind it: counted on the host from `n`, pca_accum.hip:466-480, before the
    # call's first device call at :546 -- no pointer of the frame is followed)
    ('more than 16384 tiles', dict(frame=(0, 'n', 16384 * 512)), r'k1n: batch too large \(split it: at most 16384 tiles of 512 points\)'),   # pca_accum.hip:477
]

_K0N = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:647
    ('ncam -1', dict(ncam=-1), 'k0n: ncam out of range'),                                # pca_accum.hip:648
    ('ncam MAX_CAMS + 1', dict(ncam=MAX_CAMS + 1), 'k0n: ncam out of range'),            # pca_accum.hip:648
    # (:651 and :652 were added for this table: the matrices are read on the host right behind them)
    ('pc_lidar NULL', dict(pc=None), 'k0n: bad arguments'),                              # pca_accum.hip:651
    ('T_ego_from_lidar NULL', dict(ego_from_lidar=None), 'k0n: bad arguments'),          # pca_accum.hip:651
    ('T_glob_from_ego NULL', dict(glob_from_ego=None), 'k0n: bad arguments'),            # pca_accum.hip:651
    ('pc_in_ego NULL', dict(out_ego=None), 'k0n: bad arguments'),                        # pca_accum.hip:651
    ('uv NULL', dict(out_uv=None), 'k0n: bad arguments'),                                # pca_accum.hip:651
    ('cam_idx NULL', dict(out_cam=None), 'k0n: bad arguments'),                          # pca_accum.hip:651
    ('T_cam_from_glob NULL', dict(cam_from_glob=None), 'k0n: cameras without T_cam_from_glob, K or wh'),   # pca_accum.hip:652
    ('K NULL', dict(K=None), 'k0n: cameras without T_cam_from_glob, K or wh'),           # pca_accum.hip:652
    ('wh NULL', dict(wh=None), 'k0n: cameras without T_cam_from_glob, K or wh'),         # pca_accum.hip:652
]

_BILINEAR = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:585
    ('n -1', dict(n=-1), 'bilinear: bad arguments'),                                     # pca_accum.hip:586
    ('map NULL', dict(map=None), 'bilinear: bad arguments'),                             # pca_accum.hip:586
    ('uv NULL', dict(uv=None), 'bilinear: bad arguments'),                               # pca_accum.hip:586
    ('out NULL', dict(out=None), 'bilinear: bad arguments'),                             # pca_accum.hip:586
    ('H 0', dict(H=0), 'bilinear: bad arguments'),                                       # pca_accum.hip:586
    ('W 0', dict(W=0), 'bilinear: bad arguments'),                                       # pca_accum.hip:586
]

_NCHW = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:815
    ('rgb NULL', dict(rgb=None), 'normalise: bad arguments'),                            # pca_accum.hip:816
    ('out NULL', dict(out=None), 'normalise: bad arguments'),                            # pca_accum.hip:816
    ('mean NULL', dict(mean=None), 'normalise: bad arguments'),                          # pca_accum.hip:816
    ('std NULL', dict(std=None), 'normalise: bad arguments'),                            # pca_accum.hip:816
    ('H 0', dict(H=0), 'normalise: bad arguments'),                                      # pca_accum.hip:816
    ('W -1', dict(W=-1), 'normalise: bad arguments'),                                    # pca_accum.hip:816
]

_K2 = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:752
    ('store NULL', dict(store=None), 'k2: bad arguments'),                               # pca_accum.hip:754
    ('frame_off NULL', dict(frame_off=None), 'k2: bad arguments'),                       # pca_accum.hip:754
    ('Ts NULL', dict(Ts=None), 'k2: bad arguments'),                                     # pca_accum.hip:754
    ('n_T -1', dict(n_T=-1), 'k2: bad arguments'),                                       # pca_accum.hip:754
    ('slot_end < slot_begin', dict(slot_begin=3, slot_end=2), 'k2: bad arguments'),      # pca_accum.hip:754
    ('n_T 65536', dict(n_T=65536), 'k2: at most 65535 transforms per call'),             # pca_accum.hip:755 (added: no bound before)
]
_K2_TAIL = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:773
    ('store NULL', dict(store=None), 'k2 tail: bad arguments'),                          # pca_accum.hip:775
    ('frame_off NULL', dict(frame_off=None), 'k2 tail: bad arguments'),                  # pca_accum.hip:775
    ('Ts NULL', dict(Ts=None), 'k2 tail: bad arguments'),                                # pca_accum.hip:775
    ('n_frames -1', dict(n_frames=-1), 'k2 tail: bad arguments'),                        # pca_accum.hip:775
    ('n_frames 65536', dict(n_frames=65536), 'k2 tail: bad arguments'),                  # pca_accum.hip:775
]
_K3 = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:854
    ('store NULL', dict(store=None), 'k3: bad arguments'),                               # pca_accum.hip:856
    ('frame_off NULL', dict(frame_off=None), 'k3: bad arguments'),                       # pca_accum.hip:856
    ('n_pairs -1', dict(n_pairs=-1), 'k3: bad arguments'),                               # pca_accum.hip:856
    ('pairs without slots', dict(slots=None), 'k3: bad arguments'),                      # pca_accum.hip:856
    ('pairs without inst_idx', dict(inst_idx=None), 'k3: bad arguments'),                # pca_accum.hip:856
]
_DEDUP = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_accum.hip:1040
    ('store NULL', dict(store=None), 'dedup: bad arguments'),                            # pca_accum.hip:1042
    ('frame_off NULL', dict(frame_off=None), 'dedup: bad arguments'),                    # pca_accum.hip:1042
    ('workspace NULL', dict(workspace=None), 'dedup: bad arguments'),                    # pca_accum.hip:1042
    ('slot_end < slot_begin', dict(slot_begin=2, slot_end=1), 'dedup: bad arguments'),   # pca_accum.hip:1042
    ('voxel_size 0', dict(voxel_size=0.0), 'dedup: voxel_size must be positive'),        # pca_accum.hip:1043
    ('voxel_size negative', dict(voxel_size=-0.5), 'dedup: voxel_size must be positive'),   # pca_accum.hip:1043
    ('voxel_size NaN', dict(voxel_size=NAN), 'dedup: voxel_size must be positive'),      # pca_accum.hip:1043
    ('max_points 2^31', dict(max_points=1 << 31), 'dedup: window too large'),            # pca_accum.hip:1046
    ('a workspace of need - 1 bytes', dict(short=1), 'dedup: workspace too small'),      # pca_accum.hip:1048
]

BEV_ARGS, BEV_PX = 'bev: bad arguments', r'bev: px must be in 1\.\.4096'
BEV_R = r'bev: R must be a rotation about the z axis'
BEV_SLOTS = 'bev: need slot_begin <= slot_split <= slot_end'
_BEV_PREPARE = [                                             # (bev_prepare: what every raster, and every job of _many, goes through)
    ('store NULL', dict(store=None), BEV_ARGS),                                          # pca_bev.hip:1707
    ('frame_off NULL', dict(frame_off=None), BEV_ARGS),                                  # pca_bev.hip:1707
    ('workspace NULL', dict(workspace=None), BEV_ARGS),                                  # pca_bev.hip:1707
    ('neither planes nor planes_f16', dict(planes=None, planes_f16=None), BEV_ARGS),     # pca_bev.hip:1707
    ('px 0', dict(px=0), BEV_PX),                                                        # pca_bev.hip:1708 (PX_CHECK, :1599)
    ('px 4097', dict(px=4097), BEV_PX),                                                  # pca_bev.hip:1708
    ('R tilts z', dict(R=(8, 0.5)), BEV_R),                                              # pca_bev_view.h:122-123
    ('R mixes z into x', dict(R=(2, 0.125)), BEV_R),                                     # pca_bev_view.h:122-123
    ('slot_begin > slot_split', dict(slot_begin=3, slot_split=2), BEV_SLOTS),            # pca_bev.hip:1710
    ('slot_split > slot_end', dict(slot_split=5), BEV_SLOTS),                            # pca_bev.hip:1710
    ('max_points 2^32', dict(max_points=1 << 32), 'bev: window too large for 32-bit positions'),   # pca_bev.hip:1711
    ('a workspace of need - 1 bytes', dict(short=1), 'bev: workspace too small'),        # pca_bev.hip:1713
]
_BEV_ONE = [('ctx NULL', dict(null_ctx=True), 'null context'),                           # pca_bev.hip:1891
            ('prm NULL', dict(prm=None), BEV_ARGS)] + _BEV_PREPARE                        # pca_bev.hip:1707
_BEV_EX = _BEV_ONE + [
    ('an owed transform beyond the window', dict(pending_T=True, pending_slot_end=5), 'bev: a pending slot end lies beyond the window'),   # pca_bev_view.h:141
]
BEV_CHAIN = 'bev: bad chain of owed transforms'
_BEV_CHAIN = _BEV_ONE + [
    ('n_pending -1', dict(n_pending=-1), BEV_CHAIN),                                     # pca_bev_view.h:131
    ('n_pending PCA_BEV_MAX_CHAIN + 1', dict(n_pending=5), BEV_CHAIN),                   # pca_bev_view.h:131
    ('a chain without pending_Ts', dict(n_pending=2, pending_Ts=None), BEV_CHAIN),       # pca_bev_view.h:131
    ('a chain without pending_slot_ends', dict(n_pending=2, pending_slot_ends=None), BEV_CHAIN),   # pca_bev_view.h:131
    ('a pending slot end beyond the window', dict(n_pending=2, ends=(2, 5)), 'bev: a pending slot end lies beyond the window'),   # pca_bev_view.h:141
    ('pending slot ends that descend', dict(n_pending=2, ends=(3, 2)), 'bev: pending slot ends must ascend'),   # pca_bev_view.h:142
]
_BEV_MANY = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_bev.hip:1937
    ('jobs NULL', dict(jobs=None), 'bev: bad job list'),                                 # pca_bev.hip:1940
    ('n_jobs 0', dict(n_jobs=0), 'bev: bad job list'),                                   # pca_bev.hip:1940
    ('n_jobs 65536', dict(n_jobs=65536), 'bev: at most 65535 rasters per call'),         # pca_bev.hip:1941 (before jobs[0] is read, :1945)
    ('the first job with px 0', dict(job=(0, 'px', 0)), BEV_PX),                         # pca_bev.hip:1946
    ('the first job with px 4097', dict(job=(0, 'px', 4097)), BEV_PX),                   # pca_bev.hip:1946
    ('a workspace one byte short of n_jobs slices', dict(short=1), 'bev: workspace too small for this many rasters'),   # pca_bev.hip:1949
    ('jobs with different px', dict(job=(1, 'px', 32)), 'bev: the rasters of one call share the grid size'),   # pca_bev.hip:1968
    ('store NULL', dict(store=None), BEV_ARGS),                                          # pca_bev.hip:1707 (through :1969)
    ('frame_off NULL', dict(frame_off=None), BEV_ARGS),                                  # pca_bev.hip:1707
    ('a job without planes', dict(job=(1, 'planes', None)), BEV_ARGS),                   # pca_bev.hip:1707
    ('a job whose R tilts z', dict(job=(1, 'R', (8, 0.5))), BEV_R),                      # pca_bev_view.h:122-123
    ('a job with slot_begin > slot_split', dict(job=(1, 'slot_begin', 3)), BEV_SLOTS),   # pca_bev.hip:1710
    ('a job with slot_split > slot_end', dict(job=(0, 'slot_end', 1)), BEV_SLOTS),       # pca_bev.hip:1710
    ('max_points 2^32', dict(max_points=1 << 32), 'bev: window too large for 32-bit positions'),   # pca_bev.hip:1711 (the workspace check before it, :1949, is given 2^62 bytes: a number, never followed)
]
_WARP = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_bev.hip:2050
    ('planes_f16 NULL', dict(planes=None), 'warp: bad arguments'),                       # pca_bev.hip:2051
    ('out_f16 NULL', dict(out=None), 'warp: bad arguments'),                             # pca_bev.hip:2051
    ('planes_f16 == out_f16', dict(same=True), 'warp: bad arguments'),                   # pca_bev.hip:2051
    ('n_planes 0', dict(n_planes=0), 'warp: bad arguments'),                             # pca_bev.hip:2051
    ('px 0', dict(px=0), 'warp: bad arguments'),                                         # pca_bev.hip:2051
    ('px 65536', dict(px=65536), 'warp: bad arguments'),                                 # pca_bev.hip:2051
    ('a_1 NaN', dict(coef=(0, NAN)), 'warp: NaN coefficient'),                           # pca_bev.hip:2052
    ('a_2 NaN', dict(coef=(1, NAN)), 'warp: NaN coefficient'),                           # pca_bev.hip:2052
    ('b_1 NaN', dict(coef=(2, NAN)), 'warp: NaN coefficient'),                           # pca_bev.hip:2052
    ('b_2 NaN', dict(coef=(3, NAN)), 'warp: NaN coefficient'),                           # pca_bev.hip:2052
]

KI_ARGS = 'kitti_integrate: bad arguments'
KI_TRACK = 'kitti_integrate: the pose track needs T_new_prev and its outputs'
_INTEGRATE = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_session.hip:24
    ('obs NULL', dict(obs=None), KI_ARGS),                                               # pca_session.hip:25
    ('obs.n -1', dict(n=-1), KI_ARGS),                                                   # pca_session.hip:25
    ('P NULL', dict(P=None), KI_ARGS),                                                   # pca_session.hip:25
    ('filter_mask NULL', dict(filter_mask=None), KI_ARGS),                               # pca_session.hip:25
    ('store NULL', dict(store=None), KI_ARGS),                                           # pca_session.hip:25
    ('frame_off NULL', dict(frame_off=None), KI_ARGS),                                   # pca_session.hip:25
    ('a track without T_new_prev', dict(T_new_prev=None), KI_TRACK),                     # pca_session.hip:26
    # K1's own checks, run by pca_k1_check_frames before anything is staged, noted or stepped (pca_session.hip:33):
    ('unknown sample_mode', dict(sample_mode=3), 'k1: unknown sample_mode'),             # pca_k1.hip:348
    ('points without pts', dict(pts=None), r'k1: bad frame'),                            # pca_k1.hip:354
    ('H -1', dict(H=-1), 'k1: H and W must not be negative'),                            # pca_k1.hip:350
    ('W -1', dict(W=-1), 'k1: H and W must not be negative'),                            # pca_k1.hip:350
    ('H W 3 >= 2^31', dict(H=HW_TOO_LARGE[0], W=HW_TOO_LARGE[1]), 'k1: image too large'),   # pca_k1.hip:351
    ('no rgb, no sem_gt', dict(rgb=None), 'k1: frame needs rgb\\+sem or sem_gt'),        # pca_k1.hip:355
    ('no sem, no sem_gt', dict(sem=None), 'k1: frame needs rgb\\+sem or sem_gt'),        # pca_k1.hip:355
]
_INTEGRATE_PLAIN = _INTEGRATE + [
    ('a track without evicted', dict(evicted=None), KI_TRACK),                           # pca_session.hip:26
    ('a track without path_length', dict(path_length=None), KI_TRACK),                   # pca_session.hip:26
]
_INTEGRATE_V = _INTEGRATE + [('no argument block', dict(block=None), 'kitti_integrate_v: no argument block')]   # pca_session.hip:170

KG_ARGS = r'kitti_generate_bev: bad arguments \(prm, planes_f16, track, traj_rows, traj_start and n_rows are needed\)'
_GENERATE = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_session.hip:136
    ('prm NULL', dict(prm=None), KG_ARGS),                                               # pca_session.hip:139-141
    ('planes_f16 NULL', dict(planes_f16=None), KG_ARGS),                                 # pca_session.hip:139-141
    ('track NULL', dict(track=None), KG_ARGS),                                           # pca_session.hip:139-141
    ('traj_rows NULL', dict(traj_rows=None), KG_ARGS),                                   # pca_session.hip:139-141
    ('traj_start NULL', dict(traj_start=None), KG_ARGS),                                 # pca_session.hip:139-141
    ('a window one frame longer than the track', dict(slot_begin=-1),
     'kitti_generate_bev: the pose track and the window disagree about the number of frames'),   # pca_session.hip:145-147
    # the raster's own refusals, through pca_bev_generate_chain (:150): nothing of the call's outputs is written
    ('store NULL', dict(store=None), BEV_ARGS),                                          # pca_bev.hip:1707
    ('workspace NULL', dict(workspace=None), BEV_ARGS),                                  # pca_bev.hip:1707
    ('px 0', dict(px=0), BEV_PX),                                                        # pca_bev.hip:1708
    ('R tilts z', dict(R=(8, 0.5)), BEV_R),                                              # pca_bev_view.h:122-123
    ('slot_split > slot_end', dict(slot_split=5), BEV_SLOTS),                            # pca_bev.hip:1710
    ('a workspace of need - 1 bytes', dict(short=1), 'bev: workspace too small'),        # pca_bev.hip:1713
    ('n_pending 5', dict(n_pending=5), BEV_CHAIN),                                       # pca_bev_view.h:131
]
_GENERATE_PLAIN = _GENERATE + [('n_rows NULL', dict(n_rows=None), KG_ARGS)]              # pca_session.hip:139-141
# (with prm NULL the _v form does not get that far: its hint, which reads prm, refuses first -- pca_session.hip:182, pca_api.hip:204)
_GENERATE_V = [c if c[0] != 'prm NULL' else ('prm NULL', dict(prm=None), 'kitti_generate_bev_v: bad view hint') for c in _GENERATE] + [
    ('no argument block', dict(block=None), 'kitti_generate_bev_v: no argument block'),  # pca_session.hip:178
    ('a hint without `then`', dict(hint_then=None), 'kitti_generate_bev_v: bad view hint'),   # pca_session.hip:182 (pca_api.hip:133)
    ('a hint without `now`', dict(hint_now=None), 'kitti_generate_bev_v: bad view hint'),     # pca_session.hip:182
]

HINT = r'view_hint: bad arguments \(F >= 0; then, now and prm are needed\)'
_VIEW_HINT = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_api.hip:201
    ('F -1', dict(F=-1), HINT),                                                          # pca_api.hip:204 (pca_host_view_hull, :133)
    ('then NULL', dict(then=None), HINT),                                                # pca_api.hip:204
    ('now NULL', dict(now=None), HINT),                                                  # pca_api.hip:204
    ('prm NULL', dict(prm=None), HINT),                                                  # pca_api.hip:204
]
_BIN_RANGE = [('ctx NULL', dict(null_ctx=True), 'null context')]                         # pca_api.hip:213: its only refusal (end < first arms nothing and returns 0)

# The three calls that run a K1 noted by pca_k1_defer (their valid call: a noted frame, run by them, equals the oracle)
_K1_DEFER = [('ctx NULL', dict(null_ctx=True), 'null context')]                          # pca_k1.hip:477
_K1_FLUSH = [('ctx NULL', dict(null_ctx=True), 'null context')]                          # pca_k1.hip:481
_STATUS = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_api.hip:362
    ('status_out NULL', dict(status_out=None), 'status: status_out must not be NULL'),   # pca_api.hip:363 (before the noted K1 is run, :364)
]

_D2H_ASYNC = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_host.hip:462
    ('dev NULL', dict(dev=None), 'd2h_async: bad arguments'),                            # pca_host.hip:463
    ('pinned NULL', dict(pinned=None), 'd2h_async: bad arguments'),                      # pca_host.hip:463
    ('bytes -1', dict(bytes=-1), 'd2h_async: bad arguments'),                            # pca_host.hip:463
]
_D2H_WAIT = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_host.hip:473
    ('ticket -1', dict(ticket=-1), 'd2h_wait: bad ticket'),                              # pca_host.hip:474
    ('ticket 64', dict(ticket=64), 'd2h_wait: bad ticket'),                              # pca_host.hip:474
    ('a ticket that was never given out', dict(ticket=9), 'd2h_wait: bad ticket'),       # pca_host.hip:474 (a private context: its first copy is ticket 0)
]

# The output writer's kernels (the device codec and the preview sheets): one host-side check each.
DEFLATE_MAX_CHUNKS = 1 << 20                                                             # include/pca.h: PCA_DEFLATE_MAX_CHUNKS
DF = 'deflate_chunks: bad arguments'
_DEFLATE = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_deflate.hip:816 (df_launch: both forms)
    ('n_chunks -1', dict(n_chunks=-1), DF),                                              # pca_deflate.hip:817
    ('n_chunks above the limit', dict(n_chunks=DEFLATE_MAX_CHUNKS + 1), DF),             # pca_deflate.hip:817
    ('src NULL', dict(src=None), DF),                                                    # pca_deflate.hip:817
    ('chunk_table NULL', dict(table=None), DF),                                          # pca_deflate.hip:817
    ('out NULL', dict(out=None), DF),                                                    # pca_deflate.hip:817
    ('out_sizes NULL', dict(sizes=None), DF),                                            # pca_deflate.hip:817
    ('out_crcs NULL', dict(crcs=None), DF),                                              # pca_deflate.hip:817
    ('workspace NULL', dict(workspace=None), DF),                                        # pca_deflate.hip:817
]
AD = 'adler32_chunks: bad arguments'
_ADLER = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_preview.hip:330
    ('n_chunks -1', dict(n_chunks=-1), AD),                                              # pca_preview.hip:331
    ('n_chunks above the limit', dict(n_chunks=DEFLATE_MAX_CHUNKS + 1), AD),             # pca_preview.hip:331
    ('src NULL', dict(src=None), AD),                                                    # pca_preview.hip:331
    ('chunk_table NULL', dict(table=None), AD),                                          # pca_preview.hip:331
    ('out NULL', dict(out=None), AD),                                                    # pca_preview.hip:331
]
PV = 'preview_sheets: bad arguments'
_PREVIEW = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_preview.hip:297
    ('k -1', dict(k=-1), PV),                                                            # pca_preview.hip:298
    ('px 0', dict(px=0), PV),                                                            # pca_preview.hip:298
    ('px 4097', dict(px=4097), PV),                                                      # pca_preview.hip:298
    ('filter -1', dict(filter=-1), PV),                                                  # pca_preview.hip:298
    ('filter 3', dict(filter=3), PV),                                                    # pca_preview.hip:298
    ('n_polylines -1', dict(n_polylines=-1), PV),                                        # pca_preview.hip:298
    ('n_verts -1', dict(n_verts=-1), PV),                                                # pca_preview.hip:298
    ('ranges NULL', dict(ranges=None), PV),                                              # pca_preview.hip:298
    ('k 3 px beyond int32', dict(k=1 << 27), PV),                                        # pca_preview.hip:299
    ('planes NULL', dict(planes=None), PV),                                              # pca_preview.hip:299
    ('lut NULL', dict(lut=None), PV),                                                    # pca_preview.hip:299
    ('out_stream NULL', dict(out=None), PV),                                             # pca_preview.hip:299
    ('workspace NULL', dict(workspace=None), PV),                                        # pca_preview.hip:299
    ('polylines NULL', dict(polylines=None), PV),                                        # pca_preview.hip:300
    ('vertices NULL', dict(verts=None), PV),                                             # pca_preview.hip:300
]

_ICP = [
    ('ctx NULL', dict(null_ctx=True), 'null context'),                                   # pca_icp.hip:1295
    ('src_pts NULL', dict(src=None), 'icp: bad arguments'),                              # pca_icp.hip:1296
    ('tgt_pts NULL', dict(tgt=None), 'icp: bad arguments'),                              # pca_icp.hip:1296
    ('n_src 0', dict(n_src=0), 'icp: bad arguments'),                                    # pca_icp.hip:1296
    ('n_tgt -1', dict(n_tgt=-1), 'icp: bad arguments'),                                  # pca_icp.hip:1296
    ('workspace NULL', dict(workspace=None), 'icp: bad arguments'),                      # pca_icp.hip:1296
    ('T_out NULL', dict(T_out=None), 'icp: bad arguments'),                              # pca_icp.hip:1296
    ('a workspace of need - 1 bytes', dict(short=1), 'icp: workspace too small'),        # pca_icp.hip:1297
    ('max_iter one above the limit', dict(max_iter=ICP_MAX_ITER + 1), 'icp: max_iter must not exceed 32766'),   # pca_icp.hip:1299
]

TABLES = {
    'pca_kitti_project_sample_filter': _K1,
    'pca_kitti_project_sample_filter_ex': _K1_EX,
    'pca_nusc_sample_filter_transform': _K1N,
    'pca_nusc_sample_filter_transform_ex': _K1N_EX,
    'pca_nusc_sample_filter_transform_batch': _K1N_BATCH,
    'pca_nusc_project_cams': _K0N,
    'pca_sample_bilinear': _BILINEAR,
    'pca_image_to_nchw_f32': _NCHW,
    'pca_retransform': _K2,
    'pca_retransform_batch_tail': _K2_TAIL,
    'pca_mark_dynamic': _K3,
    'pca_voxel_dedup': _DEDUP,
    'pca_bev_generate': _BEV_ONE,
    'pca_bev_generate_ex': _BEV_EX,
    'pca_bev_generate_chain': _BEV_CHAIN,
    'pca_bev_generate_many': _BEV_MANY,
    'pca_bev_warp': _WARP,
    'pca_kitti_integrate': _INTEGRATE_PLAIN,
    'pca_kitti_integrate_v': _INTEGRATE_V,
    'pca_kitti_generate_bev': _GENERATE_PLAIN,
    'pca_kitti_generate_bev_v': _GENERATE_V,
    'pca_bev_view_hint': _VIEW_HINT,
    'pca_bev_bin_range': _BIN_RANGE,
    'pca_host_d2h_async': _D2H_ASYNC,
    'pca_host_d2h_wait': _D2H_WAIT,
    'pca_icp_register': _ICP,
    'pca_k1_defer': _K1_DEFER,
    'pca_k1_flush': _K1_FLUSH,
    'pca_status': _STATUS,
    'pca_deflate_chunks': _DEFLATE,
    'pca_deflate_chunks_dyn': _DEFLATE,
    'pca_adler32_chunks': _ADLER,
    'pca_preview_sheets': _PREVIEW,
}

# The ctx->err sites of those entry points' sources that NO case reaches, and why (4 of 62 sites):
UNREACHED = {
    'pca_k1.hip:278': '"k1: batch too large": needs more than 65535 frames per queue of a SPLIT call; the call has grown the '
                      'context\'s device blocks for that many descriptors by then (k1_stage_descriptors)',
    'pca_k1.hip:415': '"k1: frame too large": more than 2^28 tiles of 512 points in one frame -- no int32 n gets there',
    'pca_bev.hip:1880': '"bev: no heavy kernel for a split banded raster": an invariant of the host\'s own decisions '
                        '(bev_decide_split never splits a banded raster), no argument reaches it',
    'pca_session.hip:114': 'behind a failing hipEventRecord',
}
