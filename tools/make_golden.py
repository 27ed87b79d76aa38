#!/usr/bin/env python3
"""Generate golden input/output vectors by running the REAL reference.

Test infrastructure only.  Runs in the build container (needs the read-only
reference checkout at /root/reference); never runs on the GPU box.  Nothing of
the reference is copied: the reference modules are imported from where they
lie, executed on small seeded synthetic inputs, and only the numeric inputs and
outputs are written to ``tests/golden/*.npz``.

Third-party modules the reference imports at module level but that are absent
from this image (open3d, onnxruntime, torchvision, nuscenes-devkit,
pyquaternion) are replaced by empty ``types.ModuleType`` stubs; the only
behaviour injected is
  * a fake semseg model  ``pred(rgb) -> (1,1,H,W)``  (see ``fake_semseg``),
  * a fake ICP result carrying the pose we inject,
  * ``view_points`` implementing the documented nuscenes-devkit formula
    (viewpad @ [p;1], normalise by row 2) -- parity at that boundary is
    "unpinned" (SURVEY.md 8c), the stub pins our own restatement only.

Usage:  python tools/make_golden.py [--out tests/golden]
"""
import argparse
import os
import random
import sys
import types

import numpy as np

REF = '/root/reference'


# --------------------------------------------------------------------------
#  reference import with stubs
# --------------------------------------------------------------------------
class _FakeICPResult:
    def __init__(self, T):
        self.transformation = T


class _FakePointCloud:
    def __init__(self):
        self.points = None

    def estimate_normals(self):
        pass


_icp_queue = []


def _fake_registration_icp(target, source, thr, init, est):
    return _FakeICPResult(_icp_queue.pop(0))


def view_points_stub(points, view, normalize):
    """Documented behaviour of nuscenes.utils.geometry_utils.view_points."""
    viewpad = np.eye(4)
    viewpad[:view.shape[0], :view.shape[1]] = view
    nbr_points = points.shape[1]
    points = np.concatenate((points, np.ones((1, nbr_points))))
    points = np.dot(viewpad, points)
    points = points[:3, :]
    if normalize:
        points = points / points[2:3, :].repeat(3, 0).reshape(3, nbr_points)
    return points


def import_reference():
    assert os.path.isdir(REF), 'reference checkout not present'
    sys.dont_write_bytecode = True
    names = [
        'open3d', 'onnxruntime', 'torchvision', 'torchvision.transforms',
        'nuscenes', 'nuscenes.nuscenes', 'nuscenes.utils',
        'nuscenes.utils.data_classes', 'nuscenes.utils.geometry_utils',
        'nuscenes.map_expansion', 'nuscenes.map_expansion.map_api',
        'pyquaternion'
    ]
    for name in names:
        sys.modules[name] = types.ModuleType(name)
    sys.modules['nuscenes.nuscenes'].NuScenes = object
    sys.modules['nuscenes.utils.data_classes'].LidarPointCloud = object
    sys.modules['nuscenes.utils.geometry_utils'].transform_matrix = None
    sys.modules['nuscenes.utils.geometry_utils'].view_points = view_points_stub
    sys.modules['nuscenes.map_expansion.map_api'].NuScenesMap = object
    sys.modules['pyquaternion'].Quaternion = object
    o3d = sys.modules['open3d']
    o3d.geometry = types.SimpleNamespace(PointCloud=_FakePointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: a)
    o3d.pipelines = types.SimpleNamespace(registration=types.SimpleNamespace(
        registration_icp=_fake_registration_icp,
        TransformationEstimationPointToPlane=lambda: None))
    ds = types.ModuleType('datasets')
    ds.__path__ = [os.path.join(REF, 'datasets')]
    sys.modules['datasets'] = ds
    sys.path.insert(0, REF)
    import sem_pc_accum  # noqa
    import kitti360_sem_pc_accum  # noqa
    import nuscenes_oracle_sem_pc_accum  # noqa
    import datasets.nuscenes_utils as nu  # noqa
    from bev_generator.sem_bev import SemBEVGenerator  # noqa
    from bev_generator.rgb_bev import RGBBEVGenerator  # noqa
    return types.SimpleNamespace(
        sem_pc_accum=sem_pc_accum,
        kitti=kitti360_sem_pc_accum,
        oracle=nuscenes_oracle_sem_pc_accum,
        nu=nu,
        SemBEVGenerator=SemBEVGenerator,
        RGBBEVGenerator=RGBBEVGenerator)


# --------------------------------------------------------------------------
#  synthetic inputs (shared with the tests through the stored arrays)
# --------------------------------------------------------------------------
CAM_TO_VELO = np.array(
    [[0.04307104361, -0.08829286498, 0.995162929, 0.8043914418],
     [-0.999004371, 0.007784614041, 0.04392796942, 0.2993489574],
     [-0.01162548558, -0.9960641394, -0.08786966659, -0.1770225824],
     [0, 0, 0, 1]])


def small_calib(H, W, f):
    p_cam = np.array([[f, 0, W / 2 + 0.049453, 0], [0, f, H / 2 - 0.230451, 0],
                      [0, 0, 1, 0]], dtype=float)
    h_velo_cam = np.linalg.inv(CAM_TO_VELO)
    return {
        'h_velo_cam': h_velo_cam,
        'p_cam_frame': p_cam,
        'p_velo_frame': np.matmul(p_cam, h_velo_cam)
    }


def fake_semseg(rgb):
    """Deterministic stand-in for SemSegONNX.pred: (1,1,H,W) int64, 0..18."""
    a = np.asarray(rgb).astype(np.int64)
    sem = (a[..., 0] + 2 * a[..., 1] + 3 * a[..., 2]) % 19
    return sem[None, None]


class FakeSemSeg:
    def pred(self, rgb):
        return fake_semseg(rgb)


def rigid(rx, ry, rz, tx, ty, tz):
    cx, sx = np.cos(rx), np.sin(rx)
    cy, sy = np.cos(ry), np.sin(ry)
    cz, sz = np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [tx, ty, tz]
    return T


def kitti_frame(rng, N, H, W, lim=30.0):
    from PIL import Image
    pc = np.stack([
        rng.uniform(-lim, lim, N),
        rng.uniform(-lim, lim, N),
        rng.uniform(-2, 3, N),
        rng.uniform(0, 1, N)
    ], 1).astype(np.float32)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return pc, Image.fromarray(img), img


BEV_PARAMS_KITTI = dict(type='sem', view_size=40, pixel_size=32,
                        max_trans_radius=0., zoom_thresh=0., do_warp=False,
                        int_scaler=20., int_sep_scaler=20.,
                        int_mid_threshold=0.5, height_filter=None)
BEV_PARAMS_NUSC = dict(type='sem', view_size=30, pixel_size=32,
                       max_trans_radius=0., zoom_thresh=0., do_warp=False,
                       int_scaler=1., int_sep_scaler=30.,
                       int_mid_threshold=0.12, height_filter=3.)
SEM_IDXS = {'road': 0, 'car': 13, 'truck': 14, 'bus': 15, 'motorcycle': 17}
KITTI_FILTERS = [10, 11, 12, 16, 18, 255]
NUSC_FILTERS = [10, 11, 12, 16, 18]


def flat_bev(prefix, bev, out):
    """Flatten a reference BEV dict into npz entries."""
    for k, v in bev.items():
        if k.startswith('trajs_') or k == 'gt_lanes':
            out[f'{prefix}{k}_n'] = np.array(len(v))
            for i, t in enumerate(v):
                out[f'{prefix}{k}_{i}'] = np.asarray(t, dtype=float)
        else:
            out[f'{prefix}{k}'] = np.asarray(v)


# --------------------------------------------------------------------------
#  case generators
# --------------------------------------------------------------------------
def case_k1(ref, out_dir):
    """velo2img / gen_semantic_pc / filter on one frame incl. edge cases."""
    rng = np.random.default_rng(101)
    H, W = 64, 96
    calib = small_calib(H, W, 40.0)
    acc = ref.kitti.Kitti360SemanticPointCloudAccumulator(
        8., calib, 1e3, None, KITTI_FILTERS, SEM_IDXS, True, BEV_PARAMS_KITTI)
    pc, _, img = kitti_frame(rng, 4096, H, W)
    sem = rng.integers(0, 19, (H, W)).astype(np.int64)
    sem[rng.random((H, W)) < 0.02] = 255
    P = calib['p_velo_frame']
    out = dict(pc=pc, img=img, sem=sem, P=P, H=np.array(H), W=np.array(W))
    out['velo2img'] = acc.velo2img(pc.copy(), P, H, W)
    out['sem_rgb'] = acc.gen_semantic_pc(pc.copy(), img, P)
    out['sem_sem'] = acc.gen_semantic_pc(pc.copy(), sem[..., None], P)
    rgbsem = np.concatenate((out['sem_rgb'], out['sem_sem'][:, -1:]), axis=1)
    out['filtered'] = acc.filter_semseg_pc(rgbsem)

    # axis-aligned camera: exact .5 rounding, depth == 0, <0, tiny, inf, nan
    P2 = np.array([[8., 0, 48, 0], [0, 8, 32, 0], [0, 0, 1, 0]])
    e = []
    for x in (0.25, 0.75, -24.25, -24.75, 23.25, 23.75, 23.5, -24.0):
        for y in (0.25, 0.75, -16.25, -16.75, 15.25, 15.75, 15.5, -16.0):
            e.append([x, y, 4.0, 0.5])
    e += [[1, 1, 0, .1], [0, 0, 0, .2], [1, 1, -4, .3], [1, 1, 1e-30, .4],
          [1e30, 1, 1, .5], [np.inf, 1, 1, .6], [1, np.nan, 1, .7],
          [1, 1, np.inf, .8], [np.nan, np.nan, np.nan, .9], [0, 0, 1e-38, 1.],
          [3, -2, 2, 0.]]
    pc2 = np.array(e, dtype=np.float32)
    pc2 = np.concatenate([pc2, kitti_frame(rng, 512, H, W, 8.0)[0]])
    pc2[-512:, 2] = np.abs(pc2[-512:, 2]) + 0.5
    out['pc2'] = pc2
    out['P2'] = P2
    with np.errstate(all='ignore'):
        out['velo2img2'] = acc.velo2img(pc2.copy(), P2, H, W)
        out['sem_rgb2'] = acc.gen_semantic_pc(pc2.copy(), img, P2)
        out['sem_sem2'] = acc.gen_semantic_pc(pc2.copy(), sem[..., None], P2)
    np.savez_compressed(os.path.join(out_dir, 'k1.npz'), **out)
    print('k1: kept', out['velo2img'].shape[0], 'of', pc.shape[0],
          '| filtered', out['filtered'].shape[0], '| edge kept',
          out['velo2img2'].shape[0], 'of', pc2.shape[0])


def case_kitti_accum(ref, out_dir):
    """Kitti360 accumulator: integrate() x14 with injected poses, eviction,
    then generate_bev (semseg from images) + a use_gt_sem variant."""
    rng = np.random.default_rng(202)
    H, W = 64, 96
    calib = small_calib(H, W, 40.0)
    ref.sem_pc_accum.SemSegONNX = lambda path: FakeSemSeg()
    acc = ref.kitti.Kitti360SemanticPointCloudAccumulator(
        8., calib, 1e3, 'fake.onnx', KITTI_FILTERS, SEM_IDXS, False,
        BEV_PARAMS_KITTI)
    F, N = 14, 3000
    out = dict(P=calib['p_velo_frame'], H=np.array(H), W=np.array(W),
               F=np.array(F), horizon=np.array(8.))
    Ts = []
    for k in range(F):
        T = rigid(0.001 * (k % 3), -0.002, -0.02 - 0.001 * k, -1.0 - 0.01 * k,
                  0.05, 0.01)
        Ts.append(T)
    out['Ts'] = np.stack(Ts)
    removed = []
    for k in range(F):
        pc, pil, img = kitti_frame(rng, N - 100 * (k % 4), H, W)
        out[f'pc_{k}'] = pc
        out[f'img_{k}'] = img
        _icp_queue.append(Ts[k])
        removed.append(acc.integrate([(pil, pc, None)]))
        if k in (0, 4, F - 1):
            out[f'step{k}_sizes'] = np.array([a.shape[0] for a in acc.sem_pcs])
            out[f'step{k}_sem_pcs'] = np.concatenate(acc.sem_pcs)
            out[f'step{k}_poses'] = np.array(acc.poses)
            out[f'step{k}_seg_dists'] = np.array(acc.seg_dists)
    out['removed'] = np.array(removed)
    out['incr_path_dists'] = acc.get_incremental_path_dists()
    present_idx = len(acc.poses) // 2
    out['present_idx'] = np.array(present_idx)
    bev = acc.generate_bev(present_idx, 1, gen_future=True)[0]
    flat_bev('bev_', bev, out)
    np.savez_compressed(os.path.join(out_dir, 'kitti_accum.npz'), **out)
    print('kitti_accum: live frames', len(acc.poses), 'removed', removed)

    # use_gt_sem variant (no projection at all, rgb = 0)
    acc = ref.kitti.Kitti360SemanticPointCloudAccumulator(
        50., calib, 1e3, None, KITTI_FILTERS, SEM_IDXS, True,
        BEV_PARAMS_KITTI)
    out = dict(P=calib['p_velo_frame'])
    Ts = [rigid(0, 0.001, 0.03, -1.5, 0.1, 0.0) for _ in range(4)]
    out['Ts'] = np.stack(Ts)
    for k in range(4):
        pc, pil, img = kitti_frame(rng, 2000, H, W, 15.0)
        sem_gt = rng.integers(0, 19, (2000, 1)).astype(np.int16)
        sem_gt[rng.random(2000) < 0.03] = 255
        out[f'pc_{k}'] = pc
        out[f'sem_gt_{k}'] = sem_gt
        _icp_queue.append(Ts[k])
        acc.integrate([(pil, pc, sem_gt)])
    out['sizes'] = np.array([a.shape[0] for a in acc.sem_pcs])
    out['sem_pcs'] = np.concatenate(acc.sem_pcs)
    out['poses'] = np.array(acc.poses)
    bev = acc.generate_bev(2, 1, gen_future=True)[0]
    flat_bev('bev_', bev, out)
    np.savez_compressed(os.path.join(out_dir, 'kitti_gtsem.npz'), **out)
    print('kitti_gtsem: sizes', out['sizes'])


def random_sem_pc(rng, n, lim, int255=False, dyn_frac=0.1):
    pc = np.zeros((n, 10))
    pc[:, 0] = rng.uniform(-lim, lim, n)
    pc[:, 1] = rng.uniform(-lim, lim, n)
    pc[:, 2] = rng.uniform(-2, 4, n)
    if int255:
        pc[:, 3] = rng.integers(0, 256, n) / 255.
    else:
        pc[:, 3] = rng.uniform(0, 1, n).astype(np.float32)
    pc[:, 4:7] = rng.integers(0, 256, (n, 3))
    pc[:, 7] = rng.choice([0, 0, 0, 1, 2, 8, 9, 13, 14, 15, 17, 5], n)
    pc[:, 8] = rng.integers(-1, 4, n)
    pc[:, 9] = (rng.random(n) < dyn_frac).astype(float)
    return pc


def bev_inputs(rng, n_p, n_f, lim, int255=False):
    pc_present = random_sem_pc(rng, n_p, lim, int255)
    pc_future = random_sem_pc(rng, n_f, lim, int255)
    pc_full = np.concatenate([pc_present, pc_future])
    k = 9
    s = np.linspace(-0.9 * lim, 0.9 * lim, 2 * k)
    traj = np.stack([s, 0.3 * s + 0.02 * s**2 / lim, 0 * s + 1.0], 1)
    other = [
        np.stack([s[:k] * 1.3 + 2.0, -0.5 * s[:k] - 1.0, 0 * s[:k]], 1),
        np.stack([0 * s[:4] + 1e3, s[:4], 0 * s[:4]], 1),   # fully outside
    ]
    pcs = dict(pc_present=pc_present, pc_future=pc_future, pc_full=pc_full)
    trajs = dict(ego_traj_present=traj[:k].copy(),
                 ego_traj_future=traj[k:].copy(), ego_traj_full=traj.copy(),
                 other_trajs_present=[o.copy() for o in other],
                 other_trajs_future=[other[0][::-1].copy()],
                 other_trajs_full=[])
    return pcs, trajs


def copy_inputs(pcs, trajs):
    p = {k: (None if v is None else v.copy()) for k, v in pcs.items()}
    t = {}
    for k, v in trajs.items():
        t[k] = [a.copy() for a in v] if isinstance(v, list) else v.copy()
    return p, t


def store_inputs(out, pcs, trajs):
    out['pc_present'] = pcs['pc_present']
    out['pc_future'] = pcs['pc_future']
    for k, v in trajs.items():
        if isinstance(v, list):
            out[f'in_{k}_n'] = np.array(len(v))
            for i, a in enumerate(v):
                out[f'in_{k}_{i}'] = a
        else:
            out[f'in_{k}'] = v


def ref_planes(gen, pcs, trajs, out, rot=None, dx=0., dy=0., zoom=1.):
    """Pre-fp16-cast f64 planes for the three point sets, obtained by calling
    the reference's own sub-functions in the order generate()/generate_bev()
    call them.  Stored as pre_<plane>_<set>."""
    p, t = copy_inputs(pcs, trajs)
    if rot is None:
        ego = t['ego_traj_present']
        rot = 0.5 * np.pi
        if len(ego) > 1:
            rot += np.arctan2(ego[-1][1] - ego[-2][1], ego[-1][0] - ego[-2][0])
        rot = np.pi - rot
    out['rot_ang'] = np.array(rot)
    aug = zoom * gen.view_size
    for name in ('present', 'future', 'full'):
        pc_g, _ = gen.preprocess_pc_and_trajs(p[f'pc_{name}'], [], rot, dx, dy,
                                              aug)
        out[f'pre_n_grid_{name}'] = np.array(pc_g.shape[0])
        _, pc_s = gen.partition_semantic_pc(pc_g, [1], 9)
        r, g, b = gen.get_rgb_maps(pc_s)
        out[f'pre_rgb_{name}'] = np.stack([r, g, b]) / 255.
        out[f'pre_elevation_{name}'] = gen.get_elevation_map(pc_s)[0]
        out[f'pre_road_{name}'] = gen.gen_sem_probmap(pc_s, ['road'])
        im = gen.gen_intensity_map(pc_s, 'road')
        out[f'pre_intraw_{name}'] = im
        out[f'pre_intensity_{name}'] = gen.road_marking_transform(
            im, gen.int_scaler, gen.int_sep_scaler, gen.int_mid_threshold)
        out[f'pre_dynamic_{name}'] = gen.gen_sem_probmap(
            pc_s, ['car', 'truck', 'bus', 'motorcycle'])
        if name == 'present':
            out['pre_grid_rows_present'] = pc_g


def case_bev(ref, out_dir):
    rng = np.random.default_rng(303)
    # ---- A: KITTI params, heading from trajectory, intermediates stored ----
    gen = ref.SemBEVGenerator(SEM_IDXS, 20, 32, 0., 0., False, 20., 20., 0.5,
                              None)
    pcs, trajs = bev_inputs(rng, 8000, 12000, 14.0)
    out = {}
    store_inputs(out, pcs, trajs)
    p, t = copy_inputs(pcs, trajs)
    flat_bev('bev_', gen.generate(p, t), out)
    ref_planes(gen, pcs, trajs, out)
    np.savez_compressed(os.path.join(out_dir, 'bev_a.npz'), **out)

    # ---- B: NuScenes params, height filter, explicit rot/trans/zoom ----
    gen = ref.SemBEVGenerator(SEM_IDXS, 51.2, 64, 0., 0., False, 1., 30., 0.12,
                              3.)
    pcs, trajs = bev_inputs(rng, 15000, 9000, 33.0, int255=True)
    out = {}
    store_inputs(out, pcs, trajs)
    args = (0.7, 1.5, -2.25, 1.1, True)
    out['args'] = np.array(args[:4])
    p, t = copy_inputs(pcs, trajs)
    flat_bev('bev_', gen.generate(p, t, *args), out)
    ref_planes(gen, pcs, trajs, out, *args[:4])
    np.savez_compressed(os.path.join(out_dir, 'bev_b.npz'), **out)

    # ---- C: 256 x 256, view 80 ----
    gen = ref.SemBEVGenerator(SEM_IDXS, 80, 256, 0., 0., False, 20., 20., 0.5,
                              None)
    pcs, trajs = bev_inputs(rng, 14000, 14000, 55.0)
    # pile-ups: many points in few cells (contention + long medians)
    pcs['pc_present'][:3000, :2] = rng.uniform(-0.6, 0.6, (3000, 2))
    pcs['pc_future'][:2000, :2] = rng.uniform(-0.6, 0.6, (2000, 2))
    pcs['pc_full'] = np.concatenate([pcs['pc_present'], pcs['pc_future']])
    out = {}
    store_inputs(out, pcs, trajs)
    p, t = copy_inputs(pcs, trajs)
    flat_bev('bev_', gen.generate(p, t), out)
    ref_planes(gen, pcs, trajs, out)
    np.savez_compressed(os.path.join(out_dir, 'bev_c.npz'), **out)

    # ---- D: empty future set, single-pose trajectory (no heading) ----
    gen = ref.SemBEVGenerator(SEM_IDXS, 20, 16, 0., 0., False, 20., 20., 0.5,
                              None)
    pcs, trajs = bev_inputs(rng, 500, 0, 14.0)
    trajs['ego_traj_present'] = trajs['ego_traj_present'][:1]
    out = {}
    store_inputs(out, pcs, trajs)
    p, t = copy_inputs(pcs, trajs)
    flat_bev('bev_', gen.generate(p, t), out)
    np.savez_compressed(os.path.join(out_dir, 'bev_d.npz'), **out)

    # ---- E: do_warp=True with pinned warp parameters ----
    gen = ref.SemBEVGenerator(SEM_IDXS, 20, 32, 0., 0., True, 20., 20., 0.5,
                              None)
    gen.get_random_warp_params = lambda *a: (16 + 3.7, 16 - 2.2)
    pcs, trajs = bev_inputs(rng, 6000, 6000, 14.0)
    out = dict(warp=np.array([16 + 3.7, 16 - 2.2]))
    store_inputs(out, pcs, trajs)
    p, t = copy_inputs(pcs, trajs)
    flat_bev('bev_', gen.generate(p, t), out)
    np.savez_compressed(os.path.join(out_dir, 'bev_e.npz'), **out)
    print('bev: a,b,c,d,e written')


# --------------------------------------------------------------------------
#  BEV edge fixtures: cell boundaries, crop edges, height filter, medians
# --------------------------------------------------------------------------
EDGE_CFGS = {
    # name: (view, px, height_filter, (int_scaler, int_sep_scaler, int_mid_threshold), intensity_div255)
    'kitti': (20, 32, None, (20., 20., 0.5), False),
    'nusc': (51.2, 64, 3., (1., 30., 0.12), True),
    'px30': (33, 30, 3., (20., 20., 0.5), False),     # not a multiple of the 8 x 8 tile
    'px7': (10, 7, 1.5, (1., 30., 0.12), True),       # smaller than one tile
}
EDGE_ROTS = (0., 0.5 * np.pi, np.pi, 0.7, -2.1)
EDGE_SHIFTS = ((0., 0., 1.), (1.5, -2.25, 1.1))
EDGE_CLASSES = (0, 0, 0, 1, 2, 8, 9, 13, 14, 15, 17, 10, 255)   # road / static / dynamic classes / filtered-looking


def edge_gen(ref, cfg):
    view, px, hf, ints, _ = cfg
    return ref.SemBEVGenerator(SEM_IDXS, view, px, 0., 0., False, *ints, hf)


def edge_intensity(rng, n, div255):
    if div255:
        return rng.integers(0, 256, n) / 255.
    return rng.integers(0, 65, n) / 64.               # exact in f32


def edge_rows(rng, xy, div255, dyn_frac=0.1):
    n = xy.shape[0]
    rows = np.zeros((n, 10))
    rows[:, :2] = xy
    rows[:, 2] = rng.integers(-8, 17, n) / 4.         # -2 .. 4 in steps of 0.25 (+0.0 included)
    rows[:, 3] = edge_intensity(rng, n, div255)
    rows[:, 4:7] = rng.integers(0, 256, (n, 3))
    rows[:, 7] = rng.choice(EDGE_CLASSES, n)
    rows[:, 8] = rng.integers(-1, 4, n)
    rows[:, 9] = (rng.random(n) < dyn_frac).astype(float)
    return rows


def edge_transformed(gen, rows, rot, dx, dy, aug):
    """The reference's own geometric_transform output (rotated, shifted, cropped) with the surviving rows' indices."""
    tagged = np.concatenate([rows, np.arange(rows.shape[0], dtype=float)[:, None]], 1)
    t = gen.geometric_transform(tagged, rot, dx, dy, aug)
    return t, t[:, -1].astype(int)


def edge_drop_px_hits(gen, rows, rot, dx, dy, aug):
    """Removes the rows whose grid coordinate floors to px (the reference raises or wraps there)."""
    px = gen.pixel_size
    t, idx = edge_transformed(gen, rows, rot, dx, dy, aug)
    hit = (np.floor(t[:, 0:2] / aug * px + 0.5 * px) == px).any(1)
    keep = np.ones(rows.shape[0], bool)
    keep[idx[hit]] = False
    return rows[keep], int(hit.sum())


def edge_check_inputs(gen, rows, rot, dx, dy, aug):
    """The exclusions every edge fixture keeps: finite coordinates, no grid coordinate == px, no cell with both
    zeros as z.  Returns (transformed kept rows, their grid coordinates)."""
    px = gen.pixel_size
    assert np.isfinite(rows[:, :3]).all()
    t, _ = edge_transformed(gen, rows, rot, dx, dy, aug)
    if gen.height_filter is not None:
        t = t[t[:, 2] < gen.height_filter]
    t = t[t[:, 9] != 1]
    ij = np.floor(t[:, 0:2] / aug * px + 0.5 * px)
    assert not (ij == px).any() and (ij >= 0).all()
    cell = (ij[:, 1] * px + ij[:, 0]).astype(int)
    zero = t[:, 2] == 0
    neg = set(cell[zero & np.signbit(t[:, 2])])
    pos = set(cell[zero & ~np.signbit(t[:, 2])])
    assert not (neg & pos), 'a cell holds both +0.0 and -0.0'
    return t, ij


def edge_trajs(view):
    return bev_inputs(np.random.default_rng(0), 0, 0, 0.45 * view)[1]


def edge_write(ref, cfg, pcs_list, out_path, extra=None):
    """Runs every (present, future, rot, dx, dy, zoom) through generate() and ref_planes(); one npz, keys k<n>_<name>."""
    view, px, hf, ints, div255 = cfg
    gen = edge_gen(ref, cfg)
    trajs = edge_trajs(view)
    out = dict(n_cases=np.array(len(pcs_list)))
    for k, (present, future, rot, dx, dy, zoom) in enumerate(pcs_list):
        aug = zoom * gen.view_size
        for rows in (present, future, np.concatenate([present, future])):
            edge_check_inputs(gen, rows, rot, dx, dy, aug)
        pcs = dict(pc_present=present, pc_future=future, pc_full=np.concatenate([present, future]))
        one = {}
        store_inputs(one, pcs, trajs)
        one['cfg'] = np.array([view, px, np.nan if hf is None else hf, *ints, float(div255), rot, dx, dy, zoom])
        p, t = copy_inputs(pcs, trajs)
        flat_bev('bev_', gen.generate(p, t, rot, dx, dy, zoom, True), one)
        ref_planes(gen, pcs, trajs, one, rot, dx, dy, zoom)
        del one['pre_grid_rows_present']
        for key, v in one.items():
            out[f'k{k}_{key}'] = v
    for key, v in (extra or {}).items():
        out[key] = v
    np.savez_compressed(out_path, **out)
    assert os.path.getsize(out_path) < 1 << 20, out_path
    return out


def lattice_1d(aug, px):
    """Cell boundaries (k - px/2) aug/px with both neighbours, cell centres, +-aug/2 with two neighbours each side."""
    k = np.arange(px + 1)
    b = (k - 0.5 * px) * aug / px
    vals = [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf), (k[:-1] + 0.5 - 0.5 * px) * aug / px]
    for e in (-0.5 * aug, 0.5 * aug):
        lo1, hi1 = np.nextafter(e, -np.inf), np.nextafter(e, np.inf)
        vals.append([e, lo1, hi1, np.nextafter(lo1, -np.inf), np.nextafter(hi1, np.inf)])
    return np.unique(np.concatenate([np.asarray(v, dtype=float) for v in vals]))


def lattice_set(rng, gen, cfg, rot, dx, dy, zoom, which):
    """One point set on the lattice in VIEW coordinates, taken back through the shift and the rotation."""
    view, px, hf, ints, div255 = cfg
    aug = zoom * gen.view_size
    t1 = lattice_1d(aug, px)
    if px <= 8:
        tx, ty = [a.ravel() for a in np.meshgrid(t1, t1)]
    else:
        m = -(-500 // t1.size)
        tx = np.concatenate([np.tile(t1, m), rng.choice(t1, m * t1.size)])
        ty = np.concatenate([rng.choice(t1, m * t1.size), np.tile(t1, m)])
    target = np.stack([tx, ty], 1)
    # reserved cells (grid coordinates i, j) hold hand-made points only
    reserved = {'neg0_present': (1, 1), 'neg0_future': (3, 2), 'neg0_both': (5, 1), 'min_twice': (2, 4),
                'only_dyn': (4, 5), 'at_filter': (1, 5), 'below_filter': (5, 4)}
    ij = np.floor(target / aug * px + 0.5 * px)
    near = np.zeros(target.shape[0], bool)
    for ci, cj in reserved.values():                  # keep a margin: a boundary point may land on either side
        lo = ((np.array([ci, cj]) - 0.5 * px) * aug / px)
        near |= ((target >= lo - 1e-6) & (target <= lo + aug / px + 1e-6)).all(1)
    target = target[~near]
    R = gen.rotation_matrix_3d(rot)[:2, :2]
    xy = (target - [dx, dy]) @ R                      # R^T (t - d) as row vectors
    rows = edge_rows(rng, xy, div255)
    n = rows.shape[0]
    fz = 3. if hf is None else hf
    idx = np.arange(n)
    rows[idx % 7 == 0, 2] = fz
    rows[idx % 7 == 1, 2] = np.nextafter(fz, -np.inf)
    # hand-made cells
    def centre(name):
        ci, cj = reserved[name]
        c = (np.array([ci, cj]) + 0.5 - 0.5 * px) * aug / px
        return (c - [dx, dy]) @ R
    def point(name, z, sem=0, dyn=0., col=(10, 20, 30), inten=None):
        r = np.zeros(10)
        r[:2] = centre(name)
        r[2] = z
        r[3] = (51 / 255. if div255 else 0.25) if inten is None else inten
        r[4:7] = col
        r[7], r[8], r[9] = sem, -1, dyn
        return r
    special = []
    if which == 'present':
        special += [point('neg0_present', -0.0), point('neg0_both', -0.0, sem=1)]
        special += [point('min_twice', -1.5), point('min_twice', 0.25, sem=2), point('min_twice', -1.5, sem=13)]
    else:
        special += [point('neg0_future', -0.0, sem=13), point('neg0_both', -0.0)]
        special += [point('min_twice', -1.5, sem=1)]
    special += [point('only_dyn', -1.0, dyn=1.), point('only_dyn', 0.5, sem=13, dyn=1.)]
    special += [point('at_filter', fz), point('below_filter', np.nextafter(fz, -np.inf)), point('below_filter', fz)]
    rows = np.concatenate([rows, np.array(special)])
    rows = rows[rng.permutation(rows.shape[0])]
    rows, n_hit = edge_drop_px_hits(gen, rows, rot, dx, dy, aug)
    return rows, n_hit, reserved


def case_bev_edges(ref, out_dir):
    """Hand-built edge inputs through the real reference: tests/golden/bev_edges_<name>.npz (see tools/README.md)."""
    # ---- lattice: one file per parameter set, rotations x shifts inside ----
    for c, (cname, cfg) in enumerate(EDGE_CFGS.items()):
        view, px, hf, ints, div255 = cfg
        gen = edge_gen(ref, cfg)
        rng = np.random.default_rng(700 + c)
        for r, rot in enumerate(EDGE_ROTS):           # one file per rotation, the shifts inside
            cases, stats = [], []
            for dx, dy, zoom in EDGE_SHIFTS:
                aug = zoom * gen.view_size
                present, hit_p, reserved = lattice_set(rng, gen, cfg, rot, dx, dy, zoom, 'present')
                future, hit_f, _ = lattice_set(rng, gen, cfg, rot, dx, dy, zoom, 'future')
                full = np.concatenate([present, future])
                t, _ = edge_transformed(gen, full, rot, dx, dy, aug)
                n_in, n_out = t.shape[0], full.shape[0] - t.shape[0]
                fz = 3. if hf is None else hf
                n_at, n_below = int((t[:, 2] == fz).sum()), int((t[:, 2] == np.nextafter(fz, -np.inf)).sum())
                s = t[:, 0:2] / aug * px + 0.5 * px
                n_exact = int((s == np.floor(s)).any(1).sum())
                # many points on each side of the crop and of the height filter, or the fixture has degenerated
                assert n_in > 200 and n_out > 40, (cname, rot, n_in, n_out)
                assert n_at > 40 and n_below > 40, (cname, rot, n_at, n_below)
                if rot == 0. and dx == 0.:
                    assert n_exact > 100, (cname, n_exact)         # exact arithmetic: points ON cell boundaries
                stats.append((n_in, n_out, n_exact, hit_p + hit_f))
                cases.append((present, future, rot, dx, dy, zoom))
            res = np.array([[i, j] for i, j in reserved.values()])
            edge_write(ref, cfg, cases, os.path.join(out_dir, f'bev_edges_lattice_{cname}_r{r}.npz'),
                       dict(reserved_names=np.array(list(reserved)), reserved_ij=res))
            print(f'bev_edges lattice_{cname}_r{r}: (in view, cropped, on a boundary, dropped at px) per case', stats)
    case_bev_edges_counts(ref, out_dir)
    case_bev_edges_intensity(ref, out_dir)
    case_bev_edges_empty(ref, out_dir)


def centre_xy(i, j, view, px):
    return np.array([(i + 0.5 - 0.5 * px) * view / px, (j + 0.5 - 0.5 * px) * view / px])


COUNTS_CFG = (32, 64, None, (1., 30., 0.12), True)    # cell 0.5 m, tile 4 m: every centre is exact


def counts_cell(rng, i, j, n, scheme, sem='mixed', dyn=0., div255=True):
    """n points at the centre of cell (i, j); colours take two values only.  scheme: per channel how many get the low
    value -- 'half' (even n: an x.5 median), 'all' (all equal), 'mid' (the two middle values equal)."""
    view, px = COUNTS_CFG[:2]
    rows = np.zeros((n, 10))
    rows[:, :2] = centre_xy(i, j, view, px)
    rows[:, 2] = rng.integers(-8, 17, n) / 4.
    rows[:, 3] = edge_intensity(rng, n, div255)
    lo, hi = (10, 60, 200), (201, 61, 255)
    for ch, how in enumerate(scheme):
        n_lo = {'half': n // 2, 'all': n, 'mid': min(n, n // 2 + 1), 'none': 0}[how]
        col = np.full(n, hi[ch], dtype=float)
        col[:n_lo] = lo[ch]
        rows[:, 4 + ch] = rng.permutation(col)
    if sem == 'mixed':
        rows[:, 7] = rng.choice([0, 0, 1, 2, 13, 17], n)
    else:
        rows[:, 7] = sem
    rows[:, 8] = -1
    rows[:, 9] = dyn
    return rows


def case_bev_edges_counts(ref, out_dir):
    cfg = COUNTS_CFG
    view, px = cfg[:2]
    gen = edge_gen(ref, cfg)
    rng = np.random.default_rng(811)
    present, future = [], []
    table = []                                        # (i, j, n_present, n_future)
    schemes = (('half', 'all', 'mid'), ('mid', 'half', 'all'), ('all', 'mid', 'half'))
    counts = (1, 2, 3, 4, 63, 64, 65, 66, 128)
    for k, n in enumerate(counts):
        for v, sch in enumerate(schemes):             # rows j = 2 + v (present only), 6 + v (future only)
            present.append(counts_cell(rng, 2 + 2 * k, 2 + v, n, sch))
            table.append((2 + 2 * k, 2 + v, n, 0))
            future.append(counts_cell(rng, 2 + 2 * k, 6 + v, n, sch))
            table.append((2 + 2 * k, 6 + v, 0, n))
    # 'full' crossing 64 with neither set above it, and landing exactly on the counts again
    for k, (n_p, n_f) in enumerate(((32, 32), (63, 1), (1, 63), (33, 32), (40, 26), (64, 64), (64, 1), (2, 2), (1, 1),
                                    (1, 2), (63, 65), (60, 3))):
        sch = schemes[k % 3]
        present.append(counts_cell(rng, 2 + 2 * k, 12, n_p, sch))
        future.append(counts_cell(rng, 2 + 2 * k, 12, n_f, sch))
        table.append((2 + 2 * k, 12, n_p, n_f))
    # one class only / dynamic only (the static partition leaves the last cell empty)
    for k, (sem, dyn) in enumerate(((0, 0.), (1, 0.), (13, 0.), (0, 1.), (13, 1.))):
        for v, n in enumerate((1, 2, 64, 65)):
            present.append(counts_cell(rng, 30 + 2 * k, 16 + 2 * v, n, schemes[v % 3], sem, dyn))
            future.append(counts_cell(rng, 30 + 2 * k, 16 + 2 * v, n + 1, schemes[v % 3], sem, dyn))
            table.append((30 + 2 * k, 16 + 2 * v, n if not dyn else 0, n + 1 if not dyn else 0))
    # a tile with more colour records than stay resident (batches; heavy kernel): grid columns 32..39, rows j 32..39;
    # and a heavy tile that still fits (columns 40..47).  One cell of each holds exactly 64 / 63 + 1 values.
    for i0, per_p, per_f in ((32, 60, 45), (40, 30, 22)):
        for ci in range(8):
            for cj in range(8):
                n_p, n_f = per_p + (ci * 8 + cj) % 5, per_f + (ci + cj) % 3
                if (ci, cj) == (3, 4):
                    n_p, n_f = 64, 0
                if (ci, cj) == (4, 3):
                    n_p, n_f = 63, 1
                if (ci, cj) == (0, 7):
                    n_p, n_f = 0, 64
                sch = schemes[(ci + cj) % 3]
                if n_p:
                    present.append(counts_cell(rng, i0 + ci, 32 + cj, n_p, sch))
                if n_f:
                    future.append(counts_cell(rng, i0 + ci, 32 + cj, n_f, sch))
                table.append((i0 + ci, 32 + cj, n_p, n_f))
    present, future = np.concatenate(present), np.concatenate(future)
    # points outside the view (identical rows): the window is larger than what level 1 keeps in registers when it
    # runs as one piece
    far = np.zeros((18000 - present.shape[0] - future.shape[0], 10))
    far[:, 0], far[:, 3], far[:, 8] = 1000., 1., -1
    assert far.shape[0] > 0
    present = np.concatenate([present, far[:far.shape[0] // 2]])
    future = np.concatenate([future, far[far.shape[0] // 2:]])
    present = present[rng.permutation(present.shape[0])]
    future = future[rng.permutation(future.shape[0])]
    table = np.array(table)
    # the table is what the reference sees: static points per cell and set
    for rows, col in ((present, 2), (future, 3)):
        t, ij = edge_check_inputs(gen, rows, 0., 0., 0., float(view))
        got = np.bincount((ij[:, 1] * px + ij[:, 0]).astype(int), minlength=px * px)
        want = np.zeros(px * px, int)
        want[table[:, 1] * px + table[:, 0]] = table[:, col]
        assert np.array_equal(got, want)
    tile_records = [(table[(table[:, 0] // 8 == a) & (table[:, 1] // 8 == 4), 2:].sum()) for a in (4, 5)]
    assert tile_records[0] > 4096 and 2560 < tile_records[1] <= 4096, tile_records
    edge_write(ref, cfg, [(present, future, 0., 0., 0., 1.)], os.path.join(out_dir, 'bev_edges_counts.npz'),
               dict(cell_counts=table))
    print('bev_edges counts:', present.shape[0], '+', future.shape[0], 'points, dense tiles hold', tile_records)


def case_bev_edges_intensity(ref, out_dir):
    """Road cells whose mean intensity sum / (count + 1) sits at and around int_mid_threshold, at 0 and at the largest
    raw value, for counts 1 .. 255; both parameter triples of the drivers."""
    rng = np.random.default_rng(822)
    for cname in ('kitti', 'nusc'):
        cfg = EDGE_CFGS[cname]
        view, px, hf, ints, div255 = cfg
        gen = edge_gen(ref, cfg)
        thr = ints[2]
        sets = {'present': [], 'future': []}
        cell = 0
        for n in (1, 2, 3, 9, 50, 255):
            want = thr * (n + 1) / n                  # n v / (n + 1) == thr
            if div255:
                k0 = int(np.floor(want * 255.))
                vals = [0., 1.] + [k / 255. for k in range(max(k0 - 2, 0), min(k0 + 4, 256))]
            else:
                w32 = np.float32(min(want, 1.))
                vals = [0., 1., float(w32), float(np.nextafter(w32, np.float32(0))),
                        float(np.nextafter(w32, np.float32(2))), float(np.float32(0.9) * w32), float(np.float32(thr))]
            for v in vals:
                for which in ('present', 'future'):
                    i, j = 1 + cell % (px - 2), 1 + cell // (px - 2)
                    cell += 1
                    rows = np.zeros((n, 10))
                    rows[:, :2] = centre_xy(i, j, view, px)
                    rows[:, 2] = rng.integers(-8, 11, n) / 4.
                    rows[:, 3] = v
                    rows[:, 4:7] = rng.integers(0, 256, (n, 3))
                    rows[:, 8] = -1
                    sets[which].append(rows)
                    if n == 3:                        # non-road and dynamic points in the cell change nothing
                        other = rows.copy()
                        other[:, 7], other[:, 3] = 2, 1.
                        other[0, 7], other[0, 9] = 0, 1.
                        sets[which].append(other)
            # mixed values in one cell, seen by both sets: the sum is taken in point order
            for which in ('present', 'future'):
                i, j = 1 + cell % (px - 2), 1 + cell // (px - 2)
                rows = np.zeros((n, 10))
                rows[:, :2] = centre_xy(i, j, view, px)
                rows[:, 3] = edge_intensity(rng, n, div255)
                rows[:, 4:7] = rng.integers(0, 256, (n, 3))
                rows[:, 8] = -1
                sets[which].append(rows)
            cell += 1
        assert 1 + cell // (px - 2) < px - 1
        present, future = (np.concatenate(sets[w]) for w in ('present', 'future'))
        present = present[rng.permutation(present.shape[0])]
        future = future[rng.permutation(future.shape[0])]
        out = edge_write(ref, cfg, [(present, future, 0., 0., 0., 1.)],
                         os.path.join(out_dir, f'bev_edges_intensity_{cname}.npz'))
        raw = out['k0_pre_intraw_present']
        assert (raw == 0).sum() > 0 and (raw > thr).sum() > 5 and ((raw < thr) & (raw > 0)).sum() > 5
        print(f'bev_edges intensity_{cname}:', present.shape[0], '+', future.shape[0], 'points; cells at the threshold:',
              int((raw == thr).sum()))


def case_bev_edges_empty(ref, out_dir):
    """Present empty with future populated, the reverse, and every point outside the view by one ulp."""
    cfg = EDGE_CFGS['nusc']
    view, px, hf, ints, div255 = cfg
    rng = np.random.default_rng(833)
    some = edge_rows(rng, rng.integers(-200, 201, (600, 2)) / 8., div255)
    empty = np.zeros((0, 10))
    e = 0.5 * view
    out1 = [np.nextafter(e, np.inf), e, -e, np.nextafter(-e, -np.inf)]
    xy = [(a, b) for a in out1 for b in (0.4, -25.6, 25.5, e)] + [(b, a) for a in out1 for b in (0.4, -25.6, 25.5, -e)]
    outside = edge_rows(rng, np.array(xy), div255, dyn_frac=0.)
    inside_but_high = edge_rows(rng, rng.integers(-200, 201, (40, 2)) / 8., div255, dyn_frac=0.)
    inside_but_high[:, 2] = hf                        # z == height_filter: dropped
    gone = np.concatenate([outside, inside_but_high])
    cases = [(empty, some, 0., 0., 0., 1.), (some, empty, 0., 0., 0., 1.), (gone[:40], gone[40:], 0., 0., 0., 1.)]
    out = edge_write(ref, cfg, cases, os.path.join(out_dir, 'bev_edges_empty_sets.npz'))
    assert int(out['k2_pre_n_grid_full']) == 0 and int(out['k0_pre_n_grid_present']) == 0
    assert int(out['k0_pre_n_grid_future']) > 300 and int(out['k1_pre_n_grid_future']) == 0
    print('bev_edges empty_sets written')


def case_nusc(ref, out_dir):
    from PIL import Image
    rng = np.random.default_rng(404)
    H, W = 45, 80
    ref.sem_pc_accum.SemSegONNX = lambda path: FakeSemSeg()
    acc = ref.oracle.NuScenesOracleSemanticPointCloudAccumulator(
        'fake.onnx', NUSC_FILTERS, SEM_IDXS, False, BEV_PARAMS_NUSC, 'boston',
        False, None)
    F, N = 7, 2500
    out = dict(F=np.array(F), H=np.array(H), W=np.array(W))
    tokens_all = []
    for k in range(F):
        pc = np.zeros((N, 7))
        pc[:, 0] = rng.uniform(-20, 20, N)
        pc[:, 1] = rng.uniform(-20, 20, N)
        pc[:, 2] = rng.uniform(-2, 4, N)
        pc[:, 3] = rng.integers(0, 256, N)
        pc[:, 4] = rng.uniform(1.01, W - 1.01, N)
        pc[:, 5] = rng.uniform(1.01, H - 1.01, N)
        pc[:, 6] = rng.integers(-1, 4, N)
        # exact .5 pixel coordinates (round-half-even) on a few points
        pc[:8, 4] = [1.5, 2.5, 3.5, 4.5, 77.5, 78.5, 10.5, 11.5]
        pc[:8, 5] = [1.5, 2.5, 43.5, 42.5, 3.5, 4.5, 20.5, 21.5]
        cam_idx = rng.integers(-1, 6, N)
        imgs = rng.integers(0, 256, (6, H, W, 3), dtype=np.uint8)
        T = rigid(0.002 * k, -0.001 * k, 0.02 * k, 1000 + 1.0 * k,
                  500 + 0.1 * k, 0.3)
        tokens = ['a', 'b', 'c']
        clss = [0, 7, 1]
        centers = [
            np.array([1010 + 0.6 * k, 505., 0.5]),
            np.array([1005., 495. + 2.0 * k, 0.2]),
            np.array([990., 500., 0.4])
        ]
        if k >= 3:
            tokens.append('d')
            clss.append(5)
            centers.append(np.array([1000. - 0.8 * k, 510., 0.1]))
        if k == 5:      # 'a' unobserved at ts 5 -> split trajectory
            tokens, clss, centers = tokens[1:], clss[1:], centers[1:]
        obs = dict(images=[Image.fromarray(im) for im in imgs], pc=pc,
                   pc_cam_idx=cam_idx, ego_at_lidar_ts=T,
                   ego_global_x=T[0, 3], ego_global_y=T[1, 3],
                   inst_tokens=tokens, inst_cls=clss, inst_center=centers)
        out[f'pc_{k}'] = pc
        out[f'cam_idx_{k}'] = cam_idx
        out[f'imgs_{k}'] = imgs
        out[f'T_{k}'] = T
        out[f'inst_cls_{k}'] = np.array(clss)
        out[f'inst_center_{k}'] = np.stack(centers)
        tokens_all.append(','.join(tokens))
        acc.integrate([obs])
        if k == 0:
            out['frame0_after_integrate'] = acc.sem_pcs[0].copy()
    out['inst_tokens'] = np.array(tokens_all)
    out['sizes'] = np.array([a.shape[0] for a in acc.sem_pcs])
    out['sem_pcs'] = np.concatenate(acc.sem_pcs)
    out['poses'] = np.array(acc.poses)
    out['seg_dists'] = np.array(acc.seg_dists)
    out['dyn_instances'] = np.array(acc.dyn_instances)
    out['incr_path_dists'] = acc.get_incremental_path_dists()
    present_idx = 3
    out['present_idx'] = np.array(present_idx)
    bev = acc.generate_bev(present_idx, 1, gen_future=True)[0]
    flat_bev('bev_', bev, out)
    np.savez_compressed(os.path.join(out_dir, 'nusc_oracle.npz'), **out)
    print('nusc_oracle: sizes', out['sizes'], 'dyn', acc.dyn_instances)


def case_utils(ref, out_dir):
    rng = np.random.default_rng(505)
    nu = ref.nu
    out = {}
    # homo_transform
    T = rigid(0.1, -0.2, 0.3, 1000.5, -500.25, 3.125)
    pts = rng.uniform(-50, 50, (777, 3))
    out['ht_T'] = T
    out['ht_pts'] = pts
    out['ht_out'] = nu.homo_transform(T, pts)
    # pts_feat_from_img
    H, W = 45, 80
    img = rng.integers(0, 256, (H, W, 4)).astype(np.int64)
    uv = np.stack([rng.uniform(1.01, W - 1.01, 600),
                   rng.uniform(1.01, H - 1.01, 600)], 1)
    uv[:6] = [[1.5, 1.5], [2.5, 2.5], [3.5, 43.5], [78.5, 42.5], [10.5, 20.],
              [11., 21.5]]
    out['pf_img'] = img
    out['pf_uv'] = uv
    out['pf_nearest'] = nu.pts_feat_from_img(uv, img, 'nearest')
    # bilinear divides by zero for integer coordinates in the reference
    uvb = uv[uv[:, 0] != np.floor(uv[:, 0])]
    uvb = uvb[uvb[:, 1] != np.floor(uvb[:, 1])]
    out['pf_uv_bil'] = uvb
    # NOTE: the reference's bilinear branch only broadcasts for 2-D (H,W)
    # feature maps ((n,) weights times (n,C) features raises ValueError).
    out['pf_bilinear'] = nu.pts_feat_from_img(uvb, img[..., 0], 'bilinear')
    # project_pts3d (view_points stubbed with the documented formula)
    cam = nu.NuScenesCamera.__new__(nu.NuScenesCamera)
    cam.img_wh = np.array([1600, 900], dtype=float)
    cam.cam_K = np.array([[1266.417203046554, 0.0, 816.2670197447984],
                          [0.0, 1266.417203046554, 491.50706579294757],
                          [0.0, 0.0, 1.0]])
    pc = np.stack([rng.uniform(-30, 30, 900), rng.uniform(-10, 10, 900),
                   rng.uniform(-5, 60, 900)], 1)
    pc[:4, 2] = [0, 1e-3, 1.0000001e-3, -1]
    out['pp_K'] = cam.cam_K
    out['pp_wh'] = cam.img_wh
    out['pp_pc'] = pc
    out['pp_uv'], out['pp_mask'] = cam.project_pts3d(pc)
    # 6-camera projection loop shape (nuscenes_obs_dataloader.py:162-202)
    N = 1200
    pc_l = np.stack([rng.uniform(-40, 40, N), rng.uniform(-40, 40, N),
                     rng.uniform(-3, 5, N)], 1).astype(np.float32).astype(
                         float)
    ego_from_lidar = rigid(0.003, 0.01, -1.57, 0.94, 0.0, 1.84)
    glob_from_ego = rigid(0.01, -0.005, 0.6, 1010.2, 612.7, 0.1)
    cams_glob_from_self = []
    for j in range(6):
        ego_from_cam = rigid(-1.57, 0.0, -1.57 + j * 1.047, 1.5, 0.1 * j, 1.5)
        # a slightly different ego pose per camera timestamp
        g_e = rigid(0.01, -0.005, 0.6 + 0.001 * j, 1010.2 + 0.05 * j, 612.7,
                    0.1)
        cams_glob_from_self.append(g_e @ ego_from_cam)
    pc_in_ego = nu.homo_transform(ego_from_lidar, pc_l)
    pc_in_glob = nu.homo_transform(glob_from_ego, pc_in_ego)
    pc_uv = np.zeros((N, 2))
    pc_cam_idx = -np.ones(N, dtype=int)
    for j in range(6):
        pc_in_cam = nu.homo_transform(np.linalg.inv(cams_glob_from_self[j]),
                                      pc_in_glob)
        uvj, m = cam.project_pts3d(pc_in_cam)
        pc_uv[m] = uvj[m]
        pc_cam_idx[m] = j
    out['c6_pc'] = pc_l
    out['c6_ego_from_lidar'] = ego_from_lidar
    out['c6_glob_from_ego'] = glob_from_ego
    out['c6_glob_from_cam'] = np.stack(cams_glob_from_self)
    out['c6_pc_in_ego'] = pc_in_ego
    out['c6_uv'] = pc_uv
    out['c6_cam_idx'] = pc_cam_idx
    # path distances
    sd = rng.uniform(0.5, 1.5, 37)
    out['pd_seg'] = sd
    out['pd_incr'] = ref.sem_pc_accum.SemanticPointCloudAccumulator.\
        comp_incr_path_dist(sd)
    # trajectories: crop + intersection
    gen = ref.SemBEVGenerator(SEM_IDXS, 20, 32)
    trajs = [
        np.array([[-15., 0, 0], [-5, 1, 0], [0, 2, 1], [5, 14, 2],
                  [7, 3, 3], [8, 2, 4]]),
        np.array([[0., 0, 0], [1, 1, 1], [2, 2, 2]]),
        np.array([[-20., -20, 0], [20, 20, 1]]),
        np.array([[3., 3, 3]]),
        np.array([[9.9999, 0, 0], [10.0001, 0, 0], [9.5, 0.5, 0]]),
    ]
    out['ct_n'] = np.array(len(trajs))
    for i, tr in enumerate(trajs):
        out[f'ct_in_{i}'] = tr
        out[f'ct_out_{i}'] = gen.crop_trajectory(tr.copy(), 20.)
    # warps
    a1, a2 = gen.cal_warp_params(19.7, 16, 31)
    b1, b2 = gen.cal_warp_params(13.8, 16, 31)
    out['wp_params'] = np.array([a1, a2, b1, b2])
    maps = rng.uniform(0, 1, (3, 32, 32))
    out['wp_in'] = maps
    out['wp_out'] = gen.warp_dense_probmaps(maps, a1, a2, b1, b2)
    pts = np.stack([rng.integers(0, 32, 40).astype(float),
                    rng.integers(0, 32, 40).astype(float),
                    np.zeros(40)], 1)
    out['ws_in'] = pts
    out['ws_out'] = gen.warp_sparse_points(pts.copy(), a1, a2, b1, b2, 16, 16,
                                           19.7, 13.8)
    # RGB BEV generator medians
    rgen = ref.RGBBEVGenerator(20, 16, 7)
    pc = random_sem_pc(rng, 1500, 9.9)
    pc[:, :2] = np.floor(pc[:, :2] / 20 * 16 + 8)
    out['rg_pc'] = pc
    r, g, b = rgen.get_rgb_maps(pc)
    out['rg_out'] = np.stack([r, g, b])
    np.savez_compressed(os.path.join(out_dir, 'utils.npz'), **out)
    print('utils written')


def case_sweeps(ref, out_dir):
    """The reference's inst_centric_get_sweeps + load_data_to_tensor on a fake dataset object (tests/fake_nuscenes.py):
    inputs (the tables) and outputs (points, tokens, centres, last boxes, class indices)."""
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    import fake_nuscenes as fk
    ref.nu.Quaternion = fk.FakeQuaternion          # pyquaternion stand-in (textbook formula; third-party, unpinned)
    tables = fk.synth_tables()
    with tempfile.TemporaryDirectory() as tmp:
        nusc = fk.FakeNuScenes(tables, tmp)
        res = ref.nu.inst_centric_get_sweeps(nusc, 'sample0', **fk.SWEEP_CFG)
        ref.nu.load_data_to_tensor(res)
    out = {'in_' + k: np.asarray(v) for k, v in tables.items()}
    out['points'] = res['points'].numpy()
    out['instances_token'] = np.array(res['instances_token'])
    out['instances_center'] = np.stack(res['instances_center'])
    out['instances_last_box'] = res['instances_last_box'].numpy()
    out['instances_name'] = res['instances_name'].numpy()
    assert (out['points'][:, 6] >= 0).sum() > 50 and len(set(res['instances_token'])) >= 4
    np.savez_compressed(os.path.join(out_dir, 'nusc_sweeps.npz'), **out)
    print('nusc_sweeps written:', out['points'].shape, len(res['instances_token']), 'labelled boxes')


def case_sweeps_edges(ref, out_dir):
    """The reference's inst_centric_get_sweeps + load_data_to_tensor on the scenarios of tests/nusc_sweeps_edges_common.py
    (points on box faces and on the radius circle with their f32 neighbours; empty file, sweep without box, tile-sized
    sweeps, overlapping boxes, a track opened by a later box): the tables and the recorded outputs, per scenario."""
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    import fake_nuscenes as fk
    import nusc_sweeps_edges_common as ec
    ref.nu.Quaternion = fk.FakeQuaternion          # pyquaternion stand-in (textbook formula; third-party, unpinned)
    out = {}
    for name in sorted(ec.SCENARIOS):
        tables = ec.TABLES[name]()
        with tempfile.TemporaryDirectory() as tmp:
            nusc = fk.FakeNuScenes(tables, tmp)
            res = ref.nu.inst_centric_get_sweeps(nusc, 'sample0', **ec.cfg(name))
            ref.nu.load_data_to_tensor(res)
        ec.store_tables(out, name, tables)
        out[name + '_points'] = res['points'].numpy()
        out[name + '_instances_token'] = np.array(res['instances_token'])
        out[name + '_instances_center'] = np.stack(res['instances_center'])
        out[name + '_instances_last_box'] = res['instances_last_box'].numpy()
        out[name + '_instances_name'] = res['instances_name'].numpy()
        print('nusc_sweeps_edges', name, out[name + '_points'].shape, list(res['instances_token']))
    print('  scenario a (face labelled, face unlabelled, circle kept, circle dropped) per record:',
          ec.coverage_a(ec.TABLES['a'](), out['a_points']))
    pb = out['b_points']
    assert [int((pb[:, 5] == k).sum()) for k in range(4)] == list(ec.KEPT_B)
    toks = list(out['b_instances_token'])
    assert toks.count('inst2') == 1 and 'inst6' in toks and 'inst0' in toks
    path = os.path.join(out_dir, 'nusc_sweeps_edges.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 400 * 1000, os.path.getsize(path)
    print('nusc_sweeps_edges written:', os.path.getsize(path), 'bytes')


def case_k1_edges(ref, out_dir):
    """The reference's velo2img / gen_semantic_pc / filter_semseg_pc on the frames of tests/k1_edges_common.py (points at the
    frustum's planes and their f32 neighbours, a ladder of magnitudes up to FLT_MAX, special values): one file per camera with
    the points, the per-point mask, u / v of the masked points and the indices kept after the class filter.  The image and
    the class map are drawn from the case's seed and not stored.  The intensity column carries the point's index through the
    reference (it copies the column; the stored points hold the case's own intensities)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    import k1_edges_common as kc
    for name in kc.CASES:
        fr = kc.frame(name)
        pts, P, H, W, filters, seed = fr.case()
        img, sem = kc.image_of(seed, H, W)
        acc = ref.kitti.Kitti360SemanticPointCloudAccumulator(
            8., {'h_velo_cam': np.eye(4), 'p_cam_frame': P, 'p_velo_frame': P}, 1e3, None, filters, SEM_IDXS, True, BEV_PARAMS_KITTI)
        n = pts.shape[0]
        tagged = pts.astype(np.float64)
        tagged[:, 3] = np.arange(n)
        with np.errstate(all='ignore'):
            vi = acc.velo2img(tagged.copy(), P, H, W)
            rgb = acc.gen_semantic_pc(tagged.copy(), img, P)
            cls = acc.gen_semantic_pc(tagged.copy(), sem.astype(np.int64)[..., None], P)
            kept = acc.filter_semseg_pc(np.concatenate((rgb, cls[:, -1:]), axis=1))
        idx = vi[:, 3].astype(np.int64)
        assert np.array_equal(tagged[idx, :3], vi[:, :3]) and np.array_equal(rgb[:, 3], vi[:, 3]) and np.array_equal(cls[:, 3], vi[:, 3])
        mask = np.zeros(n, bool)
        mask[idx] = True
        assert np.array_equal(np.flatnonzero(mask), idx)                 # the reference keeps the order
        u, v = vi[:, 4].astype(np.int64), vi[:, 5].astype(np.int64)
        assert np.array_equal(rgb[:, 4:7], img[v, u]) and np.array_equal(cls[:, 4], sem[v, u])
        out = dict(pts=pts, mask=mask, u=u.astype(np.int16), v=v.astype(np.int16), kept=kept[:, 3].astype(np.int32))
        path = os.path.join(out_dir, f'k1_edges_{name}.npz')
        np.savez_compressed(path, **out)
        print(f'k1_edges_{name}: {n} points, {int(mask.sum())} in the image, {len(kept)} kept, {os.path.getsize(path)} bytes')


def case_sem_planes(ref, out_dir):
    """Class-group planes: the reference's gen_sem_probmap / gen_gridmap_count_map of the static partition for five class
    groups and the three point sets (tests/golden/sem_planes.npz).  Augmented frame with a height filter; dyn = 1 rows, rows
    above the filter, rows on the crop edge and a row one ulp inside +view/2 are part of the data."""
    rng = np.random.default_rng(808)
    view, px, hf = 20, 32, 1.5
    rot, dx, dy, zoom = 0.7, 1.5, -2.25, 1.1
    aug = zoom * view
    gen = ref.SemBEVGenerator(SEM_IDXS, view, px, 0., 0., False, 20., 20., 0.5, hf)
    gen.sem_idxs = {c: c for c in range(256)}          # groups are integer classes: the reference's own lookup, identity
    groups = [[1], [13, 14, 15, 17], [0, 2, 8], [200, 201], [0, 255]]
    classes = (0, 0, 0, 1, 1, 2, 8, 9, 13, 14, 15, 17, 5, 255)
    R = gen.rotation_matrix_3d(rot)

    def make(n):
        rows = np.zeros((n, 10))
        rows[:, :2] = rng.uniform(-14., 14., (n, 2))
        rows[:, 2] = rng.integers(-8, 13, n) / 4.      # -2 .. 3: a quarter of them at or above the filter
        rows[:, 3] = rng.integers(0, 65, n) / 64.
        rows[:, 4:7] = rng.integers(0, 256, (n, 3))
        rows[:, 7] = rng.choice(classes, n)
        rows[:, 8] = rng.integers(-1, 4, n)
        rows[:, 9] = (rng.random(n) < 0.1).astype(float)
        # crop edges: ladders of neighbouring doubles around the points that land on +-view/2
        vhi = 0.5 * aug
        k = 0
        for axis, target in ((0, vhi), (0, np.nextafter(vhi, -np.inf)), (0, -vhi), (1, vhi), (1, -vhi)):
            t = np.array([0.3 * vhi, -0.2 * vhi])
            t[axis] = target
            xy = (t - [dx, dy]) @ R[:2, :2]
            for step in range(-12, 13):
                r = rows[k]
                r[:2] = xy
                for _ in range(abs(step)):
                    r[axis] = np.nextafter(r[axis], np.inf if step > 0 else -np.inf)
                r[2], r[7], r[9] = 0.25, classes[k % len(classes)], 0.
                k += 1
        return rows[rng.permutation(n)]

    present, future = make(1500), make(1200)
    sets = dict(present=present, future=future, full=np.concatenate([present, future]))
    out = dict(pc_present=present, pc_future=future, cfg=np.array([view, px, hf, rot, dx, dy, zoom]),
               groups=np.array([g + [-1] * (4 - len(g)) for g in groups], dtype=np.int16))
    on_edge = inside = 0
    for name, rows in sets.items():
        xyz = np.matmul(R, rows[:, :3].copy().T).T      # (what geometric_transform computes, to count the edge rows)
        tx = xyz[:, 0] + dx
        on_edge += int((np.abs(tx) == 0.5 * aug).sum())
        inside += int((tx == np.nextafter(0.5 * aug, -np.inf)).sum())
        grid, _ = gen.preprocess_pc_and_trajs(rows.copy(), [], rot, dx, dy, aug)
        assert (grid[:, 0:2] >= 0).all() and (grid[:, 0:2] <= px).all()
        _, static = gen.partition_semantic_pc(grid, [1], 9)
        if name != 'full':
            out[f'grid_{name}'] = grid
        prob = np.stack([gen.gen_sem_probmap(static, g) for g in groups])
        out[f'prob_{name}'] = prob
        out[f'prob16_{name}'] = prob.astype(np.float16)
        out[f'count_{name}'] = gen.gen_gridmap_count_map(static)
        for k, g in enumerate(groups):
            sem, _ = gen.partition_semantic_pc(static, g, 7)
            out[f'count_{name}_g{k}'] = gen.gen_gridmap_count_map(sem).astype(np.uint32)
        assert name == 'full' or ((grid[:, 9] == 1).sum() > 20 and (rows[:, 2] >= hf).sum() > 100)
    assert on_edge >= 4 and inside >= 1, (on_edge, inside)
    assert (out['grid_present'][:, 0] == px).any() or (out['grid_future'][:, 0] == px).any()   # one ulp inside floors to px
    assert out['count_full_g3'].sum() == 0 and out['count_full_g4'].sum() > 0
    path = os.path.join(out_dir, 'sem_planes.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 200 * 1024, os.path.getsize(path)
    print('sem_planes:', {k: v.shape[0] for k, v in sets.items()}, 'rows,', on_edge, 'on the crop edge,', inside,
          'one ulp inside,', os.path.getsize(path), 'bytes')


def case_elev_partition(ref, out_dir):
    """The reference's static_obj_partitioning_by_elev (sem_bev.py:556-591) on a three-frame window, behind its own
    preprocess_pc_and_trajs and -- for the static-only cases -- partition_semantic_pc: tests/golden/elev_partition.npz.
    Thresholds 0.2, 0.0 and -0.1, with and without a height filter, with and without the dyn == 1 rows; variant 'z0' has
    origin z = 0 (stored z of -0.0).  Column 3 of every row is its index in the window.  Reserved cells hold hand-made rows
    only: a minimum m, a row at fl(m + 0.2) and its two neighbours; single rows; the -0.0 rows.  See the case list and the
    names in tests/elev_partition_common.py."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    import elev_partition_common as ec
    rng = np.random.default_rng(556)
    view, px, hf = 10, 20, 1.5
    rot, dx, dy = 0.3, 0.15, -0.1
    origins = dict(a=np.array([3.25, -1.5, 0.6]), z0=np.array([3.25, -1.5, 0.0]))
    oz = origins['a'][2]
    R = ec.rotation(rot)
    frames = [[], [], []]

    def add(f, i, j, Z, c8=0., dyn=0., jitter=0.3):
        t = (np.array([i, j]) + 0.5 + rng.uniform(-jitter, jitter, 2) - 0.5 * px) * view / px
        xy = (t - [dx, dy]) @ R[:2, :2] + origins['a'][:2]
        row = np.zeros(10)
        row[0:2], row[2] = xy, Z
        row[4:7], row[7] = rng.integers(0, 256, 3), rng.integers(0, 19)
        row[8], row[9] = c8, dyn
        frames[f].append(row)

    def stored_z(target):
        """A stored Z with fl(Z - origin z) == target, searched in ulps around target + origin z; None if there is none."""
        z0 = target + oz
        for k in sorted(range(-16, 17), key=abs):
            Z = z0
            for _ in range(abs(k)):
                Z = np.nextafter(Z, np.inf if k > 0 else -np.inf)
            if Z - oz == target:
                return Z
        return None

    edge_i, edge_j = (0, 7, 8, 15, 16, 19), (0, 3, 4, 11, 12, 19)      # image rows 19 | 16, 15 | 8, 7 | 0
    free = [(i, j) for i in range(px) for j in range(px) if i not in edge_i and j not in edge_j]
    reserved = [free[k] for k in rng.permutation(len(free))[:64]]
    boundary, single, zeros = reserved[:44], reserved[44:58], reserved[58:64]
    n_boundary = 0
    for n, (i, j) in enumerate(boundary):
        m = rng.integers(-1900, -1000) / 1000.
        Zm = stored_z(m)
        target = m + 0.2
        Zs = [stored_z(target), stored_z(np.nextafter(target, np.inf)), stored_z(np.nextafter(target, -np.inf))]
        if Zm is None or any(Z is None for Z in Zs):
            continue                                               # (the cell stays empty)
        n_boundary += 1
        f_min, f_hi = (2, 0) if n % 2 else (0, 2)                  # both orders: the minimum after / before the rows it decides
        add(f_min, i, j, Zm)
        for Z, c8 in zip(Zs, (0., 2., 0.)):
            add(f_hi, i, j, Z, c8=c8)
        add(1, i, j, Zm + 0.7, c8=float(n % 3))                    # clearly elevated, whatever its column 8
        add(1, i, j, Zm + 0.05, c8=float((n + 1) % 3))             # clearly not
    for n, (i, j) in enumerate(single):
        add(n % 3, i, j, rng.integers(-1500, 1000) / 1000. + oz)
    for n, (i, j) in enumerate(zeros):                             # z0: the cell's minimum is a stored -0.0
        add(0, i, j, -0.0)
        add(2 if n % 2 else 0, i, j, 0.0 if n < 3 else 0.5)
        add(1, i, j, 0.25, c8=2.)
    for i in range(px):
        for j in range(px):
            if i in edge_i[1:5] or j in edge_j[1:5] or (i in (0, px - 1) and j in (0, px - 1)):   # both sides of every tile edge, the corners
                add(int(rng.integers(0, 3)), i, j, rng.integers(-1500, 1400) / 1000. + oz, c8=float(rng.integers(0, 3)))
    n_designed = sum(len(f) for f in frames)
    taken = set(reserved)
    while sum(len(f) for f in frames) < 1500:                      # the rest: random rows, also beyond the view and above the filter
        i, j = int(rng.integers(-2, px + 2)), int(rng.integers(-2, px + 2))
        if (i, j) in taken:
            continue
        add(int(rng.integers(0, 3)), i, j, rng.integers(-2000, 3000) / 1000. + oz, c8=float(rng.integers(0, 3)),
            dyn=float(rng.random() < 0.15), jitter=0.45)
    frames = [np.stack(f)[rng.permutation(len(f))] for f in frames]
    k = 0
    for f in frames:                                               # column 3: the row's index in the window
        f[:, 3] = np.arange(k, k + f.shape[0])
        k += f.shape[0]
    n_rows = k
    out = dict(frame0=frames[0], frame1=frames[1], frame2=frames[2], origin_a=origins['a'], origin_z0=origins['z0'],
               cfg=np.array([view, px, hf, rot, dx, dy]))
    grids = {}
    for name, variant, use_hf, static_only, kt in ec.CASES:
        gname = ec.grid_name(name)
        if gname not in grids:
            gen = ref.SemBEVGenerator(SEM_IDXS, view, px, 0., 0., False, 20., 20., 0.5, hf if use_hf else None)
            rows = np.concatenate(frames)
            rows[:, :3] = rows[:, :3] - origins[variant]           # kitti360_sem_pc_accum.py:193
            grid, _ = gen.preprocess_pc_and_trajs(rows, [], rot, dx, dy, float(view))
            if static_only:
                _, grid = gen.partition_semantic_pc(grid, [1], 9)
            assert (grid[:, 0:2] >= 0).all() and (grid[:, 0:2] < px).all()        # no cell index equal to px
            assert not (np.signbit(grid[:, 2]) & (grid[:, 2] == 0)).any()         # no pre-gridded z of -0.0
            grids[gname] = (gen, grid)
            out[gname] = grid
        gen, grid = grids[gname]
        work = grid.copy()
        pc_static, pc_dynamic, elevmap, mask = gen.static_obj_partitioning_by_elev(work, ec.THRESHOLDS[kt])
        assert np.array_equal(pc_static, work[work[:, 8] == 0]) and np.array_equal(pc_dynamic, work[work[:, 8] == 1])
        fate = np.full(n_rows, ec.FATE_OUT, dtype=np.int8)
        fate[work[:, 3].astype(int)] = np.where(work[:, 8] == 0, ec.FATE_STATIC,
                                                np.where(work[:, 8] == 1, ec.FATE_DYNAMIC, ec.FATE_NEITHER))
        out[f'elev_{name}'], out[f'mask_{name}'], out[f'fate_{name}'] = elevmap, mask, fate
    # what the reference delivers for a stored -0.0 under origin z 0: +0.0 in the map
    emap, mask = out['elev_z0_hf0_dyn1_t0'], out['mask_z0_hf0_dyn1_t0']
    for i, j in zeros:
        assert mask[px - 1 - j, i] and emap[px - 1 - j, i] == 0. and not np.signbit(emap[px - 1 - j, i]), (i, j)
    assert n_boundary >= 30, n_boundary
    path = os.path.join(out_dir, 'elev_partition.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 400 * 1024, os.path.getsize(path)
    print('elev_partition:', [f.shape[0] for f in frames], 'rows,', n_designed, 'designed,', n_boundary, 'boundary cells,',
          len(single), 'single-row cells,', os.path.getsize(path), 'bytes')


def lanes_map_and_views():
    """The hand-built lane map and views of tests/golden/lanes.npz (design coordinates are those of the 'world' frame; the
    map is handed to the reference in 'global' coordinates, T_global_world brings it back -- up to rounding, which is why
    the views that need a vertex exactly on their border are sized from the transformed vertex itself, in case_lanes)."""
    rng = np.random.default_rng(101)
    c, s_ = np.cos(0.3), np.sin(0.3)
    # planar, as the inverse of an ego pose with yaw only
    T = np.array([[c, -s_, 0., 300.], [s_, c, 0., 200.], [0., 0., 1., 0.5], [0., 0., 0., 1.]])
    views = [  # origin, rot, dx, dy, zoom, px, view_size
        ((0., 0., 0.), 0., 0., 0., 1., 64, 40.),
        ((3.5, -2.25, 0.5), 0.7, 1.5, -0.75, 1.07, 256, 40.),
        ((-6., 4., 1.), 0.5 * np.pi, -2., 0.5, 0.9, 7, 40.),
        ((1., 1., 0.), -2.1, 0.3, 0.4, 1., 64, 40.),
        ((0., 0., 0.), 0., 0., 0., 1.07, 256, 40.),
        ((10., -12., 0.3), 0.7, 0., 0., 0.9, 7, 40.),
        ((500., 500., 0.), 0.7, 0., 0., 1., 64, 40.),          # no lane survives
        ((0., 0., 0.), 0.7, 0., 0., 1., 256, 400.),            # every finite vertex is inside
        ((-3., 7., 0.), 0.5 * np.pi, 2.5, -1.5, 1.07, 64, 40.),
        ((5., 5., 0.5), -2.1, 0., 0., 0.9, 256, 40.),
        ((-2., 3., 0.), 0., 4.25, -3.5, 0.9, 7, 40.),
        ((0., 0., 0.), 0.7, 0., 0., 1., 64, 40.),
    ]

    def rot2(ang):
        return np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])

    def to_world(v, pts):
        """Design points given in the (metric) frame of view v -> world."""
        origin, rot, dx, dy = v[0], v[1], v[2], v[3]
        pts = np.array(pts, dtype=np.float64)
        out = pts.copy()
        out[:, :2] = (pts[:, :2] - [dx, dy]) @ rot2(rot) + origin[:2]      # inverse of the rotation: R^T p as rows p R
        out[:, 2] = pts[:, 2] + origin[2]
        return out

    lanes, names = [], {}

    def add(name, pts):
        names[name] = len(lanes)
        lanes.append(np.array(pts, dtype=np.float64).reshape(-1, 3))

    add('len0', np.zeros((0, 3)))
    add('len1', [[1., 2., 0.1]])
    add('len2', [[-3., 2., 0.2], [-2., 3., 0.3]])
    add('len3', [[4., -5., 0.1], [5., -6., 0.], [6., -5.5, -0.1]])
    add('inside', np.c_[np.linspace(-8, 8, 10), 3 * np.sin(np.linspace(0, 3, 10)), np.linspace(0, 1, 10)])
    add('outside', np.c_[np.linspace(42, 55, 10), np.linspace(44, 47, 10), np.zeros(10)])
    add('zigzag', np.c_[np.linspace(-12, 12, 12), np.where(np.arange(12) % 2, 26., 15.), np.linspace(-0.3, 0.3, 12)])
    add('through', [[-35., 3., 0.1], [35., 4., 0.2], [36., 30., 0.3]])
    add('long_in_out', [[2., 1., 0.4], [70., 33., 0.5]])
    add('long_out_in', [[-80., -5., 0.6], [1., -2., 0.7], [2., -3., 0.8]])
    add('tiny_x', [[19.5, 5., 0.1], [19.99999, 5., 0.2], [20.00001, 5.000001, 0.3], [20.5, 5., 0.4]])
    add('tiny_y', [[-7., -19.5, 0.1], [-7., -19.999992, 0.2], [-7.000001, -20.000009, 0.3], [-7., -19.5, 0.4]])
    add('nan_mid', [[6., 6., 0.1], [7., 7., 0.2], [8., 8., 0.3], [9., 7., 0.4], [10., 6., 0.5]])
    add('inf_mid', [[-6., 6., 0.1], [-7., 7., 0.2], [-8., 8., 0.3], [-9., 7., 0.4], [-10., 6., 0.5]])
    add('border_xp', [[1., 2., 0.1], [13.3, 3., 0.2], [2., 1., 0.3]])
    add('border_xm', [[-1., 2., 0.1], [-11.7, -3., 0.2], [-2., 1., 0.3]])
    add('border_yp', [[1., 2., 0.1], [3., 12.1, 0.2], [2., 1., 0.3]])
    add('border_ym', [[1., -2., 0.1], [-3., -14.9, 0.2], [2., -1., 0.3]])
    v1 = views[1]
    h1 = 0.5 * v1[4] * v1[6]
    lanes.append(to_world(v1, [[h1 - 0.5, 2., 0.1], [h1 - 0.00001, 2., 0.2], [h1 + 0.00001, 2., 0.3], [h1 + 1., 2., 0.4]]))
    names['tiny_v1'] = len(lanes) - 1
    lanes.append(to_world(v1, [[-3., -4., 0.1], [1.6 * 42.8, 11., 0.2], [-60., -70., 0.3], [0., 1., 0.4]]))
    names['long_v1'] = len(lanes) - 1
    for k in range(120):
        n = int(rng.integers(2, 13))
        start = np.r_[rng.uniform(-35, 35, 2), rng.uniform(-0.5, 0.5)]
        steps = np.c_[rng.normal(0, 3, (n, 2)), rng.normal(0, 0.05, n)]
        steps[0] = 0
        lanes.append(start + np.cumsum(steps, axis=0))
    world_design = lanes
    Ti = np.linalg.inv(T)
    glob = []
    for lane in world_design:
        glob.append(lane @ Ti[:3, :3].T + Ti[:3, 3])
    glob[names['nan_mid']][2, 0] = np.nan
    glob[names['inf_mid']][2, 0] = np.inf
    return T, glob, views, names


def case_lanes(ref, out_dir):
    """GT lane centrelines through the reference itself: homo_transform per lane (nuscenes_oracle_sem_pc_accum.py:173-176),
    lane - bev_frame_coords (:552-554), then BEVGenerator.preprocess_pc_and_trajs on a dummy cloud with every lane and the
    non-empty filter (bev_generator.py:101-109), for every view: tests/golden/lanes.npz.  Data only: the map ('global' and
    'world' vertices, packed, with the lanes' first vertices), T, the views and per view the surviving lanes' rows, packed,
    with their lengths."""
    T, glob, views, names = lanes_map_and_views()
    world = [ref.nu.homo_transform(T, lane) for lane in glob]
    # A stored z of -0.0 cannot come out of homo_transform (numpy's product adds onto +0.0), so the lanes that hold one are
    # a second, tiny set in 'world' coordinates that goes through the same subtraction and preprocess_pc_and_trajs:
    # p - origin in the (+, +) quadrant, where the rotation's 0 x + 0 y is +0.0, and in the (-, -) quadrant, where every
    # product is a -0.0: the z comes out +0.0 in both (numpy adds the products onto +0.0)
    nz = [np.array([[3., 4., -0.0], [4., 5., 0.25], [30., 5., -0.0]]), np.array([[-3., -4., -0.0], [-4., -5., -0.0], [-30., -5., 0.25]])]
    # views with a vertex exactly on +-view/2 (outside), and with the border one ulp beyond it (inside): origin 0, no
    # rotation, no shift, zoom 1, sized from the transformed vertex
    n_general = len(views)
    for name, axis in (('border_xp', 0), ('border_xm', 0), ('border_yp', 1), ('border_ym', 1)):
        cval = abs(world[names[name]][1, axis])
        views.append(((0., 0., 0.), 0., 0., 0., 1., 64, 2. * cval))
        views.append(((0., 0., 0.), 0., 0., 0., 1., 64, 2. * np.nextafter(cval, np.inf)))
    start = np.zeros(len(glob) + 1, dtype=np.int32)
    np.cumsum([g.shape[0] for g in glob], out=start[1:])
    out = dict(T=T, start=start, xyz_global=np.concatenate(glob), xyz_world=np.concatenate(world),
               names=np.array(sorted(names, key=names.get)), name_lane=np.array(sorted(names.values()), dtype=np.int32))
    table, Rs = [], []
    survivors = []
    for k, (origin, rot, dx, dy, zoom, px, view_size) in enumerate(views):
        gen = ref.SemBEVGenerator(SEM_IDXS, view_size, px, 0., 0., False, 20., 20., 0.5, None)
        origin = np.array(origin)
        lanes_k = [lane - origin for lane in world]                                    # :552-554
        # which lanes survive: the reference drops the empty ones; their indices come from a marker run on copies
        dummy = np.zeros((1, 10))
        with np.errstate(invalid='ignore'):
            _, res = gen.preprocess_pc_and_trajs(dummy, [lane.copy() for lane in lanes_k], rot, dx, dy, zoom * view_size)
        kept = [i for i, lane in enumerate(res) if lane.shape[0] > 0]
        res = [lane for lane in res if lane.shape[0] > 0]                              # bev_generator.py:107-109
        out[f'rows_{k}'] = np.concatenate(res) if res else np.zeros((0, 3))
        out[f'len_{k}'] = np.array([lane.shape[0] for lane in res], dtype=np.int32)
        out[f'kept_{k}'] = np.array(kept, dtype=np.int32)
        table.append([origin[0], origin[1], origin[2], rot, dx, dy, zoom, px, view_size])
        Rs.append(gen.rotation_matrix_3d(rot))
        survivors.append(kept)
    out['views'], out['R'] = np.array(table), np.stack(Rs)
    # the cases the map was built for, checked on what the reference returned
    def rows_of(k, name):
        i = names[name]
        if i not in survivors[k]:
            return np.zeros((0, 3))
        j = survivors[k].index(i)
        o = int(out[f'len_{k}'][:j].sum())
        return out[f'rows_{k}'][o:o + out[f'len_{k}'][j]]
    assert len(survivors[6]) == 0 and len(survivors[7]) == sum(g.shape[0] >= 2 for g in glob)
    assert rows_of(0, 'inside').shape[0] == 9 and rows_of(0, 'outside').shape[0] == 0
    assert rows_of(0, 'through').shape[0] == 0                     # both ends outside: nothing, although it passes through
    assert rows_of(0, 'zigzag').shape[0] >= 3 * 3                  # in and out again and again
    assert rows_of(0, 'long_in_out').shape[0] == 2 and rows_of(0, 'long_out_in').shape[0] == 2
    assert rows_of(0, 'tiny_x').shape[0] == 3 and rows_of(0, 'tiny_y').shape[0] == 4
    assert rows_of(1, 'tiny_v1').shape[0] == 3 and rows_of(1, 'long_v1').shape[0] == 3
    out['nz_xyz'], out['nz_start'] = np.concatenate(nz), np.array([0, 3, 6], dtype=np.int32)
    for k in (0, 3):
        origin, rot, dx, dy, zoom, px, view_size = views[k]
        gen = ref.SemBEVGenerator(SEM_IDXS, view_size, px, 0., 0., False, 20., 20., 0.5, None)
        _, res = gen.preprocess_pc_and_trajs(np.zeros((1, 10)), [lane - np.array(origin) for lane in nz], rot, dx, dy,
                                             zoom * view_size)
        assert all(lane.shape[0] > 0 for lane in res)
        out[f'nz_rows_{k}'] = np.concatenate(res)
        out[f'nz_len_{k}'] = np.array([lane.shape[0] for lane in res], dtype=np.int32)
    z = out['nz_rows_0'][0, 2]
    assert z == 0 and not np.signbit(z)
    z = out['nz_rows_0'][out['nz_len_0'][0], 2]
    assert z == 0 and not np.signbit(z)
    assert rows_of(0, 'nan_mid').shape[0] == 5 and np.isnan(rows_of(0, 'nan_mid')[2, 0])
    assert rows_of(0, 'inf_mid').shape[0] == 5 and not np.isfinite(rows_of(0, 'inf_mid')[2, :2]).all()
    for j, name in enumerate(('border_xp', 'border_xm', 'border_yp', 'border_ym')):
        assert rows_of(n_general + 2 * j, name).shape[0] == 3, name        # on the border: outside, two crossings
        assert rows_of(n_general + 2 * j + 1, name).shape[0] == 2, name    # one ulp inside: no crossing
    path = os.path.join(out_dir, 'lanes.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 256 * 1024, os.path.getsize(path)
    print('lanes:', len(glob), 'lanes,', int(start[-1]), 'vertices,', len(views), 'views, survivors',
          [len(s) for s in survivors], os.path.getsize(path), 'bytes')


def save_npz_reproducible(path, out):
    """np.savez_compressed with a fixed member date and order, so that a second run writes the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(out[key]), allow_pickle=False)


def case_nusc_front_edges(ref, out_dir):
    """The NuScenes front end at its edges (tests/nusc_front_edges_common.py): homo_transform, NuScenesCamera.project_pts3d and
    the camera loop, shaped as case_utils restates it, on every K0n scene -- per rig the indices the search chose, pc_in_ego, uv,
    cam_idx, every camera's own mask and per family the largest distance from its bound in ulps, beside the rig's matrices;
    pts_feat_from_img 'nearest' on image and class map camera by camera and homo_transform on every K1n scene without an
    offender -- the stored rows (who goes to which camera and who is dropped is this file's own numpy); pts_feat_from_img 'bilinear' on a 2-D map at the sampler's coordinates, integer ones included."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
    import nusc_front_edges_common as ec
    nu = ref.nu
    out = {}
    for name in ec.RIGS:
        sel = ec.select(name)
        sc = ec.k0n_scene(name, sel)
        r, pc = sc['rig'], sc['pc']
        n, ncam = pc.shape[0], len(r['wh'])
        with np.errstate(all='ignore'):
            pc_in_ego = nu.homo_transform(r['ego_from_lidar'], pc)
            pc_in_glob = nu.homo_transform(r['glob_from_ego'], pc_in_ego)
            pc_uv = np.zeros((n, 2))
            pc_cam_idx = -np.ones(n, dtype=int)
            masks = np.zeros((ncam, n), bool)
            ulps = np.zeros(ncam * len(ec.BOUNDS))
            for j in range(ncam):
                cam = nu.NuScenesCamera.__new__(nu.NuScenesCamera)
                cam.img_wh, cam.cam_K = r['wh'][j].copy(), r['K'][j].copy()
                assert np.array_equal(np.linalg.inv(r['glob_from_cam'][j]), r['cam_from_glob'][j])     # (what the fixture keeps)
                pc_in_cam = nu.homo_transform(np.linalg.inv(r['glob_from_cam'][j]), pc_in_glob)
                uvj, m = cam.project_pts3d(pc_in_cam)
                pc_uv[m] = uvj[m]
                pc_cam_idx[m] = j
                masks[j] = m
                for b, bound in enumerate(ec.BOUNDS):
                    s = sc['sections']['fam_%d_%s' % (j, bound)]
                    val, inside = ec.bound_side(r, j, bound, uvj[s], pc_in_cam[s, 2])
                    assert np.array_equal(inside, m[s]), (name, j, bound)      # nothing but this bound decides a family's points
                    bv = ec.bound_value(r, j, bound)
                    ulps[j * len(ec.BOUNDS) + b] = np.max(np.abs(val - bv)) / np.spacing(bv)
        p = 'k0n_%s_' % name
        for key in ('fam_idx', 'ovl_idx') + ec.RIG_KEYS:
            out[p + key] = sel[key]
        out[p + 'pc_in_ego'], out[p + 'uv'], out[p + 'cam_idx'] = pc_in_ego, pc_uv, pc_cam_idx.astype(np.int8)
        out[p + 'masks'] = np.packbits(masks, axis=1)
        out[p + 'fam_ulps'] = ulps
        print('nusc_front_edges k0n', name, n, 'points,', int((pc_cam_idx >= 0).sum()), 'assigned; largest distance per family (ulps): %.3g .. %.3g'
              % (ulps.min(), ulps.max()))
    for name in ec.K1N_STACKS:
        sc = ec.k1n_scene(name)
        imgs, sems = ec.stack(name)
        pc, cam = sc['pc'], sc['cam']
        # the reference's own sampler per camera, on that camera's colour and class planes side by side; which points go to
        # which camera, what is dropped and in what order the rest stays are written here in the project's words
        feat = np.full((pc.shape[0], 4), -1.0)
        for c in range(imgs.shape[0]):
            of_c = np.flatnonzero(cam == c)
            feat[of_c] = nu.pts_feat_from_img(pc[of_c, 4:6], np.dstack([imgs[c], sems[c]]), 'nearest')
        keep = np.flatnonzero((feat >= 0).all(axis=1) & ~np.isin(feat[:, 3], sc['filters']))
        rows = np.zeros((len(keep), 10))
        rows[:, :3] = nu.homo_transform(sc['T'], pc[keep, :3])
        rows[:, 3], rows[:, 4:8], rows[:, 8] = pc[keep, 3], feat[keep], pc[keep, 6]
        p = 'k1n_%s_' % name
        out[p + 'pc'], out[p + 'cam_idx'], out[p + 'filters'], out[p + 'T'], out[p + 'rows'] = pc, cam, np.array(sc['filters']), sc['T'], rows
        out[p + 'kept'] = keep.astype(np.int32)
        print('nusc_front_edges k1n', name, pc.shape[0], 'points,', rows.shape[0], 'stored, filters', sc['filters'])
    fmap, uv = ec.bilinear_scene()
    with np.errstate(all='ignore'):
        out['bil_map'], out['bil_uv'], out['bil_out'] = fmap, uv, nu.pts_feat_from_img(uv, fmap, 'bilinear')
    path = os.path.join(out_dir, 'nusc_front_edges.npz')
    save_npz_reproducible(path, out)
    assert os.path.getsize(path) < 1000 * 1000, os.path.getsize(path)
    print('nusc_front_edges written:', os.path.getsize(path), 'bytes;', int(np.isnan(out['bil_out']).sum()), 'NaN of', len(uv), 'bilinear samples')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(
        os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    random.seed(0)
    np.random.seed(0)
    ref = import_reference()
    cases = dict(k1=case_k1, kitti=case_kitti_accum, bev=case_bev,
                 bev_edges=case_bev_edges, k1_edges=case_k1_edges, nusc=case_nusc,
                 utils=case_utils, sweeps=case_sweeps, sem_planes=case_sem_planes,
                 sweeps_edges=case_sweeps_edges, elev_partition=case_elev_partition,
                 lanes=case_lanes, nusc_front_edges=case_nusc_front_edges)
    for name, fn in cases.items():
        if args.only and name not in args.only.split(','):
            continue
        fn(ref, args.out)


if __name__ == '__main__':
    main()
