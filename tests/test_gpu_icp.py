"""Device point-to-plane ICP (replaces the reference's Open3D calls).  Parity with Open3D is
unpinned (third-party, unpinned version, absent here): the tests check (1) known ego motions on a ray-cast street
scene, (2) agreement with a k-d-tree numpy model of the same algorithm, (3) the accumulator's pose hook."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENSOR_H = 1.73
BOXES = []
for j in range(-3, 8):
    BOXES += [(12.0 * j, 9.0, 4.0, 2.5, 6.0), (12.0 * j + 6.0, -9.0, 4.0, 2.5, 6.0)]           # facades
    BOXES += [(12.0 * j + 3.0, 4.2, 2.1, 0.9, 1.5), (12.0 * j + 9.0, -4.2, 2.1, 0.9, 1.5)]       # parked cars
BOXES += [(20.0, 0.5, 0.3, 0.3, 3.0), (33.0, -1.5, 0.25, 0.25, 3.5), (8.0, -6.5, 0.2, 0.2, 4.0)]  # poles


def sweep(x, y, yaw, seed, n_beams=32, n_az=900, max_range=45.0):
    """Ray-casts a 32-beam lidar at world pose (x, y, yaw) over a ground plane and axis-aligned boxes fixed in the
    WORLD; returns points in the SENSOR frame (N,4)."""
    rng = np.random.default_rng(seed)
    az = np.repeat(np.linspace(-np.pi, np.pi, n_az, endpoint=False)[None], n_beams, 0).ravel()
    el = np.repeat(np.deg2rad(np.linspace(3.0, -24.0, n_beams))[:, None], n_az, 1).ravel()
    az = az + rng.normal(0, 2e-4, az.shape)
    d_s = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.]])
    d_w = d_s @ R.T
    o_w = np.array([x, y, 0.0])
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(d_w[:, 2] < 0, -SENSOR_H / d_w[:, 2], np.inf)
        for cx, cy, hx, hy, h in BOXES:
            lo = (np.array([cx - hx, cy - hy, -SENSOR_H]) - o_w) / d_w
            hi = (np.array([cx + hx, cy + hy, -SENSOR_H + h]) - o_w) / d_w
            tn = np.nanmax(np.minimum(lo, hi), 1)
            tf = np.nanmin(np.maximum(lo, hi), 1)
            hit = (tn <= tf) & (tn > 0) & (tn < t)
            t = np.where(hit, tn, t)
    ok = np.isfinite(t) & (t < max_range)
    t = t[ok] + rng.normal(0, 0.01, ok.sum())
    pts = d_s[ok] * t[:, None]
    return np.concatenate([pts, np.zeros((len(pts), 1))], 1).astype(np.float32)


def pose_T(x, y, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:2, 3] = [x, y]
    return T


def rot_err_deg(R):
    return np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def icp_model(src, tgt, max_iter=30, rel=1e-6):
    """The algorithm of csrc/pca_icp.hip with exact k-d-tree neighbours (scipy)."""
    from scipy.spatial import cKDTree
    src = src[:, :3].astype(np.float64)
    tgt = tgt[:, :3].astype(np.float64)
    tree = cKDTree(tgt)
    _, nb = tree.query(tgt, k=30)
    P = tgt[nb] - tgt[:, None, :]
    m = P.mean(1, keepdims=True)
    cov = np.einsum('nki,nkj->nij', P - m, P - m) / 30
    _, vec = np.linalg.eigh(cov)
    normals = vec[:, :, 0]
    T = np.eye(4)
    prev = None
    for it in range(max_iter + 1):
        q = src @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(q)
        fit, rmse = 1.0, np.sqrt(np.mean(d**2))
        if prev is not None and abs(prev[0] - fit) < rel and abs(prev[1] - rmse) < rel:
            break
        prev = (fit, rmse)
        if it == max_iter:
            break
        n = normals[j]
        r = np.einsum('ij,ij->i', q - tgt[j], n)
        J = np.concatenate([np.cross(q, n), n], 1)
        x = np.linalg.solve(J.T @ J, -J.T @ r)
        ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
        U = np.eye(4)
        U[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa], [-sb, cb * sa, cb * ca]]
        U[:3, 3] = x[3:]
        T = U @ T
    return T, rmse, it


@pytest.mark.parametrize('dx,dy,dyaw', [(1.0, 0.0, 0.0), (0.8, 0.05, 0.01), (1.5, -0.1, -0.02), (0.0, 0.0, 0.0)])
def test_icp_recovers_known_ego_motion(dx, dy, dyaw):
    from pca_amd.icp import GpuIcp
    prev = sweep(0.0, 0.0, 0.0, 1)
    new = sweep(dx, dy, dyaw, 2)
    icp = GpuIcp()
    res = icp.register(GpuIcp.to_device(prev), GpuIcp.to_device(new), 1e3, np.eye(4))
    T_true = np.linalg.inv(pose_T(dx, dy, dyaw))          # previous-sweep coordinates -> new-sweep coordinates
    assert np.linalg.norm(res.transformation[:3, 3] - T_true[:3, 3]) < 0.03, (res.transformation, T_true)
    assert rot_err_deg(res.transformation[:3, :3] @ T_true[:3, :3].T) < 0.1
    assert res.fitness > 0.95 and res.inlier_rmse < 0.5 and 1 <= res.iterations <= 30
    assert np.array_equal(res.transformation[3], [0, 0, 0, 1])
    again = icp.register(GpuIcp.to_device(prev), GpuIcp.to_device(new), 1e3, np.eye(4))
    np.testing.assert_allclose(again.transformation, res.transformation, rtol=0, atol=1e-9)   # sums: fixed order


@pytest.mark.parametrize('n_beams,n_az,max_range,tol', [(64, 700, 18.0, 1e-5), (96, 500, 14.0, 1e-5), (32, 900, 30.0, 1e-2)])
def test_icp_matches_kdtree_model(n_beams, n_az, max_range, tol):
    """Same algorithm with exact k-d-tree neighbours (scipy).  Where every 30-neighbourhood and every correspondence
    lies inside the device search caps (3 m / 4 m) the two agree to rounding; on the sparse far rings of the third
    scene the caps change a few (ill-conditioned, collinear) normals and the poses differ by millimetres."""
    from pca_amd.icp import GpuIcp
    prev = sweep(0.0, 0.0, 0.0, 5, n_beams=n_beams, n_az=n_az, max_range=max_range)
    new = sweep(0.9, 0.03, 0.008, 6, n_beams=n_beams, n_az=n_az, max_range=max_range)
    res = GpuIcp().register(GpuIcp.to_device(prev), GpuIcp.to_device(new), 1e3, np.eye(4))
    T_ref, rmse_ref, it_ref = icp_model(prev, new)
    assert np.linalg.norm(res.transformation[:3, 3] - T_ref[:3, 3]) < tol
    assert rot_err_deg(res.transformation[:3, :3] @ T_ref[:3, :3].T) < 60 * tol
    assert abs(res.inlier_rmse - rmse_ref) < tol
    if tol < 1e-3:
        assert res.iterations == it_ref


def test_icp_threshold_and_init_are_honoured():
    from pca_amd.icp import GpuIcp
    prev = sweep(0.0, 0.0, 0.0, 7)
    new = sweep(1.0, 0.0, 0.0, 8)
    icp = GpuIcp()
    tight = icp.register(GpuIcp.to_device(prev), GpuIcp.to_device(new), 0.05, np.eye(4))
    loose = icp.register(GpuIcp.to_device(prev), GpuIcp.to_device(new), 1e3, np.eye(4))
    assert tight.fitness < loose.fitness                  # 5 cm gate at 1 m offset: few correspondences
    good = np.linalg.inv(pose_T(1.0, 0.0, 0.0))
    warm = icp.register(GpuIcp.to_device(prev), GpuIcp.to_device(new), 1e3, good)
    assert warm.iterations <= loose.iterations
    assert np.linalg.norm(warm.transformation[:3, 3] - good[:3, 3]) < 0.03


def test_kitti_accumulator_uses_device_icp_when_asked(monkeypatch):
    """PCA_POSE_PROVIDER=gpu_icp: the unchanged integrate() path gets its T_new_prev from the device ICP."""
    import sem_pc_accum
    from kitti360_sem_pc_accum import Kitti360SemanticPointCloudAccumulator
    monkeypatch.setenv('PCA_POSE_PROVIDER', 'gpu_icp')
    monkeypatch.setattr(sem_pc_accum, 'SemSegONNX', lambda path: None)
    P = np.array([[552.554261, 0, 682.049453, 0], [0, 552.554261, 238.769549, 0], [0, 0, 1, 0.]]) @ np.linalg.inv(
        np.array([[0.04307104361, -0.08829286498, 0.995162929, 0.8043914418],
                  [-0.999004371, 0.007784614041, 0.04392796942, 0.2993489574],
                  [-0.01162548558, -0.9960641394, -0.08786966659, -0.1770225824], [0, 0, 0, 1]]))
    bev = dict(type='sem', view_size=40, pixel_size=32, max_trans_radius=0., zoom_thresh=0., do_warp=False,
               int_scaler=20., int_sep_scaler=20., int_mid_threshold=0.5, height_filter=None)
    acc = Kitti360SemanticPointCloudAccumulator(200., {'h_velo_cam': None, 'p_cam_frame': None, 'p_velo_frame': P}, 1e3,
                                                'none', [255], {'road': 0, 'car': 13}, True, bev)
    for k in range(5):
        pc = sweep(1.0 * k, 0.0, 0.004 * k, 20 + k)
        acc.integrate([(None, pc, np.zeros((len(pc), 1), dtype=np.int64))])
    poses = np.array(acc.poses)
    # the newest pose is the origin; the oldest lies ~4 m behind along -x of the current frame
    assert np.allclose(poses[-1], 0.0)
    assert abs(np.linalg.norm(poses[0]) - 4.0) < 0.1 and poses[0][0] < -3.8
    assert np.all(np.abs(np.diff(np.linalg.norm(poses, axis=1))) > 0.9)


def test_icp_degenerate_inputs_leave_the_initial_pose():
    """No correspondence inside the gate / sweeps outside the search grid / a handful of points: the initial transform
    comes back unchanged with fitness 0 (Open3D returns the init pose when the correspondence set is empty)."""
    from pca_amd.icp import GpuIcp
    icp = GpuIcp()
    a = sweep(0.0, 0.0, 0.0, 3)
    far = a.copy()
    far[:, 2] += 10.0
    init = pose_T(0.3, -0.2, 0.05)
    res = icp.register(GpuIcp.to_device(a), GpuIcp.to_device(far), 0.5, init)
    assert res.fitness == 0.0 and np.array_equal(res.transformation, init)
    outside = a.copy()
    outside[:, 0] += 500.0                                  # beyond the +-128 m grid
    res = icp.register(GpuIcp.to_device(outside), GpuIcp.to_device(outside), 1e3, np.eye(4))
    assert res.fitness == 0.0 and np.array_equal(res.transformation, np.eye(4))
    few = GpuIcp.to_device(a[:4])
    res = icp.register(few, few, 1e3, np.eye(4))
    assert np.array_equal(res.transformation, np.eye(4))
    xyz_only = GpuIcp.to_device(a[:, :3])                   # (N,3) input is padded to the [N,4] layout
    assert tuple(xyz_only.shape) == (len(a), 4)


@pytest.mark.parametrize('step,tol', [(1.0, 1e-5), (2.0, 1e-3), (3.0, 5e-3)])
def test_icp_search_cap_against_the_uncapped_model(step, tol):
    """The reference passes icp_threshold = 1e3 (kitti360_sem_pc_accum.py:115-127): every source point is matched with its
    nearest neighbour, however far.  The device search is capped at 4 m.  Against the same algorithm with UNCAPPED exact
    neighbours (scipy k-d tree), on sweep pairs 1, 2 and 3 m apart (36, 72, 108 km/h at 10 Hz): at 1 m the poses agree to
    1e-5 -- once the first iterations have pulled the sweeps together no nearest neighbour is farther than the cap; at 2 and
    3 m they differ by 0.37 mm and 2.2 mm (measured): the points at the sweeps' non-overlapping ends
    keep partners beyond 4 m at convergence, which pull on the uncapped optimum and are left out of the capped one.  Both stay
    within centimetres of the true motion (7 cm at the 3 m step).  (Dense scene: every 30-neighbourhood lies inside the normals' search cap.)"""
    from pca_amd.icp import GpuIcp
    prev = sweep(0.0, 0.0, 0.0, 11, n_beams=64, n_az=700, max_range=18.0)
    new = sweep(step, 0.04, 0.01, 12, n_beams=64, n_az=700, max_range=18.0)
    res = GpuIcp().register(GpuIcp.to_device(prev), GpuIcp.to_device(new), 1e3, np.eye(4))
    T_ref, rmse_ref, _ = icp_model(prev, new)
    assert np.linalg.norm(res.transformation[:3, 3] - T_ref[:3, 3]) < tol, (res.transformation, T_ref)
    assert rot_err_deg(res.transformation[:3, :3] @ T_ref[:3, :3].T) < 60 * tol
    T_true = np.linalg.inv(pose_T(step, 0.04, 0.01))
    assert np.linalg.norm(res.transformation[:3, 3] - T_true[:3, 3]) < 0.02 + 0.03 * step      # (7 cm at 3 m, either model)


def _register_pairs_for_child():
    """(run in a child process by the test below) poses, fitness, rmse, iterations of a few registrations, printed as hex."""
    import torch  # noqa: F401
    from pca_amd.icp import GpuIcp
    out = []
    for (x1, yaw1, seed, shift_z) in ((0.9, 0.010, 1, 0.0), (0.4, -0.02, 5, 0.0), (1.6, 0.03, 9, 6.5)):
        a = sweep(0.0, 0.0, 0.0, seed)
        b = sweep(x1, 0.05, yaw1, seed + 100)
        a[:, 2] += shift_z                                   # (the last pair sits in other slabs of the grids)
        b[:, 2] += shift_z
        r = GpuIcp().register(GpuIcp.to_device(a), GpuIcp.to_device(b), 1e3, np.eye(4))
        out.append(np.concatenate([r.transformation.ravel(), [r.fitness, r.inlier_rmse, float(r.iterations)]]))
    print('ICPHEX ' + np.stack(out).astype(np.float64).tobytes().hex())


def test_icp_shortcut_is_bit_identical_to_searching_every_pass():
    """From the third pass on a query keeps its partner without a search when it provably is still the unique nearest target
    (csrc/pca_icp.hip, icp_match).  PCA_ICP_NO_SKIP=1 (read once per process) searches every query in every pass: poses,
    fitness, rmse and iteration counts of both forms are equal, and the shortcut does take place (PCA_ICP_DBG=1
    prints the searched queries per pass).  "Equal": see the comment at the comparison."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_icp as t; t._register_pairs_for_child()'
            % (here, os.path.join(os.path.dirname(here), 'pc-accumulation-lib_amd')))
    res = {}
    for name, extra in (('skip', {'PCA_ICP_DBG': '1'}), ('search', {'PCA_ICP_NO_SKIP': '1', 'PCA_ICP_DBG': '1'})):
        r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('ICPHEX ')][-1]
        counts = [[float(v) for v in ln.split(':')[-1].split()] for ln in r.stderr.splitlines() if ln.startswith('icp: searched')]
        res[name] = (bytes.fromhex(line.split()[1]), counts)
    vals = np.frombuffer(res['skip'][0], np.float64).reshape(3, 19)
    ref = np.frombuffer(res['search'][0], np.float64).reshape(3, 19)
    # (the two forms keep the same partners and evaluate the same expressions: bit-equal in every run so far.  The comparison allows
    # 1e-10 because the order of a grid cell's points comes from atomics -- the normals' sums may round differently from one
    # PROCESS to the next, with or without the shortcut)
    assert np.array_equal(vals[:, 18], ref[:, 18])
    assert np.allclose(vals, ref, rtol=0.0, atol=1e-10)
    assert np.all(vals[:, 18] >= 3) and np.all(vals[:, 16] > 0.5)            # real registrations: iterations, fitness
    for with_skip, without in zip(res['skip'][1], res['search'][1]):
        n = without[0]
        passes = int(sum(1 for v in without if v > 0))
        assert all(v == n for v in without[:passes])                         # every pass searched every query
        assert with_skip[:2] == [n, n] and min(with_skip[:passes]) < 0.5 * n   # the late passes search less than half


@pytest.mark.parametrize('updates', [1, 4])
def test_icp_final_evaluation_equals_exact_nearest_neighbours(updates):
    """fitness / rmse of the returned pose are sums over EVERY source point's nearest target within the cap: recomputed with a
    k-d tree at that pose.  The clouds carry what the searches treat specially: isolated far returns whose partner is 3-4 m
    away (all coarse rings, rows mode), some without any target within the cap (no partner), dense near-field points, and a
    second pass onwards the partners kept without a search."""
    from scipy.spatial import cKDTree
    from pca_amd.icp import GpuIcp
    cap = 3.9                                             # below the search box's reach (4 m): "within the cap" is a ball, exactly
    rng = np.random.default_rng(5)
    a = sweep(0.0, 0.0, 0.0, 21)
    b = sweep(0.8, 0.05, 0.01, 22)
    n_far = 400
    ang = rng.uniform(-np.pi, np.pi, n_far)
    far = np.stack([70.0 * np.cos(ang), 70.0 * np.sin(ang), rng.uniform(-1.5, 3.0, n_far), np.zeros(n_far)], 1).astype(np.float32)
    step = rng.normal(size=(n_far, 3))
    step *= (rng.uniform(2.2, 4.6, n_far) / np.linalg.norm(step, axis=1))[:, None]       # partner 2.2 .. 4.6 m away
    twin = far.copy()
    twin[:, :3] += step.astype(np.float32) + np.float32([0.8, 0.05, 0.0])
    a = np.concatenate([a, far]).astype(np.float32)
    b = np.concatenate([b, twin]).astype(np.float32)
    icp = GpuIcp()
    icp.max_iteration = updates
    r = icp.register(GpuIcp.to_device(a), GpuIcp.to_device(b), cap, np.eye(4))
    assert r.iterations == updates
    T = r.transformation
    q = a[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d, _ = cKDTree(b[:, :3].astype(np.float64)).query(q)
    inl = d < cap
    assert 0 < (~inl).sum() < n_far                       # some far returns have no partner, most have one
    assert abs(r.fitness - inl.mean()) < 1e-12
    assert abs(r.inlier_rmse - np.sqrt((d[inl] ** 2).mean())) < 1e-9


_SMALL = {}


def small_pair():
    """Two ~9 k-point sweeps 0.9 m apart, cast once and shared (read-only)."""
    if not _SMALL:
        for name, args in (('a', (0.0, 0.0, 0.0, 31)), ('b', (0.9, 0.03, 0.008, 32))):
            pts = sweep(*args, n_beams=32, n_az=300)
            pts.setflags(write=False)
            _SMALL[name] = pts
    return _SMALL['a'], _SMALL['b']


def result_bytes(r):
    """Pose, fitness, rmse and iteration count of an IcpResult as 19 doubles' bytes: equal bytes = bitwise equal."""
    return np.concatenate([r.transformation.ravel(), [r.fitness, r.inlier_rmse, float(r.iterations)]]).astype(np.float64).tobytes()


def register_c(src, tgt, ws_ptr, ws_bytes):
    """pca_icp_register itself, with the defaults of GpuIcp; returns (rc, the 19 doubles' bytes)."""
    import ctypes as C
    from pca_amd import _lib
    ctx = _lib.Context.get()
    T = (C.c_double * 16)()
    fit, rmse, it = C.c_double(0), C.c_double(0), C.c_int(0)
    rc = ctx.lib.pca_icp_register(ctx.h, src.data_ptr(), int(src.shape[0]), tgt.data_ptr(), int(tgt.shape[0]), 1e3,
                                  _lib.f64_array(np.eye(4), 16), 30, 1e-6, 1e-6, ws_ptr, ws_bytes, T, C.byref(fit),
                                  C.byref(rmse), C.byref(it), ctx.stream())
    return rc, np.array(list(T) + [fit.value, rmse.value, float(it.value)], dtype=np.float64).tobytes()


def test_icp_ragged_sizes_through_an_exact_unaligned_workspace():
    """n_src = 1 (mod 32), n_tgt = 1 (mod 256), n_src > n_tgt and, roles swapped, n_src < n_tgt: the C entry point with a
    workspace of exactly pca_icp_workspace_bytes(max) bytes at a base that is not 256-aligned gives bitwise what
    GpuIcp.register gives; one byte less is refused before anything is launched."""
    import torch
    from pca_amd import _lib
    from pca_amd.icp import GpuIcp
    a, b = small_pair()
    n_long = (len(a) - 1) // 32 * 32 + 1
    n_short = (min(len(b), n_long) - 2) // 256 * 256 + 1
    assert n_long % 32 == 1 and n_short % 256 == 1 and 256 < n_short < n_long
    long_, short = GpuIcp.to_device(a[:n_long]), GpuIcp.to_device(b[:n_short])
    ctx = _lib.Context.get()
    need = ctx.lib.pca_icp_workspace_bytes(n_long)
    big = torch.empty(need + 512, dtype=torch.uint8, device=long_.device)
    base = big.data_ptr() + 8
    assert base % 256 == 8
    for src, tgt in ((long_, short), (short, long_)):
        ref = GpuIcp().register(src, tgt, 1e3, np.eye(4))
        assert ref.iterations >= 3 and ref.fitness > 0.5               # a real registration
        rc, got = register_c(src, tgt, base, need)
        assert rc == 0, ctx.lib.pca_last_error(ctx.h)
        assert got == result_bytes(ref)
        assert ctx.status() == 0
        rc, _ = register_c(src, tgt, base, need - 1)
        assert rc == -1 and b'workspace too small' in ctx.lib.pca_last_error(ctx.h)
        assert ctx.status() == 0


def test_icp_one_context_changing_sizes():
    """Large pair, a pair a third of its size, the large pair again on one GpuIcp: the third result is bitwise the first (the
    count tables are zero again, the layout is worked out per call), the small one is what a fresh GpuIcp gives.  The
    reported workspace size never shrinks with n and holds no slot for the count tables (they are the context's)."""
    from pca_amd import _lib
    from pca_amd.icp import GpuIcp
    a, b = small_pair()
    A = (GpuIcp.to_device(a), GpuIcp.to_device(b))
    B = (GpuIcp.to_device(a[::3]), GpuIcp.to_device(b[::3]))
    icp = GpuIcp()
    first = icp.register(*A, 1e3, np.eye(4))
    small = icp.register(*B, 1e3, np.eye(4))
    third = icp.register(*A, 1e3, np.eye(4))
    assert first.iterations >= 3 and first.fitness > 0.5 and small.iterations >= 3
    assert result_bytes(third) == result_bytes(first)
    assert result_bytes(small) == result_bytes(GpuIcp().register(*B, 1e3, np.eye(4)))
    lib = _lib.Context.get().lib
    sizes = [lib.pca_icp_workspace_bytes(n) for n in (1, 31, 32, 33, 255, 257, 4096, 9001, 120000, 1 << 20)]
    assert all(lo <= hi for lo, hi in zip(sizes, sizes[1:]))
    assert sizes[0] < 2 * 4 * 512 * 512 * 64 * 2
