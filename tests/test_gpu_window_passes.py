"""GPU: what the four read-only passes over a window of the store have in common (DeviceStore.bev_class_planes,
bev_elev_partition, bev_voxel_labels, bev_voxel_rays): a K1 that integrate() noted runs before the pass, and a refused call
leaves the noted K1 and the owed re-transforms as they were.  KITTI fake tree, 6 frames, 32^2 cells, 4 height bins.
And what the passes that visit the window one point per thread have in common (the rays, the carving, the camera render:
csrc/pca_point_pass.h): the silent cut of the window at the store's capacity."""
import ctypes as C

import numpy as np
import pytest

import render_camera_common as rcc
import voxel_carve_common as cc
import voxel_rays_common as rc
from test_gpu_kernels import DYNOBJ, T  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, frames_of, kitti_accumulator, loaded, params

pytestmark = pytest.mark.gpu

PASSES = ('class_planes', 'elev_partition', 'voxel_labels', 'voxel_rays')
TABLE = np.where(np.arange(256) < 19, np.arange(256), 255).astype(np.uint8)


def run(name, acc, bad=False):
    """The pass over the whole window of acc.store; bad: with one argument of the pass's own that the C call refuses."""
    st, prm = acc.store, params((0., 0., 0.), 0.3, 0., 0., 50., 32, None)
    nz = 0 if bad else 4
    if name == 'class_planes':
        return st.bev_class_planes(st.n_frames - 1, prm, [] if bad else [[0], DYNOBJ, [1]], want_counts=True)
    if name == 'elev_partition':
        return st.bev_elev_partition(prm, float('nan') if bad else 0.2)
    if name == 'voxel_labels':
        return st.bev_voxel_labels(prm, -2., 1.6, nz, TABLE, 19)
    return st.bev_voxel_rays(prm, -2., 1.6, nz, acc._track.as_array())


def host(out):
    return [v.cpu().numpy() for v in (out.values() if isinstance(out, dict) else out)]


def same(a, b):
    assert len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def owed(st):
    return [(np.array(Tm).copy(), e) for Tm, e in st._pending]


def same_owed(a, b):
    assert len(a) == len(b) and all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(a, b))


@pytest.mark.parametrize('name', PASSES)
def test_noted_k1_runs_before_the_pass(T, tmp_path, monkeypatch, name):
    out = []
    for fuse in ('1', '0'):
        monkeypatch.setenv('PCA_FUSE_K1', fuse)
        acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=6)
        st = acc.store
        assert (st._k1_noted is not None) == (fuse == '1')       # integrate() left the newest frame's K1 for the next raster
        out.append(host(run(name, acc)))
        assert st._k1_noted is None
        st.check_status()
        st.set_defer_k1(False)
    same(out[0], out[1])
    assert all(x.any() for x in out[0])


@pytest.mark.parametrize('name', PASSES)
def test_refused_call_leaves_the_noted_k1_and_the_owed_chain_usable(T, tmp_path, monkeypatch, name):
    monkeypatch.setenv('PCA_FUSE_K1', '1')
    out = []
    for refuse_first in (False, True):
        acc = kitti_accumulator(tmp_path, dict(BEV_KITTI), n_frames=6)
        st = acc.store
        chain = owed(st)
        assert st._k1_noted is not None and chain                # a K1 is noted and re-transforms are owed
        if refuse_first:
            with pytest.raises(RuntimeError, match='bev '):
                run(name, acc, bad=True)
            assert st._k1_noted is not None                      # nothing ran: the K1 is still noted
            same_owed(owed(st), chain)
        out.append(host(run(name, acc)))
        assert st._k1_noted is None
        same_owed(owed(st), chain)                               # a read-only pass: still owed, and the same list
        st.check_status()
        st.set_defer_k1(False)
    same(out[0], out[1])
    assert all(x.any() for x in out[0])


# ---------------------------------------------------------------------------------------------- the capacity cut
CAPACITY_CUT = 9000                                               # inside the third of the three frames of 4 000 rows
GRID = ((0.3, -0.2, 0.125), rc.rotation(0.3), 0., 0., 40., 20)    # origin, R, dx, dy, view, px
Z_LO, Z_STEP, NZ = -1., 0.5, 5
SENSORS = np.array([[1.0, 2.0, 0.5], [-8.0, 5.0, 1.0], [30.0, -3.0, 0.75]])
IMAGE = (65, 33, 32.)                                             # W, H, f


@pytest.mark.parametrize('name', ['voxel_rays', 'voxel_carve', 'render_camera'])
def test_window_is_cut_at_the_capacity_in_silence(T, name):
    """The pass through its C entry with a COPY of the store block whose capacity says 9 000 (the arrays behind it keep their
    size: nothing is read outside an allocation, however the kernel behaves), max_points above the window's 12 000 points:
    the outputs are those of the window cut at 9 000, and the overflow bit stays down -- only the max_points cut raises it."""
    import torch

    from pca_amd import _lib
    frames = frames_of(1)
    st = loaded(frames)
    ctx, lib, dev = st.ctx, st.ctx.lib, st.device
    store = _lib.PcaStore.from_buffer_copy(st.c_store())
    assert store.capacity == 1 << 15 and st.c_store().capacity == 1 << 15
    store.capacity = CAPACITY_CUT
    window = (C.byref(store), st.frame_off.data_ptr(), st.head, st.head + st.n_frames, 20000)
    px = GRID[5]
    prm = params(*GRID)
    org = torch.from_numpy(SENSORS.copy()).to(dev)

    def filled(shape, dtype):
        return torch.full(shape, 7, dtype=dtype, device=dev)
    if name == 'voxel_rays':
        out = {'seen': filled((NZ, px, px), torch.uint8), 'stats': filled((4, ), torch.int64)}
        r = lib.pca_bev_voxel_rays(ctx.h, *window, C.byref(prm), Z_LO, Z_STEP, NZ, 0, org.data_ptr(), None, None, 0,
                                   out['seen'].data_ptr(), out['stats'].data_ptr(), ctx.stream())
        want = rc.model(frames, SENSORS, *GRID, Z_LO, Z_STEP, NZ, False, max_points=CAPACITY_CUT)
        compare = rc.compare
    elif name == 'voxel_carve':
        group = _lib.PcaClassGroup()
        group.mask[:] = list(_lib.class_mask(DYNOBJ))
        ws = torch.empty(int(lib.pca_bev_carve_workspace_bytes(20000, px, NZ)), dtype=torch.uint8, device=dev)
        out = {'hits': filled((NZ, px, px), torch.int32), 'cross': filled((NZ, px, px), torch.int32),
               'flags': filled((20000, ), torch.uint8), 'stats': filled((6, ), torch.int64)}
        r = lib.pca_bev_voxel_carve(ctx.h, *window, C.byref(prm), Z_LO, Z_STEP, NZ, 0, org.data_ptr(), group, 1, 2, 1.0, None, None, 0,
                                    ws.data_ptr(), ws.numel(), out['hits'].data_ptr(), out['cross'].data_ptr(),
                                    out['flags'].data_ptr(), out['stats'].data_ptr(), ctx.stream())
        torch.cuda.synchronize()
        assert (out['flags'][CAPACITY_CUT:] == 7).all().item()   # no flag is written behind the cut
        out['flags'] = out['flags'][:CAPACITY_CUT]
        want = cc.model(frames, SENSORS, *GRID, Z_LO, Z_STEP, NZ, False, DYNOBJ, max_points=CAPACITY_CUT)
        compare = cc.compare
    else:
        W, H, f = IMAGE
        P = rcc.camera(W, H, f)
        cam = _lib.make_camera(P, W, H, 1, True, (0., np.inf))
        keys = filled((H, W), torch.int64)
        out = {'depth': filled((H, W), torch.float32), 'index': filled((H, W), torch.int64), 'rgb': filled((H, W, 3), torch.uint8),
               'sem': filled((H, W), torch.uint8), 'stats': filled((3, ), torch.int64)}
        r = lib.pca_render_camera(ctx.h, *window, C.byref(cam), None, None, None, 0, keys.data_ptr(),
                                  *(out[k].data_ptr() for k in ('depth', 'index', 'rgb', 'sem', 'stats')), ctx.stream())
        want = rcc.model(frames, P, W, H, 1, max_points=CAPACITY_CUT)
        compare = rcc.compare
    assert r == 0, lib.pca_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    compare(out, want)
    assert want['stats'][0] == (CAPACITY_CUT if name == 'render_camera' else 7691)     # (the whole window: 12 000 and 10 250)
    assert ctx.status() == 0                                      # the capacity cut raises no bit
    st.check_status()
