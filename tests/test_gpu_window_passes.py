"""GPU: what the four read-only passes over a window of the store have in common (DeviceStore.bev_class_planes,
bev_elev_partition, bev_voxel_labels, bev_voxel_rays): a K1 that integrate() noted runs before the pass, and a refused call
leaves the noted K1 and the owed re-transforms as they were.  KITTI fake tree, 6 frames, 32^2 cells, 4 height bins."""
import numpy as np
import pytest

from test_gpu_kernels import DYNOBJ, T  # noqa: F401  (T: fixture)
from window_pass_common import BEV_KITTI, kitti_accumulator, params

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
