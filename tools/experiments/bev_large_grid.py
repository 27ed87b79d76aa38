"""Cost of one raster per grid size on the headline window: the bench.py workload (synthetic KITTI-shaped frames of 120 000
points, 200 m horizon, ~201 frames in the window, 80 m view), one DeviceStore.bev call at px in {1024, 1536, 2048, 4096}
(px > 1024: banded).  Prints the mean over REPS calls (HIP events around each call, no owed
transforms) and the library's per-kernel event times (pca_profile, every launch bracketed).

    python tools/experiments/bev_large_grid.py [px ...]
Per-kernel split on the device:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/experiments/bev_large_grid.py
"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
import bench  # noqa: E402  (puts the package on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pca_amd import _lib, host_logic as hl  # noqa: E402
from pca_amd.device_store import make_bev_params  # noqa: E402

REPS, WARM = 20, 3


def main(sizes):
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    stepper = bench.Stepper(acc, pool)
    stepper.fill()
    idx = bench.present_index(acc)
    st = acc.store
    st.flush_pending()
    poses = np.array(acc.poses)
    origin = poses[idx]
    Rm = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:idx] - origin))
    ctx = _lib.Context.get()
    print('window: %d frames, %d points, present_idx %d' % (st.n_frames, int(st.sizes().sum()), idx))
    print('%6s %6s %10s %12s   %s' % ('px', 'bands', 'ms/raster', 'Mpoints/s', 'per-kernel ms (pca_profile)'))
    for px in sizes:
        prm = make_bev_params(origin, Rm, 0., 0., bench.VIEW_M, px, None, 20., 20., 0.5, 0, [13, 14, 15, 17], False)
        out = torch.empty((21, px, px), dtype=torch.float16, device='cuda')
        for _ in range(WARM):
            st.bev(idx, prm, out16=out)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * REPS)]
        for k in range(REPS):
            ev[2 * k].record()
            st.bev(idx, prm, out16=out)
            ev[2 * k + 1].record()
        torch.cuda.synchronize()
        ms = np.array([ev[2 * k].elapsed_time(ev[2 * k + 1]) for k in range(REPS)])
        ctx.profile(1)
        p0 = ctx.profile_read()
        for _ in range(REPS):
            st.bev(idx, prm, out16=out)
        p1 = ctx.profile_read()
        ctx.profile(0)
        st.check_status()
        prof = {k: p1[k][0] - p0[k][0] for k in p1}
        tx = (px + 7) // 8
        rows = tx if tx * tx <= 16384 else 16384 // tx
        bands = (tx + rows - 1) // rows
        kern = ', '.join('%s %.3f' % (k, v / REPS) for k, v in sorted(prof.items()) if v > 0)
        print('%6d %6d %10.3f %12.1f   %s' % (px, bands, np.median(ms), st.sizes().sum() / np.median(ms) / 1e3, kern))
        del out


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [1024, 1536, 2048, 4096])
