"""Per-kernel event times (pca_profile) of one raster over the headline window at the given grid sizes, in us to 0.01:
bev_large_grid.py's set-up with 50 bracketed rasters per size, for A/B runs of two builds of the library (one process each,
alternating; profiles/bev_tile_slots.txt).

    python tools/experiments/bev_kernel_times.py LABEL [px ...]
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

REPS, WARM = 50, 5


def main(label, sizes):
    import builtins
    real_print = builtins.print
    builtins.print = lambda *a, **k: None                  # the accumulator prints one line per frame
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    bench.Stepper(acc, pool).fill()
    builtins.print = real_print
    idx = bench.present_index(acc)
    st = acc.store
    st.flush_pending()
    poses = np.array(acc.poses)
    origin = poses[idx]
    Rm = hl.rotation_matrix_3d(hl.heading_rot_ang(poses[:idx] - origin))
    ctx = _lib.Context.get()
    for px in sizes:
        prm = make_bev_params(origin, Rm, 0., 0., bench.VIEW_M, px, None, 20., 20., 0.5, 0, [13, 14, 15, 17], False)
        out = torch.empty((21, px, px), dtype=torch.float16, device='cuda')
        for _ in range(WARM):
            st.bev(idx, prm, out16=out)
        torch.cuda.synchronize()
        ctx.profile(1)
        p0 = ctx.profile_read()
        for _ in range(REPS):
            st.bev(idx, prm, out16=out)
        p1 = ctx.profile_read()
        ctx.profile(0)
        st.check_status()
        print('%-8s px %5d ' % (label, px) + ' '.join('%s %.2f' % (k, 1e3 * (p1[k][0] - p0[k][0]) / REPS)
                                                       for k in sorted(p1) if p1[k][0] - p0[k][0] > 0), flush=True)
        del out


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '-', [int(a) for a in sys.argv[2:]] or [256, 1024, 2048])
