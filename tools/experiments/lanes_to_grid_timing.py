"""Times the GT lane clipping of one BEV sample on a synthetic city map: the host path (what generate() costs with a plain
list under trajs['gt_lanes']: lane - origin for every lane, _copy_trajs' copy of every lane, transform_traj per lane and the
non-empty filter -- the parent commit's expressions, unchanged under PCA_GT_LANES=host) against the device path
(DeviceLanes.to_grid: launch set, one copy to pinned memory, decode into the list), for one sample and for S samples in one
call.  The map: `n_lanes` polylines of `n_poses` vertices 1 m apart, spread over a square that gives about one lane per
450 m^2; view 80 m, px 256.  Every timed device result is compared with the host path's, bit for bit.
A second mode (`kernels`) only issues the calls, for a kernel trace taken from outside.
Usage: python tools/experiments/lanes_to_grid_timing.py [report path] | kernels"""
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit('/tools/', 1)[0] + '/pc-accumulation-lib_amd')
from pca_amd import host_logic as hl  # noqa: E402

HBM_PEAK = 8.0e12
VIEW, PX, S_MANY = 80., 256, 40


def city(n_lanes, n_poses, seed=0):
    rng = np.random.default_rng(seed)
    side = np.sqrt(450. * n_lanes)
    lanes = []
    for _ in range(n_lanes):
        heading = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0, 0.03, n_poses))
        d = np.c_[np.cos(heading), np.sin(heading), np.zeros(n_poses)]
        lanes.append(np.r_[rng.uniform(0, side, 2), 0.] + np.cumsum(d, axis=0))
    return lanes


def sample_views(lanes, n, seed=1):
    rng = np.random.default_rng(seed)
    views = []
    for k in range(n):
        lane = lanes[int(rng.integers(0, len(lanes)))]
        views.append((lane[len(lane) // 2] + [0.5, -0.5, 1.], hl.rotation_matrix_3d(rng.uniform(0, 2 * np.pi)), 0., 0., VIEW, PX))
    return views


def host_path(lanes, view):
    """(seconds for the subtraction, for the copy, for to_grid and the filter; the list)"""
    origin, R, dx, dy, aug, px = view
    t0 = time.perf_counter()
    shifted = [lane - origin for lane in lanes]                          # _window_inputs
    t1 = time.perf_counter()
    copied = [np.array(t) for t in shifted]                              # _copy_trajs
    t2 = time.perf_counter()
    out = [hl.transform_traj(t, R, dx, dy, aug, px, mutate=False) for t in copied]
    out = [lane for lane in out if lane.shape[0] > 0]                    # generate()
    t3 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2), out


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


def med(v):
    return 1e3 * statistics.median(v)


def main():
    import torch
    from pca_amd.lanes import DeviceLanes, LaneView
    mode = sys.argv[1] if len(sys.argv) > 1 else 'profiles/lanes_to_grid.txt'
    lines = []
    for n_lanes, n_poses in ((5000, 40), (20000, 40)):
        lanes = city(n_lanes, n_poses)
        views = sample_views(lanes, S_MANY)
        lv = [LaneView(*v) for v in views]
        t = time.perf_counter()
        dev = DeviceLanes(lanes)
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t
        P = dev.n_vertices
        for _ in range(3):                                               # warm-up: allocator, pinned blocks, the row hint
            [p.resolve() for p in dev.to_grid(lv, asynchronous=True)]
            dev.to_grid(lv[:1], asynchronous=True)[0].resolve()
        if mode == 'kernels':
            for _ in range(10):
                dev.to_grid(lv[:1], asynchronous=True)[0].resolve()
            for _ in range(10):
                [p.resolve() for p in dev.to_grid(lv, asynchronous=True)]
            continue
        host_t, host_out = [], []
        for v in views[:5]:
            tt, out = host_path(lanes, v)
            host_t.append(tt)
            host_out.append(out)
        one, one_gpu = [], []
        for rep in range(20):
            k = rep % 5
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            a.record()
            pend = dev.to_grid(lv[k:k + 1], asynchronous=True)[0]
            b.record()
            got = pend.resolve()
            one.append(time.perf_counter() - t)
            b.synchronize()
            one_gpu.append(a.elapsed_time(b) * 1e-3)
            assert same(got, host_out[k])
        many, many_gpu = [], []
        for rep in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            a.record()
            pend = dev.to_grid(lv, asynchronous=True)
            b.record()
            got = [p.resolve() for p in pend]
            many.append(time.perf_counter() - t)
            b.synchronize()
            many_gpu.append(a.elapsed_time(b) * 1e-3)
            assert all(same(got[k], host_out[k]) for k in range(5))
        sub, cp, tg = (med([t[i] for t in host_t]) for i in range(3))
        host_ms = sub + cp + tg
        rows = [sum(x.shape[0] for x in o) for o in host_out]
        lines += [
            f'map {n_lanes} lanes x {n_poses} poses = {P} vertices, view {VIEW:.0f} m, px {PX}; upload once {1e3 * t_up:.1f} ms; '
            f'survivors of the 5 checked samples {[len(o) for o in host_out]} lanes, {rows} rows',
            f'  host path per sample [ms], median of 5: subtract {sub:.1f} + _copy_trajs {cp:.1f} + to_grid and filter {tg:.1f} = {host_ms:.1f}',
            f'  device path, 1 sample, launch + copy + decode into the list [ms], n = 20: median {med(one):.3f} min {1e3 * min(one):.3f} '
            f'max {1e3 * max(one):.3f}  -> {host_ms / med(one):.0f} x the host path',
            f'      of which the launch set on the device (event pair) {med(one_gpu):.3f} ms: 24 P S = {24 * P / 1e6:.1f} MB at '
            f'{24 * P / (med(one_gpu) * 1e-3) / 1e12:.2f} TB/s, {24 * P / (med(one_gpu) * 1e-3) / HBM_PEAK:.2f} of the HBM peak',
            f'  device path, S = {S_MANY} samples in one call [ms], n = 10: median {med(many):.3f} min {1e3 * min(many):.3f} max '
            f'{1e3 * max(many):.3f} = {med(many) / S_MANY:.3f} per sample  -> {host_ms * S_MANY / med(many):.0f} x the host path',
            f'      of which the launch set on the device {med(many_gpu):.3f} ms: 24 P S = {24 * P * S_MANY / 1e6:.1f} MB at '
            f'{24 * P * S_MANY / (med(many_gpu) * 1e-3) / 1e12:.2f} TB/s, {24 * P * S_MANY / (med(many_gpu) * 1e-3) / HBM_PEAK:.2f} of the HBM peak',
            f'      every timed result equals the host path\'s list bit for bit; rows per sample the calls made room for: {dev._cap_hint}',
        ]
    if mode == 'kernels':
        return
    text = '\n'.join(lines)
    with open(mode, 'w') as f:
        f.write(text + '\n')
    print(text)
    print(json.dumps(dict(ok=True)))


if __name__ == '__main__':
    main()
