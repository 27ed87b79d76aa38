"""Times pca_bev_voxel_camera on the occupancy labels of the headline window of bench.py (~200 live frames, ~5 M stored
points) at 256 x 256 x 32 (80 m view, z [-2, 4.4)), the grid around the NEWEST pose with the identity heading, through the
accumulator's own p_velo_frame and a 1408 x 376 image, rays to camera depth 80 m: stride 1 and stride 2, the form the
library keeps as its default (PCA_BEV_CAMERA_DEPTH unset), the plain form of the walk (1: every step waits for its own label)
and the look-ahead forms (2, 4, 8 voxels loaded before the first is tested).  Every case: an event pair around the C call
(two memsets + the kernel) on preallocated outputs, after a warm-up, in one process; the cases are taken in turn, round
after round, so that a drift of the box hits them all alike.  The results of all forms are compared with each other, every byte.  Beside it, as context and not as a
threshold: pca_bev_voxel_rays (one lidar ray per stored point) on the same window and grid.
Writes a text report (default profiles/bev_voxel_camera.txt) and prints one JSON line.
Usage: python tools/experiments/voxel_camera_time.py [reps] [report path]"""
import builtins
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

W, H = 1408, 376
NZ, N_LABELS, Z_LO, Z_HI = 32, 19, -2.0, 4.4
THIN = 64
DEPTHS, STRIDES = (None, 1, 2, 4, 8), (1, 2)     # None: the variable unset, the form the library keeps as its default


def main():
    import torch as T
    np = bench.np
    from pca_amd._lib import make_ray_camera
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    report = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'bev_voxel_camera.txt')
    rp, builtins.print = builtins.print, (lambda *a, **k: None)       # (the accumulator narrates every integrate)
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    st_ = bench.Stepper(acc, pool)
    st_.fill()
    for _ in range(10):
        st_.step()
    builtins.print = rp
    store, gen = acc.store, acc.sem_bev_generator
    store.flush_pending()                            # nothing owed
    store.flush_k1()
    n_points = int(store.sizes().sum())
    poses = np.ascontiguousarray(acc._track.as_array(), dtype=np.float64)
    assert poses.shape == (store.n_frames, 3), poses.shape
    px, view = gen.pixel_size, float(gen.view_size)
    prm = gen._raster_params(poses[-1].copy(), np.eye(3), 0., 0., view, store.intensity_div255)
    z_step = (Z_HI - Z_LO) / NZ
    table = np.full(256, 255, dtype=np.uint8)
    table[:N_LABELS] = np.arange(N_LABELS)
    dense = store.bev_voxel_labels(prm, Z_LO, z_step, NZ, table, N_LABELS)['labels']
    # the benchmark's synthetic points fill nearly half of the voxels, the camera's own included: every ray is stopped where it
    # starts.  'thinned' keeps one occupied voxel in THIN (chosen by a hash of its place), so that the rays walk
    place = T.arange(dense.numel(), dtype=T.int64, device=dense.device).reshape(dense.shape)
    thinned = T.where(((place * 2654435761) >> 11) % THIN == 0, dense, T.full_like(dense, 255))
    volumes = {'headline': dense, 'thinned': thinned}
    occupied = {k: int((v != 255).sum().item()) for k, v in volumes.items()}
    P = np.asarray(acc.P_velo_frame, dtype=np.float64)[:3]
    ctx, lib, dev = store.ctx, store.ctx.lib, store.device
    cams = {s: make_ray_camera(P, W, H, s, view, clear=True) for s in STRIDES}
    outs = {}
    for s in STRIDES:
        shape = (H // s, W // s)
        outs[s] = dict(visible=T.empty((NZ, px, px), dtype=T.uint8, device=dev), hit=T.empty(shape, dtype=T.int32, device=dev),
                       depth=T.empty(shape, dtype=T.float32, device=dev), label=T.empty(shape, dtype=T.uint8, device=dev),
                       stats=T.empty(5, dtype=T.int64, device=dev))

    def run(case):
        vol, s, depth = case
        labels = volumes[vol]
        os.environ.pop('PCA_BEV_CAMERA_DEPTH', None)
        if depth is not None:
            os.environ['PCA_BEV_CAMERA_DEPTH'] = str(depth)
        o = outs[s]
        ctx.check(lib.pca_bev_voxel_camera(ctx.h, C.byref(prm), Z_LO, z_step, NZ, labels.data_ptr(), C.byref(cams[s]),
                                           o['visible'].data_ptr(), o['hit'].data_ptr(), o['depth'].data_ptr(),
                                           o['label'].data_ptr(), o['stats'].data_ptr(), ctx.stream()))

    def lidar():
        return store.bev_voxel_rays(prm, Z_LO, z_step, NZ, poses)

    def event_ms(fn):
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    cases = [(v, s, d) for v in volumes for s in STRIDES for d in DEPTHS]
    # every form gives the plain form's result, every byte
    results = {}
    for case in cases:
        run(case)
        run(case)                                    # (warm-up: every case twice)
        T.cuda.synchronize()
        results[case] = {k: v.clone() for k, v in outs[case[1]].items()}
    for v, s, d in cases:
        assert all(T.equal(results[v, s, d][k].view(T.uint8), results[v, s, 1][k].view(T.uint8)) for k in results[v, s, 1]), (v, s, d)
    lidar()
    lidar()
    T.cuda.synchronize()
    ms, ms_lidar = {case: [] for case in cases}, []
    for _ in range(reps):
        for case in cases:
            ms[case].append(event_ms(lambda: run(case)))
        ms_lidar.append(event_ms(lidar))
    os.environ.pop('PCA_BEV_CAMERA_DEPTH', None)

    def summary(t):
        return dict(median_us=1e3 * statistics.median(t), min_us=1e3 * min(t), max_us=1e3 * max(t), n=len(t))

    res = {case: summary(ms[case]) for case in cases}
    res_lidar = summary(ms_lidar)
    sets = [(v, s) for v in volumes for s in STRIDES]
    stats = {c: results[c + (1, )]['stats'].cpu().numpy().tolist() for c in sets}
    visible = {c: int(results[c + (1, )]['visible'].sum().item()) for c in sets}
    hit_depth = {c: float(results[c + (1, )]['depth'][results[c + (1, )]['hit'] >= 0].double().mean().item()) if stats[c][4] else 0.
                 for c in sets}
    out = dict(window=dict(frames=store.n_frames, points=n_points, px=px, nz=NZ, view=view, occupied=occupied, W=W, H=H),
               cases=[dict(labels=c[0], stride=c[1], depth=c[2], stats=stats[c[:2]], visible=visible[c[:2]], **res[c]) for c in cases],
               bev_voxel_rays=res_lidar)
    print(json.dumps(out))
    kept_ok = {c: res[c + (None, )]['median_us'] <= res[c + (1, )]['median_us'] for c in sets}

    lines = ['# pca_bev_voxel_camera on the occupancy labels of the headline window of bench.py',
             f'# tools/experiments/voxel_camera_time.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and stepped',
             '# into steady state, nothing owed; pca_bev_voxel_labels once (19 labels), then the cases in turn, round after round, an',
             f'# event pair around each C call (two memsets + bev_camera_rays) on preallocated outputs, {reps} timed after two warm-up',
             '# calls per case.  Every form\'s visible, hit, depth, label and stats equal the plain form\'s, every byte (checked here).',
             f'window            {store.n_frames} frames, {n_points} stored points; grid {px} x {px} x {NZ}, {view:.0f} m view around the newest pose,',
             f'                  z [{Z_LO}, {Z_HI})',
             f'labels            headline: pca_bev_voxel_labels of the window as it is, {occupied["headline"]} of {NZ * px * px} voxels occupied (the',
             '                  benchmark\'s synthetic points are dense: the camera\'s own voxel is occupied and stops every ray at once);',
             f'                  thinned: one occupied voxel in {THIN} of those kept (by a hash of its place), {occupied["thinned"]} occupied: the rays walk',
             f'camera            the accumulator\'s p_velo_frame, {W} x {H}, rays to camera depth {view:.0f} m',
             *(f'{v + ", stride " + str(s):<20}rays {stats[v, s][0]}, cast {stats[v, s][1]}, not finite {stats[v, s][2]}, too long {stats[v, s][3]}, hits {stats[v, s][4]};'
               f' visible voxels {visible[v, s]}; mean depth of a hit {hit_depth[v, s]:.2f} m' for v, s in sets),
             '',
             f'{"":<88}   median       min       max   [us], n = {reps}']
    for v, s, d in cases:
        form = 'the kept form (the variable unset)' if d is None else 'plain: every step waits for its own label' if d == 1 else \
            f'{d} voxels loaded before the first is tested'
        lines.append(f'{f"{v}, stride {s}, PCA_BEV_CAMERA_DEPTH={d}, {form}":<88}{res[v, s, d]["median_us"]:9.1f} {res[v, s, d]["min_us"]:9.1f} {res[v, s, d]["max_us"]:9.1f}')
    lines += ['',
              'the kept form is not slower than the plain form in this run (medians): '
              + ', '.join(f'{v} stride {s}: {kept_ok[v, s]}' for v, s in sets),
              'not built: a bit-packed coarse occupancy in LDS (64 x 64 x 8 blocks of 4^3 voxels) that lets a ray skip empty blocks.',
              '',
              'context, not a threshold: pca_bev_voxel_rays on the same window and grid (one lidar ray per stored point, two memsets + kernel,',
              f'  called through DeviceStore.bev_voxel_rays): median {res_lidar["median_us"]:.1f} us (min {res_lidar["min_us"]:.1f}, max {res_lidar["max_us"]:.1f})']
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
