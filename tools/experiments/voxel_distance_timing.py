"""Times pca_voxel_distance on the 256 x 256 x 32 volumes of the headline window of bench.py (labels and seen as
tools/experiments/voxel_ssc_time.py makes them: 'headline', dense, about half the voxels sites, and 'thinned', one site in 64
kept), with the default grid's metric (weights 625 : 256, unit 0.0125 m), unbounded and with max_dist = 1 m (6400), every
output asked for (fill within 0.6 m, flipped TSDF truncated at 1 m).

  python tools/experiments/voxel_distance_timing.py [reps] [report path]
      whole calls between event pairs on preallocated outputs, alternated call by call in this process with
      pca_bev_voxel_labels over the same window (the yardstick: code this feature does not touch) and, once per block, with the
      host form the feature replaces: labels .cpu() + scipy.ndimage.distance_transform_edt(return_indices=True) with the same
      sampling (where scipy is importable; else the numpy model of tests/voxel_distance_common.py on a stated sub-volume).
      Then the per-kernel times from the library's per-launch events (pca_profile_enable(1)), the bytes each kernel moves, and
      the worst case for the walk: 1024 x 1024 x 32 with a single site, and empty.
Writes a text report (default profiles/voxel_distance.txt) and prints one JSON line."""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tools', 'experiments'))
import voxel_ssc_time as vst  # noqa: E402  (puts the repository and tests/ on the path, imports bench)

WEIGHTS, UNIT = (625, 256), 0.0125
BOUND_1M, FILL = 6400, 2304                  # (1 m / unit)^2; 0.6 m: 48 units
HBM_PEAK = 8.0e12                            # bytes / s, MI355X


def distance_call(store, labels, seen, max_dist2, outputs=True):
    """The C call on preallocated outputs (all five, or dist2 alone)."""
    import torch as T
    ctx, lib, dev = store.ctx, store.ctx.lib, store.device
    nz, px = int(labels.shape[0]), int(labels.shape[1])
    ws = T.empty(int(lib.pca_voxel_distance_workspace_bytes(px, nz)), dtype=T.uint8, device=dev)
    outs = [T.empty(labels.shape, dtype=dt, device=dev) for dt in ((T.int32, T.int32, T.uint8, T.uint8, T.float32) if outputs else (T.int32, ))]
    ptrs = [o.data_ptr() for o in outs] + [None] * (5 - len(outs))

    def call():
        ctx.check(lib.pca_voxel_distance(ctx.h, px, nz, labels.data_ptr(), None if seen is None else seen.data_ptr(), None,
                                         WEIGHTS[0], WEIGHTS[1], max_dist2, FILL if outputs else -1, 0, UNIT, 1.0, 1,
                                         ws.data_ptr(), ws.numel(), *ptrs, ctx.stream()))
    call.keep = (ws, outs)
    return call


def main():
    import torch as T
    np = vst.bench.np
    args = sys.argv[1:]
    reps = int(args[0]) if args else 20
    report = args[1] if len(args) > 1 else os.path.join(ROOT, 'profiles', 'voxel_distance.txt')
    made, make = {}, vst.bench.make_accumulator

    def keep_accumulator(*a, **k):         # (volumes_of returns the store and the generator; the yardstick needs the newest pose)
        made['acc'] = make(*a, **k)
        return made['acc']
    vst.bench.make_accumulator = keep_accumulator
    vols, gen, store, facts = vst.volumes_of()
    vst.bench.make_accumulator = make
    ctx = store.ctx
    px, nz = facts['px'], facts['nz']
    voxels = nz * px * px

    # the yardstick: the labels pass over the window the volumes came from
    poses = np.ascontiguousarray(made['acc'][0]._track.as_array(), dtype=np.float64)
    prm = gen._raster_params(poses[-1].copy(), np.eye(3), 0., 0., facts['view'], store.intensity_div255)
    table = np.full(256, 255, dtype=np.uint8)
    table[:vst.N_LABELS] = np.arange(vst.N_LABELS)
    z_step = (vst.Z_HI - vst.Z_LO) / vst.NZ

    def yardstick():
        store.bev_voxel_labels(prm, vst.Z_LO, z_step, vst.NZ, table, vst.N_LABELS)

    def event_ms(fn):
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def summary(t, scale=1e3):
        return dict(median=scale * statistics.median(t), min=scale * min(t), max=scale * max(t), n=len(t))

    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    sampling = (math.sqrt(WEIGHTS[1]), math.sqrt(WEIGHTS[0]), math.sqrt(WEIGHTS[0]))

    def host_form(labels):
        lab = labels.cpu().numpy()
        if ndimage is not None:
            ndimage.distance_transform_edt(lab >= 32, sampling=sampling, return_indices=True)
        else:
            import voxel_distance_common as model
            model.transform(lab[:4, :32, :32], None, WEIGHTS)

    calls, kernels, host, sites = {}, {}, {}, {}
    for name, (labels, seen, _, _) in vols.items():
        sites[name] = int((labels < 32).sum().item())
        for bound_name, bound in (('unbounded', -1), ('max_dist 1 m', BOUND_1M)):
            fn = distance_call(store, labels, seen, bound)
            for _ in range(3):
                fn()
                yardstick()
            T.cuda.synchronize()
            ms = {'distance': [], 'labels': []}
            for _ in range(reps):
                ms['distance'].append(event_ms(fn))
                ms['labels'].append(event_ms(yardstick))
            calls[name, bound_name] = {k: summary(v) for k, v in ms.items()}
            ctx.profile(1)
            for _ in range(reps):
                fn()
            prof = ctx.profile_read()
            ctx.profile(0)
            kernels[name, bound_name] = {k: 1e3 * prof[k][0] / prof[k][1] for k in ('voxel_dist_lines', 'voxel_dist_rows')}
        t = []
        for _ in range(3):
            T.cuda.synchronize()
            t0 = time.perf_counter()
            host_form(labels)
            t.append(time.perf_counter() - t0)
        host[name] = summary(t, 1e3)

    # the worst case for the walk: the largest volume, a single site; and the same volume empty
    big = T.full((32, 1024, 1024), 255, dtype=T.uint8, device=store.device)
    worst = {}
    fn = distance_call(store, big, None, -1, outputs=False)
    fn()
    worst['empty'] = summary([event_ms(fn) for _ in range(3)], 1.)
    big[31, 1023, 0] = 3
    fn()
    worst['single site'] = summary([event_ms(fn) for _ in range(3)], 1.)
    del fn, big

    out = dict(window=facts, sites=sites, calls_event_us={f'{a}, {b}': v for (a, b), v in calls.items()},
               kernels_us={f'{a}, {b}': v for (a, b), v in kernels.items()}, host_ms=host, worst_ms=worst,
               host_form='scipy' if ndimage is not None else 'numpy model on 4 x 32 x 32')
    print(json.dumps(out))

    lines_bytes, rows_bytes = voxels * (1 + 8), voxels * (8 + 3 + 14)
    lines = ['# pca_voxel_distance on the volumes of the headline window of bench.py, against pca_bev_voxel_labels and the host form',
             f'# tools/experiments/voxel_distance_timing.py {reps} -- one MI355X, one process; the volumes of tools/experiments/voxel_ssc_time.py',
             f'window            {facts["frames"]} frames, {facts["points"]} stored points; volumes {px} x {px} x {nz} = {voxels} voxels',
             f'metric            weights {WEIGHTS[0]} : {WEIGHTS[1]}, unit {UNIT} m; every output: dist2, nearest, nearest_label, filled (0.6 m), tsdf (1 m, flipped)',
             *(f'{name:<18}{n} sites ({100. * n / voxels:.1f} % of the voxels)' for name, n in sites.items()),
             '',
             f'whole calls, an event pair around each, alternated call by call, {reps} timed after 3 warm-up rounds        median       min       max   [us]']
    for (name, bound), v in calls.items():
        lines.append(f'{name + ", " + bound + ": pca_voxel_distance (two launches)":<96}{v["distance"]["median"]:9.1f} {v["distance"]["min"]:9.1f} {v["distance"]["max"]:9.1f}')
        lines.append(f'{"    pca_bev_voxel_labels over the window (the yardstick)":<96}{v["labels"]["median"]:9.1f} {v["labels"]["min"]:9.1f} {v["labels"]["max"]:9.1f}')
    lines += ['', f'per kernel, the library\'s per-launch events, mean of {reps} launches [us]; bytes moved against the HBM peak of {HBM_PEAK / 1e12:.0f} TB/s:',
              f'  voxel_dist_lines reads 1 B and writes 8 B a voxel ({lines_bytes / 1e6:.1f} MB; each round of a row reads the row\'s labels again, from L2);',
              f'  voxel_dist_rows reads 8 + 3 B and writes 14 B ({rows_bytes / 1e6:.1f} MB)']
    for (name, bound), v in kernels.items():
        a, b = v['voxel_dist_lines'], v['voxel_dist_rows']
        lines.append(f'  {name + ", " + bound:<28}lines {a:8.1f} us ({100. * lines_bytes / (a * 1e-6) / HBM_PEAK:5.1f} % of peak)   '
                     f'rows {b:8.1f} us ({100. * rows_bytes / (b * 1e-6) / HBM_PEAK:5.1f} % of peak)')
    lines += ['', 'the host form the call replaces, labels .cpu() + '
              + ('scipy.ndimage.distance_transform_edt(return_indices=True), same sampling' if ndimage is not None
                 else 'the numpy model on a 4 x 32 x 32 sub-volume (scipy is not importable here)') + ', 3 runs [ms]:']
    for name, v in host.items():
        lines.append(f'  {name:<10}median {v["median"]:9.1f}   min {v["min"]:9.1f}   max {v["max"]:9.1f}')
    lines += ['', 'the worst case for the walk, 1024 x 1024 x 32 (33.5 M voxels), unbounded, dist2 alone, 3 calls [ms]:']
    for name, v in worst.items():
        lines.append(f'  {name:<12}median {v["median"]:9.2f}   min {v["min"]:9.2f}   max {v["max"]:9.2f}')
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
