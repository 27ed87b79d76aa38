"""Times pca_bev_voxel_instances on the headline window of bench.py (~200 live frames, ~5 M stored points, 256 x 256, 80 m view,
nz = 32 over z [-2, 4.4)) beside pca_bev_voxel_labels alone, the yardstick: the instances call runs that pass first (counts
only) and then its own ten launches, timed in the same process on the same box.  The call is made with the generator's four
dynamic classes (one label each) and with a single class, 26-connectivity, min_points = min_voxels = 1.  The benchmark's classes
are uniform over the window, so the foreground is NOT a few compact objects here, unlike real data: it is what fills the grid.
Per case: the whole call with an event pair (alternated with the labels call), then every kernel from the library's own
per-launch events (pca_profile_enable) and the stats.  The structural claim -- a fixed number of launches, whatever the data --
is asserted on the launch counts of that profile read, for the two cases and for a call whose min_points no voxel reaches.
Writes a text report (default profiles/bev_voxel_instances.txt) and prints one JSON line.
Usage: python tools/experiments/bev_voxel_instances_timing.py [reps] [report path]"""
import builtins
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NZ, Z_LO, Z_HI = 32, -2.0, 4.4
MAX_INSTANCES = 4096
# launches of one call, per kernel: the two voxel levels and the ten of pca_bev_inst.hip
LAUNCHES = {'bev_voxel_bin': 1, 'bev_voxel_cells': 1, 'bev_inst_init': 1, 'bev_inst_merge': 2, 'bev_inst_compress': 2,
            'bev_inst_sums': 1, 'bev_inst_offsets': 1, 'bev_inst_number': 1, 'bev_inst_write': 1, 'bev_inst_points': 1}


def timed(fn, T, reps, other):
    """`fn` and `other` alternately, an event pair around each `fn`: [ms]."""
    out = []
    for _ in range(reps):
        other()
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms):
    return dict(median_us=1e3 * statistics.median(ms), min_us=1e3 * min(ms), max_us=1e3 * max(ms), n=len(ms))


def main():
    import torch as T
    np = bench.np
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    report = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'bev_voxel_instances.txt')
    rp, builtins.print = builtins.print, (lambda *a, **k: None)       # (the accumulator narrates every integrate)
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    st_ = bench.Stepper(acc, pool)
    st_.fill()
    for _ in range(10):
        st_.step()
    builtins.print = rp
    store, gen = acc.store, acc.sem_bev_generator
    store.flush_pending()                            # both calls read the same stored coordinates, nothing owed
    store.flush_k1()
    split = int(bench.present_index(acc))
    poses = np.ascontiguousarray(acc._track.as_array(), dtype=np.float64)
    origin = poses[split].copy()
    px, view = gen.pixel_size, float(gen.view_size)
    prm = gen._raster_params(origin, np.eye(3), 0., 0., view, store.intensity_div255)
    n_points = int(store.sizes().sum())
    ctx, lib = store.ctx, store.ctx.lib
    max_points = store.max_window_points()
    dev = store.device
    z_step = (Z_HI - Z_LO) / NZ
    counts = T.empty((NZ, px, px), dtype=T.int32, device=dev)
    inst = T.empty((NZ, px, px), dtype=T.int32, device=dev)
    ids = T.empty(max_points, dtype=T.int32, device=dev)
    table = T.empty((MAX_INSTANCES, 9), dtype=T.int32, device=dev)
    label_counts = T.empty((MAX_INSTANCES, 32), dtype=T.int32, device=dev)
    istats = T.empty(6, dtype=T.int64, device=dev)
    ws_v = T.empty(int(lib.pca_bev_voxel_workspace_bytes(max_points, px)), dtype=T.uint8, device=dev)
    ws_i = T.empty(int(lib.pca_bev_instances_workspace_bytes(max_points, px, NZ, MAX_INSTANCES)), dtype=T.uint8, device=dev)
    cst = store.c_store()

    def calls_of(classes, min_points=1):
        label_of, n_labels = gen.voxel_label_table([[c] for c in classes])

        def labels():
            ctx.check(lib.pca_bev_voxel_labels(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                               C.byref(prm), Z_LO, z_step, NZ, label_of.ctypes.data, n_labels, 0, None, None, 0,
                                               ws_v.data_ptr(), ws_v.numel(), None, counts.data_ptr(), None, ctx.stream()))

        def instances():
            ctx.check(lib.pca_bev_voxel_instances(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                                  C.byref(prm), Z_LO, z_step, NZ, label_of.ctypes.data, n_labels, 0, min_points, 26,
                                                  1, MAX_INSTANCES, None, None, 0, ws_i.data_ptr(), ws_i.numel(), inst.data_ptr(),
                                                  ids.data_ptr(), table.data_ptr(), label_counts.data_ptr(), istats.data_ptr(),
                                                  ctx.stream()))
        return labels, instances

    def launches_of(call):
        """{kernel: launches} of ONE call, from the library's own profile."""
        ctx.profile(1)
        call()
        prof = ctx.profile_read()
        ctx.profile(0)
        return {k: prof[k][1] for k in LAUNCHES}

    dyn_classes = gen.dynamic_classes()
    cases = [('the four dynamic classes ' + str(dyn_classes), dyn_classes), (f'one class [{dyn_classes[0]}]', dyn_classes[:1])]
    results = []
    for label, classes in cases:
        labels, instances = calls_of(classes)
        for _ in range(3):
            labels()
            instances()
        T.cuda.synchronize()
        t_labels = timed(labels, T, reps, instances)
        whole = timed(instances, T, reps, labels)
        ctx.profile(1)
        for _ in range(reps):
            instances()
        prof = ctx.profile_read()
        ctx.profile(0)
        per_kernel = {k: 1e3 * prof[k][0] / reps for k in LAUNCHES}          # per CALL (merge and compress: two launches)
        launches = launches_of(instances)
        assert launches == LAUNCHES, launches
        results.append(dict(classes=label, labels_call=stats(t_labels), call=stats(whole), kernels_us=per_kernel,
                            stats=istats.cpu().numpy().tolist(), launches=launches))
    # a very different mask: no voxel reaches min_points -- the same launches
    _, nothing = calls_of(dyn_classes, min_points=1 << 30)
    launches = launches_of(nothing)
    assert launches == LAUNCHES and istats.cpu().numpy().tolist()[1:] == [0] * 5, (launches, istats)
    out = dict(window=dict(frames=store.n_frames, points=n_points, px=px, nz=NZ, z_lo=Z_LO, z_step=z_step, view=view),
               launches_per_call=LAUNCHES, cases=results)
    print(json.dumps(out))

    lines = [
        '# pca_bev_voxel_instances beside pca_bev_voxel_labels (the yardstick) on the headline window of bench.py',
        f'# tools/experiments/bev_voxel_instances_timing.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and',
        f'# stepped into steady state, nothing owed; whole calls alternated with the labels call (counts only), an event pair around',
        f'# each, {reps} timed after a warm-up; the kernels from the library\'s per-launch events, the mean per call of {reps} calls.',
        '# The benchmark\'s classes are uniform over the window: the foreground fills the grid here, unlike real data.',
        f'window            {store.n_frames} frames, {n_points} stored points; {px} x {px}, {view:g} m view, nz = {NZ} over z [{Z_LO}, {Z_HI})'
        f' (z_step {z_step:g})',
        f'call              connectivity 26, min_points 1, min_voxels 1, max_instances {MAX_INSTANCES}, every output asked for',
        '',
    ]
    for r in results:
        k = r['kernels_us']
        own = sum(v for name, v in k.items() if name.startswith('bev_inst'))
        lines += [
            f'{r["classes"]}',
            f'  pca_bev_voxel_labels (counts only)  call median {r["labels_call"]["median_us"]:.1f} us'
            f' (min {r["labels_call"]["min_us"]:.1f}, max {r["labels_call"]["max_us"]:.1f})',
            f'  pca_bev_voxel_instances             call median {r["call"]["median_us"]:.1f} us (min {r["call"]["min_us"]:.1f},'
            f' max {r["call"]["max_us"]:.1f}) = {r["call"]["median_us"] / max(r["labels_call"]["median_us"], 1e-9):.2f} x the labels call',
            f'  its voxel pass: bev_voxel_bin {k["bev_voxel_bin"]:.1f} us, bev_voxel_cells {k["bev_voxel_cells"]:.1f} us;'
            f' its own ten launches {own:.1f} us:',
            f'    init {k["bev_inst_init"]:.1f}, merge (2) {k["bev_inst_merge"]:.1f}, compress (2) {k["bev_inst_compress"]:.1f},'
            f' sums {k["bev_inst_sums"]:.1f}, offsets {k["bev_inst_offsets"]:.1f}, number {k["bev_inst_number"]:.1f},'
            f' write {k["bev_inst_write"]:.1f}, points {k["bev_inst_points"]:.1f} us',
            f'  stats: kept points {r["stats"][0]}, foreground voxels {r["stats"][1]}, components {r["stats"][2]}, surviving'
            f' {r["stats"][3]}, kept points with an instance {r["stats"][4]}, voxels of the largest {r["stats"][5]}',
            '',
        ]
    lines += [
        'launches per call (asserted on the profile\'s launch counts for both cases and for a call whose min_points no voxel reaches):',
        '  ' + ', '.join(f'{k} {v}' for k, v in LAUNCHES.items()),
        'CCL form in the tree: the plain one (global union-find over the whole grid, a row phase and a compress before the rest of',
        '  the neighbourhood); the tile-local LDS stage was not built, so there is no second number to set beside it.',
    ]
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
