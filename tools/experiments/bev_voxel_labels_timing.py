"""Times pca_bev_voxel_labels (nz = 32, 19 labels) beside pca_bev_class_planes with 16 groups on the headline window of
bench.py: ~200 live frames, ~5 M stored points, 256 x 256, 80 m view.  The class planes are the yardstick: the same scaffold,
the same bytes read, and code this change does not touch.  The two calls are timed alternately in one process with event pairs
after a warm-up; a second round with the library's per-kernel events (hipEvent pairs around every launch) gives each kernel's
time.  The host baseline is the numpy model of tests/voxel_labels_common.py on the window's rows, timed once with the wall
clock (copying the rows to the host not included), and compared with the device result.
Writes a text report (default profiles/bev_voxel_labels.txt) and prints one JSON line.
Usage: python tools/experiments/bev_voxel_labels_timing.py [reps] [report path]"""
import builtins
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))
import bench  # noqa: E402

NZ, N_LABELS, Z_LO, Z_HI, N_GROUPS = 32, 19, -2.0, 4.4, 16
SLAB_COUNTERS = 14336                               # VC_SLAB_COUNTERS of pca_bev_voxel.hip


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
    from pca_amd import _lib
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    report = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'bev_voxel_labels.txt')
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
    origin = acc._track.poses_window(split, split + 1)[0]
    px = gen.pixel_size
    prm = gen._raster_params(origin, np.eye(3), 0., 0., float(gen.view_size), store.intensity_div255)
    n_points = int(store.sizes().sum())
    ctx, lib = store.ctx, store.ctx.lib
    max_points = store.max_window_points()
    dev = store.device
    z_step = (Z_HI - Z_LO) / NZ
    table = np.full(256, 255, dtype=np.uint8)
    table[:N_LABELS] = np.arange(N_LABELS)
    ws_v = T.empty(int(lib.pca_bev_voxel_workspace_bytes(max_points, px)) + 256, dtype=T.uint8, device=dev)
    labels = T.empty((NZ, px, px), dtype=T.uint8, device=dev)
    counts = T.empty((NZ, px, px), dtype=T.int32, device=dev)
    top = T.empty((NZ, px, px), dtype=T.int32, device=dev)
    ws_c = T.empty(int(lib.pca_bev_class_workspace_bytes(max_points, px)) + 256, dtype=T.uint8, device=dev)
    cls_counts = T.empty((3, N_GROUPS + 1, px, px), dtype=T.int32, device=dev)
    cg = (_lib.PcaClassGroup * N_GROUPS)()
    for g in range(N_GROUPS):
        cg[g].mask[:] = list(_lib.class_mask([g]))
    cst = store.c_store()

    def voxel():
        ctx.check(lib.pca_bev_voxel_labels(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                           C.byref(prm), Z_LO, z_step, NZ, table.ctypes.data, N_LABELS, 0, None, None, 0,
                                           ws_v.data_ptr(), ws_v.numel(), labels.data_ptr(), counts.data_ptr(), top.data_ptr(),
                                           ctx.stream()))

    def klass():
        ctx.check(lib.pca_bev_class_planes(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.head + split,
                                           store.tail, max_points, C.byref(prm), cg, N_GROUPS, None, None, 0, ws_c.data_ptr(),
                                           ws_c.numel(), None, None, cls_counts.data_ptr(), ctx.stream()))

    for _ in range(5):
        voxel()
        klass()
    T.cuda.synchronize()
    t_voxel = timed(voxel, T, reps, klass)
    t_class = timed(klass, T, reps, voxel)
    ctx.profile(1)
    for _ in range(reps):
        voxel()
        klass()
    prof = ctx.profile_read()
    ctx.profile(0)
    kern = {k: 1e3 * ms / n for k, (ms, n) in prof.items() if n}
    n_kept = int(counts.sum(dtype=T.int64).item())
    n_static = int(cls_counts[2, N_GROUPS].sum(dtype=T.int64).item())
    # the host baseline: the numpy model on the same rows
    import voxel_labels_common as vc
    rows = store.rows()
    t0 = time.perf_counter()
    want = vc.model(rows, origin, np.eye(3), 0., 0., float(gen.view_size), px, gen.height_filter, Z_LO, z_step, NZ, table,
                    N_LABELS, False)
    host_s = time.perf_counter() - t0
    vc.compare({'labels': labels, 'counts': counts, 'top': top}, want)
    zs_max = SLAB_COUNTERS // (64 * N_LABELS)
    n_slabs = -(-NZ // zs_max)
    zs = -(-NZ // n_slabs)
    ratio1 = kern['bev_voxel_bin'] / kern['bev_class_bin']
    ratio2 = kern['bev_voxel_cells'] / kern['bev_class_cells']
    out = dict(window=dict(frames=store.n_frames, points=n_points, static_in_view=n_static, voxel_kept=n_kept, px=px, nz=NZ,
                           n_labels=N_LABELS, z_lo=Z_LO, z_step=z_step),
               voxel_labels=stats(t_voxel), class_planes_16=stats(t_class), per_kernel_us=kern, slabs=n_slabs, slab_bins=zs,
               level1_ratio=ratio1, level2_ratio=ratio2, host_model_s=host_s, equal_to_host_model=True)
    print(json.dumps(out))

    def row(label, s):
        return f'{label:<56}{s["median_us"]:8.1f} {s["min_us"]:8.1f} {s["max_us"]:8.1f}'

    lines = [
        '# pca_bev_voxel_labels beside pca_bev_class_planes (16 groups) on the headline window of bench.py',
        f'# tools/experiments/bev_voxel_labels_timing.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and',
        f'# stepped into steady state, nothing owed, then the two calls alternated, an event pair around each, {reps} timed after 5',
        '# warm-up rounds.  The class planes\' code (pca_bev_class.hip, pca_bev_side.h, pca_bev_view.h) is the parent commit\'s, byte',
        '# for byte: its time here is the parent\'s on this box.',
        f'window            {store.n_frames} frames, {n_points} stored points, {n_static} in view and static, {n_kept} of them labelled and inside',
        f'                  z [{Z_LO}, {Z_HI}) of the BEV frame; {px} x {px}, {float(gen.view_size):g} m view, nz = {NZ} (z_step {z_step:g}), {N_LABELS} labels',
        '',
        f'{"":<56}  median      min      max   [us], n = {reps}',
        row('pca_bev_voxel_labels, labels + counts + top', out['voxel_labels']),
        row(f'pca_bev_class_planes, {N_GROUPS} groups, counts only', out['class_planes_16']),
        '',
        f'per kernel (library hipEvent pairs around every launch, a round of its own; mean of {reps}):',
        f'level 1   bev_voxel_bin   {kern["bev_voxel_bin"]:6.1f} us    bev_class_bin   {kern["bev_class_bin"]:6.1f} us    ratio {ratio1:.2f}',
        f'level 2   bev_voxel_cells {kern["bev_voxel_cells"]:6.1f} us    bev_class_cells {kern["bev_class_cells"]:6.1f} us    ratio {ratio2:.2f}'
        f'    ({n_slabs} slabs of {zs} bins, {64 * zs * N_LABELS * 4} B of counters)',
        '',
        f'host baseline: the numpy model (tests/voxel_labels_common.py) on the same {n_points} rows, already on the host: {host_s:.2f} s'
        f' = {host_s * 1e6 / out["voxel_labels"]["median_us"]:.0f} x the device call;',
        'labels, counts and top of the device call equal the model\'s, every voxel.',
    ]
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
