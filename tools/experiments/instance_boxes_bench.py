"""Times pca_bev_instance_boxes on the headline window of bench.py (~200 live frames, ~5 M stored points, 256 x 256, 80 m view,
nz = 32 over z [-2, 4.4)) in the two regimes profiles/bev_voxel_instances.txt describes, under both criteria:
  the four dynamic classes, max_instances 4096 -- one component of several hundred thousand voxels, so ONE row of very many
    pieces: the path that combines by 64-bit atomics;
  one class, max_instances 65536 -- tens of thousands of small rows: the path of one piece per row, plain stores.
The ids are those pca_bev_voxel_instances writes for the same window.  In one process, in blocks, the call is alternated with
  pca_bev_voxel_instances on the same window (the sibling it should cost about as much as), and
  the host form it replaces: .cpu() of the ids and of the window's coordinates, then the vectorised numpy of the test model
    (tests/instance_boxes_common.py) without its exact-fma repair.
Per case: medians and ranges over the blocks, every kernel from the library's own per-launch events (pca_profile_enable), the
stats and the number of global atomics the extents and the near kernel issue (from the row sizes: n_angles x 4, + 2 for z, and
n_angles per piece of a row of several pieces).  Writes a text report (default profiles/bev_instance_boxes.txt) and prints one
JSON line.
Usage: python tools/experiments/instance_boxes_bench.py [reps per block] [blocks] [report path]"""
import builtins
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NZ, Z_LO, Z_HI = 32, -2.0, 4.4
N_ANGLES, EDGE, PIECE = 90, 0.2, 2048
KERNELS = ('bev_box_table', 'bev_box_count', 'bev_box_offsets', 'bev_box_scatter', 'bev_box_extents', 'bev_box_near', 'bev_box_choose')


def event_ms(fn, T):
    a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    """Median of the block medians and their range [us]."""
    return dict(median_us=1e3 * statistics.median(ms), min_us=1e3 * min(ms), max_us=1e3 * max(ms), blocks=len(ms))


def host_form(np, ids, X, Y, Z, prm, n_rows, cs, criterion):
    """The numpy of the test model, unfused: (fit-like extents at t*, t*) -- what a host would run after the copies."""
    part = (ids >= 0) & (ids < n_rows)
    pid = ids[part].astype(np.int64)
    x, y = X[part] - prm.origin[0], Y[part] - prm.origin[1]
    ax = (prm.R[1] * y + prm.R[0] * x) + prm.dx
    ay = (prm.R[4] * y + prm.R[3] * x) + prm.dy
    order = np.argsort(pid, kind='stable')
    pid, ax, ay = pid[order], ax[order], ay[order]
    starts = np.flatnonzero(np.r_[True, np.diff(pid) != 0])
    used = pid[starts]
    n_angles = cs.shape[0]
    ext = np.empty((4, used.shape[0], n_angles))
    near = np.zeros((used.shape[0], n_angles), dtype=np.int64)
    row_of = np.repeat(np.arange(used.shape[0]), np.diff(np.r_[starts, pid.shape[0]]))
    for t in range(n_angles):                               # (direction by direction: [points, 90] at once is 3 GB on the large row)
        c, s = cs[t]
        e1, e2 = (c * ax + s * ay) + 0.0, (c * ay - s * ax) + 0.0
        ext[0, :, t], ext[1, :, t] = np.minimum.reduceat(e1, starts), np.maximum.reduceat(e1, starts)
        ext[2, :, t], ext[3, :, t] = np.minimum.reduceat(e2, starts), np.maximum.reduceat(e2, starts)
        if criterion == 1:
            d = np.minimum(np.minimum(e1 - ext[0, row_of, t], ext[1, row_of, t] - e1), np.minimum(e2 - ext[2, row_of, t], ext[3, row_of, t] - e2))
            near[:, t] = np.add.reduceat((d <= EDGE).astype(np.int64), starts)
    area = (ext[1] - ext[0]) * (ext[3] - ext[2])
    key = np.lexsort((area, -near), axis=1)[:, 0] if criterion == 1 else area.argmin(axis=1)
    return used, key


def main():
    import torch as T
    np = bench.np
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    report = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, 'profiles', 'bev_instance_boxes.txt')
    rp, builtins.print = builtins.print, (lambda *a, **k: None)       # (the accumulator narrates every integrate)
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    st_ = bench.Stepper(acc, pool)
    st_.fill()
    for _ in range(10):
        st_.step()
    builtins.print = rp
    store, gen = acc.store, acc.sem_bev_generator
    store.flush_pending()                            # every call reads the same stored coordinates, nothing owed
    store.flush_k1()
    from pca_amd.host_logic import fit_angles
    split = int(bench.present_index(acc))
    origin = np.ascontiguousarray(acc._track.as_array(), dtype=np.float64)[split].copy()
    px, view = gen.pixel_size, float(gen.view_size)
    prm = gen._raster_params(origin, np.eye(3), 0., 0., view, store.intensity_div255)
    n_points = int(store.sizes().sum())
    ctx, lib = store.ctx, store.ctx.lib
    max_points = store.max_window_points()
    dev = store.device
    z_step = (Z_HI - Z_LO) / NZ
    cs = fit_angles(N_ANGLES)
    cst = store.c_store()
    lo, hi = store.frame_off[[store.head, store.tail]].tolist()
    dyn_classes = gen.dynamic_classes()
    results = []
    for label, classes, rows in (('the four dynamic classes ' + str(dyn_classes), dyn_classes, 4096),
                                 (f'one class [{dyn_classes[0]}]', dyn_classes[:1], 65536)):
        label_of, n_labels = gen.voxel_label_table([[c] for c in classes])
        ids = T.empty(max_points, dtype=T.int32, device=dev)
        table = T.empty((rows, 9), dtype=T.int32, device=dev)
        istats = T.empty(6, dtype=T.int64, device=dev)
        ws_i = T.empty(int(lib.pca_bev_instances_workspace_bytes(max_points, px, NZ, rows)), dtype=T.uint8, device=dev)
        ws_b = T.empty(int(lib.pca_bev_instance_boxes_workspace_bytes(max_points, rows, N_ANGLES)), dtype=T.uint8, device=dev)
        fit = T.empty((rows, 8), dtype=T.float64, device=dev)
        fit_n = T.empty((rows, 2), dtype=T.int32, device=dev)
        bstats = T.empty(4, dtype=T.int64, device=dev)

        def instances():
            ctx.check(lib.pca_bev_voxel_instances(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                                  C.byref(prm), Z_LO, z_step, NZ, label_of.ctypes.data, n_labels, 0, 1, 26, 1, rows,
                                                  None, None, 0, ws_i.data_ptr(), ws_i.numel(), None, ids.data_ptr(), table.data_ptr(),
                                                  None, istats.data_ptr(), ctx.stream()))

        def boxes(criterion):
            ctx.check(lib.pca_bev_instance_boxes(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                                 C.byref(prm), ids.data_ptr(), rows, cs.ctypes.data, N_ANGLES, criterion, EDGE, None,
                                                 None, 0, ws_b.data_ptr(), ws_b.numel(), fit.data_ptr(), fit_n.data_ptr(), None, None,
                                                 bstats.data_ptr(), ctx.stream()))

        def host(criterion):
            t0 = time.perf_counter()
            h_ids = ids[:hi - lo].cpu().numpy()
            X, Y, Z = (a[lo:hi].cpu().numpy() for a in (store.x, store.y, store.z))
            t1 = time.perf_counter()
            used, key = host_form(np, h_ids, X, Y, Z, prm, rows, cs, criterion)
            return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1), used, key
        for _ in range(3):
            instances()
            boxes(0)
            boxes(1)
        T.cuda.synchronize()
        per = {'instances': [], 'area': [], 'edge': []}
        for _ in range(blocks):
            ms = {k: [] for k in per}
            for _ in range(reps):                       # alternated: each call meets the caches the others left
                ms['instances'].append(event_ms(instances, T))
                ms['area'].append(event_ms(lambda: boxes(0), T))
                ms['edge'].append(event_ms(lambda: boxes(1), T))
            for k in per:
                per[k].append(statistics.median(ms[k]))
        kernels = {}
        for name, criterion in (('area', 0), ('edge', 1)):
            ctx.profile(1)
            for _ in range(reps):
                boxes(criterion)
            prof = ctx.profile_read()
            ctx.profile(0)
            kernels[name] = {k: 1e3 * prof[k][0] / reps for k in KERNELS}
            assert all(prof[k][1] == (reps if k != 'bev_box_near' or criterion else 0) for k in KERNELS), prof
        hosts = {}
        for name, criterion in (('area', 0), ('edge', 1)):
            runs = [host(criterion) for _ in range(2)]
            hosts[name] = dict(copies_ms=min(r[0] for r in runs), numpy_ms=min(r[1] for r in runs))
            boxes(criterion)                             # the host form agrees with the call on t* (apart from fma ties)
            t_dev = fit[:, 7].cpu().numpy()[runs[0][2]]
            hosts[name]['t_agree'] = float((t_dev == runs[0][3]).mean())
        n_row = np.bincount(ids[:hi - lo].cpu().numpy().clip(-1, rows) + 1, minlength=rows + 2)[1:rows + 1]
        pieces = (n_row + PIECE - 1) // PIECE
        multi = int(pieces[pieces > 1].sum())
        results.append(dict(classes=label, n_rows=rows, stats=bstats.cpu().numpy().tolist(), inst_stats=istats.cpu().numpy().tolist(),
                            calls={k: spread(v) for k, v in per.items()}, kernels_us=kernels, host=hosts,
                            pieces=int(pieces.sum()), pieces_of_rows_of_several=multi,
                            atomics=dict(extents=multi * (4 * N_ANGLES + 2), near=multi * N_ANGLES)))
    out = dict(window=dict(frames=store.n_frames, points=n_points, px=px, nz=NZ, view=view), n_angles=N_ANGLES, edge_dist=EDGE,
               reps=reps, blocks=blocks, cases=results)
    print(json.dumps(out))

    lines = [
        '# pca_bev_instance_boxes beside pca_bev_voxel_instances (its sibling) and the host form, on the headline window of bench.py',
        f'# tools/experiments/instance_boxes_bench.py {reps} {blocks} -- one MI355X, one process: the accumulator of bench.py filled and',
        f'# stepped into steady state, nothing owed; the three calls alternated, an event pair around each, {blocks} blocks of {reps}: the',
        f'# median of the block medians and their range; the kernels from the library\'s per-launch events, the mean per call of {reps}.',
        '# The benchmark\'s classes are uniform over the window: the foreground fills the grid here, unlike real data.',
        f'window            {store.n_frames} frames, {n_points} stored points; {px} x {px}, {view:g} m view, nz = {NZ} over z [{Z_LO}, {Z_HI})',
        f'call              ids of pca_bev_voxel_instances (26, min_points 1, min_voxels 1), {N_ANGLES} directions of a quarter turn,'
        f' edge_dist {EDGE}; fit, fit_n and stats asked for',
        '',
    ]
    for r in results:
        c = r['calls']
        lines += [f'{r["classes"]}, n_rows {r["n_rows"]}',
                  f'  stats: points that take part {r["stats"][0]}, ids behind the rows {r["stats"][1]}, rows with a point {r["stats"][2]},'
                  f' points of the largest row {r["stats"][3]}; pieces {r["pieces"]}, of rows of several pieces {r["pieces_of_rows_of_several"]}',
                  f'  pca_bev_voxel_instances          call median {c["instances"]["median_us"]:.1f} us (blocks {c["instances"]["min_us"]:.1f} .. {c["instances"]["max_us"]:.1f})']
        for name in ('area', 'edge'):
            k, h = r['kernels_us'][name], r['host'][name]
            lines += [
                f'  pca_bev_instance_boxes, {name:4s}     call median {c[name]["median_us"]:.1f} us (blocks {c[name]["min_us"]:.1f} .. {c[name]["max_us"]:.1f})'
                f' = {c[name]["median_us"] / c["instances"]["median_us"]:.2f} x the sibling',
                '    ' + ', '.join(f'{n[8:]} {k[n]:.1f}' for n in KERNELS) + ' us',
                f'    host form: copies {h["copies_ms"]:.1f} ms + numpy {h["numpy_ms"]:.1f} ms = {1e3 * (h["copies_ms"] + h["numpy_ms"]) / c[name]["median_us"]:.0f} x the call'
                f' (t* equal on {100 * h["t_agree"]:.2f} % of the rows: the host form does not fuse)']
        lines += [f'  global atomics of the rows of several pieces: extents {r["atomics"]["extents"]} (64-bit min / max), near {r["atomics"]["near"]} (32-bit add)', '']
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
