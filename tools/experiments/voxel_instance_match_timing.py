"""Times pca_voxel_instance_match on the instance volumes of the headline window of bench.py (256 x 256 x 32, 80 m view, z [-2,
4.4)): two samples one integrate() step apart, the index map from the accumulator's own store_frame(), in the two regimes
profiles/bev_voxel_instances.txt describes:
  the four dynamic classes, rows 4096 -- the benchmark's classes are uniform over the window, so the foreground is mostly ONE
    component: few pairs, long runs of equal keys;
  one class, rows 65536 -- tens of thousands of small components: a busy pair table, short runs.

  python tools/experiments/voxel_instance_match_timing.py [reps] [report path] [--trace DIR]
      whole calls between event pairs on preallocated outputs (all but track_ids), alternated call by call in this process with
      the same call with PCA_VOXEL_MATCH_FOLD=0 (every voxel its own atomics) and with pca_bev_voxel_instances over the same
      window (the sibling that makes the volumes); then the host form the call replaces, .cpu() of both volumes plus the numpy
      model of tests/voxel_tracks_common.py, which must agree with the call; and the global atomics the count kernel issues
      per cur voxel with and without folding, counted on the host from the volumes (runs of equal keys per 64-lane segment).
      --trace DIR: the per-kernel rows of rocprofv3's *kernel_stats.csv under DIR go into the report.
  python tools/experiments/voxel_instance_match_timing.py --kernels [calls]
      only the calls, folded then unfolded, for `rocprofv3 --kernel-trace --stats -- python ... --kernels`.
Writes a text report (default profiles/voxel_instance_match.txt) and prints one JSON line."""
import builtins
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

sys.path.append(os.path.join(ROOT, 'tests'))
NZ, Z_LO, Z_HI = 32, -2.0, 4.4
KERNELS = ('voxel_match_init', 'voxel_match_count', 'voxel_match_best', 'voxel_match_decide', 'voxel_match_relabel')


def samples():
    """The two regimes: per case the instance volumes of two samples one step apart, M, and what the sibling call needs."""
    import torch as T
    np = bench.np
    from pca_amd import host_logic as hl
    from pca_amd.tracks import grid_geom
    rp, builtins.print = builtins.print, (lambda *a, **k: None)       # (the accumulator narrates every integrate)
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    stepper = bench.Stepper(acc, pool)
    stepper.fill()
    for _ in range(10):
        stepper.step()
    store, gen = acc.store, acc.sem_bev_generator
    px, view = gen.pixel_size, float(gen.view_size)
    z_step = (Z_HI - Z_LO) / NZ
    dyn = gen.dynamic_classes()
    cases = [dict(name='the four dynamic classes', classes=[[c] for c in dyn], rows=4096),
             dict(name='one class, small components', classes=[dyn[:1]], rows=65536)]

    def sample(case):
        idx = int(bench.present_index(acc))
        out = acc.voxel_instances(idx, part='full', z_range=(Z_LO, Z_HI), nz=NZ, classes=case['classes'], max_instances=case['rows'])
        pc, rot_mat, _ = acc._unaugmented_part(idx, 'full')
        return out['inst'].clone(), grid_geom(pc.window.origin, rot_mat, 0., 0., view, px, Z_LO, z_step), acc.store_frame(), \
            out['stats'].cpu().numpy().tolist()
    first = [sample(c) for c in cases]
    stepper.step()
    store.flush_pending()
    store.flush_k1()
    for case, (prev, prev_geom, prev_frame, prev_stats) in zip(cases, first):
        cur, cur_geom, cur_frame, cur_stats = sample(case)
        case.update(prev=prev, cur=cur, M=hl.voxel_index_map(prev_geom, cur_geom, cur_frame @ np.linalg.inv(prev_frame)),
                    prev_stats=prev_stats, cur_stats=cur_stats)
    builtins.print = rp
    # the sibling on the window as it stands now
    split = int(bench.present_index(acc))
    origin = np.ascontiguousarray(acc._track.as_array(), dtype=np.float64)[split].copy()
    prm = gen._raster_params(origin, np.eye(3), 0., 0., view, store.intensity_div255)
    ctx, lib, dev = store.ctx, store.ctx.lib, store.device
    max_points = store.max_window_points()
    cst = store.c_store()
    for case in cases:
        rows = case['rows']
        label_of, n_labels = gen.voxel_label_table(case['classes'])
        keep = (T.empty(max_points, dtype=T.int32, device=dev), T.empty((rows, 9), dtype=T.int32, device=dev),
                T.empty(6, dtype=T.int64, device=dev), T.empty((NZ, px, px), dtype=T.int32, device=dev),
                T.empty(int(lib.pca_bev_instances_workspace_bytes(max_points, px, NZ, rows)), dtype=T.uint8, device=dev), label_of)

        def instances(keep=keep, rows=rows, n_labels=n_labels):
            ids, table, stats, inst, ws, label_of = keep
            ctx.check(lib.pca_bev_voxel_instances(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                                  C.byref(prm), Z_LO, z_step, NZ, label_of.ctypes.data, n_labels, 0, 1, 26, 1, rows,
                                                  None, None, 0, ws.data_ptr(), ws.numel(), inst.data_ptr(), ids.data_ptr(),
                                                  table.data_ptr(), None, stats.data_ptr(), ctx.stream()))
        case['instances'] = instances
    facts = dict(frames=store.n_frames, points=int(store.sizes().sum()), px=px, nz=NZ, view=view)
    return cases, store, facts


def match_call(store, case):
    """The C call on preallocated outputs: everything but track_ids (there are no per-point ids of a clone)."""
    import torch as T
    ctx, lib, dev = store.ctx, store.ctx.lib, store.device
    rows, cap = case['rows'], 4 * case['rows']
    nz, px = int(case['cur'].shape[0]), int(case['cur'].shape[1])
    ws = T.empty(int(lib.pca_voxel_instance_match_workspace_bytes(rows, rows, cap)), dtype=T.uint8, device=dev)
    i32 = dict(dtype=T.int32, device=dev)
    outs = dict(cur_track=T.empty(rows, **i32), match=T.empty(rows, **i32), cur_info=T.empty((rows, 4), **i32),
                prev_info=T.empty((rows, 4), **i32), track_vol=T.empty((nz, px, px), **i32), pairs=T.empty((cap, 3), **i32),
                stats=T.empty(10, dtype=T.int64, device=dev))
    counter = T.zeros(1, **i32)
    M = bench.np.ascontiguousarray(case['M'], dtype=bench.np.float64)

    def call():
        counter.zero_()
        ctx.check(lib.pca_voxel_instance_match(ctx.h, px, nz, case['prev'].data_ptr(), rows, case['cur'].data_ptr(), rows, M.ctypes.data,
                                               1, 0.0, cap, None, counter.data_ptr(), None, 0, ws.data_ptr(), ws.numel(),
                                               outs['cur_track'].data_ptr(), outs['match'].data_ptr(), outs['cur_info'].data_ptr(),
                                               outs['prev_info'].data_ptr(), outs['track_vol'].data_ptr(), None, outs['pairs'].data_ptr(),
                                               outs['stats'].data_ptr(), ctx.stream()))
    call.outs, call.keep = outs, (ws, counter, M)
    return call


def set_fold(on):
    if on:
        os.environ.pop('PCA_VOXEL_MATCH_FOLD', None)
    else:
        os.environ['PCA_VOXEL_MATCH_FOLD'] = '0'


def atomics_of(np, vt, prev, cur, rows, M):
    """Global atomics of the count kernel, unfolded (one per voxel and counter) and folded (one per run of equal keys within a
    64-lane segment of a line), as {counter: (unfolded, folded)}."""
    nz, px, _ = cur.shape
    q0, q1, q2, view = vt.images(cur.shape, M)
    ok_cur, ok_prev = (cur >= 0) & (cur < rows), (prev >= 0) & (prev < rows)
    view &= ok_cur
    a = np.full(cur.shape, -1, dtype=np.int64)
    a[view] = prev[np.floor(q2[view]).astype(np.int64), np.floor(q1[view]).astype(np.int64), np.floor(q0[view]).astype(np.int64)]
    pair = view & (a >= 0) & (a < rows)

    def runs(ok, *keys):
        """heads: the first lane of a segment, or a lane whose (ok, keys) differ from the lane before it; counted where ok"""
        head = np.ones(ok.shape, dtype=bool)
        same = ok[:, :, 1:] == ok[:, :, :-1]
        for k in keys:
            k = np.where(ok, k, 0)
            same &= k[:, :, 1:] == k[:, :, :-1]
        head[:, :, 1:] = ~same
        head[:, :, ::64] = True
        return int((head & ok).sum())
    seg_view = np.zeros(cur.shape, dtype=bool)                 # in_view is added once per b-run that holds a voxel in view
    cur_key = np.where(ok_cur, cur, 0)
    head = np.ones(cur.shape, dtype=bool)
    head[:, :, 1:] = (ok_cur[:, :, 1:] != ok_cur[:, :, :-1]) | (cur_key[:, :, 1:] != cur_key[:, :, :-1])
    head[:, :, ::64] = True
    run_id = np.cumsum(head.reshape(-1)).reshape(cur.shape)
    seg_view = int(np.unique(run_id[view]).size)
    return {'vox_cur': (int(ok_cur.sum()), runs(ok_cur, cur)), 'in_view': (int(view.sum()), seg_view),
            'pair table': (int(pair.sum()), runs(pair, a, cur)), 'vox_prev': (int(ok_prev.sum()), runs(ok_prev, prev))}


def trace_rows(directory):
    """{kernel: (calls, average ns, min ns, max ns)} of the voxel_match rows of rocprofv3's *kernel_stats.csv under `directory`."""
    out = {}
    for path in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                row = {k.strip().lower(): v for k, v in row.items() if k}
                name = row.get('name', '')
                if 'voxel_match' in name:
                    key = name.split('(')[0].replace('void ', '').strip()
                    out[key] = (int(row['calls']), float(row['averagens']), float(row['minns']), float(row['maxns']))
    return out


def main():
    import torch as T
    np = bench.np
    args = sys.argv[1:]
    if args and args[0] == '--kernels':
        cases, store, _ = samples()
        n = int(args[1]) if len(args) > 1 else 20
        for case in cases[:1] if len(args) > 2 and args[2] == 'first' else cases:
            call = match_call(store, case)
            for fold in (True, False):
                set_fold(fold)
                for _ in range(n):
                    call()
            T.cuda.synchronize()
        set_fold(True)
        return
    trace = None
    if '--trace' in args:
        at = args.index('--trace')
        trace = trace_rows(args[at + 1])
        del args[at:at + 2]
    reps = int(args[0]) if args else 20
    report = args[1] if len(args) > 1 else os.path.join(ROOT, 'profiles', 'voxel_instance_match.txt')
    import voxel_tracks_common as vt
    cases, store, facts = samples()

    def event_ms(fn):
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def summary(t, scale=1e3):
        return dict(median=scale * statistics.median(t), min=scale * min(t), max=scale * max(t), n=len(t))

    results = []
    for case in cases:
        call, instances, rows = match_call(store, case), case['instances'], case['rows']
        for _ in range(3):
            for fold in (True, False):
                set_fold(fold)
                call()
            instances()
        T.cuda.synchronize()
        ms = {'folded': [], 'unfolded': [], 'instances': []}
        for _ in range(reps):                               # alternated: each call meets the caches the others left
            set_fold(True)
            ms['folded'].append(event_ms(call))
            set_fold(False)
            ms['unfolded'].append(event_ms(call))
            ms['instances'].append(event_ms(instances))
        set_fold(True)
        call()
        T.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in call.outs.items()}
        host = []
        for _ in range(2):
            T.cuda.synchronize()
            t0 = time.perf_counter()
            prev, cur = case['prev'].cpu().numpy(), case['cur'].cpu().numpy()
            t1 = time.perf_counter()
            want = vt.model(prev, rows, cur, rows, case['M'])
            host.append((1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)))
        agree = all(np.array_equal(got[k], want[k]) for k in ('cur_track', 'match', 'track_vol', 'stats')) and \
            np.array_equal(vt.sorted_pairs(got['pairs']), want['pairs'])
        results.append(dict(name=case['name'], rows=rows, stats=got['stats'].tolist(), inst_stats=(case['prev_stats'], case['cur_stats']),
                            calls={k: summary(v) for k, v in ms.items()}, host=dict(copies_ms=min(h[0] for h in host), numpy_ms=min(h[1] for h in host)),
                            agrees_with_model=bool(agree), atomics=atomics_of(np, vt, prev, cur, rows, case['M'])))
    print(json.dumps(dict(window=facts, reps=reps, cases=results, trace=trace)))

    px, nz = facts['px'], facts['nz']
    lines = ['# pca_voxel_instance_match on the instance volumes of the headline window of bench.py, beside pca_bev_voxel_instances and the host form',
             f'# tools/experiments/voxel_instance_match_timing.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and stepped',
             '# into steady state; two samples one integrate() step apart, M from store_frame(); an event pair around each call, the calls',
             f'# alternated, {reps} timed after 3 warm-up rounds.  The benchmark\'s classes are uniform over the window, unlike real data.',
             f'window            {facts["frames"]} frames, {facts["points"]} stored points; volumes {px} x {px} x {nz} = {px * px * nz} voxels',
             'call              min_overlap 1, min_iou 0, cap_pairs 4 x rows; every output but track_ids', '']
    for r in results:
        s, c, h = r['stats'], r['calls'], r['host']
        lines += [f'{r["name"]}, rows {r["rows"]} (instances found: {r["inst_stats"][0][3]} then {r["inst_stats"][1][3]})',
                  f'  stats: cur voxels {s[0]}, in view {s[1]}, sum C {s[2]}, pairs {s[3]}, dropped {s[4]}, matched {s[5]}, new {s[6]}, lost {s[7]},'
                  f' skipped {s[8]} / {s[9]}; equal to the numpy model: {r["agrees_with_model"]}',
                  f'{"  whole calls [us]":<58}   median       min       max']
        for key, label in (('folded', 'pca_voxel_instance_match (runs folded, the default)'), ('unfolded', 'the same with PCA_VOXEL_MATCH_FOLD=0'),
                           ('instances', 'pca_bev_voxel_instances over the window (the sibling)')):
            lines.append(f'    {label:<54}{c[key]["median"]:9.1f} {c[key]["min"]:9.1f} {c[key]["max"]:9.1f}')
        total = h['copies_ms'] + h['numpy_ms']
        lines += [f'  host form: .cpu() of both volumes {h["copies_ms"]:.1f} ms + the numpy model {h["numpy_ms"]:.1f} ms = {total:.1f} ms'
                  f' = {1e3 * total / c["folded"]["median"]:.0f} x the call',
                  '  global atomics of the count kernel, unfolded -> folded (per cur voxel with a row):']
        for key, (u, f) in r['atomics'].items():
            lines.append(f'    {key:<12}{u:>10} -> {f:>10}   ({u / max(s[0], 1):.3f} -> {f / max(s[0], 1):.3f})')
        tu, tf = sum(u for u, _ in r['atomics'].values()), sum(f for _, f in r['atomics'].values())
        lines += [f'    {"all":<12}{tu:>10} -> {tf:>10}   ({tu / max(s[0], 1):.3f} -> {tf / max(s[0], 1):.3f})', '']
    if trace:
        lines.append('rocprofv3 --kernel-trace --stats over `--kernels` (both cases, folded and unfolded calls together; count: <true> folded, <false> not) [us]:')
        for k, (n, avg, lo, hi) in sorted(trace.items()):
            lines.append(f'  {k:<40}{n:6d} calls   mean {avg / 1e3:9.1f}   min {lo / 1e3:9.1f}   max {hi / 1e3:9.1f}')
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
