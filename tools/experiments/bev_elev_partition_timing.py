"""Times pca_bev_elev_partition beside one main raster (pca_bev_generate_chain through DeviceStore.bev) on the headline window
of bench.py: ~200 live frames, ~5 M stored points, 256 x 256, 80 m view.  The calls are timed alternately in one process with
event pairs after a warm-up; a second round with the library's per-kernel events (hipEvent pairs around every launch) gives
each kernel's time -- once with the flags and once without them, which is what the scattered one-byte flag stores of level 2
cost.  Bytes come from the kernels' own counts (`counts`: the records) and the shapes: level 1 reads 25 B per stored point
(x, y, z, dyn), writes 16 B per record, 1 B per point that is not in view, and its column of the table; level 2 reads the
table and every record twice (16 B; the second pass finds them in L2), writes 1 B per record, 9 B per cell and 24 B per tile.
Writes a text report (default profiles/bev_elev_partition.txt) and prints one JSON line.
Usage: python tools/experiments/bev_elev_partition_timing.py [reps] [report path]"""
import builtins
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HBM_PEAK = 8.0e12                                   # B/s, the part's specification (achievable with plain copies: ~6.3e12)
THRESH = 0.2


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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    report = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'bev_elev_partition.txt')
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
    prm = gen._raster_params(origin, bench.np.eye(3), 0., 0., float(gen.view_size), store.intensity_div255)
    n_points = int(store.sizes().sum())
    ctx, lib = store.ctx, store.ctx.lib
    max_points = store.max_window_points()
    ws = T.empty(int(lib.pca_bev_elev_workspace_bytes(max_points, px)) + 256, dtype=T.uint8, device=store.device)
    elev = T.empty((px, px), dtype=T.float64, device=store.device)
    obs = T.empty((px, px), dtype=T.uint8, device=store.device)
    flags = T.empty(max_points, dtype=T.uint8, device=store.device)
    counts = T.empty(3, dtype=T.int64, device=store.device)
    cst = store.c_store()

    def call(with_flags=True, with_counts=True):
        ctx.check(lib.pca_bev_elev_partition(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                             C.byref(prm), THRESH, 0, None, None, 0, ws.data_ptr(), ws.numel(), elev.data_ptr(),
                                             obs.data_ptr(), flags.data_ptr() if with_flags else None,
                                             counts.data_ptr() if with_counts else None, ctx.stream()))

    def raster():
        store.bev(split, prm)

    def raster_no_hint():
        cull, store.cull = store.cull, False
        try:
            store.bev(split, prm)
        finally:
            store.cull = cull

    def python_call():
        store.bev_elev_partition(prm, THRESH)

    call()
    n_in, n_el, _ = (int(v) for v in counts.tolist())
    for _ in range(5):
        raster()
        raster_no_hint()
        call()
        call(with_flags=False)
        python_call()
    T.cuda.synchronize()
    t_call = timed(call, T, reps, raster)
    t_noflags = timed(lambda: call(with_flags=False), T, reps, raster)
    t_raster = timed(raster, T, reps, call)
    t_raster_all = timed(raster_no_hint, T, reps, call)
    # per kernel (events around every launch: slower end to end, only the kernels' own times are read); without the totals'
    # tail launch, which shares the second kernel's id
    kern = {}
    for name, with_flags in (('flags', True), ('no_flags', False)):
        ctx.profile(1)
        for _ in range(reps):
            call(with_flags=with_flags, with_counts=False)
            raster_no_hint()
        prof = ctx.profile_read()
        ctx.profile(0)
        kern[name] = {k: 1e3 * ms / n for k, (ms, n) in prof.items() if n}
    T_tiles = ((px + 7) // 8) ** 2
    G = min(512, max(1, -(-max_points // 8192)))
    Gr = 8 * ((G + 7) // 8) if G >= 16 else G
    table = T_tiles * Gr * 8
    b1 = 25 * n_points + 16 * n_in + (n_points - n_in) + table
    b2 = table + 2 * 16 * n_in + n_in + px * px * 9 + T_tiles * 24
    frac = {}
    for name, b in (('bev_elev_bin', b1), ('bev_elev_cells', b2)):
        frac[name] = b / (kern['flags'][name] * 1e-6) / HBM_PEAK
    out = dict(window=dict(frames=store.n_frames, points=n_points, in_view=n_in, elevated=n_el, px=px, split=split, thresh=THRESH),
               elev_partition=stats(t_call), elev_partition_no_flags=stats(t_noflags), main_raster=stats(t_raster),
               main_raster_whole_window=stats(t_raster_all), per_kernel_us=kern, bytes=dict(level1=b1, level2=b2),
               fraction_of_hbm_peak=frac, workspace_bytes=int(lib.pca_bev_elev_workspace_bytes(max_points, px)))
    print(json.dumps(out))
    k, kn = kern['flags'], kern['no_flags']

    def row(label, s):
        return f'{label:<52}{s["median_us"]:8.1f} {s["min_us"]:8.1f} {s["max_us"]:8.1f}'

    lines = [
        '# pca_bev_elev_partition beside one main raster on the headline window of bench.py',
        f'# tools/experiments/bev_elev_partition_timing.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and',
        f'# stepped into steady state, nothing owed, then the calls alternated, an event pair around each, {reps} timed after 5 warm-up',
        '# rounds.  The main raster\'s code (pca_bev.hip) is the parent commit\'s, byte for byte: its time here is the parent\'s on this box.',
        f'window            {store.n_frames} frames, {n_points} stored points, {n_in} in view and static, {n_el} of them elevated above',
        f'                  their cell minimum + {THRESH} m, {px} x {px}, {float(gen.view_size):g} m view',
        '',
        f'{"":<52}  median      min      max   [us], n = {reps}',
        row('pca_bev_elev_partition, every output', out['elev_partition']),
        row('the same without the flags (elev, observed, counts)', out['elev_partition_no_flags']),
        row('one main raster (DeviceStore.bev, view hint on)', out['main_raster']),
        row('one main raster over the whole window (hint off)', out['main_raster_whole_window']),
        '',
        f'per kernel (library hipEvent pairs around every launch, a round of its own, no totals launch; mean of {reps}),',
        'bytes from the kernels\' own counts and the shapes, HBM peak 8.0 TB/s:',
        f'bev_elev_bin     {k["bev_elev_bin"]:6.1f} us  {b1 / 1e6:7.1f} MB = 25 B x {n_points} + 16 B x {n_in} records + 1 B x {n_points - n_in} flags + the table'
        f'   {b1 / k["bev_elev_bin"] / 1e6:5.2f} TB/s  {frac["bev_elev_bin"]:.2f} of peak',
        f'bev_elev_cells   {k["bev_elev_cells"]:6.1f} us  {b2 / 1e6:7.1f} MB = the table + 2 x 16 B x {n_in} + 1 B x {n_in} flags + 9 B x {px}^2 + 24 B x {T_tiles}'
        f'   {b2 / k["bev_elev_cells"] / 1e6:5.2f} TB/s  {frac["bev_elev_cells"]:.2f} of peak',
        f'without the flags: bev_elev_bin {kn["bev_elev_bin"]:.1f} us, bev_elev_cells {kn["bev_elev_cells"]:.1f} us -- the scattered one-byte flag stores of',
        f'level 2 cost {k["bev_elev_cells"] - kn["bev_elev_cells"]:.1f} us of its {k["bev_elev_cells"]:.1f}; the coalesced 255s of level 1 '
        f'{k["bev_elev_bin"] - kn["bev_elev_bin"]:.1f} us of its {k["bev_elev_bin"]:.1f}.',
        f'(bev_tile_bin {k.get("bev_bin", float("nan")):.1f} us and bev_tile_cells {k.get("bev_cells", float("nan")):.1f} us in the same round, whole window)',
    ]
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
