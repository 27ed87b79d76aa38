"""Times pca_bev_class_planes (8 class groups) beside one main raster (pca_bev_generate_chain through DeviceStore.bev) on the
headline window of bench.py: ~200 live frames, ~5 M stored points, 256 x 256.  The two are timed alternately in one process
with event pairs after a warm-up; a second round with the library's per-kernel events gives each kernel's share.  The main
raster is the only way to get ONE such plane without this call (dynobj_mask swapped), so 8 groups cost 8 of them.
Bytes are counted from the shapes (29 B per stored point, 2 B per kept record written and read back, the tables, the planes),
not from counters.  Prints one JSON line.  Usage: python tools/experiments/bev_class_planes_timing.py [reps]"""
import builtins
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HBM_PEAK = 8.0e12                                   # B/s, the part's specification (achievable with plain copies: ~6.3e12)
GROUPS = [[0], [1], [2], [8], [9], [13, 14, 15, 17], [5, 6, 7], [0, 1]]


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
    ng = len(GROUPS)

    def raster():
        store.bev(split, prm)

    def raster_no_hint():
        cull, store.cull = store.cull, False
        try:
            store.bev(split, prm)
        finally:
            store.cull = cull

    def planes():
        store.bev_class_planes(split, prm, GROUPS)

    cnt = store.bev_class_planes(split, prm, GROUPS, want_counts=True)[2]
    kept = int(cnt[2, ng].sum().item())
    for _ in range(5):
        raster()
        raster_no_hint()
        planes()
    T.cuda.synchronize()
    t_planes = timed(planes, T, reps, raster)
    t_raster = timed(raster, T, reps, planes)
    t_raster_all = timed(raster_no_hint, T, reps, planes)
    # per kernel (events around every launch: slower end to end, only the kernels' own times are read)
    ctx = store.ctx
    ctx.profile(1)
    for _ in range(reps):
        planes()
        raster_no_hint()
    prof = ctx.profile_read()
    ctx.profile(0)
    kern = {k: 1e3 * ms / n for k, (ms, n) in prof.items() if n}
    lib = ctx.lib
    T_tiles = ((px + 7) // 8) ** 2
    G = min(512, max(1, -(-store.max_window_points() // 8192)))
    Gr = 8 * ((G + 7) // 8) if G >= 16 else G
    table = T_tiles * Gr * 8
    b1 = 29 * n_points + 2 * kept + table
    b2 = table + 2 * kept + 3 * ng * px * px * (8 + 2)
    out = dict(window=dict(frames=store.n_frames, points=n_points, kept=kept, px=px, groups=ng, split=split),
               class_planes=stats(t_planes), main_raster=stats(t_raster), main_raster_whole_window=stats(t_raster_all),
               per_kernel_us=kern,
               bytes=dict(level1=b1, level2=b2, main_raster_formula='see DESIGN 4'),
               workspace_bytes=int(lib.pca_bev_class_workspace_bytes(store.max_window_points(), px)))
    for name, b in (('bev_class_bin', b1), ('bev_class_cells', b2)):
        if name in kern:
            out['bytes'][name + '_fraction_of_hbm_peak'] = b / (kern[name] * 1e-6) / HBM_PEAK
    out['ratio_planes_to_one_raster'] = out['class_planes']['median_us'] / out['main_raster']['median_us']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
