"""Times pca_bev_voxel_carve on the headline window of bench.py (~200 live frames, ~5 M stored points, 256 x 256, 80 m view,
nz = 32 over z [-2, 4.4)) beside pca_bev_voxel_rays, the yardstick: the same rays, marked instead of counted, timed in the same
process on the same box.  One sensor position per stored frame: the pose track.  The carve call is made with three class sets:
the generator's four dynamic classes, a single class, and NO class -- the last one has no candidate voxel, so its traversal
does every byte load of `cand` and not one atomic: what the loads alone cost.  The benchmark's classes are uniform over the
window, so candidate voxels are NOT sparse here, unlike real data.
Per case: the whole call with an event pair (alternated with the rays call), then the three kernels from the library's own
per-launch events (pca_profile_enable), the counted crossings (the sum of `cross`), the candidate voxels and the stats.
Writes a text report (default profiles/bev_voxel_carve.txt) and prints one JSON line.
Usage: python tools/experiments/bev_voxel_carve_timing.py [reps] [report path]"""
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
RULE = (1, 2, 1.0)                                  # end_margin, min_cross, ratio: the defaults
KERNELS = ('bev_carve_ends', 'bev_carve_rays', 'bev_carve_flags')


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
    from pca_amd import _lib
    np = bench.np
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    report = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'bev_voxel_carve.txt')
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
    assert poses.shape == (store.n_frames, 3), poses.shape   # row i of the track is frame i of the store
    origin = poses[split].copy()
    px, view = gen.pixel_size, float(gen.view_size)
    prm = gen._raster_params(origin, np.eye(3), 0., 0., view, store.intensity_div255)
    n_points = int(store.sizes().sum())
    ctx, lib = store.ctx, store.ctx.lib
    max_points = store.max_window_points()
    dev = store.device
    z_step = (Z_HI - Z_LO) / NZ
    seen = T.empty((NZ, px, px), dtype=T.uint8, device=dev)
    rstats = T.empty(4, dtype=T.int64, device=dev)
    hits = T.empty((NZ, px, px), dtype=T.int32, device=dev)
    cross = T.empty((NZ, px, px), dtype=T.int32, device=dev)
    flags = T.empty(max_points, dtype=T.uint8, device=dev)
    cstats = T.empty(6, dtype=T.int64, device=dev)
    ws = T.empty(int(lib.pca_bev_carve_workspace_bytes(max_points, px, NZ)), dtype=T.uint8, device=dev)
    org = T.from_numpy(poses).to(dev)
    cst = store.c_store()

    def rays():
        ctx.check(lib.pca_bev_voxel_rays(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                         C.byref(prm), Z_LO, z_step, NZ, 0, org.data_ptr(), None, None, 0, seen.data_ptr(),
                                         rstats.data_ptr(), ctx.stream()))

    def carve_of(classes):
        only = _lib.PcaClassGroup()
        only.mask[:] = list(_lib.class_mask(classes))

        def carve():
            ctx.check(lib.pca_bev_voxel_carve(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                              C.byref(prm), Z_LO, z_step, NZ, 0, org.data_ptr(), only, RULE[0], RULE[1], RULE[2],
                                              None, None, 0, ws.data_ptr(), ws.numel(), hits.data_ptr(), cross.data_ptr(),
                                              flags.data_ptr(), cstats.data_ptr(), ctx.stream()))
        return carve

    dyn_classes = gen.dynamic_classes()
    cases = [('the four dynamic classes ' + str(dyn_classes), dyn_classes), (f'one class [{dyn_classes[0]}]', dyn_classes[:1]),
             ('no class (no candidate voxel: the cand loads, not one atomic)', [])]
    for _ in range(3):
        rays()
        carve_of(dyn_classes)()
    T.cuda.synchronize()
    t_rays = timed(rays, T, reps, carve_of(dyn_classes))
    # the rays KERNEL alone, from the library's per-launch events
    ctx.profile(1)
    for _ in range(reps):
        rays()
    prof = ctx.profile_read()
    ctx.profile(0)
    rays_kernel_us = 1e3 * prof['bev_voxel_rays'][0] / max(prof['bev_voxel_rays'][1], 1)
    results = []
    for label, classes in cases:
        carve = carve_of(classes)
        carve()
        T.cuda.synchronize()
        whole = timed(carve, T, reps, rays)
        ctx.profile(1)
        for _ in range(reps):
            carve()
        prof = ctx.profile_read()
        ctx.profile(0)
        per_kernel = {k: 1e3 * prof[k][0] / max(prof[k][1], 1) for k in KERNELS}
        crossings = int(cross.view(T.int32).to(T.int64).sum().item())
        n_in_grid_ends = int(hits.to(T.int64).sum().item())
        st6 = cstats.cpu().numpy().tolist()
        flagged_voxels = int(((cross >= RULE[1]) & (cross.to(T.float64) >= RULE[2] * hits.to(T.float64)) & (cross > 0)).sum().item())
        results.append(dict(classes=label, call=stats(whole), kernels_us=per_kernel, crossings=crossings, ends_in_grid=n_in_grid_ends,
                            crossed_voxels=int((cross != 0).sum().item()), flagged_voxels=flagged_voxels, stats=st6))
    out = dict(window=dict(frames=store.n_frames, points=n_points, px=px, nz=NZ, z_lo=Z_LO, z_step=z_step, view=view), rule=RULE,
               voxel_rays_call=stats(t_rays), voxel_rays_kernel_us=rays_kernel_us, rays_stats=rstats.cpu().numpy().tolist(),
               cases=results)
    print(json.dumps(out))

    trav = [r['kernels_us']['bev_carve_rays'] for r in results]
    lines = [
        '# pca_bev_voxel_carve beside pca_bev_voxel_rays (the yardstick) on the headline window of bench.py',
        f'# tools/experiments/bev_voxel_carve_timing.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and',
        f'# stepped into steady state, nothing owed; whole calls alternated with the rays call, an event pair around each, {reps}',
        f'# timed after a warm-up; the kernels from the library\'s per-launch events, the mean of {reps} launches each.',
        '# The benchmark\'s classes are uniform over the window: candidate voxels are NOT sparse here, unlike real data.',
        f'window            {store.n_frames} frames, {n_points} stored points; {px} x {px}, {view:g} m view, nz = {NZ} over z [{Z_LO}, {Z_HI})'
        f' (z_step {z_step:g})',
        f'rule              end_margin {RULE[0]}, min_cross {RULE[1]}, ratio {RULE[2]:g}',
        '',
        f'pca_bev_voxel_rays   call (two memsets + kernel) median {out["voxel_rays_call"]["median_us"]:.1f} us'
        f' (min {out["voxel_rays_call"]["min_us"]:.1f}, max {out["voxel_rays_call"]["max_us"]:.1f});  kernel bev_voxel_rays {rays_kernel_us:.1f} us',
        '',
    ]
    for r in results:
        k = r['kernels_us']
        lines += [
            f'pca_bev_voxel_carve, {r["classes"]}',
            f'  call (four memsets + three kernels) median {r["call"]["median_us"]:.1f} us (min {r["call"]["min_us"]:.1f}, max {r["call"]["max_us"]:.1f})',
            f'  bev_carve_ends {k["bev_carve_ends"]:.1f} us, bev_carve_rays {k["bev_carve_rays"]:.1f} us'
            f' ({k["bev_carve_rays"] / max(rays_kernel_us, 1e-9):.2f} x bev_voxel_rays), bev_carve_flags {k["bev_carve_flags"]:.1f} us',
            f'  counted crossings (sum of cross) {r["crossings"]}, in {r["crossed_voxels"]} voxels; rays that end inside the grid {r["ends_in_grid"]}',
            f'  stats: take part {r["stats"][0]}, cast {r["stats"][1]}, not finite {r["stats"][2]}, too long {r["stats"][3]},'
            f' candidate points {r["stats"][4]}, flagged {r["stats"][5]}',
            '',
        ]
    lines += [
        f'the traversal with no candidate voxel (every cand load, no atomic) takes {trav[2]:.1f} us = {trav[2] / max(rays_kernel_us, 1e-9):.2f} x bev_voxel_rays;',
        f'  the atomic counts add {trav[0] - trav[2]:.1f} us with the four classes ({results[0]["crossings"]} atomics) and {trav[1] - trav[2]:.1f} us with one'
        f' ({results[1]["crossings"]} atomics).',
    ]
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
