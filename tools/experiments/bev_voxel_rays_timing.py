"""Times pca_bev_voxel_rays on the headline window of bench.py (~200 live frames, ~5 M stored points, 256 x 256, 80 m view,
nz = 32 over z [-2, 4.4)) beside pca_bev_voxel_labels, whose code this change does not touch.  One sensor position per stored
frame: the pose track.  The two calls are timed alternately in one process with event pairs after a warm-up.  The steps per
ray (N of the contract: the voxel distance between the two ends, a closed form) come from the rows of the whole window on the
host; the share of steps inside the grid, the host model's time and the check of `seen` against the model are made on a
STATED SUBSAMPLE of frames (every 50th: the model walks every step in numpy) and are given as such, nothing is extrapolated
silently.  A lower bound of the kernel's time is derived from the step counts (see the report).
PCA_BEV_RAYS_STORE=1 in the environment times the A/B variant whose marks store without the load in front.
Writes a text report (default profiles/bev_voxel_rays.txt) and prints one JSON line.
Usage: python tools/experiments/bev_voxel_rays_timing.py [reps] [report path]"""
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

NZ, N_LABELS, Z_LO, Z_HI = 32, 19, -2.0, 4.4
SUB_EVERY = 50                                      # the subsample: every 50th frame of the window
N_SIMD, CLOCK_HZ, STEP_VALU = 1024, 2.4e9, 24       # SIMDs of the device, its clock, vector instructions of one step in the grid


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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    report = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'bev_voxel_rays.txt')
    variant = 'every mark stores (PCA_BEV_RAYS_STORE=1)' if os.environ.get('PCA_BEV_RAYS_STORE') == '1' else 'load, store where 0'
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
    sizes = store.sizes()
    n_points = int(sizes.sum())
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
    seen = T.empty((NZ, px, px), dtype=T.uint8, device=dev)
    rstats = T.empty(4, dtype=T.int64, device=dev)
    org = T.from_numpy(poses).to(dev)
    cst = store.c_store()

    def voxel():
        ctx.check(lib.pca_bev_voxel_labels(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                           C.byref(prm), Z_LO, z_step, NZ, table.ctypes.data, N_LABELS, 0, None, None, 0,
                                           ws_v.data_ptr(), ws_v.numel(), labels.data_ptr(), counts.data_ptr(), top.data_ptr(),
                                           ctx.stream()))

    def rays():
        ctx.check(lib.pca_bev_voxel_rays(ctx.h, C.byref(cst), store.frame_off.data_ptr(), store.head, store.tail, max_points,
                                         C.byref(prm), Z_LO, z_step, NZ, 0, org.data_ptr(), None, None, 0, seen.data_ptr(),
                                         rstats.data_ptr(), ctx.stream()))

    for _ in range(5):
        rays()
        voxel()
    T.cuda.synchronize()
    t_rays = timed(rays, T, reps, voxel)
    t_voxel = timed(voxel, T, reps, rays)
    dev_stats = rstats.cpu().numpy().tolist()
    seen_whole = seen.cpu().numpy()
    n_occupied = int((counts != 0).sum().item())
    n_free = int(((counts == 0) & (seen != 0)).sum().item())

    # the steps of the contract, whole window, on the host: N = the voxel distance between the two ends (no traversal needed)
    import voxel_rays_common as rc
    rows = store.rows()
    start = np.repeat(poses, sizes, axis=0)
    take = rows[:, 9] != 1
    s = rc.grid_coords(start[take], origin, np.eye(3), 0., 0., view, px, Z_LO, z_step)
    e = rc.grid_coords(rows[take, 0:3], origin, np.eye(3), 0., 0., view, px, Z_LO, z_step)
    N = np.abs(np.floor(e) - np.floor(s)).sum(axis=1)
    N = N[N <= rc.MAX_STEPS]
    steps_total, steps_mean, steps_max = float(N.sum()), float(N.mean()), int(N.max())
    # a wave runs as long as its longest ray: 64 consecutive points (a lane whose point is dynamic idles)
    Nw = np.zeros(rows.shape[0])
    Nw[take] = np.minimum(np.abs(np.floor(e) - np.floor(s)).sum(axis=1), rc.MAX_STEPS)
    pad = (-Nw.shape[0]) % 64
    wave_steps = float(np.concatenate([Nw, np.zeros(pad)]).reshape(-1, 64).max(axis=1).sum())

    # the stated subsample: the model walks every step
    sub = list(range(0, store.n_frames, SUB_EVERY))
    off = np.concatenate([[0], np.cumsum(sizes)])
    sub_frames = [rows[off[k]:off[k + 1]] for k in sub]
    t0 = time.perf_counter()
    want = rc.model(sub_frames, poses[sub], origin, np.eye(3), 0., 0., view, px, Z_LO, z_step, NZ, False)
    host_s = time.perf_counter() - t0
    sub_rays, sub_steps, sub_marks = int(want['stats'][1]), int(want['N'][want['N'] >= 0].sum()), int(want['marks'].sum())
    got_seen = np.zeros((NZ, px, px), dtype=np.uint8)
    got_stats = np.zeros(4, dtype=np.int64)
    for k in sub:                                    # (a call takes a contiguous range of frames: one call per frame, OR-ed)
        o = store.bev_voxel_rays(prm, Z_LO, z_step, NZ, poses[k:k + 1], first_frame=k, last_frame=k + 1)
        got_seen |= o['seen'].cpu().numpy()
        got_stats += o['stats'].cpu().numpy()
    equal = bool(np.array_equal(got_seen, want['seen']) and got_stats.tolist() == want['stats'].tolist())
    assert equal, 'the device result differs from the model on the subsample'
    assert not (want['seen'] & ~seen_whole).any()    # what the subsample's rays marked, the whole window's did too
    in_grid_share = sub_marks / max(sub_steps, 1)
    # lower bound: a step inside the grid costs a wave at least STEP_VALU vector instructions of 2 cycles each on its SIMD
    # (the shortest path through the loop's disassembly: range test 3, address 11, load and compare 2, axis choice 2, the
    # stepping axis 6), a wave runs as long as its longest ray, and the N_SIMD SIMDs share the waves evenly at best; counted
    # for the steps inside the grid only (share from the subsample), since a ray outside the grid may leave its loop early
    bound_us = wave_steps * in_grid_share * STEP_VALU * 2 / (N_SIMD * CLOCK_HZ) * 1e6
    out = dict(window=dict(frames=store.n_frames, points=n_points, px=px, nz=NZ, z_lo=Z_LO, z_step=z_step, view=view),
               variant=variant, voxel_rays=stats(t_rays), voxel_labels=stats(t_voxel), stats=dev_stats,
               steps=dict(total=steps_total, mean=steps_mean, max=steps_max, wave_steps=wave_steps),
               seen_voxels=int(seen_whole.sum()), occupied=n_occupied, free=n_free, unseen=NZ * px * px - n_occupied - n_free,
               subsample=dict(frames=sub, rays=sub_rays, steps=sub_steps, in_grid_steps=sub_marks, host_model_s=host_s,
                              equal_to_host_model=equal, seen_voxels=int(want['seen'].sum())),
               lower_bound_us=bound_us)
    print(json.dumps(out))

    def row(label, s_):
        return f'{label:<56}{s_["median_us"]:9.1f} {s_["min_us"]:9.1f} {s_["max_us"]:9.1f}'

    med = out['voxel_rays']['median_us']
    lines = [
        '# pca_bev_voxel_rays beside pca_bev_voxel_labels on the headline window of bench.py',
        f'# tools/experiments/bev_voxel_rays_timing.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and',
        f'# stepped into steady state, nothing owed, then the two calls alternated, an event pair around each, {reps} timed after 5',
        '# warm-up rounds.  The occupancy labels\' code (pca_bev_voxel.hip, pca_bev_side.h, pca_bev_view.h) is the parent commit\'s,',
        '# byte for byte: its time here is the parent\'s on this box.  One sensor position per stored frame: the pose track.',
        f'variant           {variant}',
        f'window            {store.n_frames} frames, {n_points} stored points; {px} x {px}, {view:g} m view, nz = {NZ} over z [{Z_LO}, {Z_HI})'
        f' (z_step {z_step:g})',
        f'stats             points considered {dev_stats[0]}, rays cast {dev_stats[1]}, dropped not finite {dev_stats[2]}, dropped too long {dev_stats[3]}',
        f'voxels            {NZ * px * px}: occupied {n_occupied}, free {n_free}, unseen {NZ * px * px - n_occupied - n_free}  (seen by a ray: {int(seen_whole.sum())})',
        '',
        f'{"":<56}   median       min       max   [us], n = {reps}',
        row('pca_bev_voxel_rays, seen + stats (two memsets + kernel)', out['voxel_rays']),
        row(f'pca_bev_voxel_labels, {N_LABELS} labels: labels + counts + top', out['voxel_labels']),
        f'ratio of the medians: {med / out["voxel_labels"]["median_us"]:.1f}',
        '',
        'steps of the contract (N = voxel distance between sensor and point; whole window, closed form on the host):',
        f'  total {steps_total:.4g}, mean {steps_mean:.1f} per ray, max {steps_max};  as waves of 64 consecutive points run (the longest'
        f' ray of each): {wave_steps:.4g} wave-steps = {wave_steps * 64 / max(steps_total, 1):.2f} x the lanes\' own steps',
        f'  = {med * 1e3 / max(steps_total, 1):.4f} ns per contract step, {steps_total / max(med, 1e-9) / 1e3:.2f} G steps/s (a ray outside the grid leaves its loop early:',
        '  the kernel walks fewer steps than the contract counts)',
        '',
        f'subsample: frames {sub} of the window ({sub_rays} rays, {sub_steps} contract steps) -- NOT extrapolated:',
        f'  steps inside the grid (each one byte load, and a byte store where it read 0): {sub_marks} = {100 * in_grid_share:.1f} % of the steps;',
        f'  voxels marked {int(want["seen"].sum())}: {100 * int(want["seen"].sum()) / max(sub_marks, 1):.2f} % of the steps inside the grid had to store at least once',
        f'  the numpy model (tests/voxel_rays_common.py) on these rows, already on the host: {host_s:.1f} s;',
        '  seen and stats of the device (one call per frame of the subsample, OR-ed) equal the model\'s, every voxel.',
        '',
        f'lower bound from the step counts: wave-steps x the subsample\'s share inside the grid x {STEP_VALU} vector instructions (the',
        f'  shortest path of one step inside the grid in the disassembly) x 2 cycles / ({N_SIMD} SIMDs x {CLOCK_HZ / 1e9:g} GHz) = {bound_us:.0f} us;',
        f'  the call is {med / max(bound_us, 1e-9):.1f} x that.  The bound leaves out what the loop really issues: the steps outside the grid (the',
        '  rest of the contract\'s steps, walked until an integer test lets the ray go), the scalar instructions and branches of',
        '  the three axis paths, which a wave whose lanes disagree walks one after the other (about 100 instructions per step',
        '  and wave in the disassembly), and the wait for the byte load of the step before.',
    ]
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
