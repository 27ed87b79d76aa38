"""Times pca_render_camera on the headline window of bench.py (~200 live frames, ~5 M stored points) rendered into a
1408 x 376 image through the accumulator's own p_velo_frame: radius 0, 1, 2, both forms of the atomic (load first, the
default, and PCA_RENDER_ALWAYS_ATOMIC=1), without and with a 4-deep chain of owed re-transforms.  Every case: HIP event pairs
around the call (two memsets + two kernels) after a warm-up, in one process; the cases are taken in turn, round after round,
so that a drift of the box hits them all alike; then the two kernels on their own (pca_profile_enable).  Beside it, as context
and not as a threshold: the same key minimum done with torch.Tensor.scatter_reduce_('amin') on PRECOMPUTED pixels and keys
(radius 0) -- what a user would write without the call, leaving out the projection itself.
Writes a text report (default profiles/render_camera.txt) and prints one JSON line.
Usage: python tools/experiments/render_camera_time.py [reps] [report path]"""
import builtins
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

W, H = 1408, 376


def main():
    import torch as T
    np = bench.np
    from pca_amd._lib import make_camera
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    report = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'render_camera.txt')
    rp, builtins.print = builtins.print, (lambda *a, **k: None)       # (the accumulator narrates every integrate)
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    st_ = bench.Stepper(acc, pool)
    st_.fill()
    for _ in range(10):
        st_.step()
    builtins.print = rp
    store = acc.store
    store.flush_pending()                            # nothing owed but what this script notes itself
    store.flush_k1()
    n_points = int(store.sizes().sum())
    P = np.asarray(acc.P_velo_frame, dtype=np.float64)[:3]
    # four small rigid transforms, owed by every frame: what four integrate() calls without a raster in between leave
    chain = []
    for k in range(4):
        a = 0.002 * (k + 1)
        Tm = np.eye(4)
        Tm[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        Tm[:3, 3] = [-0.8, 0.01 * k, 0.002]
        chain.append((np.ascontiguousarray(Tm).reshape(16).copy(), store.tail))

    cases = [(r, aa, owed) for owed in (0, 4) for r in (0, 1, 2) for aa in (0, 1)]
    cams = {r: make_camera(P, W, H, r, True) for r in (0, 1, 2)}
    cam_cls = make_camera(P, W, H, 0, False)
    classes = list(range(19))

    def run(case):
        r, aa, owed = case
        os.environ['PCA_RENDER_ALWAYS_ATOMIC'] = str(aa)
        store._pending = list(chain[:owed])
        out = store.render_camera(cams[r])
        store._pending = []
        return out

    def run_cls():
        os.environ['PCA_RENDER_ALWAYS_ATOMIC'] = '0'
        return store.render_camera(cam_cls, classes=classes)

    def event_ms(fn):
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    # the user's form, radius 0: pixels and keys of the kept points precomputed (from the call's own result: the winner's
    # index and depth per pixel would not do -- every kept point must compete), then fill + scatter_reduce_
    x, y, z = (t[store.lb_head:store.lb_head + n_points] for t in (store.x, store.y, store.z))
    Pt = T.from_numpy(P).to(store.device)
    fx, fy, d = (Pt[k, 0] * x + Pt[k, 1] * y + Pt[k, 2] * z + Pt[k, 3] for k in range(3))
    u, v = T.round(fx / d.abs()), T.round(fy / d.abs())
    keep = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (d > 0)
    pix = (v[keep] * W + u[keep]).to(T.int64)
    key = (d[keep].to(T.float32).view(T.int32).to(T.int64) << 32) | T.nonzero(keep).squeeze(1)
    buf = T.empty(H * W, dtype=T.int64, device=store.device)

    def scatter():
        buf.fill_(0x7fffffffffffffff)
        buf.scatter_reduce_(0, pix, key, 'amin')

    for case in cases:                               # warm-up: every case twice
        run(case)
        run(case)
    run_cls()
    scatter()
    T.cuda.synchronize()
    ms = {case: [] for case in cases}
    ms_cls, ms_scatter, stats = [], [], {}
    for _ in range(reps):
        for case in cases:
            t, out = event_ms(lambda: run(case))
            ms[case].append(t)
            stats[case] = out
        ms_cls.append(event_ms(run_cls)[0])
        ms_scatter.append(event_ms(scatter)[0])
    # the two kernels on their own (pca_profile_enable(1): an event pair around every launch), the default form
    per_kernel = {}
    ctx = store.ctx
    for r in (0, 1, 2):
        T.cuda.synchronize()
        ctx.profile(1)
        for _ in range(reps):
            run((r, 0, 0))
        prof = ctx.profile_read()
        ctx.profile(0)
        per_kernel[r] = [1e3 * prof[k][0] / max(prof[k][1], 1) for k in ('render_zbuffer', 'render_resolve')]
    os.environ.pop('PCA_RENDER_ALWAYS_ATOMIC', None)
    stats = {case: o['stats'].cpu().numpy().tolist() for case, o in stats.items()}
    cls_stats = run_cls()['stats'].cpu().numpy().tolist()

    def summary(t, points, bytes_per_point):
        med = statistics.median(t)
        return dict(median_us=1e3 * med, min_us=1e3 * min(t), max_us=1e3 * max(t), n=len(t),
                    gbytes_per_s=points * bytes_per_point / (med * 1e-3) / 1e9)

    # the bytes the pass must read: 24 B of coordinates and 1 B of dyn per point (dyn only where include_dyn is off), 4 B of
    # rgbs where a class set is given
    res = {case: summary(ms[case], n_points, 24) for case in cases}
    res_cls = summary(ms_cls, n_points, 29)
    res_scatter = summary(ms_scatter, int(pix.numel()), 16)
    out = dict(window=dict(frames=store.n_frames, points=n_points, W=W, H=H),
               cases=[dict(radius=c[0], always_atomic=c[1], owed=c[2], stats=stats[c], **res[c]) for c in cases],
               per_kernel_us={str(r): v for r, v in per_kernel.items()}, class_set=dict(stats=cls_stats, **res_cls), scatter_reduce=dict(points=int(pix.numel()), **res_scatter))
    print(json.dumps(out))

    def row(label, s_, st):
        return f'{label:<58}{s_["median_us"]:9.1f} {s_["min_us"]:9.1f} {s_["max_us"]:9.1f} {s_["gbytes_per_s"]:9.0f}   {st[1]:>8} {st[2]:>8}'

    lines = ['# pca_render_camera on the headline window of bench.py',
             f'# tools/experiments/render_camera_time.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and stepped',
             f'# into steady state, nothing owed but the chain noted here; the cases in turn, round after round, an event pair around each',
             f'# call (two memsets, render_zbuffer, render_resolve), {reps} timed after two warm-up calls per case.',
             f'window            {store.n_frames} frames, {n_points} stored points; image {W} x {H}, P = the accumulator\'s p_velo_frame',
             'GB/s              on the bytes the pass must read: 24 B of coordinates per stored point (+ 1 B dyn, + 4 B rgbs in the last row)',
             '',
             f'{"":<58}   median       min       max      GB/s       kept  covered   [us], n = {reps}']
    for c in cases:
        form = 'every atomic issued' if c[1] else 'load first (default)'
        lines.append(row(f'radius {c[0]}, {form}, owed chain of {c[2]}', res[c], stats[c]))
    lines += [row('radius 0, load first, include_dyn off, class set of 19', res_cls, cls_stats),
              '',
              f'per kernel, load first, no owed chain (an event pair around every launch, mean of {reps}):',
              *(f'  radius {r}: render_zbuffer {per_kernel[r][0]:7.1f} us ({n_points * 24 / per_kernel[r][0] / 1e3:5.0f} GB/s on the coordinates),'
                f' render_resolve {per_kernel[r][1]:5.1f} us' for r in (0, 1, 2)),
              '  (the rest of a call: the two memsets and the gaps between four stream operations issued from Python)',
              '',
              'context, not a threshold: the same minimum with torch on precomputed pixels and keys (no projection, radius 0):',
              f'  fill_ + scatter_reduce_(amin) over {int(pix.numel())} kept points: median {res_scatter["median_us"]:.1f} us'
              f' (min {res_scatter["min_us"]:.1f}, max {res_scatter["max_us"]:.1f})']
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
