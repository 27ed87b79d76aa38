#!/usr/bin/env python3
"""NuScenes sweep merge, host form against device form, on a NuScenes-shaped sample: 10 sweeps x 34 720 points, about 80
candidate boxes per sweep (tests/fake_nuscenes.synth_tables, its box tables tiled over the scene).

One process, the three forms alternating over warmed repeats:
  (a) datasets.nuscenes_sweeps.inst_centric_get_sweeps          host clock
  (b) datasets.nuscenes_sweeps.inst_centric_get_sweeps_device   host clock, from host arrays: dataset walk, upload, launches,
                                                                read-back, wait, bookkeeping
  (c) pca_nusc_merge_sweeps alone (table fetch + two launches)  device events
Writes the medians and ranges, the bytes and point-box tests computed from the shapes and (--resources FILE: the remarks of
`hipcc -Rpass-analysis=kernel-resource-usage` on csrc/pca_sweeps.hip) the kernels' resource lines to --out.
"""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'pc-accumulation-lib_amd'), ROOT, os.path.join(ROOT, 'tests')]


def scaled_tables(fk, n_records, n_pts, reps, seed=7):
    t = fk.synth_tables(seed, n_records, n_pts)
    rng = np.random.default_rng(seed + 1)
    nb = t['box_record'].shape[0]
    keys = [k for k in t if k.startswith('box_')]
    base = {k: t[k] for k in keys}
    for rep in range(1, reps):
        shift = np.concatenate([rng.uniform(-25, 25, (1, 2)).repeat(nb, 0), np.zeros((nb, 1))], axis=1)
        for k in keys:
            add = base[k]
            if k == 'box_center':
                add = add + shift
            elif k == 'box_instance':
                add = add + 8 * rep
            t[k] = np.concatenate([t[k], add], axis=0)
    return t


def resource_lines(path):
    if not path or not os.path.exists(path):
        return ['  kernel resources: not measured (no remarks file given)']
    out, name = [], None
    want = ('TotalSGPRs', 'VGPRs:', 'ScratchSize', 'Occupancy', 'LDS Size')
    vals = {}
    for line in open(path):
        m = re.search(r'remark:\s+(.*?) \[-Rpass', line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith('Function Name:'):
            if name:
                out.append('  %-12s %s' % (name, ', '.join(vals[w] for w in want if w in vals)))
            name, vals = re.sub(r'^_Z\d+', '', text.split(':', 1)[1].strip())[:10], {}
        for w in want:
            if text.startswith(w):
                vals[w] = text
    if name:
        out.append('  %-12s %s' % (name, ', '.join(vals[w] for w in want if w in vals)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nusc_sweeps.txt'))
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--sweeps', type=int, default=10)
    ap.add_argument('--points', type=int, default=34720)
    ap.add_argument('--reps', type=int, default=14, help='copies of the box tables (6 candidates per sweep each)')
    ap.add_argument('--resources', default='')
    args = ap.parse_args()

    import torch

    import fake_nuscenes as fk
    from datasets import nuscenes_sweeps as ns
    from pca_amd import _lib
    cfg = dict(fk.SWEEP_CFG, n_sweeps=args.sweeps)
    ctx = _lib.Context.get()
    with tempfile.TemporaryDirectory() as tmp:
        nusc = fk.FakeNuScenes(scaled_tables(fk, args.sweeps, args.points, args.reps), tmp, quaternion=lambda q: np.asarray(q))
        inputs = ns.collect_sweep_inputs(nusc, 'sample0', cfg['n_sweeps'], cfg['detection_classes'])
        raw, st, bt = ns.sweep_tables(inputs)
        n, nsw, nb = raw.shape[0], st.shape[0], bt.shape[0]
        tests = int(sum(int(s['n_rows']) * int(s['n_boxes']) for s in st))
        raw_dev = torch.from_numpy(raw).cuda()
        pad = ns._tally_words(nsw, nb)
        res = torch.empty(pad + 8 * n, dtype=torch.int32, device='cuda')
        ws = torch.empty(int(ctx.lib.pca_nusc_merge_sweeps_workspace_bytes(n, nb)), dtype=torch.uint8, device='cuda')

        def host():
            t0 = time.perf_counter()
            out = ns.inst_centric_get_sweeps(nusc, 'sample0', **cfg)
            return (time.perf_counter() - t0) * 1e3, out

        def device():
            t0 = time.perf_counter()
            out = ns.inst_centric_get_sweeps_device(nusc, 'sample0', **cfg)
            return (time.perf_counter() - t0) * 1e3, out

        def launches():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ctx.check(ctx.lib.pca_nusc_merge_sweeps(ctx.h, raw_dev.data_ptr(), n, st.ctypes.data, nsw, bt.ctypes.data, nb,
                                                    cfg['center_radius'], 0.5 + cfg['in_box_tolerance'], ws.data_ptr(), ws.numel(),
                                                    res.data_ptr() + 4 * pad, res.data_ptr(), ctx.stream()))
            b.record()
            b.synchronize()
            return a.elapsed_time(b), None

        forms = (('a host numpy', host), ('b device, host arrays -> dict', device), ('c launches alone (events)', launches))
        for _, fn in forms:                                  # warm-up: allocations, pinned blocks, code objects
            for _ in range(2):
                fn()
        _, h = host()
        _, d = device()
        same = np.array_equal(h['points'], d['points']) and h['instances_token'] == d['instances_token']
        times = {name: [] for name, _ in forms}
        for _ in range(args.repeats):
            for name, fn in forms:
                times[name].append(fn()[0])
    kept = h['points'].shape[0]
    lines = ['NuScenes sweep merge: %d sweeps x %d points = %d rows, %d candidate boxes (%s per sweep), %d point-box tests, '
             '%d rows kept, %d labelled' % (nsw, args.points, n, nb, '/'.join(str(int(s['n_boxes'])) for s in st), tests, kept,
                                            int((h['points'][:, 6] >= 0).sum())),
             'device result equals host result bit for bit: %s' % same,
             'bytes from the shapes: raw rows read %d (20 B/row; 16 used), staged rows written + read 2 x %d (20 B/kept row), '
             'rows out %d (32 B/kept row), tables %d' % (20 * n, 20 * kept, 32 * kept, 4096 + 176 * nb),
             '%d repeats, the forms alternating, after 2 warm-up runs each; milliseconds' % args.repeats]
    for name, _ in forms:
        v = np.array(times[name])
        lines.append('  %-34s median %9.3f   min %9.3f   max %9.3f' % (name, np.median(v), v.min(), v.max()))
    lines.append('kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):')
    lines += resource_lines(args.resources)
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
