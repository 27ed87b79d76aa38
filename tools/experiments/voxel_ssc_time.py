"""Times pca_voxel_pool and pca_voxel_pack, and the SSC sample they make against the host form they replace, on 256 x 256 x 32
volumes of the headline window of bench.py (~200 live frames, ~5 M stored points; 80 m view around the newest pose, identity
heading, z [-2, 4.4)): labels from pca_bev_voxel_labels (19 labels), seen from pca_bev_voxel_rays, visible from
pca_bev_voxel_camera through the accumulator's p_velo_frame (1408 x 376) -- the three passes voxel_visibility makes -- and
input_occ from the labels pass over the newest frame alone.  Two sets of volumes: 'headline', as they are, and 'thinned', one
occupied voxel in 64 kept (by a hash of its place; the camera pass is run again on the thinned labels).

  python tools/experiments/voxel_ssc_time.py --kernels headline|thinned [reps]
      only the two C calls, warmed up and repeated: the program to put behind `rocprofv3 --kernel-trace --stats -- `.
  python tools/experiments/voxel_ssc_time.py [reps] [report path] [--trace headline=<dir>] [--trace thinned=<dir>]
      event pairs around the two C calls (all three scales, every output; level 1, every payload) on preallocated outputs;
      then the SAMPLE both ways, alternated block after block in this process: device form = voxel_pyramid_device +
      write_ssc_sample through an AsyncBevWriter with 4 threads; host form = the level-1 volumes brought over with .cpu(), the
      numpy model of tests/voxel_ssc_common.py, the same ten files with open().write().  Both write to the same local
      directory; the files of the two forms are compared byte for byte once.  --trace folds the voxel_pool / voxel_pack rows
      of rocprofv3's kernel statistics found under <dir> into the report.
Writes a text report (default profiles/voxel_ssc.txt) and prints one JSON line."""
import builtins
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))
import bench  # noqa: E402

W, H = 1408, 376
NZ, N_LABELS, Z_LO, Z_HI = 32, 19, -2.0, 4.4
THIN = 64
BLOCKS, PER_BLOCK = 5, 4


def volumes_of():
    """({'headline' | 'thinned': (labels, seen, visible, input_occ)}, generator, window facts)."""
    import torch as T
    np = bench.np
    rp, builtins.print = builtins.print, (lambda *a, **k: None)       # (the accumulator narrates every integrate)
    acc, pool, _ = bench.make_accumulator(bench.synth_frame, 0)
    st_ = bench.Stepper(acc, pool)
    st_.fill()
    for _ in range(10):
        st_.step()
    builtins.print = rp
    store, gen = acc.store, acc.sem_bev_generator
    store.flush_pending()                            # nothing owed
    store.flush_k1()
    poses = np.ascontiguousarray(acc._track.as_array(), dtype=np.float64)
    assert poses.shape == (store.n_frames, 3), poses.shape
    px, view = gen.pixel_size, float(gen.view_size)
    prm = gen._raster_params(poses[-1].copy(), np.eye(3), 0., 0., view, store.intensity_div255)
    z_step = (Z_HI - Z_LO) / NZ
    table = np.full(256, 255, dtype=np.uint8)
    table[:N_LABELS] = np.arange(N_LABELS)
    dense = store.bev_voxel_labels(prm, Z_LO, z_step, NZ, table, N_LABELS)['labels']
    seen = store.bev_voxel_rays(prm, Z_LO, z_step, NZ, poses)['seen']
    one = store.bev_voxel_labels(prm, Z_LO, z_step, NZ, table, N_LABELS, first_frame=store.n_frames - 1)
    input_occ = (one['counts'] != 0).to(T.uint8)
    place = T.arange(dense.numel(), dtype=T.int64, device=dense.device).reshape(dense.shape)
    thinned = T.where(((place * 2654435761) >> 11) % THIN == 0, dense, T.full_like(dense, 255))
    cams = [(np.asarray(acc.P_velo_frame, dtype=np.float64)[:3], (W, H))]
    vols = {}
    for name, labels in (('headline', dense), ('thinned', thinned)):
        visible = store.bev_voxel_camera(prm, Z_LO, z_step, NZ, labels, cams, max_depth=view)['visible']
        vols[name] = (labels, seen, visible, input_occ if name == 'headline' else input_occ * (labels != 255).to(T.uint8))
    facts = dict(frames=store.n_frames, points=int(store.sizes().sum()), px=px, nz=NZ, view=view)
    return vols, gen, store, facts


def kernel_calls(store, vol):
    """(pool, pack): the two C calls on preallocated outputs -- all three scales with every output; level 1 with every payload."""
    import torch as T
    from pca_amd import _lib
    np = bench.np
    labels, seen, visible, input_occ = vol
    nz, px = int(labels.shape[0]), int(labels.shape[1])
    ctx, lib, dev = store.ctx, store.ctx.lib, store.device
    levels = (_lib.PcaVoxelPoolLevel * 3)()
    keep = []
    for lv, s in zip(levels, (2, 4, 8)):
        o = [T.empty((nz // s, px // s, px // s), dtype=T.uint8, device=dev) for _ in range(3)]
        keep.append(o)
        lv.scale, lv.labels, lv.state, lv.visible = s, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr()
    n = px * px * nz
    label_out = T.empty(n, dtype=T.uint16, device=dev)
    bits = [T.empty((n + 7) // 8, dtype=T.uint8, device=dev) for _ in range(3)]
    table = np.arange(1, 33, dtype=np.uint16)

    def pool():
        ctx.check(lib.pca_voxel_pool(ctx.h, px, nz, labels.data_ptr(), seen.data_ptr(), visible.data_ptr(), 1, 20, levels, 3, ctx.stream()))

    def pack():
        ctx.check(lib.pca_voxel_pack(ctx.h, px, nz, labels.data_ptr(), seen.data_ptr(), visible.data_ptr(), input_occ.data_ptr(),
                                     table.ctypes.data, 0, label_out.data_ptr(), bits[0].data_ptr(), bits[1].data_ptr(),
                                     bits[2].data_ptr(), ctx.stream()))
    pool.keep = (keep, label_out, bits, levels, table)
    return pool, pack


def trace_rows(directory):
    """{kernel: (calls, average ns, min ns, max ns)} of the voxel_pool / voxel_pack rows of rocprofv3's *kernel_stats.csv under `directory`."""
    out = {}
    for path in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                row = {k.strip().lower(): v for k, v in row.items() if k}
                for k in ('voxel_pool', 'voxel_pack'):
                    if k in row.get('name', ''):
                        out[k] = (int(row['calls']), float(row['averagens']), float(row['minns']), float(row['maxns']))
    return out


def main():
    import torch as T
    np = bench.np
    args = sys.argv[1:]
    if args and args[0] == '--kernels':
        vols, _, store, _ = volumes_of()
        pool, pack = kernel_calls(store, vols[args[1]])
        for _ in range(3 + (int(args[2]) if len(args) > 2 else 20)):
            pool()
            pack()
        T.cuda.synchronize()
        return
    traces = {}
    while '--trace' in args:
        at = args.index('--trace')
        name, directory = args[at + 1].split('=', 1)
        traces[name] = trace_rows(directory)
        del args[at:at + 2]
    reps = int(args[0]) if args else 20
    report = args[1] if len(args) > 1 else os.path.join(ROOT, 'profiles', 'voxel_ssc.txt')
    import voxel_ssc_common as model
    from pca_amd import ssc
    from pca_amd.writer import AsyncBevWriter
    vols, gen, store, facts = volumes_of()

    def event_ms(fn):
        a, b = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def summary(t, scale=1e3):
        return dict(median=scale * statistics.median(t), min=scale * min(t), max=scale * max(t), n=len(t))

    kernels, counts = {}, {}
    for name, vol in vols.items():
        pool, pack = kernel_calls(store, vol)
        for _ in range(3):
            pool()
            pack()
        T.cuda.synchronize()
        ms = {'pool': [], 'pack': []}
        for _ in range(reps):
            ms['pool'].append(event_ms(pool))
            ms['pack'].append(event_ms(pack))
        kernels[name] = {k: summary(v) for k, v in ms.items()}
        labels, seen, visible, input_occ = vol
        counts[name] = dict(occupied=int((labels != 255).sum().item()), seen=int((seen != 0).sum().item()),
                            visible=int((visible != 0).sum().item()), input_occ=int((input_occ != 0).sum().item()))

    # the sample both ways, on the headline volumes
    labels, seen, visible, input_occ = vols['headline']
    px, nz = facts['px'], facts['nz']
    out_dir = tempfile.mkdtemp(prefix='voxel_ssc_')
    writer = AsyncBevWriter(n_threads=4)

    def device_form(frame_id):
        ssc.write_ssc_sample(gen.voxel_pyramid_device(labels, seen, visible, input_occ), os.path.join(out_dir, 'device'), frame_id, writer=writer)

    def host_form(frame_id):
        host = [v.cpu().numpy() for v in (labels, seen, visible, input_occ)]
        packed = model.pyramid_model(*host)['packed']
        os.makedirs(os.path.join(out_dir, 'host'), exist_ok=True)
        for s, payloads in packed.items():
            for key, path in ssc.ssc_paths(os.path.join(out_dir, 'host'), frame_id, s).items():
                if key in payloads:
                    with open(path, 'wb') as f:
                        f.write(payloads[key].tobytes())

    device_form(0)
    writer.flush()
    host_form(0)
    names = sorted(os.listdir(os.path.join(out_dir, 'host')))
    assert names == sorted(os.listdir(os.path.join(out_dir, 'device'))) and len(names) == 10, names
    for n in names:
        with open(os.path.join(out_dir, 'host', n), 'rb') as a, open(os.path.join(out_dir, 'device', n), 'rb') as b:
            assert a.read() == b.read(), n
    file_bytes = sum(os.path.getsize(os.path.join(out_dir, 'host', n)) for n in names)
    rate = {'device': [], 'host': []}
    for block in range(BLOCKS):
        for form, fn in (('device', device_form), ('host', host_form)):
            T.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(PER_BLOCK):
                fn(1 + block * PER_BLOCK + k)
            if form == 'device':
                writer.flush()
            T.cuda.synchronize()
            rate[form].append(PER_BLOCK / (time.perf_counter() - t0))
    writer.close()
    rates = {k: summary(v, 1.) for k, v in rate.items()}
    ratio = rates['device']['median'] / rates['host']['median']
    out = dict(window=facts, volumes=counts, kernels_event_us=kernels, kernel_trace_ns=traces, samples_per_s=rates, ratio=ratio,
               files=len(names), file_bytes=file_bytes)
    print(json.dumps(out))

    voxels = nz * px * px
    lines = ['# pca_voxel_pool and pca_voxel_pack on the volumes of the headline window of bench.py, and the SSC sample against its host form',
             f'# tools/experiments/voxel_ssc_time.py {reps} -- one MI355X, one process: the accumulator of bench.py filled and stepped into',
             '# steady state, nothing owed; labels (19), seen and visible from the three passes voxel_visibility makes (grid around the',
             f'# newest pose, identity heading, camera p_velo_frame {W} x {H}), input_occ from the labels pass over the newest frame.',
             f'window            {facts["frames"]} frames, {facts["points"]} stored points; volumes {px} x {px} x {nz} = {voxels} voxels, {facts["view"]:.0f} m view, z [{Z_LO}, {Z_HI})',
             *(f'{name:<18}occupied {c["occupied"]}, seen {c["seen"]}, visible {c["visible"]}, input_occ {c["input_occ"]}'
               + ('' if name == 'headline' else f'  (one occupied voxel in {THIN} kept)') for name, c in counts.items()),
             '',
             f'C calls, an event pair around each on preallocated outputs, {reps} timed after 3 warm-up rounds            median       min       max   [us]']
    for name in kernels:
        lines.append(f'{name + ": pca_voxel_pool, scales 2 4 8, labels + state + visible (one launch)":<96}'
                     f'{kernels[name]["pool"]["median"]:9.1f} {kernels[name]["pool"]["min"]:9.1f} {kernels[name]["pool"]["max"]:9.1f}')
        lines.append(f'{name + ": pca_voxel_pack, level 1, label + invalid + occluded + bin (one launch)":<96}'
                     f'{kernels[name]["pack"]["median"]:9.1f} {kernels[name]["pack"]["min"]:9.1f} {kernels[name]["pack"]["max"]:9.1f}')
    lines += ['', 'kernel times, rocprofv3 --kernel-trace --stats, a run of its own per set of volumes (--kernels <set>: 3 warm-up rounds + 20):']
    if not traces:
        lines.append('  not measured in this run')
    for name, rows in traces.items():
        for k, (calls, avg, lo, hi) in sorted(rows.items()):
            lines.append(f'  {name:<10}{k:<12}calls {calls:4d}   average {avg / 1e3:8.1f} us   min {lo / 1e3:8.1f}   max {hi / 1e3:8.1f}')
    lines += ['',
              f'the sample (levels 1, 2, 4, 8: {len(names)} files, {file_bytes} bytes) on the headline volumes, both forms into one local directory, alternated:',
              f'{BLOCKS} blocks of {PER_BLOCK} samples each form; the files of the two forms are equal byte for byte (checked on the first sample)',
              f'{"":<72}   median       min       max   [samples/s]',
              f'{"device: voxel_pyramid_device + write_ssc_sample, 4 writer threads":<72}{rates["device"]["median"]:9.2f} {rates["device"]["min"]:9.2f} {rates["device"]["max"]:9.2f}',
              f'{"host: 4 volumes .cpu(), numpy model, open().write()":<72}{rates["host"]["median"]:9.2f} {rates["host"]["min"]:9.2f} {rates["host"]["max"]:9.2f}',
              f'ratio of the medians, device over host: {ratio:.1f}']
    os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
    with open(report, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
