"""Preview sheets on the device (PCA_VIZ=device) against the matplotlib viz_bev, on headline-shaped samples (px 256, the
benchmark's synthetic stream): sheets per second through the writer, the time of the launches of one sheet job, and the file
size per PNG filter and Huffman coder against PIL saving the same pixels.
usage: preview_device.py [sheets=200] [figures=20] [out file]
       rocprofv3 --kernel-trace --stats -d <dir> -- python preview_device.py kernels      (kernel times, in a run of its own)"""
import builtins, io, os, shutil, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ['PCA_VIZ'] = 'device'                     # samples made from here on keep their device planes for the preview
import bench  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
from pca_amd import _lib, preview  # noqa: E402
from pca_amd.writer import AsyncBevWriter  # noqa: E402

kernels_only = len(sys.argv) > 1 and sys.argv[1] == 'kernels'
if kernels_only:
    del sys.argv[1]
n_sheets = int(sys.argv[1]) if len(sys.argv) > 1 else 200
n_figures = int(sys.argv[2]) if len(sys.argv) > 2 else 20
out_file = sys.argv[3] if len(sys.argv) > 3 else None
rp, builtins.print = builtins.print, (lambda *a, **k: None)
acc, pool, model = bench.make_accumulator(bench.synth_frame, 0)
st = bench.Stepper(acc, pool)
st.fill()
builtins.print = rp
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def sample():
    st.integrate()
    return acc.generate_bev(bench.present_index(acc), 1, gen_future=True)[0]


def device_run(n, threads=4):
    """n steps of the driver (integrate + one BEV), every sample's sheet handed to a fresh writer; the clock stops when the
    last file is on disk."""
    d = tempfile.mkdtemp(prefix='pca_preview_')
    try:
        w = AsyncBevWriter(n_threads=threads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            w.submit_preview(sample(), os.path.join(d, f'viz_{k:04d}.png'))
        w.close()
        dt = time.perf_counter() - t0
        assert w.previews_written == n and len(os.listdir(d)) == n
        Image.open(os.path.join(d, 'viz_0000.png')).verify()
        size = statistics.median(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        return n / dt, size
    finally:
        shutil.rmtree(d, ignore_errors=True)


def driver_alone(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        len(sample())                                # filled in: the copy has been waited for
    return n / (time.perf_counter() - t0)


def matplotlib_run(n):
    """The same driver steps with the default viz_bev (a matplotlib figure per sample on the calling thread)."""
    d = tempfile.mkdtemp(prefix='pca_preview_')
    os.environ['PCA_VIZ'] = 'matplotlib'
    try:
        t0 = time.perf_counter()
        for k in range(n):
            acc.viz_bev(sample(), os.path.join(d, f'viz_{k:04d}.png'))
        dt = time.perf_counter() - t0
        size = statistics.median(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        return n / dt, size
    finally:
        os.environ['PCA_VIZ'] = 'device'
        shutil.rmtree(d, ignore_errors=True)


if kernels_only:
    # for a run of its own under `rocprofv3 --kernel-trace --stats`: 50 sheet jobs of one sample per coder, nothing else
    bev = sample()
    block = bev._dev_preview[0].reshape(1, 21, bench.PX, bench.PX)
    own = [tuple(bev[f'trajs_{s}'] for s in preview.SETS)]
    for huffman in ('fixed', 'dynamic'):
        for _ in range(50):
            preview.SheetJob(block, own, huffman=huffman).wait()
    sys.exit(0)

say(f'# px {bench.PX}, local temporary directory, 4 writer threads; sheet = {5 * bench.PX} x {3 * bench.PX} RGB, '
    f'{preview.stream_bytes(bench.PX)} bytes of scanlines in {preview.stream_chunks(bench.PX)[1]} chunks; default filter '
    f'{preview.DEFAULT_FILTER!r}, coder {preview.DEFAULT_HUFFMAN!r}')
device_run(20)                                       # warm-up
matplotlib_run(2)
for rep in range(3):
    rate, size = device_run(n_sheets)
    say(f'device sheets     run {rep}: {rate:9.1f} sheets/s   {1e3 / rate:8.3f} ms/sheet   median file {size / 1024:7.1f} KiB   ({n_sheets} sheets)')
say(f'driver alone (integrate + BEV + filled in, no preview): {driver_alone(n_sheets):9.1f} samples/s')
for rep in range(2):
    rate, size = matplotlib_run(n_figures)
    say(f'matplotlib viz_bev run {rep}: {rate:9.2f} figures/s  {1e3 / rate:8.1f} ms/figure  median file {size / 1024:7.1f} KiB   ({n_figures} figures)')

# ---- the launches of one sheet job, each on its own: enqueue -> waited for on an idle device (launch latency included), and
# REPS calls enqueued back to back before one wait (what a call adds to a busy side stream)
ctx = _lib.Context.get()
lib = ctx.lib
bevs = [sample() for _ in range(20)]
blocks = [b._dev_preview[0].reshape(1, 21, bench.PX, bench.PX).clone() for b in bevs]
trajs = [tuple(b[f'trajs_{s}'] for s in preview.SETS) for b in bevs]
px, REPS = bench.PX, 50
planes = blocks[0]
verts, recs = preview.polyline_tables([trajs[0]], px)
d_verts, d_recs = torch.from_numpy(verts.reshape(-1).copy()).cuda(), torch.from_numpy(recs.view(np.uint8).copy()).cuda()
d_lut = torch.from_numpy(preview.VIRIDIS.copy()).cuda()
ranges = preview.panel_ranges()
table, per = preview.stream_chunks(px)
d_table = torch.from_numpy(table.view(np.uint8).copy()).cuda()
stream = torch.empty(preview.stream_bytes(px), dtype=torch.uint8, device='cuda')
ws = torch.empty(lib.pca_preview_workspace_bytes(1, px), dtype=torch.uint8, device='cuda')
ws_d = torch.empty(lib.pca_deflate_workspace_bytes(per), dtype=torch.uint8, device='cuda')
cap = sum(preview.deflate_bound(int(l)) for l in table['length'])
out = torch.empty(12 * per + cap, dtype=torch.uint8, device='cuda')
p = out.data_ptr()


def sheets(ftype, n_lines):
    return lib.pca_preview_sheets(ctx.h, planes.data_ptr(), 1, px, d_verts.data_ptr(), len(verts), d_recs.data_ptr(), n_lines,
                                  d_lut.data_ptr(), ranges.ctypes.data, ftype, stream.data_ptr(), ws.data_ptr(), ctx.stream())


def timed(call):
    torch.cuda.synchronize()
    one = []
    for _ in range(20):
        t0 = time.perf_counter()
        ctx.check(lib.pca_host_d2h_wait(ctx.h, call()))
        one.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for _ in range(REPS):
        t = call()
    ctx.check(lib.pca_host_d2h_wait(ctx.h, t))
    return statistics.median(one) * 1e6, (time.perf_counter() - t0) / REPS * 1e6


say(f'# one sheet of px {px} ({len(recs)} polylines, {len(verts)} vertices): us per call alone (enqueue -> waited for, idle device) / '
    f'us per call of {REPS} back to back')
for name, ftype in (('none', 0), ('sub', 1), ('up', 2)):
    a, b = timed(lambda: sheets(ftype, 0))
    say(f'mask clear + preview_rows, filter {name:4s}, no polylines : {a:8.1f} / {b:8.1f}')
a, b = timed(lambda: sheets(2, len(recs)))
say(f'mask clear + preview_overlay + preview_rows, filter up   : {a:8.1f} / {b:8.1f}')
a, b = timed(lambda: lib.pca_adler32_chunks(ctx.h, stream.data_ptr(), d_table.data_ptr(), per, p + 4 * per, ctx.stream()))
say(f'adler32_chunks, {per} chunks                              : {a:8.1f} / {b:8.1f}')
for name, fn in (('fixed', lib.pca_deflate_chunks), ('dynamic', lib.pca_deflate_chunks_dyn)):
    a, b = timed(lambda: fn(ctx.h, stream.data_ptr(), d_table.data_ptr(), per, p + 12 * per, p, p + 8 * per, ws_d.data_ptr(), ctx.stream()))
    say(f'deflate of the sheet stream (filter up), {name:7s}          : {a:8.1f} / {b:8.1f}')

# ---- file size per filter and coder on the same 20 samples, against PIL on the same pixels
say('# median PNG bytes over 20 samples')
sizes = {}
for flt in ('none', 'sub', 'up'):
    for huffman in ('fixed', 'dynamic'):
        pngs = [preview.render_sheets(b, [t], filter=flt, huffman=huffman)[0] for b, t in zip(blocks, trajs)]
        sizes[flt, huffman] = statistics.median(len(x) for x in pngs)
        say(f'device filter {flt:4s} huffman {huffman:7s}: {sizes[flt, huffman] / 1024:8.1f} KiB')
pixels = [Image.open(io.BytesIO(x)).convert('RGB') for x in pngs]
for level in (1, 6):
    got = []
    for im in pixels:
        f = io.BytesIO()
        im.save(f, format='PNG', compress_level=level)
        got.append(f.tell())
    say(f'PIL compress_level {level}              : {statistics.median(got) / 1024:8.1f} KiB')
best = min(sizes, key=sizes.get)
say(f'# smallest median: filter {best[0]!r}, huffman {best[1]!r}; the module\'s default is ({preview.DEFAULT_FILTER!r}, {preview.DEFAULT_HUFFMAN!r})')
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, 'w') as f:
        f.write('\n'.join(lines) + '\n')
