"""Writer throughput and file size of the device codec with fixed and with dynamic Huffman blocks, against the host codec at
levels 1 and 9: the four take turns on the same headline-shaped stream (px 256, the benchmark's synthetic frames) in one
session.  Then the latency of one device job under either coder, and what the fixed code-length code costs.
usage: writer_device_huffman.py [samples=200] [runs=3] [out file]"""
import builtins, gzip, os, pickle, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))
import bench  # noqa: E402
import torch  # noqa: E402
from pca_amd.writer import AsyncBevWriter, _DeviceJob  # noqa: E402

n_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 200
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
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


def one_run(tag, **kw):
    """n_samples steps of the driver (integrate + one BEV), every sample handed to a fresh writer; the clock stops when
    the last file is on disk.  The writer's queue holds 64 samples, so the slower of driver and writer sets the pace."""
    d = tempfile.mkdtemp(prefix='pca_writer_')
    try:
        w = AsyncBevWriter(**kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n_samples):
            st.integrate()
            bev = acc.generate_bev(bench.present_index(acc), 1, gen_future=True)[0]
            w.submit(bev, f'bev_{k:04d}.pkl', d)
        w.close()
        dt = time.perf_counter() - t0
        files = sorted(os.listdir(d))
        assert len(files) == n_samples
        size = sum(os.path.getsize(os.path.join(d, f)) for f in files)
        raw = len(gzip.decompress(open(os.path.join(d, files[-1]), 'rb').read()))
        assert len(pickle.loads(gzip.decompress(open(os.path.join(d, files[0]), 'rb').read()))) >= 18
        say(f'{tag:28s} {n_samples / dt:9.1f} samples/s   {dt / n_samples * 1e3:8.3f} ms/sample   '
            f'{size / n_samples / 1024:9.1f} KiB/file   (pickle {raw / 1024:.0f} KiB)   fallbacks {w.fallbacks}')
        return n_samples / dt, size / n_samples
    finally:
        shutil.rmtree(d, ignore_errors=True)


say(f'# {n_samples} samples of px {bench.PX}, {runs} runs each, the four codecs taking turns; files in a local temporary '
    f'directory; host threads: 4')
one_run('warm-up (device fixed)', codec='device')
one_run('warm-up (device dynamic)', codec='device', huffman='dynamic')
configs = (('device fixed', dict(codec='device')), ('device dynamic', dict(codec='device', huffman='dynamic')),
           ('host level 1', dict(codec='host', compresslevel=1)), ('host level 9', dict(codec='host')))
res = {tag: [] for tag, _ in configs}
for _ in range(runs):
    for tag, kw in configs:
        res[tag].append(one_run(tag, **kw))
med = {tag: sorted(r[0] for r in v)[len(v) // 2] for tag, v in res.items()}
size = {tag: sum(r[1] for r in v) / len(v) for tag, v in res.items()}
say('# median samples/s: ' + ', '.join(f'{tag}: {m:.1f}' for tag, m in med.items()))
say('# KiB/file (mean of the runs): ' + ', '.join(f'{tag}: {s / 1024:.1f}' for tag, s in size.items()))
for tag in ('device fixed', 'device dynamic'):
    say(f'# {tag} / host level 9: {size[tag] / size["host level 9"]:.2f}x the file size, {med[tag] / med["host level 9"]:.1f}x the '
        f'throughput; / host level 1: {size[tag] / size["host level 1"]:.2f}x the file size, {med[tag] / med["host level 1"]:.1f}x')
lowest_fixed = min(r[0] for r in res['device fixed'])
say(f'# device dynamic, median {med["device dynamic"]:.1f} samples/s, against the lowest of the {runs} device fixed runs, '
    f'{lowest_fixed:.1f}: {"not below it" if med["device dynamic"] >= lowest_fixed else "BELOW it"}')


def job_latency(block, huffman, reps=30):
    """enqueue -> results on the host of one device job over `block` [k,21,px,px], idle device: median seconds, the job"""
    torch.cuda.synchronize()
    lat = []
    for _ in range(reps):
        t0 = time.perf_counter()
        job = _DeviceJob(block, huffman)
        job.wait()
        lat.append(time.perf_counter() - t0)
    return sorted(lat)[reps // 2], job


one = st.step()['planes_f16'].reshape(1, 21, bench.PX, bench.PX).clone()
eight = torch.cat([st.step()['planes_f16'].reshape(1, 21, bench.PX, bench.PX) for _ in range(8)])
jobs = {}
for _ in range(2):                                   # the coders take turns here too; the second round is the one reported
    for huffman in ('fixed', 'dynamic'):
        jobs[huffman] = job_latency(one, huffman), job_latency(eight, huffman)
for huffman in ('fixed', 'dynamic'):
    (t1, job1), (t8, job8) = jobs[huffman]
    say(f'# {huffman}: one sample, enqueue -> results on the host (3 kernels + one copy of {job1.host.numel() / 1024:.0f} KiB), '
        f'idle device: median {t1 * 1e6:.0f} us; {job1.n} chunks -> {int(job1.results(0)[0].sum()) / 1024:.1f} KiB.  A block of 8 '
        f'samples as ONE job: median {t8 * 1e6:.0f} us = {t8 / 8 * 1e6:.0f} us per sample')

# ---- what the ONE fixed code-length code costs: the headers of the sample's dynamic pieces, sent as the kernel sends them,
# against a Huffman code of each header's own code-length symbols (HCLEN cut behind the last used one)
from test_gpu_deflate_dynamic import CL_ORDER, decode_blocks, huffman_optimum  # noqa: E402
CL_LEN = [3, 6, 6, 6, 4, 4, 4, 4, 4, 4, 4, 6, 6, 6, 6, 6, 4, 3, 3]


def cl_symbols(lens):
    """The code-length symbols of the kernel's (and zlib's) run cutting, as a histogram, and the extra bits they carry."""
    h, extra, i = [0] * 19, 0, 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        i += r
        if v:
            h[v] += 1
            r -= 1
        while v == 0 and r >= 11:
            h[18] += 1; extra += 7; r -= min(r, 138)
        if v == 0 and r >= 3:
            h[17] += 1; extra += 3; r = 0
        while v and r >= 3:
            h[16] += 1; extra += 2; r -= min(r, 6)
        h[v] += r
    return h, extra


sizes, crcs, data = jobs['dynamic'][0][1].results(0)
at, n_dyn, fixed_cl, own_cl, piece_bits = 0, 0, 0, 0, 0
for s in sizes.tolist():
    btype, ll, dl, tokens = decode_blocks(bytes(data[at:at + s]))[0]
    at += s
    piece_bits += 8 * s
    if btype == 2:
        n_dyn += 1
        h, extra = cl_symbols(ll + dl)
        fixed_cl += 4 + 3 * 19 + sum(n * CL_LEN[k] for k, n in enumerate(h)) + extra
        sent = 1 + max(i for i, k in enumerate(CL_ORDER) if h[k])
        own_cl += 4 + 3 * max(sent, 4) + huffman_optimum(h)[0] + extra
say(f'# code-length code: {n_dyn} of {len(sizes)} chunks of the sample are dynamic blocks; their code lengths take '
    f'{fixed_cl / 8:.0f} bytes through the fixed code-length code, {own_cl / 8:.0f} bytes through a Huffman code of each header\'s own '
    f'symbols (no length limit: a lower bound): {(fixed_cl - own_cl) / 8:.0f} bytes of {piece_bits / 8 / 1024:.1f} KiB = '
    f'{100 * (fixed_cl - own_cl) / piece_bits:.2f} % of the sample\'s pieces')
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, 'w') as f:
        f.write('\n'.join(lines) + '\n')
