"""Writer throughput and file size: codec='device' against the host codec at level 9 (the default) and level 1, on
headline-shaped samples (px 256, the benchmark's synthetic stream) written to a local directory.
usage: writer_device_codec.py [samples=200] [runs=3] [out file]"""
import builtins, gzip, os, pickle, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
from pca_amd.writer import AsyncBevWriter  # noqa: E402

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
        keys = len(pickle.loads(gzip.decompress(open(os.path.join(d, files[0]), 'rb').read())))
        assert keys >= 18
        say(f'{tag:28s} {n_samples / dt:9.1f} samples/s   {dt / n_samples * 1e3:8.3f} ms/sample   '
            f'{size / n_samples / 1024:9.1f} KiB/file   (pickle {raw / 1024:.0f} KiB)   fallbacks {w.fallbacks}')
        return n_samples / dt, size / n_samples
    finally:
        shutil.rmtree(d, ignore_errors=True)


def driver_alone():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n_samples):
        st.integrate()
        bev = acc.generate_bev(bench.present_index(acc), 1, gen_future=True)[0]
        len(bev)
    dt = time.perf_counter() - t0
    say(f'{"driver alone (no writer)":28s} {n_samples / dt:9.1f} samples/s   {dt / n_samples * 1e3:8.3f} ms/sample')


say(f'# {n_samples} samples of px {bench.PX}, {runs} runs each, files in a local temporary directory; host threads: 4')
one_run('warm-up (device)', codec='device')
driver_alone()
configs = (('device', dict(codec='device')), ('host level 9 (default)', dict(codec='host')),
           ('host level 1', dict(codec='host', compresslevel=1)))
res = {tag: [one_run(tag, **kw) for _ in range(runs)] for tag, kw in configs}
med = {tag: sorted(r[0] for r in v)[len(v) // 2] for tag, v in res.items()}
size = {tag: v[0][1] for tag, v in res.items()}
say(f'# median samples/s: ' + ', '.join(f'{tag}: {m:.1f}' for tag, m in med.items()))
say(f'# device / host level 9: {med["device"] / med["host level 9 (default)"]:.1f}x the throughput, '
    f'{size["device"] / size["host level 9 (default)"]:.2f}x the file size')
say(f'# device / host level 1: {med["device"] / med["host level 1"]:.1f}x the throughput, '
    f'{size["device"] / size["host level 1"]:.2f}x the file size')
from pca_amd.writer import _DeviceJob  # noqa: E402


def job_latency(block, reps=30):
    """enqueue -> results on the host of one device job over `block` [k,21,px,px], idle device: median seconds, the job"""
    torch.cuda.synchronize()
    lat = []
    for _ in range(reps):
        t0 = time.perf_counter()
        job = _DeviceJob(block)
        job.wait()
        lat.append(time.perf_counter() - t0)
    return sorted(lat)[reps // 2], job


one = st.step()['planes_f16'].reshape(1, 21, bench.PX, bench.PX).clone()
t1, job = job_latency(one)
say(f'# one sample, enqueue -> results on the host (3 kernels + one copy of {job.host.numel() / 1024:.0f} KiB), idle device: '
    f'median {t1 * 1e6:.0f} us; {job.n} chunks -> {int(job.results(0)[0].sum()) / 1024:.1f} KiB')
eight = torch.cat([st.step()['planes_f16'].reshape(1, 21, bench.PX, bench.PX) for _ in range(8)])
t8, job = job_latency(eight)
say(f'# a block of 8 samples as ONE job (what generate_bev_many hands the writer: one launch of the kernels, one copy of '
    f'{job.host.numel() / 1024:.0f} KiB): median {t8 * 1e6:.0f} us = {t8 / 8 * 1e6:.0f} us per sample')
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, 'w') as f:
        f.write('\n'.join(lines) + '\n')
