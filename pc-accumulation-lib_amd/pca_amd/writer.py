"""Output writer: the reference writes each BEV sample as gzip(pickle(dict)) synchronously
(sem_pc_accum.py:280-294); once a sample costs < 1 ms on the GPU that dominates.  AsyncBevWriter does the device->host
copy, pickling and compression on worker threads.  Same container, same dict schema (README.md:60-99 of the reference).

codec='device' (opt-in; PCA_WRITER_CODEC=device for the shared writer) leaves the per-byte pass over the planes on the GPU:
the pickle of a sample is laid out from zero-filled stand-ins, the 15 plane payloads are located in it, and those byte
ranges of the device planes are compressed there (pca_deflate_chunks: fixed-Huffman pieces that concatenate bytewise).  The
worker threads then only splice: pickle fragments from the host as stored blocks, device pieces as they are, one gzip
member (pca_host_gzip_assemble).  The file inflates to exactly pickle.dumps(dict(bev)).

huffman='dynamic' (opt-in on top of the device codec; PCA_WRITER_HUFFMAN=dynamic for the shared writer) compresses with
pca_deflate_chunks_dyn: the same tokens, each chunk with a Huffman code of its own where that is smaller.  Same pieces,
same splice, smaller files.

submit_preview (PCA_VIZ=device routes viz_bev here) writes a sample's preview sheet as a PNG the same way: the sheet is
rendered, filtered and compressed on the device (pca_amd/preview.py), once per block of planes; the worker threads assemble
the container and write the file.

submit_files writes finished payloads as they are -- the SSC files of pca_amd/ssc.py: a payload that is a cuda tensor leaves
the device in one asynchronous copy enqueued by the submitting thread, and a worker thread writes the file."""
import atexit
import ctypes as C
import gzip
import os
import pickle
import pickletools
import queue
import threading

import numpy as np

DEFLATE_CHUNK_MAX = 32768
DEFLATE_CHUNK_DTYPE = np.dtype([('offset', '<i8'), ('length', '<i4'), ('reserved', '<i4')])      # pca_deflate_chunk
_BYTES_OPS = ('SHORT_BINBYTES', 'BINBYTES', 'BINBYTES8', 'BYTEARRAY8')
_BYTES_HEADER = {'SHORT_BINBYTES': 2, 'BINBYTES': 5, 'BINBYTES8': 9, 'BYTEARRAY8': 9}
_PLANE_GROUPS = ((0, 1), (1, 1), (2, 3), (5, 1), (6, 1))      # pack_bev: road p[0], intensity p[1], rgb p[2:5], dynamic p[5], elevation p[6]


_device_writers = [0]


def device_codec_selected():
    """True while a writer with the device codec is open or the shared writer is to be one: a LazyBev made meanwhile keeps a
    reference to its device planes (dropped by the writer once they have been compressed).  A writer stays open until its
    close() has run, whether or not that raised: its worker threads keep a writer that was merely dropped alive."""
    return _device_writers[0] > 0 or os.environ.get('PCA_WRITER_CODEC', 'host') == 'device'


def deflate_bound(n):
    """Most bytes pca_deflate_chunks makes of a chunk of n (PCA_DEFLATE_BOUND)."""
    return (9 * n + 7) // 8 + 16


def plane_payloads(px):
    """(byte offset, length) inside one [21,px,px] float16 sample of the 15 arrays of pack_bev, in the dict's order."""
    cell = px * px * 2
    return [((7 * s + k0) * cell, k * cell) for s in range(3) for k0, k in _PLANE_GROUPS]


def chunk_table(payloads, base=0, chunk_max=DEFLATE_CHUNK_MAX):
    """Cuts every payload into chunks of at most chunk_max bytes: (table as DEFLATE_CHUNK_DTYPE records, first chunk of
    each payload with the total appended)."""
    rows, first = [], []
    for off, length in payloads:
        first.append(len(rows))
        rows += [(base + off + at, min(chunk_max, length - at), 0) for at in range(0, length, chunk_max)]
    first.append(len(rows))
    return np.array(rows, dtype=DEFLATE_CHUNK_DTYPE), first


def _arrays_in_pickle_order(obj, out):
    if isinstance(obj, np.ndarray):
        out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _arrays_in_pickle_order(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _arrays_in_pickle_order(v, out)
    return out


def stand_in_sample(px, trajs_present, trajs_future, trajs_full, gt_lanes=None, extra=None):
    """The sample's dict with zero-filled stand-ins for the plane arrays: same shapes, dtype and views as pack_bev makes
    them.  Returns (dict, the zero block the stand-ins are views of)."""
    from bev_generator.sem_bev import SemBEVGenerator
    zeros = np.zeros((21, px, px), dtype=np.float16)
    out = SemBEVGenerator.pack_bev(zeros, trajs_present, trajs_future, trajs_full, gt_lanes)
    for k, v in (extra or {}).items():
        if k not in out:
            out[k] = v
    return out, zeros


def locate_payloads(blob, stand_in, zeros):
    """Where the plane payloads lie in `blob` = pickle.dumps(stand_in): [(start in blob, nbytes)] in pack_bev's order, or
    None if the pickle's byte-string ops do not match the dict's arrays one for one (the sample then takes the host codec).
    The layout of a pickle does not depend on array contents, so the same ranges hold for the real sample.  Left out on
    both sides: the one-byte marker b'b' of numpy's reconstructor and empty payloads, which pickle may memoise."""
    arrays = [a for a in _arrays_in_pickle_order(stand_in, []) if a.nbytes]
    if any(a.nbytes == 1 or a.dtype.hasobject for a in arrays):
        return None
    ops = [(op.name, arg, pos) for op, arg, pos in pickletools.genops(blob) if op.name in _BYTES_OPS and len(arg) and bytes(arg) != b'b']
    if len(ops) != len(arrays):
        return None
    found = []
    for (name, arg, pos), a in zip(ops, arrays):
        if len(arg) != a.nbytes:
            return None
        if a.base is zeros or a is zeros:
            found.append((pos + _BYTES_HEADER[name], a.nbytes))
    if [n for _, n in found] != [n for _, n in plane_payloads(zeros.shape[-1])]:
        return None
    return found


class _Layout:
    """What depends on px alone: payload ranges, their chunks, the output's capacity -- all per sample."""
    _by_px = {}

    def __init__(self, px):
        self.px = px
        self.sample_bytes = 21 * px * px * 2
        self.payloads = plane_payloads(px)
        self.table, self.first = chunk_table(self.payloads)
        self.n = len(self.table)
        self.cap = int(sum(deflate_bound(int(l)) for l in self.table['length']))
        self.dev_tables = {}                 # (device index, samples) -> device copy of the table of a [samples,21,px,px] block

    @classmethod
    def get(cls, px):
        if px not in cls._by_px:
            cls._by_px[px] = _Layout(px)
        return cls._by_px[px]

    def device_table(self, device, k):
        import torch
        key = (device.index, k)
        if key not in self.dev_tables:
            t = np.tile(self.table, k)
            t['offset'] += np.repeat(np.arange(k, dtype=np.int64) * self.sample_bytes, self.n)
            self.dev_tables[key] = torch.from_numpy(t.view(np.uint8).copy()).to(device)
        return self.dev_tables[key]


class _DeviceJob:
    """The compression of ALL samples of one [k,21,px,px] block in flight on the context's side stream: one launch of the
    kernels, then ONE copy of (sizes, crcs, bytes).  The samples of a generate_bev_many share it.  Holds planes, table,
    outputs and workspace until the copy has been waited for."""

    def __init__(self, planes, huffman='fixed'):
        import weakref

        import torch
        from . import _lib
        assert planes.is_contiguous() and planes.dtype == torch.float16 and planes.dim() == 4 and planes.shape[1] == 21
        self.layout = lay = _Layout.get(int(planes.shape[-1]))
        self.ctx = ctx = _lib.Context.get(planes.device)
        self.planes_ref = weakref.ref(planes)
        k = int(planes.shape[0])
        self.n = n = k * lay.n
        table = lay.device_table(planes.device, k)
        ws = torch.empty(int(ctx.lib.pca_deflate_workspace_bytes(n)), dtype=torch.uint8, device=planes.device)
        dev = torch.empty(8 * n + k * lay.cap, dtype=torch.uint8, device=planes.device)
        self.host = torch.empty(8 * n + k * lay.cap, dtype=torch.uint8, pin_memory=True)
        p = dev.data_ptr()
        deflate = ctx.lib.pca_deflate_chunks_dyn if huffman == 'dynamic' else ctx.lib.pca_deflate_chunks
        rc = deflate(ctx.h, planes.data_ptr(), table.data_ptr(), n, p + 8 * n, p, p + 4 * n, ws.data_ptr(), ctx.stream())
        if rc < 0:
            ctx.check(rc)
        # (rc is the ticket of the kernels alone, for callers that leave the pieces on the device.  The copy below runs behind
        # them on the same side stream, so its ticket covers both and is the only one waited for; the ring of 64 completion
        # events simply moves on by two per job -- an older ticket waits for a later event of the same stream.)
        self.ticket = ctx.lib.pca_host_d2h_async(ctx.h, p, self.host.data_ptr(), dev.numel(), ctx.stream())
        if self.ticket < 0:
            ctx.check(self.ticket)
        self.keep = (planes, table, ws, dev)

    def wait(self):
        """On the thread that talks to HIP: the results are in `host`, the device blocks go back."""
        if self.keep is not None:
            self.ctx.check(self.ctx.lib.pca_host_d2h_wait(self.ctx.h, self.ticket))
            self.keep = None
            self.ctx.poll_status()

    def results(self, index):
        """(sizes, crcs, bytes) of the chunks of sample `index`."""
        n, m = self.n, self.layout.n
        h = self.host.numpy()
        sizes, crcs = h[:4 * n].view(np.uint32), h[4 * n:8 * n].view(np.uint32)
        at = 8 * n + int(sizes[:index * m].sum(dtype=np.int64))
        return sizes[index * m:(index + 1) * m], crcs[index * m:(index + 1) * m], h[at:]

    def __del__(self):
        try:
            if self.keep is not None:
                self.ctx.lib.pca_host_d2h_wait(self.ctx.h, self.ticket)
        except Exception:                    # noqa: BLE001  (interpreter shutdown)
            pass


def gzip_assemble(pieces):
    """pieces: [(uint8 array, raw_bytes, crc)] -- raw_bytes < 0: plain bytes (stored blocks), else a deflate piece that
    inflates to raw_bytes bytes of that CRC-32.  Returns the gzip member as a uint8 array (pca_host_gzip_assemble)."""
    from . import _lib
    lib = _lib.load()
    n = len(pieces)
    arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a, _, _ in pieces]
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
    nbytes = np.array([a.size for a in arrs], dtype=np.int64)
    raw = np.array([r for _, r, _ in pieces], dtype=np.int64)
    crc = np.array([c for _, _, c in pieces], dtype=np.uint32)
    need = 20 + int(nbytes.sum()) + 5 * int(sum((int(b) + 65534) // 65535 for b, r in zip(nbytes, raw) if r < 0))
    out = np.empty(need, dtype=np.uint8)
    got = lib.pca_host_gzip_assemble(n, C.addressof(ptrs), nbytes.ctypes.data, raw.ctypes.data, crc.ctypes.data, out.ctypes.data, need)
    if got < 0:
        raise RuntimeError(f'pca_host_gzip_assemble failed ({got})')
    return out[:got]


def crc32_combine(crc_a, crc_b, len_b):
    from . import _lib
    return int(_lib.load().pca_host_crc32_combine(int(crc_a), int(crc_b), int(len_b)))


def splice_sample(blob, found, layout, sizes, crcs, data):
    """The gzip member of a sample: `blob` (the stand-in's pickle) between the payloads `found`, the device pieces in their
    place.  sizes / crcs / data: what pca_deflate_chunks left for the layout's chunk table."""
    host = np.frombuffer(blob, dtype=np.uint8)
    ends = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    lengths = layout.table['length']
    pieces, at = [], 0
    for k, (start, nbytes) in enumerate(found):
        pieces.append((host[at:start], -1, 0))
        c0, c1 = layout.first[k], layout.first[k + 1]
        crc = 0
        for c in range(c0, c1):
            crc = crc32_combine(crc, crcs[c], lengths[c])
        pieces.append((data[ends[c0]:ends[c1]], nbytes, crc))
        at = start + nbytes
    pieces.append((host[at:], -1, 0))
    return gzip_assemble(pieces)


class _PreviewItem:
    """One preview sheet on its way through the writer: sample `index` of the sheet job `job`, to be written to `path`."""
    __slots__ = ('job', 'index', 'path')

    def __init__(self, job, index, path):
        self.job, self.index, self.path = job, index, path


class _FilesItem:
    """Files whose bytes are final: [(path, bytes-like | pinned host tensor)], and the event behind the copies the pinned
    tensors are filled by (None: nothing to wait for)."""
    __slots__ = ('files', 'event')

    def __init__(self, files, event):
        self.files, self.event = files, event


class _Item:
    """One sample on its way through the writer.  job is None: the host codec takes it (bev is a plain dict by the time a
    worker sees it, unless it is the device_only form).  Else: sample `index` of that device job, meta = what
    stand_in_sample needs (filled in when the job has been waited for)."""
    __slots__ = ('bev', 'filename', 'write_dir', 'job', 'index', 'meta')

    def __init__(self, bev, filename, write_dir, job=None, index=0):
        self.bev, self.filename, self.write_dir, self.job, self.index, self.meta = bev, filename, write_dir, job, index, None


class AsyncBevWriter:

    def __init__(self, n_threads=4, compresslevel=9, max_pending=64, codec='host', huffman='fixed'):
        if codec not in ('host', 'device'):
            raise ValueError(f"codec must be 'host' or 'device', not {codec!r}")
        if huffman not in ('fixed', 'dynamic'):
            raise ValueError(f"huffman must be 'fixed' or 'dynamic', not {huffman!r}")
        self.codec = codec
        self.huffman = huffman               # the device codec's entropy coder; the host codec does not look at it
        # device codec: samples written from device pieces / samples that came from the device but were written by the host
        # codec all the same (pickle without the expected byte strings, a LazyBev made before the codec was selected or
        # submitted a second time, plane arrays replaced after the sample filled in)
        self.device_written = 0
        self.fallbacks = 0
        self._lock = threading.Lock()
        self._refill = []                    # samples a worker handed back: filled in on the submitting thread, then host codec
        self._jobs = {}                      # id(planes block) -> its device job, while the block lives
        self._parked = None
        self._preview_jobs = {}              # id(planes block) -> its sheet job, while the block lives
        self._parked_preview = None
        self.previews_written = 0
        self._parked_files = None
        self.files_written = 0
        self._open = True
        if codec == 'device':
            _device_writers[0] += 1
        self.q = queue.Queue(maxsize=max_pending)
        self.compresslevel = compresslevel
        self.errors = []
        self.threads = [threading.Thread(target=self._work, daemon=True) for _ in range(n_threads)]
        for t in self.threads:
            t.start()

    @staticmethod
    def _to_host(bev):
        """Accepts the reference dict (host arrays) or the device_only form {'planes_f16': cuda [21,px,px], trajs}."""
        if 'planes_f16' not in bev:
            return bev
        from bev_generator.sem_bev import SemBEVGenerator
        planes = bev['planes_f16'].cpu().numpy()
        out = SemBEVGenerator.pack_bev(planes, bev['trajs_present'], bev['trajs_future'], bev['trajs_full'],
                                       bev.get('gt_lanes'))
        for k, v in bev.items():
            if k not in out and k != 'planes_f16':
                out[k] = v
        return out

    def _write_host(self, it):
        blob = pickle.dumps(self._to_host(it.bev))
        with gzip.open(os.path.join(it.write_dir, f'{it.filename}.gz'), 'wb', compresslevel=self.compresslevel) as f:
            f.write(blob)

    def _write_device(self, it):
        stand_in, zeros = stand_in_sample(it.job.layout.px, *it.meta)
        blob = pickle.dumps(stand_in)
        found = locate_payloads(blob, stand_in, zeros)
        if found is None:                    # back to the submitting thread: it fills the sample in, the host codec writes it
            with self._lock:
                self.fallbacks += 1
                self._refill.append(it)
            return
        member = splice_sample(blob, found, it.job.layout, *it.job.results(it.index))
        with open(os.path.join(it.write_dir, f'{it.filename}.gz'), 'wb') as f:
            f.write(memoryview(member))
        with self._lock:
            self.device_written += 1

    def _write_preview(self, it):
        png = it.job.png(it.index)
        os.makedirs(os.path.dirname(os.path.abspath(it.path)), exist_ok=True)
        with open(it.path, 'wb') as f:
            f.write(png)
        with self._lock:
            self.previews_written += 1

    def _write_files(self, it):
        for path, data in it.files:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'wb') as f:
                f.write(memoryview(data.numpy()).cast('B') if hasattr(data, 'numpy') else data)
            with self._lock:
                self.files_written += 1

    def _work(self):
        while True:
            it = self.q.get()
            if it is None:
                return
            try:
                if type(it) is _FilesItem:
                    self._write_files(it)
                    continue
                if type(it) is _PreviewItem:
                    self._write_preview(it)
                    continue
                os.makedirs(it.write_dir, exist_ok=True)
                if it.job is not None:
                    self._write_device(it)
                else:
                    self._write_host(it)
            except Exception as e:              # reported by close(); the reference prints IOErrors and goes on
                self.errors.append(e)
            finally:
                self.q.task_done()

    @staticmethod
    def _planes_intact(bev):
        """A LazyBev that has filled in: do its plane entries still show the arrays the copy landed in?"""
        host = getattr(bev, '_host_planes', None)
        if host is None:
            return False
        px = host.shape[-1]
        keys = [f'{name}_{s}' for s in ('present', 'future', 'full') for name in ('road', 'intensity', 'rgb', 'dynamic', 'elevation')]
        for key, (off, nbytes) in zip(keys, plane_payloads(px)):
            v = dict.get(bev, key)
            if not isinstance(v, np.ndarray) or v.dtype != np.float16 or v.nbytes != nbytes or not v.flags.c_contiguous \
                    or v.ctypes.data != host.ctypes.data + off or v.flags.writeable:
                return False
        return True

    def _device_source(self, bev):
        """(planes block [k,21,px,px] on the device, index of the sample in it), or None: the host codec takes the sample."""
        if hasattr(bev, '_pending'):         # LazyBev: it holds its device planes while the device codec is selected
            dev = getattr(bev, '_dev', None)
            if dev is None and bev._pending is not None:     # made before the codec was selected: its copy may still hold them
                keep = getattr(bev._pending[2], 'keep', None)
                dev = (keep[0], bev._pending[1]) if keep else None
            if dev is None or not dev[0].is_cuda or (bev._pending is None and not self._planes_intact(bev)):
                return None
            planes = dev[0]
            return (planes if planes.dim() == 4 else planes.view((1, ) + tuple(planes.shape))), dev[1]
        planes = bev['planes_f16']
        if not planes.is_cuda or planes.dim() != 3 or planes.shape[0] != 21 or planes.shape[1] != planes.shape[2]:
            return None
        return planes.contiguous().view((1, ) + tuple(planes.shape)), 0

    def _device_job(self, planes):
        """The job that compresses `planes`: the one a sibling sample started, or a new one."""
        job = self._jobs.get(id(planes))
        if job is None or job.planes_ref() is not planes:
            self._jobs = {k: j for k, j in self._jobs.items() if j.planes_ref() is not None}
            # (the default goes out as the one-argument call it has always been: wrappers of _DeviceJob take `planes` alone)
            job = self._jobs[id(planes)] = _DeviceJob(planes, self.huffman) if self.huffman != 'fixed' else _DeviceJob(planes)
        return job

    def submit(self, bev, filename, write_dir):
        """Same arguments as SemanticPointCloudAccumulator.write_compressed_pickle.  A sample whose planes are still on
        their way from the device (LazyBev) is parked; it is filled in -- on THIS thread, the one that talks to HIP -- and
        queued when the next sample arrives (its copy has long finished by then) or at flush / close.  The worker threads
        only pickle and compress.  With the device codec the compression of the sample's block of planes is enqueued
        here, on the side stream the copy uses (once per block: the samples of a generate_bev_many share it), and the
        sample is parked with it; the worker threads then only assemble and write."""
        self._release_parked()
        self._take_refills()
        from_device = hasattr(bev, '_pending') or (type(bev) is dict and 'planes_f16' in bev)
        if type(bev) is dict and 'planes_f16' in bev:       # snapshot: the caller may reuse the device buffer
            bev = dict(bev, planes_f16=bev['planes_f16'].clone())
        if self.codec == 'device' and from_device:
            src = self._device_source(bev)
            if src is not None:
                self._parked = _Item(bev, filename, write_dir, self._device_job(src[0]), src[1])
                return
            with self._lock:
                self.fallbacks += 1
        if getattr(bev, '_pending', None) is not None:
            self._parked = _Item(bev, filename, write_dir)
            return
        self.q.put(_Item(bev if type(bev) is dict else dict(bev), filename, write_dir))

    @staticmethod
    def _meta(bev):
        """Everything of the sample but its planes: (trajs_present, trajs_future, trajs_full, gt_lanes, extra keys)."""
        pending = getattr(bev, '_pending', None)
        if pending is not None:
            trajs, gt_lanes = pending[3], pending[4]
            if gt_lanes is not None and not isinstance(gt_lanes, list):      # pca_amd.lanes.PendingLanes: decoded now
                gt_lanes = gt_lanes.resolve()
            return trajs[0], trajs[1], trajs[2], gt_lanes, None
        return (bev['trajs_present'], bev['trajs_future'], bev['trajs_full'], bev.get('gt_lanes'),
                {k: v for k, v in bev.items() if k != 'planes_f16'})

    def _release_parked(self):
        it, self._parked = self._parked, None
        if it is None:
            return
        if it.job is not None:
            it.job.wait()
            it.meta = self._meta(it.bev)
            if getattr(it.bev, '_dev', None) is not None:
                it.bev._dev = None           # compressed: the sample lets go of its device planes
        else:
            it.bev = dict(it.bev)
        self.q.put(it)

    # ---- preview sheets (pca_amd/preview.py)
    @staticmethod
    def _preview_source(bev):
        """(planes block [k,21,px,px] on the device, index of the sample in it, the block's trajectories), from the device
        planes a LazyBev made under PCA_VIZ=device has kept or, for any other sample, from its 15 arrays uploaded."""
        import torch
        from .preview import SETS, planes_of
        dev = getattr(bev, '_dev_preview', None)
        if dev is not None and dev[0].is_cuda and dev[0].is_contiguous():
            planes, index, block = dev
            if planes.dim() == 4 and block is not None and len(block) == planes.shape[0]:
                return planes, index, block
            # a sample on its own, or one whose siblings are unknown: a job of one (its trajectories without waiting for its copy)
            own = bev._pending[3] if bev._pending is not None else tuple(bev[f'trajs_{s}'] for s in SETS)
            one = planes if planes.dim() == 3 else planes[index]
            return one.view((1, ) + tuple(one.shape)), 0, [tuple(own)]
        host = planes_of(bev)
        return torch.from_numpy(host).cuda().view((1, ) + host.shape), 0, [tuple(bev[f'trajs_{s}'] for s in SETS)]

    def submit_preview(self, bev, file_path):
        """The preview sheet of `bev` (a LazyBev, or the reference's dict of host arrays) as the PNG `file_path`.  The
        kernels are enqueued here, on the thread that talks to HIP, once per block of planes (the samples of a
        generate_bev_many or bev_num > 1 share the job); the preview is parked like a sample and released -- waited for
        and queued -- by the next preview, flush or close; the worker threads assemble the container and write the file."""
        from .preview import SheetJob
        self._release_parked_preview()
        planes, index, block = self._preview_source(bev)
        job = self._preview_jobs.get(id(planes))
        if job is None or job.planes_ref() is not planes:
            self._preview_jobs = {k: j for k, j in self._preview_jobs.items() if j.planes_ref() is not None}
            job = self._preview_jobs[id(planes)] = SheetJob(planes, block)
        if getattr(bev, '_dev_preview', None) is not None:
            bev._dev_preview = None          # enqueued: the job holds the planes from here on
        self._parked_preview = _PreviewItem(job, index, file_path)

    def _release_parked_preview(self):
        it, self._parked_preview = self._parked_preview, None
        if it is not None:
            it.job.wait()
            self.q.put(it)

    # ---- finished payloads (pca_amd/ssc.py)
    def submit_files(self, files):
        """files: [(path, payload)], a payload being bytes-like (bytes, bytearray, memoryview, a numpy array) or a tensor.  The
        copy of every cuda tensor into pinned host memory is enqueued here, on the thread that talks to HIP, on torch's
        current stream; the item is parked like a sample and released -- waited for and queued -- by the next submit_files,
        flush or close; the worker threads write the files (counted in files_written).  Payloads without a device tensor
        are queued at once."""
        self._release_parked_files()
        out, copied = [], False
        for path, data in files:
            if hasattr(data, 'is_cuda'):
                import torch
                flat = data.contiguous().view(-1)
                if flat.is_cuda:
                    host = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
                    host.copy_(flat, non_blocking=True)
                    copied = True
                    flat = host
                data = flat
            elif isinstance(data, np.ndarray):
                data = np.ascontiguousarray(data).tobytes()
            out.append((str(path), data))
        if copied:
            import torch
            event = torch.cuda.Event()
            event.record()
            self._parked_files = _FilesItem(out, event)
        else:
            self.q.put(_FilesItem(out, None))

    def _release_parked_files(self):
        it, self._parked_files = self._parked_files, None
        if it is not None:
            it.event.synchronize()
            it.event = None
            self.q.put(it)

    def _take_refills(self):
        """Samples the workers could not splice: filled in here, on the submitting thread, and queued for the host codec."""
        with self._lock:
            back, self._refill = self._refill, []
        for it in back:
            self.q.put(_Item(it.bev if type(it.bev) is dict else dict(it.bev), it.filename, it.write_dir))
        return len(back)

    def flush(self):
        self._release_parked()
        self._release_parked_preview()
        self._release_parked_files()
        self.q.join()
        while self._take_refills():
            self.q.join()

    def close(self):
        if not self._open:
            return
        try:
            self.flush()
        finally:                             # whatever flush raised: the writer is closed and the codec no longer selected by it
            for _ in self.threads:
                self.q.put(None)
            for t in self.threads:
                t.join()
            if self.codec == 'device':
                _device_writers[0] -= 1
            self._open = False
        if self.errors:
            raise self.errors[0]


_shared = None


def shared_writer():
    """Process-wide writer used by SemanticPointCloudAccumulator.write_compressed_pickle for in-flight BEV samples;
    joined at interpreter exit, so every file is on disk when the unchanged driver returns."""
    global _shared
    if _shared is None:
        _shared = AsyncBevWriter(n_threads=int(os.environ.get('PCA_WRITER_THREADS', '4')),
                                 codec=os.environ.get('PCA_WRITER_CODEC', 'host'),
                                 huffman=os.environ.get('PCA_WRITER_HUFFMAN', 'fixed'))
        atexit.register(_shared.close)
    return _shared


def flush_shared():
    """Blocks until everything submitted to the shared writer is on disk (no-op if it was never used)."""
    if _shared is not None:
        _shared.flush()
        if _shared.errors:
            raise _shared.errors.pop(0)
