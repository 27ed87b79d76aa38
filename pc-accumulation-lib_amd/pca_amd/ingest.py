"""Ingest pipeline: overlaps disk reads, label remapping and host->device copies with the GPU work
of earlier frames.  Wraps any of the observation loaders; yields the same `[obs]` batches, but with the arrays already
resident in HBM (the accumulators accept cuda tensors in place of numpy / PIL inputs).

    loader = PrefetchingLoader(Kitti360Dataloader(...), depth=4)
    for observations in loader:
        acc.integrate(observations)

A small pool of reader threads (PCA_INGEST_THREADS, default 4: measured, see default_ingest_threads; the decoders release the GIL) does the part that has
nothing to do with the GPU -- file reads, PNG decode, label remapping -- up to `depth` batches ahead, delivered in
order.  Everything that talks to HIP stays on the consumer's thread (measured: HIP calls from a second
Python thread, even a lone event wait, cost the first one milliseconds per step): when batch k is handed out, batch k+1
is copied into a ring of reused pinned buffers and its H2D copies are enqueued on a side stream, so they travel while
the GPU works on batch k; the consumer's stream waits on the copy event, never on the host."""
import collections
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np


class DeviceImage:
    """An image that lives on the device for the kernels and on the host (numpy) for viz / PIL users.  Built from a decoded
    array with its device copy already on the way, or -- images not wanted ahead of time (PCA_INGEST_IMAGES=0: the
    ground-truth-semantics flow never looks at them) -- from the lazily opened file: decoded / uploaded on first use."""

    def __init__(self, host, dev, shape=None):
        self._host, self._dev = host, dev
        self.shape = tuple(shape) if shape is not None else tuple(host.shape)

    @property
    def host(self):
        if not isinstance(self._host, np.ndarray):
            self._host = np.asarray(self._host, dtype=np.uint8)
        return self._host

    @property
    def dev(self):
        if self._dev is None:
            import torch
            self._dev = torch.from_numpy(np.ascontiguousarray(self.host)).cuda()
        return self._dev

    def __array__(self, dtype=None, copy=None):
        return self.host if dtype is None else self.host.astype(dtype)


_TORCH_DTYPES = {}


def _torch_dtype(np_dtype):
    t = _TORCH_DTYPES.get(np_dtype)
    if t is None:
        import torch
        t = _TORCH_DTYPES[np_dtype] = torch.from_numpy(np.empty(0, dtype=np_dtype)).dtype
    return t


class PinnedUploader:
    """Host array -> device tensor without a pageable copy: numpy copies the array into a reused pinned block (25 us for
    2 MB) and the H2D copy is asynchronous.  torch's `.to(device)` of a pageable array is synchronous -- the host sits
    in it until the stream's earlier kernels AND the copy are done, 0.2 ms of the unchanged driver's 0.42 ms step."""

    DEPTH = 4

    def __init__(self, device):
        self.device = device
        self._slots = {}                        # kind -> [next, [(pinned tensor, event)] * DEPTH]

    def __call__(self, kind, a):
        return self.upload_many([(kind, a)])[0]

    def upload_many(self, items):
        """items: [(kind, host array)].  ONE call into the library copies the arrays into their pinned blocks -- side by side
        on its small pool of host threads (pca_host_stage_h2d; ctypes releases the GIL for it) -- and enqueues the H2D
        copies on the current stream; one event marks the blocks as reusable.  (The same in Python -- three np.copyto and
        three tensor.copy_ for one KITTI observation -- was 0.15 ms of the unchanged driver's 0.34 ms step; a Python thread
        pool for the copies cost more in wake-ups than it saved.)  Returns the device tensors in order."""
        import ctypes as C
        import torch
        from . import _lib
        arrays = [np.ascontiguousarray(a) for _, a in items]
        n = len(arrays)
        pins, slots, out = [], [], []
        for (kind, _), a in zip(items, arrays):
            ring = self._slots.setdefault(kind, [0, [None] * self.DEPTH])
            i = ring[0] % self.DEPTH
            ring[0] += 1
            slot = ring[1][i]
            if slot is None or slot[0].numel() < a.nbytes:
                slot = (torch.empty(max(a.nbytes, 1), dtype=torch.uint8, pin_memory=True), None)
            elif slot[1] is not None:
                slot[1].synchronize()            # the copy out of this block, DEPTH uploads ago: long done
            pins.append(slot[0])
            slots.append((ring, i, slot[0]))
            out.append(torch.empty(a.shape, dtype=_torch_dtype(a.dtype), device=self.device))
        vp = C.c_void_p * n
        src = vp(*[a.ctypes.data for a in arrays])
        pin = vp(*[p.data_ptr() for p in pins])
        dev = vp(*[d.data_ptr() for d in out])
        nbytes = (C.c_int64 * n)(*[a.nbytes for a in arrays])
        dix = torch.device(self.device).index
        raw = getattr(torch._C, '_cuda_getCurrentRawStream', None)      # ~10x cheaper than current_stream()
        stream = raw(dix if dix is not None else torch.cuda.current_device()) if raw is not None else torch.cuda.current_stream().cuda_stream
        rc = _lib.load().pca_host_stage_h2d(n, src, pin, dev, nbytes, C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f'pca_host_stage_h2d failed ({rc})')
        ev = torch.cuda.Event()
        ev.record()
        for ring, i, block in slots:
            ring[1][i] = (block, ev)
        return out


def _upload_stack(self, kind, arrays):
    """k equally shaped host arrays -> ONE device tensor [k, ...]: the arrays are copied side by side (staging pool) into
    one reused pinned block, which leaves in a single asynchronous H2D copy (the six camera images of a NuScenes observation:
    26 MB that np.stack + a pageable .to(device) moved twice on the consumer's thread, blocking)."""
    import torch
    arrays = [np.ascontiguousarray(a) for a in arrays]
    k, shape, tdtype = len(arrays), arrays[0].shape, _torch_dtype(arrays[0].dtype)
    assert all(a.shape == shape and a.dtype == arrays[0].dtype for a in arrays)
    n = k * int(np.prod(shape))
    ring = self._slots.setdefault(kind, [0, [None] * self.DEPTH])
    i = ring[0] % self.DEPTH
    ring[0] += 1
    slot = ring[1][i]
    if slot is None or slot[0].numel() < n or slot[0].dtype != tdtype:
        slot = (torch.empty(max(n, 1), dtype=tdtype, pin_memory=True), None)
    elif slot[1] is not None:
        slot[1].synchronize()
    import ctypes as C
    from . import _lib
    dev = torch.empty((k, ) + tuple(shape), dtype=tdtype, device=self.device)
    each = arrays[0].nbytes
    vp = C.c_void_p * k
    rc = _lib.load().pca_host_stage_h2d(k, vp(*[a.ctypes.data for a in arrays]), vp(*[slot[0].data_ptr() + j * each for j in range(k)]),
                                        vp(*[dev.data_ptr() + j * each for j in range(k)]), (C.c_int64 * k)(*([each] * k)),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f'pca_host_stage_h2d failed ({rc})')
    ev = torch.cuda.Event()
    ev.record()
    ring[1][i] = (slot[0], ev)
    return dev


PinnedUploader.upload_stack = _upload_stack


def default_ingest_threads():
    """Reader / decoder threads of the prefetching loaders.  Measured on a 256-core box (tools/experiments/loader_step.py,
    full-size synthetic KITTI-360 tree, ms per frame with / without images): 1 thread 6.4 / 2.1, 4 threads 2.2 / 0.53,
    8 threads 2.3 / 1.2, 16 threads 2.8 / 2.0, 32 threads 5.7 / 1.9 -- the decoders release the GIL, the label remap and the
    array bookkeeping around them do not, and beyond a handful of threads they queue for it.  Four."""
    return 4


def check_ring_lifetime(tensors, n_batches):
    """Raises if `n_batches` batches of a prefetching loader are about to be used together although the loader reuses its
    device buffers sooner: tensors it yields carry `_pca_ring` = the number of batches its ring holds."""
    def ring_of(t):
        # the tensor itself, or a wrapper's device copy IF it exists already (DeviceImage._dev, DeviceImages.dev): never
        # triggers a lazy upload
        d = getattr(t, '__dict__', {})
        return min(getattr(c, '_pca_ring', 1 << 30) for c in (t, d.get('_dev'), d.get('dev')))
    ring = min((ring_of(t) for t in tensors if t is not None), default=1 << 30)
    if n_batches > ring - 1:
        raise ValueError(f'these observations come from a prefetching loader that reuses its device buffers every {ring} '
                         f'batches: at most {ring - 1} of them can be integrated in one call (the earlier ones have been '
                         f'overwritten by now); integrate as they arrive, or enlarge the ring (PCA_PREFETCH_RING)')


def compose_label_lut(idx2idx, lo=-1, hi=255):
    """The reference remaps labels with a SEQUENCE of in-place masked assignments (conv_semantic_ids): a later pair
    sees the result of an earlier one.  Returns the composed table as an array indexed by (label - lo)."""
    ids = np.arange(lo, hi + 1, dtype=np.int64)
    out = ids.copy()
    for old, new in idx2idx.items():
        out[out == old] = new
    return out, lo


class PrefetchingLoader:
    """Ring of slots, each with pinned host staging AND device buffers allocated once and reused (a fresh device / pinned
    allocation costs milliseconds when the allocator cache has no free block).  A slot's device buffers are overwritten
    by the copy of a later batch only after an event recorded on the consumer's stream when it came back for the next
    batch: everything it did with the slot has been enqueued by then (a GPU-side wait, nobody blocks on the host).
    Lifetime of what is yielded: the device tensors of a batch are views of a ring of RING reused buffers -- valid for work
    ENQUEUED before the loader is asked for the batch RING - 1 batches later (integrate() per batch: always).  A consumer
    that collects many batches first and integrates them together (integrate_many) is bounded by the ring: the tensors carry
    `_pca_ring` = RING and the accumulators' batch paths refuse more than RING - 1 of them at once (`check_ring_lifetime`)
    instead of reading overwritten frames.  PCA_PREFETCH_RING enlarges the ring."""

    RING = 4                                 # batches: being used, staged ahead, and two of slack

    def __init__(self, loader, depth=4, device=None):
        import torch
        from . import _lib
        _lib.Context.get(device)            # no GPU / no library: fail here, loudly (there is no CPU fallback)
        self.RING = max(int(os.environ.get('PCA_PREFETCH_RING', self.RING)), 2)
        self.loader = loader
        self.depth = depth
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        # PCA_INGEST_SIDE_STREAM=1: copies on a stream of their own (overlap with kernels); default: the consumer's stream
        self.stream = torch.cuda.Stream(self.device) if os.environ.get('PCA_INGEST_SIDE_STREAM') else None
        # PCA_INGEST_IMAGES=0: do not decode / upload images ahead (the ground-truth-semantics flow never reads them)
        self.images = os.environ.get('PCA_INGEST_IMAGES', '1') != '0'
        self.lut = None
        if hasattr(loader, 'idx2idx'):
            self.lut = compose_label_lut(loader.idx2idx)
        bs = max(int(getattr(loader, 'batch_size', 1)), 1)
        self._ring = [dict(pin={}, dev={}, copied=None, released=None) for _ in range(self.RING * bs)]
        self._ring_next = 0

    def __len__(self):
        return len(self.loader)

    def _buffers(self, slot, name, shape, dtype):
        """(pinned, device) buffers `name` of a slot, grown on demand and reused from then on."""
        import torch
        n = int(np.prod(shape))
        pin, dev = slot['pin'].get(name), slot['dev'].get(name)
        if pin is None or pin.numel() < n or pin.dtype != dtype:
            pin = slot['pin'][name] = torch.empty(max(n, 1), dtype=dtype).pin_memory()
            dev = slot['dev'][name] = torch.empty(max(n, 1), dtype=dtype, device=self.device)
        return pin[:n].view(*shape), dev[:n].view(*shape)

    def _to_device(self, obs):
        """Consumer thread: stage one observation (host arrays) and enqueue its H2D copies on the side stream."""
        import torch
        img, pc, sem_gt = obs
        slot = self._ring[self._ring_next % len(self._ring)]
        self._ring_next += 1
        if slot['copied'] is not None:
            slot['copied'].synchronize()                                # long done: RING batches ago
        lazy_img = not isinstance(img, np.ndarray)           # images are not staged ahead: see DeviceImage
        src = [('pc', np.ascontiguousarray(pc, dtype=np.float32)),
               ('sem', np.ascontiguousarray(np.asarray(sem_gt)[:, -1]).astype(np.uint8))]
        if not lazy_img:
            src.append(('img', np.ascontiguousarray(img, dtype=np.uint8)))
        dev = {}
        stream = self.stream if self.stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(stream):
            if slot['released'] is not None and self.stream is not None:
                stream.wait_event(slot['released'])                     # kernels that read the device buffers are done
            for name, a in src:
                pin, d = self._buffers(slot, name, a.shape, _torch_dtype(a.dtype))
                # numpy does the host copy: torch's CPU copy_ fans a 2 MB copy out over every core of the box and
                # took 1-3 ms per call here
                np.copyto(pin.numpy(), a)
                d.copy_(pin, non_blocking=True)
                d._pca_ring = self.RING          # a view of a reused buffer: see "lifetime" in the class docstring
                dev[name] = d
            ev = torch.cuda.Event()
            ev.record(stream)
        slot['copied'] = ev
        image = DeviceImage(img, None, shape=(img.size[1], img.size[0], 3)) if lazy_img else DeviceImage(src[2][1], dev['img'])
        return (image, dev['pc'], dev['sem']), ev, slot

    def _read(self, idx):
        """read_obs with the label remap done through the composed table (identical result, one pass)."""
        ld = self.loader
        if self.lut is None or not hasattr(ld, 'pc_paths'):
            obs = ld.read_obs(idx)
            if self.images and not isinstance(obs[0], np.ndarray):
                obs = (np.asarray(obs[0], dtype=np.uint8), ) + tuple(obs[1:])   # decode on the reader thread
            return obs
        import os

        import PIL.Image as Image
        from datasets.kitti360_utils import read_pc_bin_file, read_sem_gt_bin_file
        pc = read_pc_bin_file(os.path.join(ld.root_path, ld.pc_paths[idx]))
        img = Image.open(os.path.join(ld.root_path, ld.img_paths[idx]))
        if self.images:
            img = np.asarray(img, dtype=np.uint8)    # decode HERE, on the reader thread (Image.open is lazy)
        sem = read_sem_gt_bin_file(os.path.join(ld.root_path, ld.sem_gt_paths[idx]))
        if sem is None:
            sem = np.zeros((pc.shape[0], 1))
        table, lo = self.lut
        k = sem[:, 0].astype(np.int64) - lo
        ok = (k >= 0) & (k < table.size)
        out = sem[:, 0].astype(np.int64)
        out[ok] = table[k[ok]]
        return (img, pc, out[:, None])

    def __iter__(self):
        import torch
        n, bs = len(self.loader), self.loader.batch_size
        torch.cuda.set_device(self.device)
        # host-only work on the pool's threads: no HIP call there.  Batches are submitted in order and collected in order.
        n_threads = int(os.environ.get('PCA_INGEST_THREADS', default_ingest_threads())) if os.environ.get('PCA_INGEST_THREAD', '1') != '0' else 0
        pool = ThreadPoolExecutor(max_workers=n_threads) if n_threads > 0 else None
        pending = collections.deque()
        state = {'idx': 0}

        def read_batch(i0):
            return [self._read(i0 + k) for k in range(bs)]

        def stage():
            # (as many batches in flight as reader threads can work on: a depth of 4 kept 28 of 32 threads idle)
            while state['idx'] + bs <= n and len(pending) < max(self.depth, n_threads + n_threads // 2, 1):
                i0 = state['idx']
                state['idx'] += bs
                pending.append(pool.submit(read_batch, i0) if pool is not None else i0)
            if not pending:
                if pool is not None:
                    pool.shutdown(wait=False)
                return None
            head = pending.popleft()
            try:
                item = head.result() if pool is not None else read_batch(head)
            except BaseException as e:           # surfaced in the consumer
                return e
            return [self._to_device(obs) for obs in item]

        ahead = stage()
        held = []
        while True:
            item = ahead
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            cur = torch.cuda.current_stream(self.device)
            for slot in held:                    # the previous batch: all its uses are on the consumer's stream by now
                rel = torch.cuda.Event()
                rel.record(cur)
                slot['released'] = rel
            held = [slot for _, _, slot in item]
            if self.stream is not None:
                for _, ev, _ in item:
                    cur.wait_event(ev)
            ahead = stage()                      # the next batch's copies travel while this one is being integrated
            yield [obs for obs, _, _ in item]


class DeviceImages(list):
    """The camera images of one NuScenes observation: a list of the host images (what the reference's observation holds:
    viz and the semseg model read those) whose stacked device copy [ncam,H,W,3] u8 is already on its way (`dev`).
    NOTE on lifetime: `dev` (and the `pc` / `pc_cam_idx` tensors of the same observation) are views of a ring of RING
    reused device buffers (default 64 batches = more than a scene; PCA_PREFETCH_RING); the loader overwrites a slot RING
    batches later, in stream order after everything the consumer had enqueued by then.  The tensors carry `_pca_ring` = RING:
    integrate_many refuses to take more than RING - 1 batches at once instead of reading overwritten frames."""

    def __init__(self, host_images, dev):
        super().__init__(host_images)
        self.dev = dev


class NuScenesPrefetchingLoader:
    """Ingest pipeline of the NuScenes flow (reference: obs_dataloaders/nuscenes_obs_dataloader.py:103-220).
    Reader threads run `loader.read_host` -- sample records, sweep merging, image decode -- up to `depth` batches ahead, in
    order.  The consumer's thread (the only one that talks to HIP) stages the six decoded images into ONE pinned block (the
    host copies side by side on the staging pool) and enqueues one 26 MB H2D copy instead of a pageable, blocking
    `.to(device)` of an `np.stack`; the lidar points go up once, K0n projects them on the device and the (N,7) rows the
    accumulator takes are assembled there -- nothing of the observation comes back to the host.
    Device mode of the sweep merge (PCA_NUSC_SWEEPS=device, no sweep_provider): the reader threads only run
    `collect_sweep_inputs` (no HIP call); the consumer's thread stages the raw f32 rows of the sweeps through the pinned ring,
    runs the merge (K0s) with the points left on the device, stages the images behind it, waits once for the hit counts (from
    which `inst_tokens` / `inst_cls` / `inst_center` follow) and feeds K0n from the device points -- the merged points never
    visit the host."""

    RING = 64                                # batches: a whole scene (~40 samples) can be collected and integrated at once

    def __init__(self, loader, depth=3, device=None):
        import torch
        from . import _lib
        self.ctx = _lib.Context.get(device)
        self.RING = max(int(os.environ.get('PCA_PREFETCH_RING', self.RING)), 2)
        self.loader = loader
        self.depth = depth
        self.device = torch.device('cuda', self.ctx.device_index)
        bs = max(int(getattr(loader, 'batch_size', 1)), 1)
        # device buffers: one slot per batch element of the ring (what the consumer may still be using); the PINNED staging
        # blocks are a small ring of their own (depth + 1 uploads in flight at most: a 26 MB page-locked block per device slot
        # was 1.8 GB of pinned memory per loader), and scratch that only ever lives on the device has no pinned twin
        self._ring = [dict(dev={}) for _ in range(self.RING * bs)]
        self._pins = [dict(pin={}, copied=None) for _ in range((max(int(depth), 1) + 1) * bs)]
        self._next = 0

    def __len__(self):
        return len(self.loader)

    def _dev_buffer(self, slot, name, shape, dtype):
        """device buffer `name` of a ring slot, grown on demand and reused from then on"""
        import torch
        n = int(np.prod(shape))
        dev = slot['dev'].get(name)
        if dev is None or dev.numel() < n or dev.dtype != dtype:
            dev = slot['dev'][name] = torch.empty(max(n, 1), dtype=dtype, device=self.device)
        return dev[:n].view(*shape)

    def _pin_buffer(self, pslot, name, shape, dtype):
        import torch
        n = int(np.prod(shape))
        pin = pslot['pin'].get(name)
        if pin is None or pin.numel() < n or pin.dtype != dtype:
            pin = pslot['pin'][name] = torch.empty(max(n, 1), dtype=dtype).pin_memory()
        return pin[:n].view(*shape)

    def _host_part(self, idx):
        # device mode of the sweep merge (PCA_NUSC_SWEEPS=device): reader threads only collect the merge's host inputs
        device_sweeps = getattr(self.loader, 'device_sweeps', None)
        if device_sweeps is not None and device_sweeps():
            obs, geom = self.loader.read_host(idx, defer_sweeps=True)
        else:
            obs, geom = self.loader.read_host(idx)
        imgs = [np.asarray(im, dtype=np.uint8) if not isinstance(im, str) else im for im in obs['images']]   # decode here
        return obs, geom, imgs

    def _to_device(self, item):
        import ctypes as C

        import torch
        from . import _lib
        obs, geom, imgs = item
        slot = self._ring[self._next % len(self._ring)]
        pslot = self._pins[self._next % len(self._pins)]
        self._next += 1
        if pslot['copied'] is not None:
            pslot['copied'].synchronize()                  # the copies out of this pinned block, a few uploads ago
        lib, ctx = self.ctx.lib, self.ctx
        ncam = len(geom['cams_K'])
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def stage(src, pin, dev, nbytes):                    # pinned copies on the library's staging threads, H2D enqueued
            vp = C.c_void_p * len(src)
            if lib.pca_host_stage_h2d(len(src), vp(*src), vp(*pin), vp(*dev), (C.c_int64 * len(src))(*nbytes), stream) != 0:
                raise RuntimeError('pca_host_stage_h2d failed')

        src, pin, dev, nbytes = [], [], [], []
        merge = None
        if geom.get('sweeps') is not None:
            # the merge on the device: the raw f32 rows of the sweeps go up through the pinned ring, the launches and the
            # tally's read-back are enqueued, and the images are staged behind them before the (one) wait
            from datasets import nuscenes_sweeps as ns
            inputs, cfg = geom['sweeps']
            tables = ns.sweep_tables(inputs)
            raw = tables[0]
            pin_raw = self._pin_buffer(pslot, 'raw', raw.shape, torch.float32)
            dev_raw = self._dev_buffer(slot, 'raw', raw.shape, torch.float32)
            if raw.shape[0]:
                stage([raw.ctypes.data], [pin_raw.data_ptr()], [dev_raw.data_ptr()], [raw.nbytes])
            merge, keep_alive = ns.merge_sweeps_launch(inputs, cfg['center_radius'], cfg['in_box_tolerance'], device_points=True,
                                                       raw_dev=dev_raw, tables=tables)
        else:
            pc = np.ascontiguousarray(geom['pc'], dtype=np.float64)
            pin_pc, dev_pc = self._pin_buffer(pslot, 'pc', pc.shape, torch.float64), self._dev_buffer(slot, 'pc', pc.shape, torch.float64)
            src, pin, dev, nbytes = [pc.ctypes.data], [pin_pc.data_ptr()], [dev_pc.data_ptr()], [pc.nbytes]
        images = obs['images']
        real = all(isinstance(im, np.ndarray) and im.ndim == 3 for im in imgs) and len({im.shape for im in imgs}) == 1
        if real:
            ishape = (len(imgs), ) + imgs[0].shape
            pin_im, dev_im = self._pin_buffer(pslot, 'img', ishape, torch.uint8), self._dev_buffer(slot, 'img', ishape, torch.uint8)
            imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
            each = imgs[0].nbytes
            for k, im in enumerate(imgs):
                src.append(im.ctypes.data); pin.append(pin_im.data_ptr() + k * each)
                dev.append(dev_im.data_ptr() + k * each); nbytes.append(each)
        if src:
            stage(src, pin, dev, nbytes)
        if real:
            images = DeviceImages(obs['images'], dev_im)
        ev = torch.cuda.Event()
        ev.record()
        pslot['copied'] = ev
        if merge is not None:
            res = merge.finish()                             # the wait; the merged points stay on the device
            del keep_alive
            obs = dict(obs)
            self.loader.fill_instances(obs, res['instances_token'], np.array([tr['cls'] for tr in res['tracks']], np.float32),
                                       res['instances_center'])
            dev_pc = self._dev_buffer(slot, 'pc', tuple(res['points'].shape), torch.float64)
            dev_pc.copy_(res['points'])                      # f32 -> f64 is exact
        n = dev_pc.shape[0]
        # projection (K0n) on the device, rows [x, y, z (ego), intensity, u, v, instance] assembled there
        xyz = dev_pc[:, :3].contiguous()
        ego = self._dev_buffer(slot, 'ego', (n, 3), torch.float64)
        uv = self._dev_buffer(slot, 'uv', (n, 2), torch.float64)
        cam = self._dev_buffer(slot, 'cam', (n, ), torch.int64)
        rows = self._dev_buffer(slot, 'rows', (n, 7), torch.float64)
        cam_from_glob = np.stack([np.linalg.inv(T) for T in geom['cams_glob_from_self']])
        ctx.check(lib.pca_nusc_project_cams(
            ctx.h, xyz.data_ptr(), n, _lib.f64_array(geom['ego_from_lidar'], 16), _lib.f64_array(geom['glob_from_ego'], 16),
            _lib.f64_array(cam_from_glob, 16 * ncam), _lib.f64_array(np.stack(geom['cams_K']), 9 * ncam),
            _lib.f64_array(np.stack(geom['cams_wh']), 2 * ncam), ncam, ego.data_ptr(), uv.data_ptr(), cam.data_ptr(),
            ctx.stream()))
        ld = self.loader
        rows[:, 0:3] = ego
        rows[:, 3] = dev_pc[:, ld.int_idx]
        rows[:, 4:6] = uv
        rows[:, 6] = dev_pc[:, ld.inst_idx]
        for t in (rows, cam) + ((dev_im, ) if real else ()):
            t._pca_ring = self.RING                # views of reused buffers (see DeviceImages)
        out = dict(obs)
        out['images'] = images
        out['pc'] = rows
        out['pc_cam_idx'] = cam
        return out

    def __iter__(self):
        import torch
        n, bs = len(self.loader), self.loader.batch_size
        torch.cuda.set_device(self.device)
        n_threads = int(os.environ.get('PCA_INGEST_THREADS', default_ingest_threads()))
        pool = ThreadPoolExecutor(max_workers=max(n_threads, 1))
        pending = collections.deque()
        idx = 0
        try:
            while True:
                while idx + bs <= n and len(pending) < max(self.depth, 1):
                    pending.append([pool.submit(self._host_part, idx + k) for k in range(bs)])
                    idx += bs
                if not pending:
                    return
                batch = [f.result() for f in pending.popleft()]
                yield [self._to_device(item) for item in batch]
        finally:
            pool.shutdown(wait=False)
