"""Preview sheets of BEV samples as PNG files made on the device (PCA_VIZ=device; include/pca.h: KP).

The drivers save a picture beside every sample (run_kitti360_bev_gen.py:267-270 of the reference calls viz_bev); the default
viz_bev builds a matplotlib figure per sample on the calling thread.  Here the picture is a sheet of 3 x 5 panels -- one row
per point set (present, future, full), the columns road, intensity, rgb, dynamic, elevation -- composed, colour-mapped,
overlaid with the set's trajectories, PNG-filtered, compressed and summed on the device (pca_preview_sheets,
pca_deflate_chunks[_dyn], pca_adler32_chunks); the host only splices the pieces into the container (pca_host_png_assemble).
The layout of the picture is not part of the parity contract with the reference.

The sheet, exactly: [21,px,px] float16 -> RGB8, 3 px high, 5 px wide; pixel (r, q) of a panel shows plane element [r][q].
Scalar panels show LUT[clamp(floor((v - lo) * scale), 0, 255)] in float32 with scale = 256 / (hi - lo) (NaN -> entry 0); road,
intensity and dynamic use the range (0, 1) as the reference's viz_bev does, elevation uses `elev_range`, by default
(-0.5, 2.0) m -- this module's choice: the reference lets matplotlib scale every elevation panel to its own extremes, which
makes panels incomparable.  The rgb panel shows floor(min(max(v, 0), 1) * 255 + 0.5) per channel.  Every polyline of
trajs_<set> is drawn in red, one pixel wide, on all five panels of that set's row (sheet_polylines).

Not drawn: the camera-image row of the matplotlib figure (`rgbs`, `semsegs`), `gt_lanes`, and extra `sem_planes`."""
import ctypes as C
import os

import numpy as np

from .writer import DEFLATE_CHUNK_DTYPE, DEFLATE_CHUNK_MAX, deflate_bound

POLYLINE_DTYPE = np.dtype([('sample', '<i4'), ('set', '<i4'), ('first', '<i4'), ('count', '<i4')])       # pca_preview_polyline
SETS = ('present', 'future', 'full')
ELEV_RANGE = (-0.5, 2.0)
FILTERS = {'none': 0, 'sub': 1, 'up': 2}
# the pair with the smallest median file on the headline samples (profiles/preview_device.txt)
DEFAULT_FILTER = 'up'
DEFAULT_HUFFMAN = 'dynamic'
COORD_MAX = 1 << 29

# (matplotlib.colormaps['viridis'](np.arange(256))[:, :3] * 255).round() as a literal, so that matplotlib is not needed
VIRIDIS = np.frombuffer(bytes.fromhex(
    '44015444025645045745055946075a46085c460a5d460b5e470d60470e61471063471164471365481467481668481769'
    '48186a481a6c481b6d481c6e481d6f481f70482071482173482374482475482576482677482878482979472a7a472c7a'
    '472d7b472e7c472f7d46307e46327e46337f463480453581453781453882443983443a83443b84433d84433e85423f85'
    '4240864241864142874144874045884046883f47883f48893e49893e4a893e4c8a3d4d8a3d4e8a3c4f8a3c508b3b518b'
    '3b528b3a538b3a548c39558c39568c38588c38598c375a8c375b8d365c8d365d8d355e8d355f8d34608d34618d33628d'
    '33638d32648e32658e31668e31678e31688e30698e306a8e2f6b8e2f6c8e2e6d8e2e6e8e2e6f8e2d708e2d718e2c718e'
    '2c728e2c738e2b748e2b758e2a768e2a778e2a788e29798e297a8e297b8e287c8e287d8e277e8e277f8e27808e26818e'
    '26828e26828e25838e25848e25858e24868e24878e23888e23898e238a8d228b8d228c8d228d8d218e8d218f8d21908d'
    '21918c20928c20928c20938c1f948c1f958b1f968b1f978b1f988b1f998a1f9a8a1e9b8a1e9c891e9d891f9e891f9f88'
    '1fa0881fa1881fa1871fa28720a38620a48621a58521a68522a78522a88423a98324aa8325ab8225ac8226ad8127ad81'
    '28ae8029af7f2ab07f2cb17e2db27d2eb37c2fb47c31b57b32b67a34b67935b77937b87838b9773aba763bbb753dbc74'
    '3fbc7340bd7242be7144bf7046c06f48c16e4ac16d4cc26c4ec36b50c46a52c56954c56856c66758c7655ac8645cc863'
    '5ec96260ca6063cb5f65cb5e67cc5c69cd5b6ccd5a6ece5870cf5773d05675d05477d1537ad1517cd2507fd34e81d34d'
    '84d44b86d54989d5488bd6468ed64590d74393d74195d84098d83e9bd93c9dd93ba0da39a2da37a5db36a8db34aadc32'
    'addc30b0dd2fb2dd2db5de2bb8de29bade28bddf26c0df25c2df23c5e021c8e020cae11fcde11dd0e11cd2e21bd5e21a'
    'd8e219dae319dde318dfe318e2e418e5e419e7e419eae51aece51befe51cf1e51df4e61ef6e620f8e621fbe723fde725'),
    dtype=np.uint8).reshape(256, 3)


def stream_bytes(px):
    """Bytes of the PNG scanline stream of one sheet (pca_preview_stream_bytes)."""
    return (1 + 15 * px) * 3 * px


def panel_ranges(elev_range=ELEV_RANGE):
    """(lo, scale) of road, intensity, dynamic, elevation as the float32 [4,2] pca_preview_sheets takes: scale = f32(256) /
    (f32(hi) - f32(lo)), computed once, here."""
    out = np.empty((4, 2), dtype=np.float32)
    for i, (lo, hi) in enumerate(((0., 1.), (0., 1.), (0., 1.), elev_range)):
        lo, hi = np.float32(lo), np.float32(hi)
        if not hi > lo:
            raise ValueError(f'empty range ({lo}, {hi})')
        out[i] = lo, np.float32(256) / (hi - lo)
    return out


def sheet_polylines(trajs, px):
    """The polylines of one set as the device draws them: a list of int32 (n, 2) arrays of grid points (x, y) = floor of
    the first two columns of every (N, 2) or (N, 3) polyline of `trajs`.  A polyline with a non-finite vertex is dropped, an
    empty one draws nothing and is left out, one vertex stays one point; nothing is clipped to the px x px grid (the device
    skips the points outside it) beyond +-2^29, far outside any grid."""
    if not 1 <= int(px) <= 4096:
        raise ValueError(f'px must be 1 .. 4096, not {px}')
    out = []
    for t in trajs if trajs is not None else ():
        t = np.asarray(t, dtype=np.float64)
        if t.ndim != 2 or t.shape[0] == 0 or t.shape[1] < 2:
            continue
        xy = t[:, :2]
        if not np.isfinite(xy).all():
            continue
        out.append(np.clip(np.floor(xy), -COORD_MAX, COORD_MAX).astype(np.int32))
    return out


def polyline_tables(trajs_per_sample, px):
    """(vertices int32 [n,2], records POLYLINE_DTYPE) of a block: trajs_per_sample[i] = (trajs_present, trajs_future,
    trajs_full) of sample i."""
    verts, rows, at = [], [], 0
    for i, sets in enumerate(trajs_per_sample):
        for s, trajs in enumerate(sets):
            for line in sheet_polylines(trajs, px):
                rows.append((i, s, at, len(line)))
                verts.append(line)
                at += len(line)
    v = np.concatenate(verts) if verts else np.zeros((0, 2), dtype=np.int32)
    return np.ascontiguousarray(v, dtype=np.int32), np.array(rows, dtype=POLYLINE_DTYPE)


def stream_chunks(px, k=1):
    """The chunk table that cuts the scanline streams of k sheets, back to back, into pieces of at most 32 768 bytes (cuts
    fall mid-row; no chunk spans two sheets): (table, chunks per sheet)."""
    sb = stream_bytes(px)
    one = [(at, min(DEFLATE_CHUNK_MAX, sb - at), 0) for at in range(0, sb, DEFLATE_CHUNK_MAX)]
    t = np.tile(np.array(one, dtype=DEFLATE_CHUNK_DTYPE), k)
    t['offset'] += np.repeat(np.arange(k, dtype=np.int64) * sb, len(one))
    return t, len(one)


def adler32_combine(adler_a, adler_b, len_b):
    from . import _lib
    return int(_lib.load().pca_host_adler32_combine(int(adler_a), int(adler_b), int(len_b)))


def png_assemble(width, height, pieces, adler):
    """One PNG from byte-aligned deflate pieces (uint8 arrays) of the scanline stream whose Adler-32 is `adler`, as bytes
    (pca_host_png_assemble)."""
    from . import _lib
    lib = _lib.load()
    arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in pieces]
    n = len(arrs)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
    nbytes = np.array([a.size for a in arrs], dtype=np.int64)
    cap = 65 + int(nbytes.sum())
    out = np.empty(cap, dtype=np.uint8)
    got = lib.pca_host_png_assemble(int(width), int(height), n, C.addressof(ptrs), nbytes.ctypes.data, int(adler), out.ctypes.data, cap)
    if got < 0:
        raise RuntimeError(f'pca_host_png_assemble failed ({got})')
    return out[:got].tobytes()


class _Tables:
    """What depends on (px, k, device) alone: the chunk table on the device; and the LUT per device."""
    _chunks, _luts = {}, {}

    @classmethod
    def chunks(cls, device, px, k):
        import torch
        key = (device.index, px, k)
        if key not in cls._chunks:
            t, per = stream_chunks(px, k)
            cls._chunks[key] = (torch.from_numpy(t.view(np.uint8).copy()).to(device), t['length'][:per].astype(np.int64), per)
        return cls._chunks[key]

    @classmethod
    def lut(cls, device):
        import torch
        if device.index not in cls._luts:
            cls._luts[device.index] = torch.from_numpy(VIRIDIS.copy()).to(device)
        return cls._luts[device.index]


class SheetJob:
    """The sheets of ALL samples of one [k,21,px,px] block in flight on the context's side stream: one launch set (overlay,
    rows, Adler-32, deflate), then ONE copy of (sizes, adlers, bytes).  Modelled on writer._DeviceJob; holds planes, tables,
    outputs and workspace until the copy has been waited for."""

    def __init__(self, planes, trajs_per_sample, elev_range=ELEV_RANGE, filter=DEFAULT_FILTER, huffman=DEFAULT_HUFFMAN):
        import weakref

        import torch
        from . import _lib
        assert planes.is_cuda and planes.is_contiguous() and planes.dtype == torch.float16 and planes.dim() == 4 and planes.shape[1] == 21
        if filter not in FILTERS:
            raise ValueError(f'filter must be one of {sorted(FILTERS)}, not {filter!r}')
        if huffman not in ('fixed', 'dynamic'):
            raise ValueError(f"huffman must be 'fixed' or 'dynamic', not {huffman!r}")
        self.k = k = int(planes.shape[0])
        self.px = px = int(planes.shape[-1])
        assert planes.shape[2] == px and len(trajs_per_sample) == k
        self.ctx = ctx = _lib.Context.get(planes.device)
        self.planes_ref = weakref.ref(planes)
        dev = planes.device
        table, self.lengths, self.per = _Tables.chunks(dev, px, k)
        self.n = n = k * self.per
        self.cap = cap = int(sum(deflate_bound(int(l)) for l in self.lengths))
        verts, lines = polyline_tables(trajs_per_sample, px)
        # (pageable uploads on the current stream: the copy has left the host arrays when .to() returns)
        d_verts = torch.from_numpy(verts.reshape(-1)).to(dev) if len(verts) else None
        d_lines = torch.from_numpy(lines.view(np.uint8).copy()).to(dev) if len(lines) else None
        d_lut = _Tables.lut(dev)
        ranges = panel_ranges(elev_range)
        sb = stream_bytes(px)
        stream = torch.empty(k * sb, dtype=torch.uint8, device=dev)
        ws = torch.empty(int(ctx.lib.pca_preview_workspace_bytes(k, px)) + int(ctx.lib.pca_deflate_workspace_bytes(n)) + 256,
                         dtype=torch.uint8, device=dev)
        ws_deflate = ws.data_ptr() + ((int(ctx.lib.pca_preview_workspace_bytes(k, px)) + 255) & ~255)
        out = torch.empty(12 * n + k * cap, dtype=torch.uint8, device=dev)          # sizes, adlers, (CRC words, unused), pieces
        self.host = torch.empty(12 * n + k * cap, dtype=torch.uint8, pin_memory=True)
        p = out.data_ptr()
        lib, s = ctx.lib, ctx.stream()
        rc = lib.pca_preview_sheets(ctx.h, planes.data_ptr(), k, px, d_verts.data_ptr() if d_verts is not None else None, len(verts),
                                    d_lines.data_ptr() if d_lines is not None else None, len(lines), d_lut.data_ptr(),
                                    ranges.ctypes.data, FILTERS[filter], stream.data_ptr(), ws.data_ptr(), s)
        if rc >= 0:
            rc = lib.pca_adler32_chunks(ctx.h, stream.data_ptr(), table.data_ptr(), n, p + 4 * n, s)
        if rc >= 0:
            deflate = lib.pca_deflate_chunks_dyn if huffman == 'dynamic' else lib.pca_deflate_chunks
            rc = deflate(ctx.h, stream.data_ptr(), table.data_ptr(), n, p + 12 * n, p, p + 8 * n, ws_deflate, s)
        if rc < 0:
            ctx.check(rc)
        # (the copy runs behind the kernels on the same side stream: its ticket covers them, as in writer._DeviceJob)
        self.ticket = lib.pca_host_d2h_async(ctx.h, p, self.host.data_ptr(), self.host.numel(), s)
        if self.ticket < 0:
            ctx.check(self.ticket)
        self.keep = (planes, table, d_verts, d_lines, d_lut, stream, ws, out)

    def wait(self):
        """On the thread that talks to HIP: the results are in `host`, the device blocks go back."""
        if self.keep is not None:
            self.ctx.check(self.ctx.lib.pca_host_d2h_wait(self.ctx.h, self.ticket))
            self.keep = None
            self.ctx.poll_status()

    def png(self, index):
        """The PNG of sample `index` as bytes (any thread, after wait(): host work only)."""
        n, m = self.n, self.per
        h = self.host.numpy()
        sizes, adlers = h[:4 * n].view(np.uint32), h[4 * n:8 * n].view(np.uint32)
        at = 12 * n + int(sizes[:index * m].sum(dtype=np.int64))
        total = int(sizes[index * m:(index + 1) * m].sum(dtype=np.int64))
        adler = 1
        for c in range(m):
            adler = adler32_combine(adler, adlers[index * m + c], self.lengths[c])
        return png_assemble(5 * self.px, 3 * self.px, [h[at:at + total]], adler)

    def __del__(self):
        try:
            if self.keep is not None:
                self.ctx.lib.pca_host_d2h_wait(self.ctx.h, self.ticket)
        except Exception:                    # noqa: BLE001  (interpreter shutdown)
            pass


def render_sheets(planes, trajs_per_sample, *, elev_range=ELEV_RANGE, filter=DEFAULT_FILTER, huffman=DEFAULT_HUFFMAN):
    """planes: cuda float16 [k,21,px,px]; trajs_per_sample[i] = (trajs_present, trajs_future, trajs_full) of sample i.
    Returns the k PNG files as bytes; one launch set and one copy for the block."""
    job = SheetJob(planes, trajs_per_sample, elev_range, filter, huffman)
    job.wait()
    return [job.png(i) for i in range(job.k)]


def planes_of(bev):
    """The [21,px,px] float16 block of a sample's 15 host arrays (a plain dict of the reference's host path, or a sample whose
    device planes are gone), in pack_bev's plane order."""
    out = None
    for s, set_name in enumerate(SETS):
        for name, k0, k in (('road', 0, 1), ('intensity', 1, 1), ('rgb', 2, 3), ('dynamic', 5, 1), ('elevation', 6, 1)):
            a = np.asarray(bev[f'{name}_{set_name}'], dtype=np.float16)
            if out is None:
                px = a.shape[-1]
                out = np.empty((21, px, px), dtype=np.float16)
            out[7 * s + k0:7 * s + k0 + k] = a.reshape(k, px, px)
    return out


def selected():
    """True while PCA_VIZ=device: viz_bev submits a device preview, and a LazyBev made meanwhile keeps its device planes for
    it."""
    return os.environ.get('PCA_VIZ', 'matplotlib') == 'device'
