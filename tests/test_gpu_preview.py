"""Preview sheets made on the device (pca_preview_sheets, pca_adler32_chunks, pca_amd/preview.py, PCA_VIZ=device) against the
numpy model of tests/preview_common.py: every byte of the scanline streams, every pixel of the PNG files."""
import os
import zlib

import numpy as np
import pytest
from conftest import PKG  # noqa: F401
from preview_common import (ELEV_RANGE, crafted_block, decode_png, filter_rows, model_lut, model_of_bev, model_sheet, stream_bytes,
                            unfilter)

pytestmark = pytest.mark.gpu

GUARD = 64
KITTI_FILTERS = [10, 11, 12, 16, 18, 255]
SEM_IDXS = {'road': 0, 'car': 13, 'truck': 14, 'bus': 15, 'motorcycle': 17}
BEV_KITTI = dict(type='sem', view_size=30, pixel_size=32, max_trans_radius=0., zoom_thresh=0., do_warp=False,
                 int_scaler=20., int_sep_scaler=20., int_mid_threshold=0.5, height_filter=None)


def random_lut():
    """256 distinct colours, none of them the overlay's red: a wrong index cannot hide behind equal neighbours."""
    rng = np.random.default_rng(5)
    lut = np.stack([np.arange(256), rng.permutation(256), rng.integers(0, 256, 256)], axis=1).astype(np.uint8)
    lut[lut[:, 0] == 255, 2] = 9
    return lut


def run_adler(src, rows):
    import torch

    from pca_amd import _lib
    from pca_amd.writer import DEFLATE_CHUNK_DTYPE
    ctx = _lib.Context.get()
    table = np.array([(o, l, 0) for o, l in rows], dtype=DEFLATE_CHUNK_DTYPE)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_tab = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    d_out = torch.full((len(rows) + 4, ), 0x55555555, dtype=torch.int32, device='cuda')
    ticket = ctx.lib.pca_adler32_chunks(ctx.h, d_src.data_ptr(), d_tab.data_ptr(), len(rows), d_out.data_ptr(), ctx.stream())
    if ticket < 0:
        ctx.check(ticket)
    ctx.check(ctx.lib.pca_host_d2h_wait(ctx.h, ticket))
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.all(out[len(rows):] == 0x55555555), 'words written behind the last chunk'
    return out[:len(rows)]


def test_adler32_of_chunks_equals_zlib():
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, 200000, dtype=np.uint8)
    src[1000:1000 + 32768 + 7] = 0xff                               # sum((n - i) d) of 32 768 bytes of 0xff does not fit 32 bits
    rows = [(1003, 32768), (1000, 32768), (5, 0), (77, 1), (78, 1), (79, 1), (80, 1), (41001, 5551), (41002, 5552), (41003, 5553),
            (60001, 2), (60002, 3), (60003, 4), (60001, 5), (70000, 32767), (70001, 32768), (110003, 32768)]
    rows += [(int(o), int(l)) for o, l in zip(rng.integers(0, 150000, 40), rng.integers(0, 32769, 40))]
    got = run_adler(src, rows)
    raw = src.tobytes()
    for c, (o, l) in enumerate(rows):
        assert got[c] == zlib.adler32(raw[o:o + l]), (c, o, l)
    assert got[2] == 1


def run_sheets(planes, trajs, ftype, lut, elev_range=ELEV_RANGE):
    """One pca_preview_sheets call on a [k,21,px,px] block into a buffer that starts at an odd address, with guards around
    it: returns the k scanline streams."""
    import torch

    from pca_amd import _lib
    from pca_amd.preview import panel_ranges, polyline_tables
    ctx = _lib.Context.get()
    k, px = planes.shape[0], planes.shape[-1]
    sb = stream_bytes(px)
    assert ctx.lib.pca_preview_stream_bytes(px) == sb
    verts, lines = polyline_tables(trajs, px)
    d_planes = torch.from_numpy(planes).cuda()
    d_verts = torch.from_numpy(verts.reshape(-1).copy()).cuda()
    d_lines = torch.from_numpy(lines.view(np.uint8).copy()).cuda()
    d_lut = torch.from_numpy(lut).cuda()
    front = GUARD + 1
    d_out = torch.full((front + k * sb + GUARD, ), 0xaa, dtype=torch.uint8, device='cuda')
    d_ws = torch.empty(ctx.lib.pca_preview_workspace_bytes(k, px), dtype=torch.uint8, device='cuda')
    ranges = panel_ranges(elev_range)
    ticket = ctx.lib.pca_preview_sheets(ctx.h, d_planes.data_ptr(), k, px, d_verts.data_ptr() if len(verts) else None, len(verts),
                                        d_lines.data_ptr() if len(lines) else None, len(lines), d_lut.data_ptr(), ranges.ctypes.data,
                                        ftype, d_out.data_ptr() + front, d_ws.data_ptr(), ctx.stream())
    if ticket < 0:
        ctx.check(ticket)
    ctx.check(ctx.lib.pca_host_d2h_wait(ctx.h, ticket))
    out = d_out.cpu().numpy()
    assert np.all(out[:front] == 0xaa) and np.all(out[front + k * sb:] == 0xaa), 'guard bytes around the streams were written'
    return [out[front + i * sb:front + (i + 1) * sb].tobytes() for i in range(k)]


@pytest.fixture(scope='module')
def blocks():
    """The crafted blocks and their model sheets, computed once: (px, k) -> (planes, trajs, lut, [model image per sample])."""
    lut = random_lut()
    out = {}
    for px in (5, 16, 64):
        planes, trajs = crafted_block(px, 3)
        sheets = [model_sheet(planes[i], trajs[i], lut) for i in range(3)]
        out[px, 3] = (planes, trajs, lut, sheets)
        out[px, 1] = (planes[:1], trajs[:1], lut, sheets[:1])
    return out


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('px', [5, 16, 64])
def test_scanline_streams_equal_the_model(blocks, px, k):
    planes, trajs, lut, sheets = blocks[px, k]
    red = np.array([255, 0, 0], np.uint8)
    # (on a scalar panel: the rgb panel can hold a red of its own)
    assert (sheets[0][:px, :px] == red).all(-1).any() and not (sheets[0][px:2 * px, :px] == red).all(-1).any(), 'present is drawn over, future is not'
    if k == 3:
        assert not (sheets[1][:, :px] == red).all(-1).any(), 'the sample without polylines'
    decoded = {}
    for ftype in (0, 1, 2):
        streams = run_sheets(planes, trajs, ftype, lut)
        for i in range(k):
            img, types = unfilter(streams[i], 3 * px, 5 * px)
            assert np.all(types == ftype)
            bad = np.argwhere((img != sheets[i]).any(-1))
            assert len(bad) == 0, (ftype, i, len(bad), bad[:5].tolist(), img[tuple(bad[0])].tolist(), sheets[i][tuple(bad[0])].tolist())
            assert streams[i] == filter_rows(sheets[i], ftype), (ftype, i)
            decoded.setdefault(i, []).append(img)
    for i in range(k):
        assert np.array_equal(decoded[i][0], decoded[i][1]) and np.array_equal(decoded[i][0], decoded[i][2])


def test_elevation_range_is_a_parameter(blocks):
    planes, trajs, lut, _ = blocks[16, 1]
    rng_ = (0.25, 3.5)
    img, _ = unfilter(run_sheets(planes, trajs, 0, lut, rng_)[0], 48, 80)
    assert np.array_equal(img, model_sheet(planes[0], trajs[0], lut, rng_))


@pytest.mark.parametrize('huffman', ['fixed', 'dynamic'])
def test_whole_png_files(blocks, huffman):
    import torch

    from pca_amd.preview import render_sheets
    planes, trajs, _, _ = blocks[64, 3]
    viridis = model_lut()
    d_planes = torch.from_numpy(planes).cuda()
    for filter in ('none', 'sub', 'up'):
        pngs = render_sheets(d_planes, trajs, filter=filter, huffman=huffman)
        assert len(pngs) == 3
        for i, png in enumerate(pngs):
            pixels, stream = decode_png(png)                       # PIL verify(), one IDAT, zlib's own Adler-32 check
            want = model_sheet(planes[i], trajs[i], viridis)
            assert np.array_equal(pixels, want), (filter, i)
            assert stream == filter_rows(want, {'none': 0, 'sub': 1, 'up': 2}[filter])
            # a block of three equals three blocks of one, byte for byte
            assert render_sheets(d_planes[i:i + 1].contiguous(), trajs[i:i + 1], filter=filter, huffman=huffman) == [png]
    default = render_sheets(d_planes[:1].contiguous(), trajs[:1])
    assert np.array_equal(decode_png(default[0])[0], model_sheet(planes[0], trajs[0], viridis))


def test_one_headline_sized_sheet():
    import torch

    from pca_amd.preview import render_sheets, stream_chunks
    planes, trajs = crafted_block(256, 1)
    assert stream_bytes(256) == 2949888 and stream_chunks(256)[1] == 91
    png = render_sheets(torch.from_numpy(planes).cuda(), trajs)[0]
    pixels, stream = decode_png(png)
    assert len(stream) == 2949888
    assert np.array_equal(pixels, model_sheet(planes[0], trajs[0], model_lut()))


# ---- drop-in: acc.generate_bev -> acc.viz_bev under PCA_VIZ=device
@pytest.fixture(scope='module')
def kitti_tree(tmp_path_factory):
    from fake_kitti import write_tree
    root = str(tmp_path_factory.mktemp('kitti') / 'KITTI-360')
    write_tree(root, first_idx=130, n_frames=14, n_pts=2000)
    return root


def _accumulator(root, monkeypatch):
    from fake_kitti import SEQ

    from datasets.kitti360_utils import get_camera_intrinsics, get_transf_matrices
    from kitti360_sem_pc_accum import Kitti360SemanticPointCloudAccumulator
    from obs_dataloaders.kitti360_obs_dataloader import Kitti360Dataloader
    monkeypatch.setenv('PCA_KITTI_T_FILE', os.path.join(root, 'T_new_prev.npy'))
    h_cam_velo, h_velo_cam = get_transf_matrices(root)
    p_cam_frame = get_camera_intrinsics(root)
    calib = {'h_velo_cam': h_velo_cam, 'p_cam_frame': p_cam_frame, 'p_velo_frame': np.matmul(p_cam_frame, h_velo_cam)}
    acc = Kitti360SemanticPointCloudAccumulator(20., calib, 1e3, 'none.onnx', KITTI_FILTERS, SEM_IDXS, True, dict(BEV_KITTI))
    for observations in Kitti360Dataloader(root, 1, [SEQ], [130], [144]):
        acc.integrate(observations)
    return acc


def _pixels_of(path):
    with open(path, 'rb') as f:
        return decode_png(f.read())[0]


@pytest.mark.parametrize('codec', ['host', 'device'])
def test_viz_bev_writes_the_sheet_of_its_sample(kitti_tree, tmp_path, monkeypatch, codec):
    """Through the kept device planes and through the upload of a plain dict, with the writer's device codec (which lets go
    of its own reference to the planes first) and without, one sample per block and two."""
    from bev_generator.sem_bev import LazyBev
    from pca_amd import writer
    monkeypatch.setenv('PCA_VIZ', 'device')
    monkeypatch.setenv('PCA_WRITER_CODEC', codec)
    monkeypatch.setattr(writer, '_shared', None)                   # a shared writer of this test's own, with this codec
    uploads = []
    real = writer.AsyncBevWriter._preview_source

    def source(bev):
        out = real(bev)
        uploads.append(getattr(bev, '_dev_preview', None) is None)
        return out
    monkeypatch.setattr(writer.AsyncBevWriter, '_preview_source', staticmethod(source))
    acc = _accumulator(kitti_tree, monkeypatch)
    viridis = model_lut()
    try:
        bevs = list(acc.generate_bev(6, 1, gen_future=True)) + list(acc.generate_bev(7, 2, gen_future=True))
        assert len(bevs) == 3 and all(isinstance(b, LazyBev) and b._dev_preview is not None for b in bevs)
        for n, bev in enumerate(bevs):
            acc.write_compressed_pickle(bev, f'bev_{n:03d}.pkl', str(tmp_path))      # first, as the drivers do
        writer.flush_shared()                                      # the device codec has compressed and let go of `_dev`
        assert all(b._dev is None for b in bevs)
        for n, bev in enumerate(bevs):
            acc.viz_bev(bev, str(tmp_path / f'viz_{n:03d}.png'), acc.get_rgb(6), acc.get_semseg(6))
            assert bev._dev_preview is None
        plain = dict(bevs[0])
        acc.viz_bev(plain, str(tmp_path / 'viz_plain.png'))
        assert uploads == [False, False, False, True]
        writer.flush_shared()
        w = writer.shared_writer()
        assert w.codec == codec and w.previews_written == 4 and not w.errors
        assert np.asarray(bevs[0]['road_full']).any() and len(bevs[0]['trajs_full'][0]) > 2, 'an empty sample would prove little'
        for n, bev in enumerate(bevs):
            assert np.array_equal(_pixels_of(str(tmp_path / f'viz_{n:03d}.png')), model_of_bev(dict(bev), viridis)), n
        assert np.array_equal(_pixels_of(str(tmp_path / 'viz_plain.png')), model_of_bev(plain, viridis))
        assert (tmp_path / 'viz_plain.png').read_bytes() == (tmp_path / 'viz_000.png').read_bytes()
        # PCA_ASYNC_WRITE=0: the file is there when viz_bev returns
        monkeypatch.setenv('PCA_ASYNC_WRITE', '0')
        acc.viz_bev(plain, str(tmp_path / 'viz_sync.png'))
        assert (tmp_path / 'viz_sync.png').read_bytes() == (tmp_path / 'viz_plain.png').read_bytes()
    finally:
        writer.shared_writer().close()
        monkeypatch.setattr(writer, '_shared', None)


def test_the_two_samples_of_a_block_share_one_job(kitti_tree, tmp_path, monkeypatch):
    from pca_amd import preview, writer
    monkeypatch.setenv('PCA_VIZ', 'device')
    jobs = []
    real = preview.SheetJob
    monkeypatch.setattr(preview, 'SheetJob', lambda planes, block: jobs.append(int(planes.shape[0])) or real(planes, block))
    acc = _accumulator(kitti_tree, monkeypatch)
    w = writer.AsyncBevWriter(n_threads=2)
    bevs = acc.generate_bev(7, 2, gen_future=True)
    for n, bev in enumerate(bevs):
        w.submit_preview(bev, str(tmp_path / f'viz_{n}.png'))
    w.close()
    assert jobs == [2] and w.previews_written == 2
    assert (tmp_path / 'viz_0.png').stat().st_size > 100 and (tmp_path / 'viz_1.png').stat().st_size > 100


def test_without_pca_viz_the_matplotlib_path_is_taken(kitti_tree, tmp_path, monkeypatch):
    from pca_amd import writer
    monkeypatch.delenv('PCA_VIZ', raising=False)
    called = []
    monkeypatch.setattr(writer.AsyncBevWriter, 'submit_preview', lambda self, *a, **kw: called.append(a))
    acc = _accumulator(kitti_tree, monkeypatch)
    bev = acc.generate_bev(6, 1, gen_future=True)[0]
    assert bev._dev_preview is None, 'no second reference to the device planes unless the device preview is selected'
    acc.viz_bev(bev, str(tmp_path / 'viz.png'), acc.get_rgb(6), acc.get_semseg(6))
    assert called == []
    from PIL import Image
    assert Image.open(str(tmp_path / 'viz.png')).size != (160, 96)          # the figure, not the 5 x 3 sheet of 32-pixel panels
