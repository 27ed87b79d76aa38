"""The host side of the device preview sheets (no GPU): Adler-32 of concatenations, the PNG container fed with pieces made
by host zlib in the shape the device makes them, the host conversion of polylines, and the committed colour table."""
import ctypes as C
import zlib

import numpy as np
import pytest
from conftest import PKG  # noqa: F401
from preview_common import decode_png, filter_rows, model_lut, png_chunks, unfilter

BASE = 65521


def test_adler32_combine_equals_zlib_on_splits():
    from pca_amd.preview import adler32_combine
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 3 * BASE + 77, dtype=np.uint8).tobytes()
    data_ff = b'\xff' * (2 * BASE + 5)                              # the largest sums
    lengths = [0, 1, 2, 5551, 5552, 5553, 32768, BASE - 1, BASE, BASE + 1, 2 * BASE - 1, 2 * BASE, 2 * BASE + 1]
    for buf in (data, data_ff):
        for len_b in lengths:
            for len_a in (0, 1, 4097, BASE, len(buf) - len_b):
                if len_a + len_b > len(buf):
                    continue
                a, b = buf[:len_a], buf[len_a:len_a + len_b]
                assert adler32_combine(zlib.adler32(a), zlib.adler32(b), len_b) == zlib.adler32(a + b), (len_a, len_b)
    for _ in range(200):                                           # random splits, folded left to right as the writer does
        cuts = np.sort(rng.integers(0, len(data), 4))
        parts = [data[i:j] for i, j in zip([0, *cuts], [*cuts, len(data)])]
        adler = 1
        for p in parts:
            adler = adler32_combine(adler, zlib.adler32(p), len(p))
        assert adler == zlib.adler32(data)
    assert adler32_combine(1, 1, 0) == 1 and adler32_combine(zlib.adler32(b'abc'), 1, -1) == 0


def sync_flush_pieces(stream, chunk=32768):
    """Raw deflate pieces of the stream's chunks, each ended by a sync flush: what the device makes, by host zlib."""
    out = []
    for at in range(0, len(stream), chunk):
        d = zlib.compressobj(1, zlib.DEFLATED, -15)
        out.append(d.compress(stream[at:at + chunk]) + d.flush(zlib.Z_SYNC_FLUSH))
        assert out[-1][-4:] == b'\x00\x00\xff\xff'
    return out


def _picture():
    rng = np.random.default_rng(2)
    px = 64
    img = rng.integers(0, 256, (3 * px, 5 * px, 3), dtype=np.uint8)
    img[40:120, 30:200] = (12, 200, 77)                            # flat areas, where the filters differ most
    img[:, 100] = (255, 0, 0)
    return img


@pytest.mark.parametrize('ftype', [0, 1, 2])
def test_png_assemble_decodes_to_the_pixels(ftype):
    from pca_amd.preview import adler32_combine, png_assemble
    img = _picture()
    stream = filter_rows(img, ftype)
    assert len(stream) == (1 + 15 * 64) * 3 * 64 == 184512
    back, types = unfilter(stream, *img.shape[:2])
    assert np.array_equal(back, img) and np.all(types == ftype)     # the test's own filters invert each other
    pieces = sync_flush_pieces(stream)
    assert len(pieces) == 6
    adler = 1
    for at in range(0, len(stream), 32768):
        adler = adler32_combine(adler, zlib.adler32(stream[at:at + 32768]), len(stream[at:at + 32768]))
    png = png_assemble(img.shape[1], img.shape[0], [np.frombuffer(p, np.uint8) for p in pieces], adler)
    pixels, inflated = decode_png(png)                             # PIL verify(), chunk CRCs, IHDR fields, zlib.decompress
    assert inflated == stream
    assert np.array_equal(pixels, img)
    kinds = png_chunks(png)
    assert kinds[1][1][-6:-4] == b'\x03\x00' and kinds[1][1][-4:] == adler.to_bytes(4, 'big') and kinds[2] == (b'IEND', b'')
    # one piece or many, and zero-length pieces between them: the same file
    joined = png_assemble(img.shape[1], img.shape[0], [np.frombuffer(b''.join(pieces), np.uint8)], adler)
    holes = png_assemble(img.shape[1], img.shape[0], [np.zeros(0, np.uint8)] + [np.frombuffer(p, np.uint8) for p in pieces] +
                         [np.zeros(0, np.uint8)], adler)
    assert joined == png and holes == png


def test_png_assemble_reports_bad_arguments_and_capacity():
    from pca_amd import _lib
    lib = _lib.load()
    piece = np.frombuffer(sync_flush_pieces(b'\x00' * 16)[0], np.uint8)
    ptrs = (C.c_void_p * 1)(piece.ctypes.data)
    nbytes = np.array([piece.size], dtype=np.int64)
    need = 65 + piece.size
    out = np.zeros(need + 8, dtype=np.uint8)

    def call(width=5, height=1, n=1, p=C.addressof(ptrs), nb=nbytes.ctypes.data, o=out.ctypes.data, cap=need):
        return lib.pca_host_png_assemble(width, height, n, p, nb, zlib.adler32(b'\x00' * 16), o, cap)
    assert call() == need and not out[need:].any()
    assert call(cap=need - 1) == -2 and call(cap=0) == -2
    assert call(n=0, p=None, nb=None, cap=64) == -2 and call(n=0, p=None, nb=None, cap=65) == 65
    assert call(width=0) == -1 and call(height=0) == -1 and call(n=-1) == -1 and call(o=None) == -1 and call(cap=-1) == -1
    assert call(p=None) == -1 and call(nb=None) == -1
    bad = np.array([-1], dtype=np.int64)
    assert call(nb=bad.ctypes.data) == -1
    null = (C.c_void_p * 1)(None)
    assert call(p=C.addressof(null)) == -1


def test_stream_sizes():
    from pca_amd import _lib
    from pca_amd.preview import stream_bytes, stream_chunks
    lib = _lib.load()
    for px in (1, 5, 64, 256, 4096):
        assert lib.pca_preview_stream_bytes(px) == stream_bytes(px) == (1 + 15 * px) * 3 * px
        assert lib.pca_preview_workspace_bytes(3, px) >= 3 * 3 * ((px * px + 31) // 32) * 4
    assert lib.pca_preview_stream_bytes(0) == -1 and lib.pca_preview_stream_bytes(4097) == -1
    assert lib.pca_preview_workspace_bytes(-1, 5) == -1 and lib.pca_preview_workspace_bytes(1, 0) == -1
    table, per = stream_chunks(64, 2)
    assert per == 6 and len(table) == 12 and table['length'].max() == 32768 and table['length'][5] == 184512 - 5 * 32768
    assert table['offset'][6] == 184512 and int(table['length'][:6].sum()) == 184512
    assert stream_chunks(256)[1] == 91


def test_sheet_polylines():
    from pca_amd.preview import polyline_tables, sheet_polylines
    trajs = [np.array([[1.5, 2.25], [3.75, -0.5]]),                 # (N, 2), fractional and negative: floor
             np.array([[-1.5, -0.25, 9.], [4., 5., 9.]]),           # (N, 3): the third column is not looked at
             np.zeros((0, 2)), np.zeros((0, 3)), [],                # empty: nothing
             np.array([[1., 2.], [np.nan, 3.]]), np.array([[np.inf, 0.]]), np.array([[0., -np.inf, 1.]]),      # non-finite: dropped
             np.array([[7., 7.]]),                                  # one vertex
             np.array([[1e12, -1e12]]),                             # beyond int32: clamped far outside any grid
             [[2, 3], [4, 5]]]                                      # a plain list
    got = sheet_polylines(trajs, 32)
    want = [[[1, 2], [3, -1]], [[-2, -1], [4, 5]], [[7, 7]], [[1 << 29, -(1 << 29)]], [[2, 3], [4, 5]]]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and g.shape == (len(w), 2) and g.tolist() == w
    assert sheet_polylines([], 32) == [] and sheet_polylines(None, 32) == []
    with pytest.raises(ValueError):
        sheet_polylines([], 0)
    with pytest.raises(ValueError):
        sheet_polylines([], 4097)
    verts, rows = polyline_tables([(trajs, [], [trajs[8]]), ([], [], []), ([], [trajs[0]], [])], 32)
    assert verts.dtype == np.int32 and verts.shape == (11, 2)
    assert rows.tolist() == [(0, 0, 0, 2), (0, 0, 2, 2), (0, 0, 4, 1), (0, 0, 5, 1), (0, 0, 6, 2), (0, 2, 8, 1), (2, 1, 9, 2)]
    verts, rows = polyline_tables([([], [], [])], 32)
    assert verts.shape == (0, 2) and len(rows) == 0


def test_panel_ranges_are_float32_computed_once():
    from pca_amd.preview import ELEV_RANGE, panel_ranges
    r = panel_ranges()
    assert r.dtype == np.float32 and r.shape == (4, 2) and ELEV_RANGE == (-0.5, 2.0)
    assert r[:3].tolist() == [[0., 256.]] * 3
    assert r[3, 0] == np.float32(-0.5) and r[3, 1] == np.float32(256) / (np.float32(2.0) - np.float32(-0.5))
    with pytest.raises(ValueError):
        panel_ranges((1., 1.))


def test_committed_lut_is_viridis():
    pytest.importorskip('matplotlib')
    from pca_amd.preview import VIRIDIS
    assert VIRIDIS.dtype == np.uint8 and VIRIDIS.shape == (256, 3)
    assert np.array_equal(VIRIDIS, model_lut())
    assert VIRIDIS[0].tolist() == [68, 1, 84] and VIRIDIS[255].tolist() == [253, 231, 37]


def test_planes_of_a_dict_are_pack_bev_inverted():
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd.preview import planes_of
    planes = np.random.default_rng(4).random((21, 6, 6)).astype(np.float16)
    bev = SemBEVGenerator.pack_bev(planes, [], [], [])
    assert np.array_equal(planes_of(bev), planes)
