"""The host side of the device codec (no GPU): CRC-32 of concatenations, the gzip member spliced from pieces, and where the
plane payloads lie in a sample's pickle."""
import gzip
import os
import pickle
import zlib

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on the path)


def _sync_flush_piece(data, level=6):
    """A byte-aligned piece of a raw DEFLATE stream without a final block, as the device makes them."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)


def test_crc32_combine_matches_zlib():
    from pca_amd.writer import crc32_combine
    rng = np.random.default_rng(0)
    blob = rng.integers(0, 256, (1 << 20) + 4097, dtype=np.uint8).tobytes()
    cuts = [(0, 0), (0, 1), (1, 0), (1, 1), (5, 1 << 20), (1 << 20, 7), (0, 1 << 20), (1 << 20, 0), (1 << 20, 4097)]
    cuts += [tuple(int(v) for v in rng.integers(0, 70000, 2)) for _ in range(40)]
    for la, lb in cuts:
        a, b = blob[:la], blob[la:la + lb]
        assert crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
    # a chain of many pieces cut at random points
    at, crc = 0, 0
    while at < len(blob):
        step = int(rng.integers(0, 40000))
        crc = crc32_combine(crc, zlib.crc32(blob[at:at + step]), len(blob[at:at + step]))
        at += step
    assert crc == zlib.crc32(blob)


def test_gzip_assemble_reads_back(tmp_path):
    from pca_amd.writer import gzip_assemble
    from sem_pc_accum import SemanticPointCloudAccumulator as Acc
    rng = np.random.default_rng(1)
    obj = {'a': rng.integers(0, 4, 300000, dtype=np.uint8), 'b': [np.arange(7.)], 'c': 'text'}
    blob = pickle.dumps(obj)
    assert len(blob) > 200000
    # host piece longer than one stored block, a zero-length host piece, a zero-length device piece, device pieces, a host tail
    cuts = [0, 70000, 70000, 150000, 150000, 150001, 230000, len(blob)]
    kinds = ['host', 'host', 'dev', 'dev', 'dev', 'dev', 'host']
    pieces = []
    for lo, hi, kind in zip(cuts[:-1], cuts[1:], kinds):
        part = blob[lo:hi]
        if kind == 'host':
            pieces.append((np.frombuffer(part, np.uint8), -1, 0))
        else:
            pieces.append((np.frombuffer(_sync_flush_piece(part) if part else b'', np.uint8), len(part), zlib.crc32(part)))
    member = gzip_assemble(pieces).tobytes()
    assert member[:4] == b'\x1f\x8b\x08\x00'
    assert gzip.decompress(member) == blob
    assert int.from_bytes(member[-8:-4], 'little') == zlib.crc32(blob) and int.from_bytes(member[-4:], 'little') == len(blob)
    path = tmp_path / 'sample.gz'
    path.write_bytes(member)
    back = Acc.read_compressed_pickle(str(path))
    assert back.keys() == obj.keys() and np.array_equal(back['a'], obj['a']) and np.array_equal(back['b'][0], obj['b'][0])
    # nothing at all: still a valid, empty member
    assert gzip.decompress(gzip_assemble([]).tobytes()) == b''
    assert gzip.decompress(gzip_assemble([(np.zeros(0, np.uint8), -1, 0)]).tobytes()) == b''
    # a host piece of exactly one and exactly two stored blocks
    for n in (65535, 65536, 131070):
        assert gzip.decompress(gzip_assemble([(np.frombuffer(blob[:n], np.uint8), -1, 0)]).tobytes()) == blob[:n]


def test_gzip_assemble_rejects_small_output():
    import ctypes as C

    from pca_amd import _lib
    lib = _lib.load()
    data = np.arange(100, dtype=np.uint8)
    ptrs = (C.c_void_p * 1)(data.ctypes.data)
    nbytes, raw, crc = np.array([100], np.int64), np.array([-1], np.int64), np.zeros(1, np.uint32)
    out = np.zeros(200, np.uint8)
    args = (1, C.addressof(ptrs), nbytes.ctypes.data, raw.ctypes.data, crc.ctypes.data, out.ctypes.data)
    assert lib.pca_host_gzip_assemble(*args, 124) == -2
    assert lib.pca_host_gzip_assemble(*args, 125) == 125
    assert gzip.decompress(out[:125].tobytes()) == data.tobytes()


def _sample(px, rng, gt_lanes, empty_trajs):
    planes = rng.integers(0, 1 << 16, (21, px, px), dtype=np.uint16).view(np.float16)
    if empty_trajs:
        trajs = ([], [], [])
    else:
        trajs = ([rng.normal(size=(5, 3))], [rng.normal(size=(9, 3)), rng.normal(size=(2, 3))], [rng.normal(size=(14, 3))])
    lanes = [rng.normal(size=(int(n), 3)) for n in rng.integers(2, 30, 6)] if gt_lanes else None
    return planes, trajs, lanes


@pytest.mark.parametrize('px', [8, 32, 256])
@pytest.mark.parametrize('gt_lanes', [False, True])
@pytest.mark.parametrize('empty_trajs', [False, True])
def test_payloads_located_in_the_pickle(px, gt_lanes, empty_trajs):
    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd.writer import locate_payloads, plane_payloads, stand_in_sample
    rng = np.random.default_rng(px)
    planes, trajs, lanes = _sample(px, rng, gt_lanes, empty_trajs)
    real = pickle.dumps(SemBEVGenerator.pack_bev(planes, *trajs, lanes))
    stand_in, zeros = stand_in_sample(px, *trajs, lanes)
    blob = pickle.dumps(stand_in)
    found = locate_payloads(blob, stand_in, zeros)
    assert found is not None and len(found) == 15
    raw = planes.tobytes()
    spliced, at = [], 0
    for (start, nbytes), (off, length) in zip(found, plane_payloads(px)):
        assert nbytes == length
        spliced += [blob[at:start], raw[off:off + length]]
        at = start + nbytes
    spliced.append(blob[at:])
    assert b''.join(spliced) == real


def test_payload_mismatch_is_reported():
    from pca_amd.writer import locate_payloads, stand_in_sample
    rng = np.random.default_rng(3)
    # a byte string the expected arrays do not account for
    stand_in, zeros = stand_in_sample(8, [rng.normal(size=(4, 3))], [], [], None, extra={'note': b'some bytes'})
    assert locate_payloads(pickle.dumps(stand_in), stand_in, zeros) is None
    # the same array twice: pickle memoises the second
    twice = rng.normal(size=(4, 3))
    stand_in, zeros = stand_in_sample(8, [twice], [twice], [])
    assert locate_payloads(pickle.dumps(stand_in), stand_in, zeros) is None
    # a trajectory as large as a plane is told from the planes by its place, not its size
    stand_in, zeros = stand_in_sample(8, [np.ones((16, ))], [], [])
    found = locate_payloads(pickle.dumps(stand_in), stand_in, zeros)
    assert found is not None and len(found) == 15


def test_chunk_table_covers_every_payload():
    from pca_amd.writer import DEFLATE_CHUNK_MAX, chunk_table, plane_payloads
    for px in (8, 32, 200, 256):
        payloads = plane_payloads(px)
        table, first = chunk_table(payloads, base=1000)
        assert first[0] == 0 and first[-1] == len(table) and table['length'].max() <= DEFLATE_CHUNK_MAX and table['length'].min() >= 1
        for k, (off, length) in enumerate(payloads):
            rows = table[first[k]:first[k + 1]]
            assert rows['offset'][0] == 1000 + off and rows['length'].sum() == length
            assert np.array_equal(rows['offset'][1:], rows['offset'][:-1] + rows['length'][:-1])
    assert sum(n for _, n in plane_payloads(256)) == 21 * 256 * 256 * 2


def test_writer_rejects_unknown_codec():
    from pca_amd.writer import AsyncBevWriter
    with pytest.raises(ValueError):
        AsyncBevWriter(n_threads=0, codec='zstd')
    w = AsyncBevWriter(n_threads=1)
    assert w.codec == 'host' and w.fallbacks == 0 and w.device_written == 0
    w.close()


def test_device_codec_is_selected_while_such_a_writer_is_open(monkeypatch):
    from pca_amd import writer
    monkeypatch.delenv('PCA_WRITER_CODEC', raising=False)
    assert not writer.device_codec_selected()
    w = writer.AsyncBevWriter(n_threads=1, codec='device')
    assert writer.device_codec_selected()
    w.close()
    w.close()                                  # closing twice counts once
    assert not writer.device_codec_selected()
    monkeypatch.setenv('PCA_WRITER_CODEC', 'device')
    assert writer.device_codec_selected()


def test_a_close_that_raises_still_deselects_the_device_codec(monkeypatch):
    from pca_amd import writer
    monkeypatch.delenv('PCA_WRITER_CODEC', raising=False)
    w = writer.AsyncBevWriter(n_threads=1, codec='device')

    def broken_flush():
        raise OSError('disk full')
    monkeypatch.setattr(w, 'flush', broken_flush)
    with pytest.raises(OSError):
        w.close()
    assert not writer.device_codec_selected() and not any(t.is_alive() for t in w.threads)
