"""What the dynamic-Huffman tests lean on, checked without a GPU: the DEFLATE decoder of test_gpu_deflate_dynamic.py is held
to zlib's own streams, its Huffman optimum to a hand-made case, and the writer's `huffman` option to its contract."""
import zlib

import numpy as np
import pytest

from conftest import PKG  # noqa: F401
from test_gpu_deflate_dynamic import (EOB, FIB, decode_blocks, depth_limit_chunk, histogram, huffman_optimum, kraft,
                                      length_symbol, replay)


def _inputs():
    rng = np.random.default_rng(3)
    plane = np.where(rng.random(20000) < 0.05, rng.integers(0, 0x3c00, 20000), 0).astype('<u2').tobytes()
    text = b''.join(bytes(rng.choice(np.frombuffer(b'abcdefgh ', np.uint8), rng.integers(3, 9))) for _ in range(6000))
    return {'plane': plane, 'text': text, 'random': rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), 'empty': b'',
            'long_runs': bytes(70000) + b'\x01' * 300 + text[:1000]}


@pytest.mark.parametrize('strategy', ['level1', 'level9', 'fixed'])
def test_the_decoder_replays_zlib_streams(strategy):
    level, strat = {'level1': (1, zlib.Z_DEFAULT_STRATEGY), 'level9': (9, zlib.Z_DEFAULT_STRATEGY), 'fixed': (9, zlib.Z_FIXED)}[strategy]
    kinds = set()
    for name, raw in _inputs().items():
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strat)
        stream = c.compress(raw) + c.flush()
        blocks = decode_blocks(stream)
        assert replay(blocks) == raw, name
        for btype, ll, dl, tokens in blocks:
            kinds.add(btype)
            if btype == 2:
                assert kraft(ll) == 1 << 15 and max(ll) <= 15 and ll[EOB] > 0, name
                assert all(ll[s] for s, n in enumerate(histogram(tokens)) if n), name
        # a sync flush in the middle: the shape of the device pieces (no final block, byte-aligned, an empty stored block)
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strat)
        piece = c.compress(raw) + c.flush(zlib.Z_SYNC_FLUSH)
        assert piece[-4:] == b'\x00\x00\xff\xff'
        blocks = decode_blocks(piece)
        assert replay(blocks) == raw and blocks[-1] == (0, None, None, [])
    assert 1 in kinds and 2 not in kinds if strategy == 'fixed' else 2 in kinds       # (random bytes are stored by either)


def test_length_symbols_and_the_huffman_optimum():
    assert [length_symbol(n) for n in (3, 10, 11, 12, 13, 127, 128, 130, 131, 257, 258)] == [257, 264, 265, 265, 266, 280, 280, 280, 281, 284, 285]
    assert huffman_optimum([5, 9, 12, 13, 16, 45]) == (224, 4)                  # the textbook case
    assert huffman_optimum([1, 1, 1, 1]) == (8, 2), 'ties go to the shallower subtree'
    assert huffman_optimum(FIB + [1])[1] == 20
    chunk = depth_limit_chunk()
    assert len(chunk) == 28655 and sorted(np.bincount(chunk)[np.bincount(chunk) > 0].tolist()) == FIB
    four = (chunk[3:] == chunk[2:-1]) & (chunk[2:-1] == chunk[1:-2]) & (chunk[1:-2] == chunk[:-3])
    five = (chunk[4:] == chunk[2:-2]) & (chunk[2:-2] == chunk[:-4]) & (chunk[3:-1] == chunk[1:-3])
    assert not four.any() and not five.any(), 'nothing for a tokeniser that looks at distances 1 and 2'


def test_the_writer_takes_fixed_or_dynamic_and_nothing_else():
    from pca_amd.writer import AsyncBevWriter
    for codec in ('host', 'device'):
        with pytest.raises(ValueError, match='huffman'):
            AsyncBevWriter(n_threads=1, codec=codec, huffman='adaptive')
    for kw, want in (({}, 'fixed'), ({'codec': 'device'}, 'fixed'), ({'codec': 'device', 'huffman': 'dynamic'}, 'dynamic'),
                     ({'codec': 'host', 'huffman': 'dynamic'}, 'dynamic')):
        w = AsyncBevWriter(n_threads=1, **kw)
        try:
            assert w.huffman == want and w.codec == kw.get('codec', 'host')
        finally:
            w.close()


def test_the_shared_writer_reads_the_environment(monkeypatch):
    from pca_amd import writer
    for env, want in ((None, 'fixed'), ('fixed', 'fixed'), ('dynamic', 'dynamic')):
        monkeypatch.setattr(writer, '_shared', None)
        if env is None:
            monkeypatch.delenv('PCA_WRITER_HUFFMAN', raising=False)
        else:
            monkeypatch.setenv('PCA_WRITER_HUFFMAN', env)
        w = writer.shared_writer()
        try:
            assert w.huffman == want and w is writer.shared_writer()
        finally:
            w.close()
    monkeypatch.setattr(writer, '_shared', None)
    monkeypatch.setenv('PCA_WRITER_HUFFMAN', 'static')
    with pytest.raises(ValueError):
        writer.shared_writer()
    assert writer._shared is None
