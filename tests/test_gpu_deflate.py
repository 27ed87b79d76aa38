"""The device codec of the output writer: every piece pca_deflate_chunks makes is inflated with Python's zlib and compared
byte for byte, every CRC word is compared with zlib.crc32, and whole samples written with codec='device' are read back
through the unchanged reader."""
import gzip
import os
import pickle
import zlib

import numpy as np
import pytest

from conftest import PKG  # noqa: F401

pytestmark = pytest.mark.gpu

SLICE = 128                        # bytes a lane tokenises (csrc/pca_deflate.hip)
CHUNK_MAX = 32768
KITTI_FILTERS = [10, 11, 12, 16, 18, 255]
SEM_IDXS = {'road': 0, 'car': 13, 'truck': 14, 'bus': 15, 'motorcycle': 17}
BEV_KITTI = dict(type='sem', view_size=40, pixel_size=32, max_trans_radius=0., zoom_thresh=0., do_warp=False,
                 int_scaler=20., int_sep_scaler=20., int_mid_threshold=0.5, height_filter=None)


def bound(n):
    return (9 * n + 7) // 8 + 16


def run_deflate(src, rows):
    """src: uint8 array; rows: [(offset, length)].  One launch; returns (sizes, crcs, out bytes incl. a guard of 64)."""
    import torch

    from pca_amd import _lib
    from pca_amd.writer import DEFLATE_CHUNK_DTYPE
    ctx = _lib.Context.get()
    n = len(rows)
    table = np.array([(o, l, 0) for o, l in rows], dtype=DEFLATE_CHUNK_DTYPE)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_tab = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    cap = sum(bound(l) for _, l in rows)
    d_out = torch.full((cap + 64, ), 0xaa, dtype=torch.uint8, device='cuda')
    d_sizes = torch.zeros(n, dtype=torch.int32, device='cuda')
    d_crcs = torch.zeros(n, dtype=torch.int32, device='cuda')
    ws_bytes = ctx.lib.pca_deflate_workspace_bytes(n)
    assert ws_bytes > 0
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    ticket = ctx.lib.pca_deflate_chunks(ctx.h, d_src.data_ptr(), d_tab.data_ptr(), n, d_out.data_ptr(), d_sizes.data_ptr(),
                                        d_crcs.data_ptr(), d_ws.data_ptr(), ctx.stream())
    if ticket < 0:
        ctx.check(ticket)
    ctx.check(ctx.lib.pca_host_d2h_wait(ctx.h, ticket))
    return d_sizes.cpu().numpy().view(np.uint32), d_crcs.cpu().numpy().view(np.uint32), d_out.cpu().numpy()


def inflate_piece(piece):
    """A piece on its own: a raw DEFLATE stream without a final block that ends with the sync-flush marker."""
    assert piece[-4:] == b'\x00\x00\xff\xff'
    d = zlib.decompressobj(-15)
    data = d.decompress(piece)
    assert not d.eof and d.unused_data == b'' and d.unconsumed_tail == b''
    return data


def check_launch(src, rows, sizes, crcs, out):
    """Sizes, compaction offsets, contents and CRCs of one launch; returns the pieces."""
    raw = src.tobytes()
    offs = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
    assert np.all(out[offs[-1]:] == 0xaa), 'bytes written behind the last piece'
    pieces = []
    for c, (o, l) in enumerate(rows):
        assert sizes[c] <= bound(l), (c, l, sizes[c])
        piece = out[offs[c]:offs[c + 1]].tobytes()
        assert inflate_piece(piece) == raw[o:o + l], (c, o, l)
        assert crcs[c] == zlib.crc32(raw[o:o + l]), (c, o, l)
        pieces.append(piece)
    # the pieces concatenate bytewise: one stream, closed by an empty final block
    d = zlib.decompressobj(-15)
    whole = d.decompress(b''.join(pieces) + b'\x03\x00')
    assert d.eof and whole == b''.join(raw[o:o + l] for o, l in rows)
    return pieces


class Cases:
    """Named chunks laid back to back into one source buffer (odd lengths make the later ones start at any alignment)."""

    def __init__(self):
        self.parts, self.rows, self.names, self.at = [], [], {}, 0

    def add(self, name, data):
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        self.names[name] = len(self.rows)
        self.rows.append((self.at, len(data)))
        self.parts.append(data)
        self.at += len(data)


@pytest.fixture(scope='module')
def edge_launch():
    """Every edge case of the issue as one table, compressed in ONE launch and checked once."""
    rng = np.random.default_rng(7)
    cs = Cases()

    def noise(n):                  # no two equal neighbours at distance 1 or 2, all below 144: literals only
        return ((np.arange(n) % 3) * 40 + rng.integers(0, 30, n)).astype(np.uint8)
    for n in (1, 2, 3, 255, 257, 258, 259, 32767, 32768):
        cs.add(f'zeros_{n}', np.zeros(n, np.uint8))
        cs.add(f'random_{n}', rng.integers(0, 256, n, dtype=np.uint8))
        cs.add(f'sparse_{n}', rng.integers(0, 256, n, dtype=np.uint8) * (rng.random(n) < 0.03))
    cs.add('empty', b'')
    for pos in [0, CHUNK_MAX - 1] + [b + d for b in range(SLICE, CHUNK_MAX, SLICE) for d in (-1, 0)]:
        one = np.zeros(CHUNK_MAX, np.uint8)
        one[pos] = 1 + pos % 255
        cs.add(f'one_{pos}', one)
    for name, lo, hi in (('run_to_boundary', 100, 2 * SLICE), ('run_over_two', 100, 3 * SLICE + 17), ('run_258', 5, 5 + 258),
                         ('run_259', 5, 5 + 259), ('run_from_boundary', SLICE, SLICE + 40)):
        a = noise(1000)
        a[lo:hi] = 0x55 if a[lo - 1] != 0x55 else 0x56
        cs.add(name, a)
    a = noise(3000)
    a[301:2301] = np.tile(np.array([0x12, 0x34], np.uint8), 1000)            # equal half-words, unequal bytes: distance 2 only
    cs.add('halfwords', a)
    cs.add('fp16_plane', np.where(rng.random(16384) < 0.05, rng.integers(0, 0x3c00, 16384), 0).astype('<u2').view(np.uint8))
    cs.add('nine_bit', rng.integers(144, 256, 5000, dtype=np.uint8))
    cs.add('urandom', os.urandom(CHUNK_MAX))
    cs.add('urandom_odd', os.urandom(4097))
    twin = rng.integers(0, 4, 3001, dtype=np.uint8)
    cs.add('twin_a', twin)
    cs.add('twin_b', twin)
    src = np.concatenate(cs.parts)
    sizes, crcs, out = run_deflate(src, cs.rows)
    pieces = check_launch(src, cs.rows, sizes, crcs, out)
    return cs, src, sizes, pieces


def test_every_edge_chunk_inflates_to_its_bytes(edge_launch):
    cs, src, sizes, pieces = edge_launch
    assert len(pieces) == len(cs.rows) > 500
    # an empty chunk is still a piece: block header, end of block, marker
    assert sizes[cs.names['empty']] == 6
    # 32 KiB of zeros: a literal and a match of 127 in the first slice, one match of 128 (it cites the slice before) in the rest
    assert sizes[cs.names['zeros_32768']] < 600


def test_runs_become_matches(edge_launch):
    cs, src, sizes, pieces = edge_launch
    literal_only = 1000 + 6                                        # 1000 eight-bit literals and the frame
    for name, run in (('run_to_boundary', 156), ('run_over_two', 301), ('run_258', 258), ('run_259', 259), ('run_from_boundary', 40)):
        # a run costs one literal and at most one match (18 bits) per slice it touches, four slices at the most here
        assert sizes[cs.names[name]] <= literal_only - run + 4 * 4 + 1, name
    assert sizes[cs.names['halfwords']] <= 3000 + 6 - 2000 + 2 + 16 * 3, 'half-word runs must be found at distance 2'
    assert sizes[cs.names['fp16_plane']] < 16384


def test_nine_bit_literals_stay_within_the_bound(edge_launch):
    cs, src, sizes, pieces = edge_launch
    for name in ('nine_bit', 'urandom', 'urandom_odd', 'random_32768', 'random_32767', 'random_1'):
        n = cs.rows[cs.names[name]][1]
        assert sizes[cs.names[name]] <= (9 * n + 7) // 8 + 16, name
    n = cs.rows[cs.names['nine_bit']][1]
    assert sizes[cs.names['nine_bit']] >= 9 * n // 8, 'bytes >= 144 cost nine bits each'


def test_a_chunk_never_cites_its_neighbour(edge_launch):
    cs, src, sizes, pieces = edge_launch
    a, b = cs.names['twin_a'], cs.names['twin_b']
    assert cs.rows[b][0] == cs.rows[a][0] + cs.rows[a][1]
    o, l = cs.rows[b]
    assert inflate_piece(pieces[b]) == src[o:o + l].tobytes()       # on its own: no window before it
    assert sizes[a] == sizes[b]
    # a run that continues the previous chunk's last bytes starts with a literal all the same
    o, l = cs.rows[cs.names['zeros_258']]
    assert inflate_piece(pieces[cs.names['zeros_258']]) == bytes(l)


def test_three_hundred_mixed_chunks_in_one_launch():
    rng = np.random.default_rng(11)
    lengths = np.concatenate([rng.integers(1, 400, 150), rng.integers(1, CHUNK_MAX + 1, 140),
                              [CHUNK_MAX] * 5, [1, 2, 3, 4, 5]]).astype(int)
    rng.shuffle(lengths)
    assert len(lengths) == 300
    total = int(lengths.sum())
    src = (rng.integers(0, 256, total, dtype=np.uint8) * (rng.random(total) < 0.02)).astype(np.uint8)
    dense = rng.integers(0, total - 5000)
    src[dense:dense + 5000] = rng.integers(0, 256, 5000, dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    rows = [(int(o), int(l)) for o, l in zip(starts, lengths)]
    sizes, crcs, out = run_deflate(src, rows)
    check_launch(src, rows, sizes, crcs, out)
    # table order is free: the same chunks listed backwards give the same pieces, compacted in that order
    sizes_r, crcs_r, out_r = run_deflate(src, rows[::-1])
    assert np.array_equal(sizes_r, sizes[::-1]) and np.array_equal(crcs_r, crcs[::-1])
    check_launch(src, rows[::-1], sizes_r, crcs_r, out_r)


def _kitti_accumulator(golden, px):
    from PIL import Image

    from kitti360_sem_pc_accum import Kitti360SemanticPointCloudAccumulator
    g = golden('kitti_gtsem')
    calib = {'h_velo_cam': None, 'p_cam_frame': None, 'p_velo_frame': g['P']}
    acc = Kitti360SemanticPointCloudAccumulator(50., calib, 1e3, None, KITTI_FILTERS, SEM_IDXS, True, dict(BEV_KITTI, pixel_size=px))
    queue = list(g['Ts'])
    acc.pose_provider = lambda pc: queue.pop(0)
    dummy = Image.fromarray(np.zeros((64, 96, 3), np.uint8))
    for k in range(4):
        acc.integrate([(dummy, g[f'pc_{k}'], g[f'sem_gt_{k}'])])
    return acc


def _same_dict(a, b):
    assert list(a.keys()) == list(b.keys())
    for key in a:
        if key.startswith('trajs') or key == 'gt_lanes':
            assert len(a[key]) == len(b[key]) and all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), key
        else:
            x, y = np.asarray(a[key]), np.asarray(b[key])
            assert x.dtype == y.dtype == np.float16 and x.shape == y.shape and np.array_equal(x.view(np.uint16), y.view(np.uint16)), key


def _is_device_member(member):
    """pca_host_gzip_assemble writes MTIME 0 and OS 255; gzip.open stamps the time."""
    return member[:4] == b'\x1f\x8b\x08\x00' and member[4:8] == bytes(4) and member[9] == 255


def _write_both_ways(make, tmp_path, touch=()):
    """Samples made while a device-codec writer is open, written by it and by a host-codec writer; `touch`: samples filled
    in (dict(bev)) before anything is submitted.  EVERY sample must have gone through the device codec."""
    from bev_generator.sem_bev import LazyBev
    from pca_amd.writer import AsyncBevWriter
    from sem_pc_accum import SemanticPointCloudAccumulator as Acc
    dev, host = AsyncBevWriter(n_threads=2, codec='device'), AsyncBevWriter(n_threads=2, codec='host')
    samples = make()
    assert all(isinstance(b, LazyBev) for b in samples)
    for k in touch:
        assert len(dict(samples[k])) >= 18
    for k, bev in enumerate(samples):
        dev.submit(bev, f'bev_{k:03d}.pkl', str(tmp_path / 'device'))
        host.submit(bev, f'bev_{k:03d}.pkl', str(tmp_path / 'host'))
    dev.close()
    host.close()
    assert dev.fallbacks == 0 and dev.device_written == len(samples)
    assert host.fallbacks == 0 and host.device_written == 0
    for k, bev in enumerate(samples):
        member = (tmp_path / 'device' / f'bev_{k:03d}.pkl.gz').read_bytes()
        assert _is_device_member(member), k
        assert not _is_device_member((tmp_path / 'host' / f'bev_{k:03d}.pkl.gz').read_bytes())
        a = Acc.read_compressed_pickle(str(tmp_path / 'device' / f'bev_{k:03d}.pkl.gz'))
        b = Acc.read_compressed_pickle(str(tmp_path / 'host' / f'bev_{k:03d}.pkl.gz'))
        assert type(a) is dict and type(b) is dict
        _same_dict(a, b)
        _same_dict(a, dict(bev))
        assert gzip.decompress(member) == pickle.dumps(dict(bev))
    return samples


def _one_and_three(acc):
    return [acc.generate_bev(2, 1, gen_future=True)[0]] + list(acc.generate_bev_many([1, 2, 3], gen_future=True))


def test_samples_written_on_the_device_equal_the_host_files(golden, tmp_path, monkeypatch):
    from pca_amd import writer
    jobs = []
    real = writer._DeviceJob
    monkeypatch.setattr(writer, '_DeviceJob', lambda planes: jobs.append(int(planes.shape[0])) or real(planes))
    acc = _kitti_accumulator(golden, 32)
    samples = _write_both_ways(lambda: _one_and_three(acc), tmp_path)
    assert len(samples) == 4
    assert jobs == [1, 3], 'the three samples of a generate_bev_many share one launch and one copy'
    assert np.asarray(samples[0]['road_full']).any(), 'an empty sample would prove little'


def test_samples_looked_at_before_they_are_written_still_take_the_device_codec(golden, tmp_path):
    """A dict(bev) access fills a sample in and ends the copy it shares with its siblings: the sample and the siblings keep
    their device planes all the same."""
    acc = _kitti_accumulator(golden, 32)
    samples = _write_both_ways(lambda: _one_and_three(acc), tmp_path, touch=(0, 2))
    with pytest.raises(ValueError):
        samples[2]['road_present'][0, 0] = 1.          # the device planes are what gets written: no silent edits of the copy


def test_a_sample_whose_arrays_were_replaced_takes_the_host_codec_and_is_counted(golden, tmp_path):
    from pca_amd.writer import AsyncBevWriter
    from sem_pc_accum import SemanticPointCloudAccumulator as Acc
    acc = _kitti_accumulator(golden, 32)
    w = AsyncBevWriter(n_threads=1, codec='device')
    bev = acc.generate_bev(2, 1, gen_future=True)[0]
    assert len(bev) >= 18                                             # filled in, then one entry replaced
    bev['road_present'] = np.full((32, 32), 0.5, np.float16)
    w.submit(bev, 'bev_000.pkl', str(tmp_path))
    w.submit({'road_present': np.zeros((32, 32), np.float16)}, 'host_dict.pkl', str(tmp_path))       # never on the device: not counted
    w.close()
    assert w.fallbacks == 1 and w.device_written == 0
    assert not _is_device_member((tmp_path / 'bev_000.pkl.gz').read_bytes())
    back = Acc.read_compressed_pickle(str(tmp_path / 'bev_000.pkl.gz'))
    assert np.all(back['road_present'] == np.float16(0.5))
    _same_dict(back, dict(bev))


def test_one_headline_sized_sample(golden, tmp_path):
    acc = _kitti_accumulator(golden, 256)
    _write_both_ways(lambda: [acc.generate_bev(2, 1, gen_future=True)[0]], tmp_path)
    # the device_only form (planes stay on the device) takes the same path
    import torch

    from pca_amd.writer import AsyncBevWriter
    bev = acc.generate_bev(2, 1, gen_future=True)[0]
    parts = [np.asarray(bev[f'{p}_{s}']).reshape(-1, 256, 256) for s in ('present', 'future', 'full')
             for p in ('road', 'intensity', 'rgb', 'dynamic', 'elevation')]
    planes = torch.from_numpy(np.concatenate(parts)).cuda()
    assert tuple(planes.shape) == (21, 256, 256)
    w = AsyncBevWriter(n_threads=1, codec='device')
    w.submit({'planes_f16': planes, 'trajs_present': bev['trajs_present'], 'trajs_future': bev['trajs_future'],
              'trajs_full': bev['trajs_full'], 'frame': 7}, 'only.pkl', str(tmp_path / 'only'))
    w.close()
    assert w.fallbacks == 0 and w.device_written == 1
    assert _is_device_member((tmp_path / 'only' / 'only.pkl.gz').read_bytes())
    back = pickle.loads(gzip.decompress((tmp_path / 'only' / 'only.pkl.gz').read_bytes()))
    assert back['frame'] == 7 and list(back.keys())[:-1] == list(bev.keys())
    _same_dict({k: v for k, v in back.items() if k != 'frame'}, dict(bev))


def test_a_sample_whose_pickle_does_not_match_takes_the_host_codec(golden, tmp_path, monkeypatch):
    from pca_amd import writer
    from sem_pc_accum import SemanticPointCloudAccumulator as Acc
    acc = _kitti_accumulator(golden, 32)
    bev = acc.generate_bev(2, 1, gen_future=True)[0]
    monkeypatch.setattr(writer, 'locate_payloads', lambda blob, stand_in, zeros: None)
    import threading

    from bev_generator.sem_bev import LazyBev
    filled_on, real_fill = [], LazyBev._fill

    def fill(self):
        if self._pending is not None:
            filled_on.append(threading.current_thread())
        return real_fill(self)
    monkeypatch.setattr(LazyBev, '_fill', fill)
    w = writer.AsyncBevWriter(n_threads=1, codec='device')
    w.submit(bev, 'bev_000.pkl', str(tmp_path))
    w.close()
    assert w.fallbacks == 1 and w.device_written == 0
    assert filled_on == [threading.main_thread()], 'the worker hands the sample back: only the submitting thread waits on the device'
    assert not _is_device_member((tmp_path / 'bev_000.pkl.gz').read_bytes())
    _same_dict(Acc.read_compressed_pickle(str(tmp_path / 'bev_000.pkl.gz')), dict(bev))
