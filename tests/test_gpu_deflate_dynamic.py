"""The dynamic-Huffman coder of the device codec (pca_deflate_chunks_dyn): every piece is inflated with Python's zlib,
decoded token by token with the small DEFLATE decoder below, and compared with the fixed-Huffman piece pca_deflate_chunks
makes of the same chunk in the same test -- same tokens, never more bytes, and where the block is dynamic a complete code
whose cost is the optimum of the chunk's own histogram whenever the unlimited Huffman tree is no deeper than 15."""
import heapq
import os
import zlib

import numpy as np
import pytest

from conftest import PKG  # noqa: F401

pytestmark = pytest.mark.gpu

SLICE = 128                        # bytes a lane tokenises (csrc/pca_deflate.hip)
CHUNK_MAX = 32768
EOB = 256
KITTI_FILTERS = [10, 11, 12, 16, 18, 255]
SEM_IDXS = {'road': 0, 'car': 13, 'truck': 14, 'bus': 15, 'motorcycle': 17}
BEV_KITTI = dict(type='sem', view_size=40, pixel_size=32, max_trans_radius=0., zoom_thresh=0., do_warp=False,
                 int_scaler=20., int_sep_scaler=20., int_mid_threshold=0.5, height_filter=None)

# ---- a DEFLATE decoder that keeps what zlib throws away: block types, the header's code lengths, the tokens
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


def _table(lens):
    """Canonical code of `lens` as a lookup by the next `mx` bits of the stream (first bit lowest): (symbol, length)."""
    mx = max(lens)
    nxt, code = [0] * (mx + 2), 0
    for l in range(1, mx + 1):
        code = (code + (lens.count(l - 1) if l > 1 else 0)) << 1
        nxt[l] = code
    tab = [None] * (1 << mx)
    for s, l in enumerate(lens):
        if l:
            r = int(format(nxt[l], f'0{l}b')[::-1], 2)
            nxt[l] += 1
            for k in range(r, 1 << mx, 1 << l):
                tab[k] = (s, l)
    return tab, mx


def decode_blocks(data):
    """Every block of the raw DEFLATE stream `data`, up to the final block or the end of the bytes:
    [(btype, literal/length code lengths, distance code lengths, tokens)], a token being a literal (int) or (length,
    distance).  A stored block gives its bytes as literals."""
    pos = buf = cnt = 0
    blocks = []

    def need(n):
        nonlocal pos, buf, cnt
        while cnt < n:
            buf |= (data[pos] if pos < len(data) else 0) << cnt
            pos += 1
            cnt += 8

    def get(n):
        nonlocal buf, cnt
        need(n)
        v = buf & ((1 << n) - 1)
        buf >>= n
        cnt -= n
        return v

    def sym(t):
        nonlocal buf, cnt
        need(t[1])
        s, l = t[0][buf & ((1 << t[1]) - 1)]
        buf >>= l
        cnt -= l
        return s

    final = 0
    while not final and 8 * pos - cnt < 8 * len(data):
        final, btype = get(1), get(2)
        if btype == 0:
            get(cnt % 8)
            n, nn = get(16), get(16)
            assert n ^ nn == 0xffff
            blocks.append((0, None, None, [get(8) for _ in range(n)]))
            continue
        assert btype in (1, 2)
        ll, dl = FIXED_LL, FIXED_D
        if btype == 2:
            hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[CL_ORDER[k]] = get(3)
            clt, lens = _table(cl), []
            while len(lens) < hlit + hdist:
                s = sym(clt)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + get(2))
                else:
                    lens += [0] * (3 + get(3) if s == 17 else 11 + get(7))
            assert len(lens) == hlit + hdist
            ll, dl = lens[:hlit], lens[hlit:]
        llt, dt = _table(ll), _table(dl)
        tokens = []
        while True:
            s = sym(llt)
            if s < EOB:
                tokens.append(s)
            elif s == EOB:
                break
            else:
                length = LEN_BASE[s - 257] + get(LEN_EXTRA[s - 257])
                d = sym(dt)
                tokens.append((length, DIST_BASE[d] + get(DIST_EXTRA[d])))
        blocks.append((btype, list(ll), list(dl), tokens))
    assert 8 * pos - cnt <= 8 * len(data), 'read past the end'
    return blocks


def replay(blocks):
    out = bytearray()
    for _, _, _, tokens in blocks:
        for t in tokens:
            if isinstance(t, tuple):
                for _ in range(t[0]):
                    out.append(out[-t[1]])
            else:
                out.append(t)
    return bytes(out)


def length_symbol(length):
    return 257 + max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 285


def histogram(tokens):
    h = [0] * 286
    for t in tokens:
        h[length_symbol(t[0]) if isinstance(t, tuple) else t] += 1
    h[EOB] += 1
    return h


def huffman_optimum(h):
    """(cost in bits, depth) of the unrestricted Huffman tree of the histogram h, ties to the shallower subtree."""
    heap = [(w, 0) for w in h if w]
    if len(heap) < 2:
        return sum(h), 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (wa, da), (wb, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += wa + wb
        heapq.heappush(heap, (wa + wb, max(da, db) + 1))
    return cost, heap[0][1]


def kraft(lens):
    return sum(2 ** (15 - l) for l in lens if l)        # in units of 2^-15: exact


# ---- the launch helpers of test_gpu_deflate.py, with the entry point as a parameter
def bound(n):
    return (9 * n + 7) // 8 + 16


def run_deflate(src, rows, entry='pca_deflate_chunks_dyn'):
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
    ticket = getattr(ctx.lib, entry)(ctx.h, d_src.data_ptr(), d_tab.data_ptr(), n, d_out.data_ptr(), d_sizes.data_ptr(),
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


FIB = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946]


def depth_limit_chunk():
    """28 655 bytes of 20 values with Fibonacci counts -- with end of block a Huffman tree 20 deep -- laid out so that the
    tokeniser finds no match: always the value with the most left that makes neither four equal bytes in a row nor x y x y x."""
    left = list(FIB)
    out = []
    for _ in range(sum(FIB)):
        for v in sorted(range(20), key=lambda v: -left[v]):
            if not left[v]:
                continue
            if len(out) >= 3 and out[-1] == out[-2] == out[-3] == v:
                continue
            if len(out) >= 4 and out[-4] == out[-2] == v and out[-3] == out[-1]:
                continue
            out.append(v)
            left[v] -= 1
            break
        else:
            raise AssertionError('the greedy layout is stuck')
    return (np.array(out, np.uint8) * 11 + 3).astype(np.uint8)


@pytest.fixture(scope='module')
def launches():
    """Every edge chunk as one table, through ONE launch of each entry point, each checked against zlib and
    decoded once."""
    rng = np.random.default_rng(7)
    cs = Cases()

    def noise(n):                  # no two equal neighbours at distance 1 or 2, all below 144: literals only
        return ((np.arange(n) % 3) * 40 + rng.integers(0, 30, n)).astype(np.uint8)
    for n in (0, 1, 2, 3, 255, 257, 258, 259, 32767, 32768):
        cs.add(f'zeros_{n}', np.zeros(n, np.uint8))
        cs.add(f'random_{n}', rng.integers(0, 256, n, dtype=np.uint8))
        cs.add(f'sparse_{n}', rng.integers(0, 256, n, dtype=np.uint8) * (rng.random(n) < 0.03))
    values = rng.permutation(256)[:12].astype(np.uint8)
    weights = 0.6 ** np.arange(12)
    for n in range(1, 601):        # back to back: every alignment of the chunk's start, every bit phase of its end
        cs.add(f'skewed_{n}', rng.choice(values, n, p=weights / weights.sum()))
    a = noise(4000)
    a[301:2301] = np.tile(np.array([0x12, 0x34], np.uint8), 1000)            # equal half-words, unequal bytes: distance 2 only
    cs.add('halfwords', a)
    a = noise(2000)
    a[100:417] = 0x55 if a[99] != 0x55 else 0x56                            # one byte run: distance 1 only
    cs.add('run', a)
    cs.add('noise', noise(2000))
    cs.add('fp16_plane', np.where(rng.random(16384) < 0.05, rng.integers(0, 0x3c00, 16384), 0).astype('<u2').view(np.uint8))
    cs.add('nine_bit', rng.integers(144, 256, 5000, dtype=np.uint8))
    cs.add('urandom', os.urandom(CHUNK_MAX))
    cs.add('urandom_odd', os.urandom(4097))
    cs.add('depth_limit', depth_limit_chunk())
    twin = rng.integers(0, 4, 3001, dtype=np.uint8)
    cs.add('twin_a', twin)
    cs.add('twin_b', twin)
    src = np.concatenate(cs.parts)
    out = {}
    for entry in ('pca_deflate_chunks', 'pca_deflate_chunks_dyn'):
        sizes, crcs, data = run_deflate(src, cs.rows, entry)
        pieces = check_launch(src, cs.rows, sizes, crcs, data)       # rule 1: zlib, marker, CRC, one stream, guard
        decoded = []
        for piece in pieces:
            blocks = decode_blocks(piece)
            assert len(blocks) == 2 and blocks[1][0] == 0 and blocks[1][3] == [], 'one Huffman block and the empty stored block'
            assert blocks[0][0] == (piece[0] >> 1) & 3
            decoded.append(blocks[0])
        out[entry] = (sizes, pieces, decoded)
    return cs, src, out['pca_deflate_chunks'], out['pca_deflate_chunks_dyn']


def test_no_piece_is_larger_and_every_token_is_the_same(launches):
    cs, src, (size_f, piece_f, dec_f), (size_d, piece_d, dec_d) = launches
    assert len(cs.rows) > 600
    kinds = set()
    for c in range(len(cs.rows)):
        assert dec_f[c][0] == 1, 'pca_deflate_chunks makes fixed blocks only'
        assert size_d[c] <= size_f[c], (c, size_d[c], size_f[c])
        assert dec_d[c][3] == dec_f[c][3], f'chunk {c}: the coder changed, the tokeniser did not'
        assert replay([dec_d[c]]) == src[cs.rows[c][0]:cs.rows[c][0] + cs.rows[c][1]].tobytes()
        if dec_d[c][0] == 1:
            assert piece_d[c] == piece_f[c], f'chunk {c}: a chunk that chose fixed is the fixed piece'
        kinds.add(dec_d[c][0])
    assert kinds == {1, 2}, 'one table with fixed-chosen and dynamic-chosen chunks: compaction offsets of both'
    for name in ('zeros_0', 'random_0', 'sparse_0'):                  # the empty chunk: block header, end of block, marker
        assert size_d[cs.names[name]] == 6 and dec_d[cs.names[name]][0] == 1
    # the crossover lies inside the sweep: short chunks cannot pay a header, long ones of 12 skewed values can
    sweep = [dec_d[cs.names[f'skewed_{n}']][0] for n in range(1, 601)]
    assert sweep[0] == 1 and sweep[-1] == 2
    print(f'first dynamic chunk of the sweep: {1 + sweep.index(2)} bytes')


def test_dynamic_blocks_carry_complete_codes_of_optimal_cost(launches):
    cs, src, fixed, (size_d, piece_d, dec_d) = launches
    names = {c: name for name, c in cs.names.items()}
    optimal, limited = 0, []
    for c, (btype, ll, dl, tokens) in enumerate(dec_d):
        if btype != 2:
            continue
        assert max(ll) <= 15 and max(dl) <= 15
        assert kraft(ll) == 1 << 15 and kraft(dl) == 1 << 15, (names[c], 'both codes must be complete')
        assert len(ll) >= 257 and ll[-1] != 0, 'HLIT ends at the highest used symbol'
        h = histogram(tokens)
        assert all(ll[s] for s in range(286) if h[s]), names[c]
        cost = sum(h[s] * ll[s] for s in range(len(ll)))
        best, depth = huffman_optimum(h)
        if depth <= 15:
            assert cost == best, (names[c], cost, best)
            optimal += 1
        else:
            assert cost >= best
            limited.append((names[c], depth, cost, best))
            print(f'{names[c]}: unrestricted depth {depth}, cost {cost} bits, unrestricted optimum {best} bits, excess {cost - best}')
    assert optimal > 100
    assert [x[0] for x in limited] == ['depth_limit'], limited


def test_named_chunks_take_the_expected_block_type(launches):
    cs, src, fixed, (size_d, piece_d, dec_d) = launches
    for k, name in enumerate(('fp16_plane', 'nine_bit', 'urandom', 'random_32768', 'sparse_32768', 'zeros_32768')):
        btype, ll, dl, tokens = dec_d[cs.names[name]]
        assert btype == 2, name
        if k < 5:
            assert huffman_optimum(histogram(tokens))[1] <= 15, (name, 'the equality of the cost must run on this chunk')
    matches = {name: [t for t in dec_d[cs.names[name]][3] if isinstance(t, tuple)] for name in ('halfwords', 'run', 'noise')}
    assert matches['halfwords'] and {d for _, d in matches['halfwords']} == {2}
    assert matches['run'] and {d for _, d in matches['run']} == {1}
    assert matches['noise'] == [] and dec_d[cs.names['noise']][0] == 2, 'a dynamic block without a single distance'
    assert min(t for t in dec_d[cs.names['nine_bit']][3] if not isinstance(t, tuple)) >= 144
    for name in ('halfwords', 'run', 'noise'):
        assert dec_d[cs.names[name]][2] == [1, 1], 'two distance codes of one bit each, whatever the chunk uses'
    # three symbols out of 281: the literal 0, the match of 128 (and of 127: the same length code) and end of block
    z = dec_d[cs.names['zeros_32768']]
    assert sorted(s for s, l in enumerate(z[1]) if l) == [0, EOB, 280] and size_d[cs.names['zeros_32768']] < 250


def test_the_depth_limit_chunk_exercises_the_limiter(launches):
    cs, src, fixed, (size_d, piece_d, dec_d) = launches
    btype, ll, dl, tokens = dec_d[cs.names['depth_limit']]
    assert len(tokens) == sum(FIB) == 28655 and not any(isinstance(t, tuple) for t in tokens), 'zero matches'
    h = histogram(tokens)
    assert sorted(w for w in h if w) == sorted(FIB + [1])
    assert huffman_optimum(h)[1] == 20
    assert btype == 2 and max(ll) == 15 and kraft(ll) == 1 << 15


def test_identical_chunks_give_identical_pieces(launches):
    cs, src, fixed, (size_d, piece_d, dec_d) = launches
    a, b = cs.names['twin_a'], cs.names['twin_b']
    assert cs.rows[b][0] == cs.rows[a][0] + cs.rows[a][1]
    assert piece_d[a] == piece_d[b] and dec_d[a][0] == 2


# ---- the writer
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


def _one_and_three(acc):
    return [acc.generate_bev(2, 1, gen_future=True)[0]] + list(acc.generate_bev_many([1, 2, 3], gen_future=True))


def test_samples_written_with_dynamic_blocks_equal_the_host_files_and_are_no_larger(golden, tmp_path):
    from pca_amd.writer import AsyncBevWriter
    from sem_pc_accum import SemanticPointCloudAccumulator as Acc
    acc = _kitti_accumulator(golden, 32)
    dyn = AsyncBevWriter(n_threads=2, codec='device', huffman='dynamic')
    fix = AsyncBevWriter(n_threads=2, codec='device', huffman='fixed')
    host = AsyncBevWriter(n_threads=2, codec='host', huffman='dynamic')          # the host codec does not look at it
    samples = _one_and_three(acc)
    for k, bev in enumerate(samples):
        dyn.submit(bev, f'bev_{k:03d}.pkl', str(tmp_path / 'dynamic'))
        host.submit(bev, f'bev_{k:03d}.pkl', str(tmp_path / 'host'))
    again = _one_and_three(acc)        # the same samples once more: a writer lets go of a sample's device planes
    for k, bev in enumerate(again):
        fix.submit(bev, f'bev_{k:03d}.pkl', str(tmp_path / 'fixed'))
    for w in (dyn, fix, host):
        w.close()
    assert dyn.fallbacks == 0 and dyn.device_written == len(samples) == 4
    assert fix.fallbacks == 0 and fix.device_written == 4
    assert host.fallbacks == 0 and host.device_written == 0
    kinds = set()
    for k in range(4):
        name = f'bev_{k:03d}.pkl.gz'
        a, b, f = (Acc.read_compressed_pickle(str(tmp_path / d / name)) for d in ('dynamic', 'host', 'fixed'))
        assert type(a) is dict and type(b) is dict
        _same_dict(a, b)
        _same_dict(a, f)
        _same_dict(a, dict(samples[k]))
        member = (tmp_path / 'dynamic' / name).read_bytes()
        assert member[:4] == b'\x1f\x8b\x08\x00' and member[4:8] == bytes(4) and member[9] == 255, 'spliced, not gzip.open'
        assert len(member) <= len((tmp_path / 'fixed' / name).read_bytes()), k
        kinds |= {blk[0] for blk in decode_blocks(member[10:-8])}
    assert 2 in kinds, 'no dynamic block in any of the files: the writer did not call the dynamic coder'
