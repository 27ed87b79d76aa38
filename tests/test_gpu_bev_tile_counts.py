"""GPU parity of the BEV tile kernel where its slot and round accounting can go wrong.  bev_tile_cells reads a tile of n
records coalesced, record u * 256 + t in slot u of thread t, in rounds of C_SLOT_Q = 4 slots, and skips the rounds no record
falls into: the cases put exactly n records into one tile for every n next to a slot boundary (a multiple of 256) or a round
boundary (a multiple of 1024), up to 2560, the last count the light kernel keeps, and 2561, the first the heavy path takes.

Points sit on cell centres of an axis-aligned raster with view = px (cells of 1.0: the coordinates are exact binary
fractions), so a tile's count is exact by construction; every case checks its counts on the oracle's own cell ids before it
compares.  Same bar as tests/test_gpu_kernels.py: all 21 planes bit-equal to the oracle's, intensity within 1e-12."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_kernels import DYNOBJ, assert_planes_match, dev_store, run_dev_bev

pytestmark = pytest.mark.gpu

INTS = (20., 20., 0.5)
Q = 4                                   # csrc/pca_bev.hip C_SLOT_Q
THREADS = 256                           # C_THREADS
LIGHT_MAX = 2560                        # HEAVY_MIN_DEFAULT = CONTIG_MIN
PX = 32
TARGET = (1, 2)                         # (tile row, tile column) of the tile under test

# every slot boundary up to LIGHT_MAX from both sides -- the round boundaries (multiples of Q * THREADS) are among them --,
# the empty tile, a single record, and the hand-over to the heavy path
COUNTS = sorted({0, 1, LIGHT_MAX + 1} | {k * THREADS + d for k in range(1, LIGHT_MAX // THREADS + 1) for d in (-1, 0, 1)
                                         if k * THREADS + d <= LIGHT_MAX})
assert {255, 256, 257, Q * 256 - 1, Q * 256, Q * 256 + 1, 2047, 2048, 2049, 2559, 2560, 2561} <= set(COUNTS)
assert all(k * Q * THREADS + d in COUNTS for k in range(1, LIGHT_MAX // (Q * THREADS) + 1) for d in (-1, 0, 1))


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


# ---------------------------------------------------------------------------------------------------------- inputs
def rows_of(rng, cells, px, genuine_f64=False):
    """cells: {(row, col): (n_present, n_future)} -> (rows_p, rows_f), (M,10) each: the points of a cell at its centre."""
    out = []
    for s in (0, 1):
        rc = np.array([k for k, v in cells.items() for _ in range(v[s])], dtype=np.int64).reshape(-1, 2)
        m = rc.shape[0]
        rows = np.zeros((m, 10))
        rows[:, 0] = rc[:, 1] + 0.5 - 0.5 * px                    # col = floor(x / view * px + px / 2), view = px
        rows[:, 1] = (px - 1 - rc[:, 0]) + 0.5 - 0.5 * px         # row = px - 1 - floor(y / view * px + px / 2)
        rows[:, 2] = rng.integers(-64, 128, m) / 32.
        rows[:, 3] = rng.uniform(0, 1, m) if genuine_f64 else rng.integers(0, 256, m) / 256.
        rows[:, 4:7] = rng.integers(0, 256, (m, 3))
        rows[:, 7] = rng.choice([0, 1, 13, 17], m)
        out.append(rows[rng.permutation(m)])
    return out


def spread(rng, n, tile, only_cells=None):
    """n records over the cells of a tile (all 64, or the listed ones), present or future by the toss of a coin."""
    idx = np.arange(64) if only_cells is None else np.asarray(only_cells)
    per = rng.multinomial(n, np.full(len(idx), 1. / len(idx)))
    pres = rng.binomial(per, 0.5)
    return {(8 * tile[0] + int(i) // 8, 8 * tile[1] + int(i) % 8): (int(p), int(k - p)) for i, k, p in zip(idx, per, pres) if k}


def sparse_tiles(rng, tx, skip, lo=1, hi=40):
    """Every other tile of a tx x tx grid with lo..hi - 1 records in a few of its cells, the tiles between them empty."""
    cells = {}
    for t in range(tx * tx):
        tile = (t // tx, t % tx)
        if tile in skip or (t & 1) == 0:
            continue
        cells.update(spread(rng, int(rng.integers(lo, hi)), tile, rng.choice(64, 5, replace=False)))
    return cells


def oracle_bev(orc, rows_p, rows_f, px, i64=False):
    """The oracle's planes and cell ids of the axis-aligned raster with view = px (read-only)."""
    from pca_amd import host_logic as hl
    rows = np.concatenate([rows_p, rows_f])
    prm = orc.make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.), 0., 0., float(px), px, None, *INTS, 0, DYNOBJ, False)
    ref = orc.bev(orc.Store.from_rows(rows), rows_p.shape[0], prm, intensity64=rows[:, 3] if i64 else None, want_cells=True)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def tile_counts(ref, px):
    """Records per tile, [tile rows, tile columns], from the oracle's cell ids (a culled point has -1)."""
    tx = (px + 7) // 8
    c = ref['cells']
    assert (c >= 0).all()                                          # every point of a case is meant to land in the raster
    return np.bincount((c // px // 8) * tx + (c % px) // 8, minlength=tx * tx).reshape(tx, tx)


def cell_set_counts(ref, n_present, px):
    c = ref['cells']
    return np.bincount(c[:n_present], minlength=px * px), np.bincount(c[n_present:], minlength=px * px)


def check_single(T, orc, rows_p, rows_f, px, want, name, i64=False):
    """want: {tile: count}; every other tile holds less than one slot's worth of records."""
    ref = oracle_bev(orc, rows_p, rows_f, px, i64)
    got = tile_counts(ref, px)
    for tile, n in want.items():
        assert got[tile] == n, (name, tile)
    rest = got.copy()
    for tile in want:
        rest[tile] = 0
    assert rest.max() < THREADS and (rest == 0).any() and (rest > 0).any(), name
    p16, p64, used = run_dev_bev(T, rows_p, rows_f, float(px), px, None, INTS, False, 0.0)
    assert used == i64
    assert_planes_match(p16, p64, ref, name)
    return ref


# ---------------------------------------------------------------------------------------------------------- 1: counts
@pytest.mark.parametrize('n', COUNTS)
def test_one_tile_of_exactly_n_records(T, orc, n):
    """One tile of exactly n records among sparse and empty ones.  2561 is the heavy path's (the first dense tile of a fresh
    context: the light kernel's last workgroup works it off)."""
    rng = np.random.default_rng(1000 + n)
    cells = sparse_tiles(rng, PX // 8, {TARGET})
    cells.update(spread(rng, n, TARGET))
    rows_p, rows_f = rows_of(rng, cells, PX)
    check_single(T, orc, rows_p, rows_f, PX, {TARGET: n}, f'n={n}')


# ---------------------------------------------------------------------------------------------------------- 2: populations
def populations(total):
    """Cells 0..: 1, 32, 33, 64, 65 values (half-wave and full-wave transpose, the histogram path), each all present, all
    future and mixed; then cells of 100 until `total` is reached; the cells after them stay empty."""
    pop = [(1, 0), (0, 1), (1, 1), (32, 0), (0, 32), (16, 16), (33, 0), (0, 33), (16, 17), (64, 0), (0, 64), (32, 32), (63, 1),
           (65, 0), (0, 65), (64, 1), (1, 64), (40, 30)]
    left = total - sum(p + f for p, f in pop)
    while left > 0:
        k = min(left, 100)
        pop.append((k - k // 3, k // 3))
        left -= k
    assert left == 0 and len(pop) <= 64
    return pop


def dead_select_rounds():
    """1024 records in eight cells: a wave's 16 cells x 18 targets make five select rounds of 64 lanes; with cells 0..3 (one
    per wave) small, 60..63 above 64 values and the rest empty, rounds 1..3 have no live target in any wave, round 0 has lanes
    whose set is empty, and round 4 sees only cells that are the histogram path's -- but for cell 63, small again."""
    pop = {0: (1, 0), 1: (0, 1), 2: (32, 1), 3: (64, 0), 60: (300, 0), 61: (0, 300), 62: (131, 130), 63: (0, 0)}
    pop[63] = (40, 1024 - 40 - sum(p + f for p, f in pop.values()))
    assert 0 < sum(pop[63]) <= 64 and sum(p + f for p, f in pop.values()) == 1024
    return pop


@pytest.mark.parametrize('case', ['mixed_1024', 'mixed_2048', 'dead_rounds_1024'])
def test_cell_populations_on_a_round_boundary(T, orc, case):
    rng = np.random.default_rng(7)
    total = int(case.rsplit('_', 1)[1])
    assert total % (Q * THREADS) == 0
    pop = dict(enumerate(populations(total))) if case.startswith('mixed') else dead_select_rounds()
    cells = sparse_tiles(rng, PX // 8, {TARGET})
    want_p, want_f = np.zeros(PX * PX, int), np.zeros(PX * PX, int)
    for i, (p, f) in pop.items():
        r, c = 8 * TARGET[0] + i // 8, 8 * TARGET[1] + i % 8
        cells[(r, c)] = (p, f)
        want_p[r * PX + c], want_f[r * PX + c] = p, f
    rows_p, rows_f = rows_of(rng, cells, PX)
    ref = check_single(T, orc, rows_p, rows_f, PX, {TARGET: total}, case)
    got_p, got_f = cell_set_counts(ref, rows_p.shape[0], PX)
    rr, cc = np.divmod(np.arange(PX * PX), PX)
    inside = (rr // 8 == TARGET[0]) & (cc // 8 == TARGET[1])
    assert np.array_equal(got_p[inside], want_p[inside]) and np.array_equal(got_f[inside], want_f[inside])


# ---------------------------------------------------------------------------------------------------------- 3: several pieces
def test_boundary_tile_fed_by_several_level1_pieces(T, orc, monkeypatch):
    """Four frames, level 1 in pieces of 1024 points (PCA_BEV_CHUNK): the tile of exactly 1024 records and the one of 1025
    are fed by every piece, the tiles around them hold a slot or two."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    monkeypatch.setenv('PCA_BEV_CHUNK', '1024')
    rng = np.random.default_rng(11)
    other = (2, 1)
    cells = {}
    for t in range(16):
        if (t // 4, t % 4) not in (TARGET, other):
            cells.update(spread(rng, int(rng.integers(100, 500)), (t // 4, t % 4)))
    cells.update(spread(rng, Q * THREADS, TARGET))
    cells.update(spread(rng, Q * THREADS + 1, other))
    rows_p, rows_f = rows_of(rng, cells, PX)
    ref = oracle_bev(orc, rows_p, rows_f, PX)
    got = tile_counts(ref, PX)
    assert got[TARGET] == Q * THREADS and got[other] == Q * THREADS + 1
    frames = [rows_p[:rows_p.shape[0] // 2], rows_p[rows_p.shape[0] // 2:], rows_f[:rows_f.shape[0] // 3], rows_f[rows_f.shape[0] // 3:]]
    st = dev_store(capacity=rows_p.shape[0] + rows_f.shape[0], max_frames=4)
    assert st.load_rows(frames) is None
    prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.), 0., 0., float(PX), PX, None, *INTS, 0, DYNOBJ, False)
    p16, p64 = st.bev(2, prm, want_f64=True)
    st.check_status()
    lvl = (C.c_int * 4)()
    assert st.ctx.lib.pca_debug_bev_level1(st.ctx.h, lvl) == 0
    G = lvl[0]
    assert G > 1
    # a piece is a contiguous stretch of the window: the tile's records lie in more than one of G equal stretches
    n = ref['cells'].shape[0]
    for tile in (TARGET, other):
        at = np.flatnonzero((ref['cells'] // PX // 8 == tile[0]) & (ref['cells'] % PX // 8 == tile[1]))
        assert len(set(at * G // n)) > 1
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), ref, 'several pieces')


# ---------------------------------------------------------------------------------------------------------- 4: shared bodies
def test_two_samples_of_bev_many(T, orc):
    """pca_bev_generate_many (bev_tile_cells_many): two samples in one launch, a tile of exactly 1024 records in one and of
    1025 in the other.  The launch returns fp16 planes: bit-equal to the oracle's, intensity within one fp16 ulp."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    rng = np.random.default_rng(13)
    frames, refs = [], []
    for n, tile in ((Q * THREADS, TARGET), (Q * THREADS + 1, (3, 0))):
        cells = sparse_tiles(rng, PX // 8, {tile})
        cells.update(spread(rng, n, tile))
        rows_p, rows_f = rows_of(rng, cells, PX)
        ref = oracle_bev(orc, rows_p, rows_f, PX)
        assert tile_counts(ref, PX)[tile] == n
        frames += [rows_p, rows_f]
        refs.append(ref)
    st = dev_store(capacity=sum(f.shape[0] for f in frames), max_frames=4)
    assert st.load_rows(frames) is None
    prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.), 0., 0., float(PX), PX, None, *INTS, 0, DYNOBJ, False)
    out = T.empty((2, 21, PX, PX), dtype=T.float16, device='cuda')
    st.bev_many([(1, prm, 0, 2), (3, prm, 2, 4)], out)
    st.check_status()
    out = out.cpu().numpy()
    for k, ref in enumerate(refs):
        for s in range(3):
            for p in range(7):
                a, b = out[k][7 * s + p].view(np.uint16), ref['f16'][7 * s + p].view(np.uint16)
                if p == 1:
                    d = np.abs(a.astype(int) - b.astype(int))
                    assert d.max() <= 1 and (d != 0).mean() < 1e-3, (k, s)
                else:
                    assert np.array_equal(a, b), (k, s, p)


def test_banded_grid_tiles_on_a_round_boundary(T, orc):
    """px = 1025, the first banded size (bev_tile_cells_band; bands of 127 tile rows): a tile of exactly 1025 records in band 0
    and one of exactly 1024 in the first tile row of band 1, two thousand points on scattered cells around them."""
    px = 1025
    rng = np.random.default_rng(17)
    tiles = {(60, 7): Q * THREADS + 1, (127, 5): Q * THREADS}
    cells = {}
    for r, c in rng.integers(0, px, (2000, 2)):
        if (r // 8, c // 8) not in tiles:
            p, f = cells.get((int(r), int(c)), (0, 0))
            cells[(int(r), int(c))] = (p + 1, f) if rng.random() < 0.5 else (p, f + 1)
    for tile, n in tiles.items():
        cells.update(spread(rng, n, tile))
    rows_p, rows_f = rows_of(rng, cells, px)
    check_single(T, orc, rows_p, rows_f, px, tiles, 'banded 1025')


def test_f64_intensity_on_a_round_boundary(T, orc):
    """The f64-intensity instantiation (24-byte records, loads under the bounds check): 1024 and 1025 records."""
    rng = np.random.default_rng(19)
    other = (3, 3)
    cells = sparse_tiles(rng, PX // 8, {TARGET, other})
    cells.update(spread(rng, Q * THREADS, TARGET))
    cells.update(spread(rng, Q * THREADS + 1, other))
    rows_p, rows_f = rows_of(rng, cells, PX, genuine_f64=True)
    check_single(T, orc, rows_p, rows_f, PX, {TARGET: Q * THREADS, other: Q * THREADS + 1}, 'f64 intensity', i64=True)
