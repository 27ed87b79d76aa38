"""Level 1's third residence: the points of a piece beyond the 12 288 of the registers wait in LDS (up to 4 096 more, key and
transformed z) instead of taking the memory path.  One level-1 workgroup (PCA_BEV_G=1) makes the window the piece, so small
windows reach every size at which the code takes another path:

    12 288  registers only            12 289  one parked point          13 300  a typical overflow
    16 384  the parked block full     16 385  one point on the memory path behind it

Every case is checked against the ORACLE (planes against orc.bev of the oracle's own transformed rows, stored coordinates
against the oracle's K2) and leaves a digest of its 21 planes (f16 and f64) and of the stored x, y, z.  PCA_BEV_LDS_P is read
once per process, so the switched-off runs are child processes: they run the same self-checking cases and must arrive at the
same digests, byte for byte (and so does PCA_BEV_SPLIT=2, the only setting under which pieces ordered by halves of tiles and
parked points meet: with the default the kernels order by halves only while every piece fits the registers)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cull_chain_common as cc
from test_gpu_cull_chain import DYNOBJ, INTS, P_CULL, H_CULL, W_CULL, VIEW, level1, loaded_store, owe, owed_frames
from test_gpu_dropin import KITTI_FILTERS
from test_gpu_kernels import _tilting_transform, assert_planes_match, cu

pytestmark = pytest.mark.gpu

REG, PARK = 12288, 4096                                     # BIN_REG_P x 1024, BIN_LDS_P x 1024
SIZES = (12288, 12289, 13300, 16384, 16385)
SPLIT = 6                                                   # 'present' = frames 0..5: the set flips at bounds(n)[6]
CHAINS = {'owe0': (), 'owe1': (5, ), 'owe4': (2, 5, 6, 7)}  # slot ends of the owed transforms, oldest first


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need the MI355X'
    return torch


@pytest.fixture(scope='module')
def orc():
    from oracle import oracle
    return oracle


def bounds(n):
    """Frame offsets of the 8-frame window of n points: four frames of 3 000 in the registers, then boundaries 5, 6 and 7 at the
    quarters of the parked range (n - 12 288 points) -- or, where that range holds fewer than four points, in front of it."""
    p = n - REG
    tail = [REG + p // 4, REG + p // 2, REG + 3 * p // 4] if p >= 4 else [12100, 12200, REG if p == 1 else 12250]
    return [0, 3000, 6000, 9000, 12000] + tail + [n]


def special_points(n):
    """(a dynamic point, a point with z = inf, a point with z = NaN) among the parked points, where there are enough of them."""
    p = min(n, REG + PARK) - REG
    return (REG + 1, REG + p // 3, REG + p // 3 + 1) if p >= 6 else None


_windows = {}


def window(n, heavy=False):
    """The frames of the n-point window: computed once, never written to.  heavy: frame 0 lies in ONE tile (3 000 records, above
    the 2 560 at which a tile goes to the heavy kernel)."""
    if (n, heavy) not in _windows:
        rows = cc.skewed_rows(np.random.default_rng(4000 + n), n)
        if heavy:
            rows[:3000, 0:2] = np.random.default_rng(5).uniform(1.5, 2.5, (3000, 2))
        sp = special_points(n)
        if sp:
            rows[REG:REG + 8, 9] = 0
            rows[sp[0], 9] = 1
            rows[sp[1], 2], rows[sp[2], 2] = np.inf, np.nan
        elif n > REG:
            rows[REG:, 9] = 0                                 # (the one parked point is an ordinary kept point)
        b = bounds(n)
        frames = [rows[b[f]:b[f + 1]] for f in range(8)]
        for r in frames:
            r.setflags(write=False)
        _windows[(n, heavy)] = frames
    return _windows[(n, heavy)]


def bev_args(px=64):
    return ((0.25, -0.125, 0.0625), np.eye(3), 0., 0., VIEW, px, None, *INTS, 0, DYNOBJ, True)


def oracle_planes(orc, frames, n_present, px=64):
    return orc.bev(orc.Store.from_rows(np.concatenate(frames), intensity_div255=True), n_present, orc.make_bev_params(*bev_args(px)))


def level1_lds(ctx):
    """(points per thread parked in LDS, bytes of dynamic LDS) of the process's last single raster (pca_debug_bev_lds)."""
    out = (C.c_int * 2)()
    assert ctx.lib.pca_debug_bev_lds(out) == 0
    return tuple(out)


def expected_lds_p(fits=True):
    return 4 if fits and os.environ.get('PCA_BEV_LDS_P', '1') != '0' else 0


def stored_xyz(st):
    """x, y, z as the store holds them now (read directly: owed transforms stay owed)."""
    return np.stack([t[:st.ub_tail].cpu().numpy() for t in (st.x, st.y, st.z)], 1)


def digest(p16, p64, st):
    h = hashlib.sha256()
    for a in (p16, p64, stored_xyz(st)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------- the cases
# Each case asserts against the oracle and returns the digest of what it computed.  PCA_BEV_G=1 is set by the caller.
def case_piece(T, orc, n, chain, write_back, heavy=False):
    """One window of n points as ONE piece, `chain` owed transforms that change z, written back or not."""
    from pca_amd.device_store import make_bev_params
    frames, ends = window(n, heavy), CHAINS[chain]
    st = loaded_store(frames)
    st.CHAIN_K = max(len(ends), 1) if write_back else 5     # (write back when this many are owed: now, or never)
    Ts = [_tilting_transform(s) for s in range(len(ends))]
    owe(st, Ts, ends)
    moved = owed_frames(orc, frames, Ts, ends)
    b = bounds(n)
    if heavy:                                               # a tile of the raster really holds more records than the heavy threshold
        r = np.concatenate(moved)
        ax, ay = r[:, 0] - 0.25, r[:, 1] + 0.125
        ok = (np.abs(ax) < 0.5 * VIEW) & (np.abs(ay) < 0.5 * VIEW) & np.isfinite(r[:, 2]) & (r[:, 9] != 1)
        i, j = np.floor(ax[ok] / VIEW * 64 + 32).astype(int), np.floor(ay[ok] / VIEW * 64 + 32).astype(int)
        assert np.bincount((63 - j) // 8 * 8 + i // 8).max() > 2560
    prm = make_bev_params(*bev_args())
    for rep in range(2 if heavy else 1):                    # (heavy: the first raster reports the heavy tile, the second launches with it)
        p16, p64 = st.bev(SPLIT, prm, want_f64=True)
        st.check_status()
        if rep == 0 and heavy and ends:
            assert (st._pending == []) == bool(write_back)
    assert level1(st.ctx)[:2] == (1, 0) and level1_lds(st.ctx)[0] == expected_lds_p()
    name = f'{n} {chain} wb={write_back} heavy={heavy}'
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), oracle_planes(orc, moved, b[SPLIT]), name)
    got, lo, hi = stored_xyz(st), REG, min(n, REG + PARK)
    want = np.concatenate(moved if (ends and write_back) else frames)[:, :3]
    assert np.array_equal(got[lo:hi], want[lo:hi], equal_nan=True), name + ': parked points'
    assert np.array_equal(got, want, equal_nan=True), name
    assert (st._pending == []) == (not ends or bool(write_back)), name
    if ends:                                                # (the chain moves z; frame 4 reaches into the parked range)
        assert not np.array_equal(moved[4][:, 2], frames[4][:, 2], equal_nan=True)
    return digest(p16.cpu().numpy(), p64.cpu().numpy(), st)


def case_riding_k1(T, orc):
    """A K1 noted by pca_kitti_integrate rides in the raster of a 13 300-point window: its 74 240 B of static LDS, the histogram
    and the parked block of the one store piece share the CU."""
    from pca_amd import _lib
    from pca_amd.device_store import make_bev_params
    frames = window(13300)
    rng = np.random.default_rng(31)
    n = 9000
    pc = np.stack([rng.uniform(0.5, 15, n), rng.uniform(-12, 12, n), rng.uniform(-2, 3, n), rng.integers(0, 256, n)], 1).astype(np.float32)
    img = rng.integers(0, 256, (H_CULL, W_CULL, 3), dtype=np.uint8)
    sem = rng.integers(0, 19, (H_CULL, W_CULL)).astype(np.uint8)
    ost = orc.Store(n, intensity_div255=True)
    orc.kitti_project_sample_filter(ost, pc, P_CULL, img, sem, None, H_CULL, W_CULL, KITTI_FILTERS)
    newest = ost.rows()
    assert len(newest) > 1000
    st = loaded_store(frames, room=n)
    f = dict(pts=cu(T, pc), rgb=cu(T, img), sem=cu(T, sem))
    st.set_defer_k1(True)
    try:
        o = _lib.PcaKittiObs()
        o.pts, o.rgb, o.sem, o.sem_gt, o.n, o.host_mask = f['pts'].data_ptr(), f['rgb'].data_ptr(), f['sem'].data_ptr(), None, n, 0
        st.append_kitti_obs(o, P_CULL, H_CULL, W_CULL, KITTI_FILTERS, keep=f)
        p16, p64 = st.bev(SPLIT, make_bev_params(*bev_args()), want_f64=True)
        grid, lds = level1(st.ctx), level1_lds(st.ctx)
        st.check_status()
    finally:
        st.set_defer_k1(False)
    assert grid[:2] == (4, 3), grid                           # three K1 tiles rode, the store's part is one piece
    assert lds[0] == expected_lds_p() and lds[1] >= 64 * 8 + lds[0] * 1024 * 12
    ref = oracle_planes(orc, list(frames) + [newest], bounds(13300)[SPLIT])
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), ref, 'riding K1')
    assert np.array_equal(st.rows(8), newest)
    return digest(p16.cpu().numpy(), p64.cpu().numpy(), st)


def case_no_room(T, orc):
    """px = 1024: histogram and cursors of 16 384 tiles take 128 KiB, the parked block does not fit -- lds_p = 0, the memory path."""
    from pca_amd.device_store import make_bev_params
    frames = window(13300)
    st = loaded_store(frames)
    p16, p64 = st.bev(SPLIT, make_bev_params(*bev_args(1024)), want_f64=True)
    st.check_status()
    assert level1(st.ctx)[:2] == (1, 0) and level1_lds(st.ctx) == (0, 16384 * 8)
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), oracle_planes(orc, frames, bounds(13300)[SPLIT], 1024), 'px 1024')
    return digest(p16.cpu().numpy(), p64.cpu().numpy(), st)


def case_intensity64(T, orc):
    """f64 intensities: 24-byte records, no register path and no parked points."""
    from pca_amd.device_store import make_bev_params
    frames = window(13300)
    st = loaded_store(frames)
    i64 = T.from_numpy(np.ascontiguousarray(np.concatenate(frames)[:, 3])).cuda()
    p16, p64 = st.bev(SPLIT, make_bev_params(*bev_args()), want_f64=True, intensity64=i64)
    st.check_status()
    assert level1(st.ctx)[:2] == (1, 0) and level1_lds(st.ctx)[0] == 0
    assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), oracle_planes(orc, frames, bounds(13300)[SPLIT]), 'intensity64')
    return digest(p16.cpu().numpy(), p64.cpu().numpy(), st)


def case_many(T, orc):
    """pca_bev_generate_many gets the parked block through the shared body: two jobs, the window and frames 1..6 of it."""
    from pca_amd.device_store import make_bev_params
    from test_gpu_bev_edges import assert_f16_matches_oracle
    frames = window(16385)
    st = loaded_store(frames)
    prm = make_bev_params(*bev_args())
    out = T.empty((2, 21, 64, 64), dtype=T.float16, device='cuda')
    st.bev_many([(SPLIT, prm, 0, None), (SPLIT, prm, 1, 7)], out)
    st.check_status()
    out = out.cpu().numpy()
    b = bounds(16385)
    assert b[7] - b[1] > REG
    assert_f16_matches_oracle(out[0], oracle_planes(orc, frames, b[SPLIT]), 'job 0')
    assert_f16_matches_oracle(out[1], oracle_planes(orc, frames[1:7], b[SPLIT] - b[1]), 'job 1')
    return digest(out, out[:0], st)


PIECES = [(n, chain, wb) for n in SIZES for chain in CHAINS for wb in ((1, ) if chain == 'owe0' else (0, 1))]
CASES = {f'piece-{n}-{chain}-wb{wb}': (case_piece, (n, chain, wb)) for n, chain, wb in PIECES}
CASES['heavy-13300-owe4-wb0'] = (case_piece, (13300, 'owe4', 0, True))
CASES['heavy-16385-owe1-wb1'] = (case_piece, (16385, 'owe1', 1, True))
CASES['riding_k1'] = (case_riding_k1, ())
CASES['no_room'] = (case_no_room, ())
CASES['intensity64'] = (case_intensity64, ())
CASES['many'] = (case_many, ())
HEAVY = [k for k in CASES if k.startswith('heavy')]
_digests = {}


def run_case(T, orc, name):
    """The case's digest in THIS process (run once)."""
    if name not in _digests:
        fn, args = CASES[name]
        old = os.environ.get('PCA_BEV_G')
        os.environ['PCA_BEV_G'] = '1'
        try:
            _digests[name] = fn(T, orc, *args)
        finally:
            if old is None:
                del os.environ['PCA_BEV_G']
            else:
                os.environ['PCA_BEV_G'] = old
    return _digests[name]


def _child(names):
    """A child process: the named cases (all: '*'), self-checked against the oracle; one DIGEST line per case."""
    import torch
    from oracle import oracle
    for name in (sorted(CASES) if names == '*' else names.split(',')):
        print('DIGEST', name, run_case(torch, oracle, name), flush=True)


def start_child(env, names):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_bev_lds_overflow as t; '
            't._child(%r)' % (here, os.path.join(root, 'pc-accumulation-lib_amd'), root, names))
    return subprocess.Popen([sys.executable, '-c', code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def child_digests(proc, what):
    out, err = proc.communicate(timeout=600)
    assert proc.returncode == 0, (what, out[-1500:] + err[-3000:])
    return {ln.split()[1]: ln.split()[2] for ln in out.splitlines() if ln.startswith('DIGEST ')}


@pytest.fixture(scope='module')
def children():
    """The three switched processes, started together: parked points off; halves of tiles always; both."""
    procs = {'off': start_child({'PCA_BEV_LDS_P': '0'}, '*'),
             'split2': start_child({'PCA_BEV_SPLIT': '2'}, ','.join(HEAVY)),
             'split2_off': start_child({'PCA_BEV_SPLIT': '2', 'PCA_BEV_LDS_P': '0'}, ','.join(HEAVY))}
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()


# ------------------------------------------------------------------------------------------------------------- the tests
def test_the_windows_are_what_the_cases_need():
    for n in SIZES:
        b, frames = bounds(n), window(n)
        assert b == sorted(b) and sum(len(r) for r in frames) == n
        if n - REG >= 4:                                      # frame ends 5, 6, 7 -- chain ends and the split -- inside the parked range
            assert all(REG < b[k] < min(n, REG + PARK) for k in (5, 6, 7))
        rows = np.concatenate(frames)
        sp = special_points(n)
        if sp:
            assert rows[sp[0], 9] == 1 and np.isinf(rows[sp[1], 2]) and np.isnan(rows[sp[2], 2]) and REG <= min(sp) and max(sp) < REG + PARK
    assert special_points(12289) is None and special_points(13300) and bounds(12289)[7:] == [REG, 12289]
    assert len(window(13300, heavy=True)[0]) == 3000 > 2560


@pytest.mark.parametrize('n,chain,wb', PIECES)
def test_piece_sizes_and_owed_chains_against_the_oracle(T, orc, children, n, chain, wb):
    run_case(T, orc, f'piece-{n}-{chain}-wb{wb}')


@pytest.mark.parametrize('name', HEAVY)
def test_with_a_heavy_tile_and_halves_allowed(T, orc, children, name):
    """A tile above the heavy threshold: the second raster is launched with the heavy kernel and with LDS for a histogram by
    halves of tiles, in front of the parked block."""
    run_case(T, orc, name)


@pytest.mark.parametrize('name', ['riding_k1', 'no_room', 'intensity64', 'many'])
def test_the_other_routes(T, orc, children, name):
    run_case(T, orc, name)


def test_the_switch_off_gives_the_same_bytes(T, orc, children):
    """PCA_BEV_LDS_P=0 against the default, every case: 21 planes (f16 and f64) and the stored x, y, z byte-identical."""
    off = child_digests(children['off'], 'PCA_BEV_LDS_P=0')
    assert sorted(off) == sorted(CASES)
    for name in sorted(CASES):
        assert off[name] == run_case(T, orc, name), name


def test_halves_of_tiles_with_parked_points_give_the_same_bytes(T, orc, children):
    """PCA_BEV_SPLIT=2 orders every piece by halves of tiles, parked points or not: the oracle's planes (checked in the child),
    and the bytes of the default, with the parked block and without."""
    on, off = child_digests(children['split2'], 'PCA_BEV_SPLIT=2'), child_digests(children['split2_off'], 'PCA_BEV_SPLIT=2 PCA_BEV_LDS_P=0')
    assert sorted(on) == sorted(off) == sorted(HEAVY)
    for name in HEAVY:
        assert on[name] == off[name] == run_case(T, orc, name), name
