"""Scenes and CPU models (numpy only; the C oracle is handed in) for the kernels of csrc/pca_accum.hip that maintain the point
store in place: K2 (pca_retransform), its batch tail (pca_retransform_batch_tail), K3 (pca_mark_dynamic) and the voxel
de-duplication (pca_voxel_dedup).  tests/test_store_edges_models.py checks the models and the scenes on the CPU,
tests/test_gpu_store_edges.py runs the scenes on the device.

A scene is a dict: 'frames' (a list of (M,10) rows, one per slot, as DeviceStore.load_rows takes them: guard frames, then the
window, then -- where the call allows one -- a guard frame) plus the call's own arguments.  `off` is always the whole frame_off
array, indexed by ABSOLUTE slot; `rows` the concatenation of all frames.  Nothing here needs a tolerance:

  k2_model       the oracle's retransform on [off[slot_begin], off[slot_end]), once per transform, in order
  k2_tail_model  frame i of the batch takes Ts[i+1:], one oracle call per transform
  k3_model       dyn = 1 where inst == idx inside the slot's segment (idx = -1 matches unlabelled points)
  dedup_model    voxel = clip(floor(v / size) + 2^20, 0, 2^21 - 1) per axis in f64 (the kernel's own expression); of the window's
                 points in one voxel the first in store order stays; the new offsets count the kept points before each boundary
"""
import functools

import numpy as np

TILE = 1024                  # points per tile of dedup_compact
K2_TRIP = 2 * 2048 * 256     # points one trip of k2_retransform's grid-stride loop covers (2048 x 256 pairs)
K2_CHAIN = 16                # transforms per launch of K2 and of its tail
TAIL_ROW = 32 * 256          # threads per frame of k2_retransform_tail
K3_PAIRS = 32                # pairs per launch of K3
K3_ROW = 64 * 256            # threads per pair of k3_mark_dynamic


# ---- scenes -------------------------------------------------------------------------------------
def hash_name(name):
    """A seed from a scene's name that does not change from run to run."""
    return int.from_bytes(name.encode(), 'little') % (1 << 31)


def frame(rng, n, lim=50.0):
    """(n,10) rows with every column populated: finite coordinates, an f32-representable column 3, colours and class 0..255,
    instances -1..6, mixed dyn."""
    r = np.zeros((n, 10))
    r[:, :3] = rng.uniform(-lim, lim, (n, 3))
    r[:, 3] = rng.integers(0, 2048, n) / 8.0
    r[:, 4:8] = rng.integers(0, 256, (n, 4))
    r[:, 8] = rng.integers(-1, 7, n)
    r[:, 9] = rng.random(n) < 0.3
    return r


def offsets(frames):
    return np.concatenate([[0], np.cumsum([f.shape[0] for f in frames])]).astype(np.int64)


def all_rows(frames):
    return np.concatenate([np.asarray(f).reshape(-1, 10) for f in frames]) if frames else np.zeros((0, 10))


def transforms(rng, n):
    """n distinct near-rigid 4x4 transforms (a rotation about z, a little shear, a shift): any two differ in every row."""
    Ts = np.zeros((n, 4, 4))
    for k in range(n):
        a = rng.uniform(-0.05, 0.05)
        c, s = np.cos(a), np.sin(a)
        Ts[k] = np.eye(4)
        Ts[k, :3, :3] = [[c, -s, 0.001], [s, c, -0.002], [0.0005, 0.001, 1.0]]
        Ts[k, :3, 3] = rng.uniform(-2, 2, 3)
    return Ts


def soa(rows):
    """The store's seven arrays for (M,10) rows, as DeviceStore.load_rows encodes them (intensity_div255 off)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 10)
    c = rows[:, 4:8].astype(np.uint32)
    return dict(x=rows[:, 0].copy(), y=rows[:, 1].copy(), z=rows[:, 2].copy(), intensity=rows[:, 3].astype(np.float32),
                rgbs=(c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)).astype(np.uint32),
                inst=rows[:, 8].astype(np.int32), dyn=(rows[:, 9] == 1).astype(np.uint8))


def same_bits(a, b):
    """Equal shape, type and bit patterns (-0.0 is not 0.0; a NaN equals only itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(a.view(u), b.view(u))


# ---- K2 -----------------------------------------------------------------------------------------
def apply_chain(rows, lo, hi, Ts, orc):
    """rows with the transforms Ts applied to points [lo, hi), one oracle pass per transform, in order."""
    st = orc.Store.from_rows(rows)
    for T in Ts:
        orc.retransform(st, T, int(lo), int(hi))
    out = np.array(rows, dtype=np.float64)
    n = out.shape[0]
    out[:, 0], out[:, 1], out[:, 2] = st.x[:n], st.y[:n], st.z[:n]
    return out


def k2_model(rows, off, slot_begin, slot_end, Ts, orc):
    return apply_chain(rows, off[slot_begin], off[slot_end], Ts, orc)


def k2_scene(name):
    """Windows of 0, 1, 2, 3 and 7 points at even and odd lo (all four parities of (lo, hi)); windows of empty frames only;
    empty frames at both ends; slot_begin == slot_end; n_T around the 16-transform pass on a few thousand points; one window
    that needs the second trip of the grid-stride loop."""
    rng = np.random.default_rng(hash_name(name))
    split = {0: [0], 1: [1], 2: [2], 3: [1, 2], 7: [3, 4]}
    if name.startswith('lo'):                                  # 'lo<parity>_n<points>'
        par, n = int(name[2]), int(name.split('_n')[1])
        sizes, sb, se, n_T = [6 + par] + split[n] + [4], 1, 1 + len(split[n]), 3
    elif name.startswith('empties_lo'):
        sizes, sb, se, n_T = [6 + int(name[-1]), 0, 0, 0, 4], 1, 4, 3
    elif name == 'empty_ends':
        sizes, sb, se, n_T = [5, 0, 0, 5, 0, 8, 0, 4], 1, 7, 3
    elif name == 'begin_is_end':
        sizes, sb, se, n_T = [5, 3, 4, 4], 1, 1, 3
    elif name.startswith('nT'):
        sizes, sb, se, n_T = [7, 1000, 0, 1501, 733, 10], 1, 5, int(name[2:])
    elif name == 'second_trip':
        sizes, sb, se, n_T = [1, 600000, K2_TRIP + 7 - 600000, 3], 1, 3, 2
    else:
        raise KeyError(name)
    return dict(frames=[frame(rng, n) for n in sizes], slot_begin=sb, slot_end=se, Ts=transforms(rng, n_T))


K2_SCENES = (['lo%d_n%d' % (p, n) for p in (0, 1) for n in (0, 1, 2, 3, 7)] + ['empties_lo0', 'empties_lo1', 'empty_ends', 'begin_is_end']
             + ['nT%d' % n for n in (0, 1, 16, 17, 32, 33)] + ['second_trip'])
K2_UNCHANGED = ('lo0_n0', 'lo1_n0', 'empties_lo0', 'empties_lo1', 'begin_is_end', 'nT0')


# ---- K2 tail ------------------------------------------------------------------------------------
def k2_tail_model(rows, off, first_slot, n_frames, Ts, orc):
    out = rows
    for i in range(n_frames):
        out = apply_chain(out, off[first_slot + i], off[first_slot + i + 1], Ts[i + 1:], orc)
    return np.array(out, dtype=np.float64)


TAIL_FRAMES = (0, 1, 2, 16, 17, 18, 33, 34)


def k2_tail_scene(n_frames):
    """Two guard frames, a batch of n_frames frames from slot 2 on, one guard frame.  The batch holds empty and one-point frames;
    from 2 frames on frame 0 has 8193 points (one more than a row of the launch has threads), from 18 on frame 1 has 20 000."""
    rng = np.random.default_rng(100 + n_frames)
    small = [37, 0, 1, 300, 2, 0, 129, 1, 64]
    sizes = [small[i % len(small)] for i in range(n_frames)]
    if n_frames >= 2:
        sizes[0] = TAIL_ROW + 1
    if n_frames >= 18:
        sizes[1] = 20000
    frames = [frame(rng, 5), frame(rng, 0)] + [frame(rng, n) for n in sizes] + [frame(rng, 4)]
    return dict(frames=frames, first_slot=2, n_frames=n_frames, Ts=transforms(rng, max(n_frames, 1)))


# ---- K3 -----------------------------------------------------------------------------------------
def k3_model(rows, off, slots, idxs):
    out = np.array(rows, dtype=np.float64)
    for s, i in zip(slots, idxs):
        seg = out[off[s]:off[s + 1]]
        seg[seg[:, 8] == i, 9] = 1
    return out


K3_PAIR_COUNTS = (0, 1, 32, 33, 65)
K3_HEAD = 1                  # the scene's first frame is evicted: slots are absolute, not relative to the first live slot


def k3_scene(n_pairs):
    """Slot 0 is evicted by the test; slots 1.. hold 500, 0, 16 385, 40 000, 700 and 3 points.  The pair list cycles over two
    instances on the 16 385-point slot, the unlabelled points of the 500-point slot and a pair on the empty slot (so pairs
    repeat); its LAST pair is the only one on the 40 000-point slot.  Slots 5 and 6 are named by nobody."""
    rng = np.random.default_rng(200)
    frames = [frame(rng, n) for n in (9, 500, 0, K3_ROW + 1, 40000, 700, 3)]
    frames[3][-1, 8:10] = [0, 0]                               # the one point beyond the threads of a row: instance 0, static
    cycle = [(3, 0), (3, 1), (1, -1), (2, 3)]
    pairs = [cycle[k % 4] for k in range(max(n_pairs - 1, 0))] + [(4, 5)] * min(n_pairs, 1)
    return dict(frames=frames, slots=[s for s, _ in pairs], idxs=[i for _, i in pairs])


# ---- voxel de-duplication -----------------------------------------------------------------------
def voxels(xyz, size, rnd=np.floor, clamp=True):
    """(N,3) f64 voxel indices + 2^20, clamped to the key's 21 bits per axis."""
    with np.errstate(invalid='ignore'):
        v = rnd(np.asarray(xyz, dtype=np.float64) / size) + 2.0 ** 20
    return np.clip(v, 0, 2 ** 21 - 1) if clamp else v


def first_of_each(vox):
    """keep (N,) bool: the first row of every distinct row of vox."""
    keep = np.zeros(len(vox), bool)
    if len(vox):
        keep[np.unique(vox, axis=0, return_index=True)[1]] = True
    return keep


def compacted(rows, off, slot_begin, slot_end, keep):
    """The window's frames with only the kept points, and frame_off after the compaction: a boundary becomes lo + the kept
    points before it (leading empty frames stay at lo, boundaries at the old end move to the new end)."""
    lo = int(off[slot_begin])
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    new_off = np.array(off, dtype=np.int64)
    new_off[slot_begin + 1:slot_end + 1] = lo + before[off[slot_begin + 1:slot_end + 1] - lo]
    frames = [rows[off[f]:off[f + 1]][keep[off[f] - lo:off[f + 1] - lo]] for f in range(slot_begin, slot_end)]
    return frames, new_off


def dedup_model(rows, off, slot_begin, slot_end, size):
    keep = first_of_each(voxels(rows[off[slot_begin]:off[slot_end], :3], size))
    return compacted(rows, off, slot_begin, slot_end, keep)


def voxel_key(q):
    """The kernel's packed key of clamped indices q (N,3) uint64."""
    q = np.asarray(q, dtype=np.uint64)
    return (np.uint64(1) << np.uint64(63)) | (q[:, 0] << np.uint64(42)) | (q[:, 1] << np.uint64(21)) | q[:, 2]


def voxel_hash(k):
    """The kernel's 64-bit finaliser (wrapping uint64 arithmetic)."""
    k = np.asarray(k, dtype=np.uint64).copy()
    s = np.uint64(33)
    k ^= k >> s
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> s
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> s
    return k


def home_slot(xyz, size, cap):
    return voxel_hash(voxel_key(voxels(xyz, size).astype(np.uint64))) & np.uint64(cap - 1)


@functools.lru_cache(maxsize=None)
def colliding_voxels(side, cap, count):
    """`count` distinct integer voxels of the lattice [-side/2, side/2)^3 whose home slot is the table's last: (count,3) int64."""
    g = np.arange(-(side // 2), side - side // 2, dtype=np.int64)
    c = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    home = voxel_hash(voxel_key((c + 2 ** 20).astype(np.uint64))) & np.uint64(cap - 1)
    hit = c[home == np.uint64(cap - 1)]
    assert len(hit) >= count, (len(hit), count)
    return hit[:count]


def table_slots(max_points):
    """Slots of the de-duplication's table for a window bound: a power of two >= 1024, load factor <= 1/2."""
    cap = 1024
    while cap < 2 * max_points:
        cap *= 2
    return cap


def _with_voxels(rng, vox, size, n):
    """n rows whose points lie inside the integer voxels vox[choice], at random places of the voxel."""
    r = frame(rng, n)
    pick = rng.integers(0, len(vox), n) if n else np.zeros(0, np.int64)
    r[:, :3] = (vox[pick] + rng.uniform(0.05, 0.95, (n, 3))) * size
    return r


def _guard_of(rng, window, n=5):
    """An odd number of guard rows: copies of the window's first points (which must not count as their first occurrences),
    filled up with random rows."""
    w = all_rows(window)[:n]
    return np.concatenate([w, frame(rng, n - len(w))])


def _split(rows, sizes):
    assert sum(sizes) == len(rows), (sum(sizes), len(rows))
    b = offsets([np.zeros((n, 10)) for n in sizes])
    return [rows[b[k]:b[k + 1]] for k in range(len(sizes))]


DEDUP_SCENES = ('n0', 'n1', 'n1023', 'n1024', 'n1025', 'tile_edges', 'empty_runs', 'one_voxel', 'no_duplicates', 'frame_copies',
                'collide_1024', 'collide_4096', 'clamp')
DEDUP_KEEPS_ALL = ('n0', 'n1', 'no_duplicates')      # every other scene is meant to drop points


def dedup_scene(name):
    """One guard frame of five rows (copies of window points: lo is odd, slot_begin = 1), then the window up to the last used
    slot.  'max_points' is the bound the call is given (None: the window's own size)."""
    rng = np.random.default_rng(hash_name(name))
    size, max_points = 1.0, None
    cube = np.stack(np.meshgrid(*[np.arange(-4, 4)] * 3, indexing='ij'), -1).reshape(-1, 3)      # 512 voxels
    if name in ('n0', 'n1', 'n1023', 'n1024', 'n1025'):
        n = int(name[1:])
        sizes = {0: [0, 0], 1: [1], 1023: [500, 523], 1024: [1024], 1025: [1024, 1]}[n]
        window = _split(_with_voxels(rng, cube, size, n), sizes)
    elif name == 'tile_edges':                                 # boundaries at 1023, 1024, 1025, 2048 and the end, 2049
        window = _split(_with_voxels(rng, cube, size, 2049), [1023, 1, 1, 1023, 1])
    elif name == 'empty_runs':
        window = _split(_with_voxels(rng, cube[:200], size, 700), [0, 0, 300, 0, 0, 0, 400, 0, 0])
    elif name == 'one_voxel':                                  # one point stays; every later frame becomes empty
        window = _split(_with_voxels(rng, cube[:1], size, 1025), [200, 300, 0, 524, 1])
    elif name == 'no_duplicates':
        size = 0.25
        r = frame(rng, 1025)
        r[:, :3] = (rng.permutation(np.stack(np.meshgrid(*[np.arange(-6, 6)] * 3, indexing='ij'), -1).reshape(-1, 3))[:1025] + 0.5) * size
        window = _split(r, [300, 0, 724, 1])
    elif name == 'frame_copies':                               # exact copies of a frame several frames later
        size = 0.5
        a, b, c, d = (frame(rng, n, lim=6.0) for n in (400, 300, 500, 200))
        window = [a, b, c, a.copy(), d, b.copy()]
    elif name in ('collide_1024', 'collide_4096'):             # every probe chain runs through the last slot and wraps to slot 0
        cap = int(name.split('_')[1])
        vox = colliding_voxels(80 if cap == 1024 else 128, cap, 230 if cap == 1024 else 320)
        n = 500 if cap == 1024 else 1500
        r = _with_voxels(rng, vox, size, n)
        r[:len(vox), :3] = (vox + 0.5) * size                  # every voxel at least once
        r = r[rng.permutation(n)]
        window = _split(r, [n // 3, 0, n - n // 3])
        max_points = 512 if cap == 1024 else 2048
    elif name == 'clamp':
        # per axis, in this order: voxel -2^20-1, -2^20 (one boundary voxel), 2^20-1, 2^20, +inf (the other), -inf (the first again)
        size = 0.5
        edge = [(-2.0 ** 20 - 1 + 0.5) * size, (-2.0 ** 20 + 0.5) * size, (2.0 ** 20 - 1 + 0.5) * size, (2.0 ** 20 + 0.5) * size, np.inf, -np.inf]
        r = frame(rng, 18 + 40, lim=3.0)
        for ax in range(3):
            r[6 * ax:6 * ax + 6, :3] = 0.25
            r[6 * ax:6 * ax + 6, ax] = edge
        window = _split(r, [7, 30, 21])
    else:
        raise KeyError(name)
    frames = [_guard_of(rng, window)] + window
    return dict(frames=frames, slot_begin=1, slot_end=len(frames), size=size, max_points=max_points)
