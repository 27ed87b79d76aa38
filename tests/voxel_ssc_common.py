"""The numpy model of pca_voxel_pool and pca_voxel_pack (include/pca.h) and the scenes the tests of tests/test_voxel_ssc_model.py
and tests/test_gpu_voxel_ssc.py share.  Both contracts are restated with reshape / transpose / np.packbits; nothing here
knows how the kernels work.  A plain module: no test, no fixture."""
import numpy as np

MAX_LABELS = 32
SCALES = (2, 4, 8)
THRESHOLD = {2: 1, 4: 4, 8: 26}           # occupied fine voxels a coarse voxel needs under occupied_fraction = (1, 20)
LABEL_MAP = (0x1234 + 37 * np.arange(32)).astype(np.uint16)       # values above 255: the byte order shows
EMPTY_VALUE = 0xBEEF


# ------------------------------------------------------------------------------------------------------------------ pool
def blocks(vol, s):
    """[nz, px, px] -> [nz/s, px/s, px/s, s^3]: the fine voxels of every coarse voxel of scale s, aligned at 0."""
    nz, px, _ = vol.shape
    return vol.reshape(nz // s, s, px // s, s, px // s, s).transpose(0, 2, 4, 1, 3, 5).reshape(nz // s, px // s, px // s, s ** 3)


def pool_counts(labels, seen, s):
    """n_occ, n_free, n_unseen [coarse] and c [coarse, 32] of scale s: counts of fine voxels."""
    lab = blocks(labels, s)
    occ = lab < MAX_LABELS                                        # any other byte is 255
    n_occ = occ.sum(-1).astype(np.int64)
    n_free = (~occ & (blocks(seen, s) != 0)).sum(-1).astype(np.int64)
    c = np.stack([(lab == l).sum(-1) for l in range(MAX_LABELS)], -1).astype(np.int64)
    return n_occ, n_free, s ** 3 - n_occ - n_free, c


def pool_model(labels, seen, visible=None, s=2, fraction=(1, 20)):
    """{'labels', 'state'[, 'visible']} of scale s, decided from the FINE voxels."""
    n_occ, n_free, n_unseen, c = pool_counts(labels, seen, s)
    occupied = (n_occ > 0) & (n_occ * int(fraction[1]) >= s ** 3 * int(fraction[0]))
    out = {'labels': np.where(occupied, c.argmax(-1), 255).astype(np.uint8),          # (argmax: the first = smallest label)
           'state': np.where(occupied, 2, np.where(n_free > n_unseen, 1, 0)).astype(np.uint8)}
    if visible is not None:
        out['visible'] = (blocks(visible, s) != 0).any(-1).astype(np.uint8)
    return out


def pool_hierarchical(labels, seen, s, fraction=(1, 20)):
    """What the contract is NOT: scale s pooled from the scale-s/2 RESULT (its labels, and state != 0 as `seen`)."""
    out = pool_model(labels, seen, None, 2, fraction)
    at = 2
    while at < s:
        out = pool_model(out['labels'], (out['state'] != 0).astype(np.uint8), None, 2, fraction)
        at *= 2
    return out


def state_of(labels, seen):
    return np.where(labels < MAX_LABELS, 2, (seen != 0).astype(np.uint8)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ pack
def places(vol):
    """[nz, px, px] -> [px px nz] in place order t = (i px + j) nz + k, voxel (i, j, k) at [k, px - 1 - j, i]."""
    return np.ascontiguousarray(vol[:, ::-1, :].transpose(2, 1, 0)).reshape(-1)


def pack_model(labels, seen=None, visible=None, input_occ=None, label_map=None, empty_value=0):
    table = np.arange(1, 33, dtype=np.uint16) if label_map is None else np.asarray(label_map, dtype=np.uint16)
    occ = labels < MAX_LABELS
    out = {'label': places(np.where(occ, table[np.minimum(labels, 31)], np.uint16(empty_value)).astype(np.uint16))}
    if seen is not None:
        out['invalid'] = np.packbits(places(~occ & (seen == 0)))
    if visible is not None:
        out['occluded'] = np.packbits(places(visible == 0))
    if input_occ is not None:
        out['bin'] = np.packbits(places(input_occ != 0))
    return out


def pack_loop(labels, seen, visible, input_occ, label_map, empty_value):
    """The same, voxel by voxel and bit by bit (small shapes only)."""
    nz, px, _ = labels.shape
    n = px * px * nz
    out = {'label': np.zeros(n, dtype=np.uint16)}
    for key in ('invalid', 'occluded', 'bin'):
        out[key] = np.zeros((n + 7) // 8, dtype=np.uint8)
    for i in range(px):
        for j in range(px):
            for k in range(nz):
                t, at = (i * px + j) * nz + k, (k, px - 1 - j, i)
                occ = labels[at] < MAX_LABELS
                out['label'][t] = label_map[labels[at]] if occ else empty_value
                for key, bit in (('invalid', not occ and seen[at] == 0), ('occluded', visible[at] == 0), ('bin', input_occ[at] != 0)):
                    if bit:
                        out[key][t // 8] |= 1 << (7 - t % 8)
    return out


def pyramid_model(labels, seen, visible=None, input_occ=None, scales=(1, 2, 4, 8), label_map=None, empty_value=0, fraction=(1, 20)):
    """SemBEVGenerator.voxel_pyramid_device on the host: {'levels', 'packed'} as numpy arrays."""
    levels, packed = {}, {}
    for s in scales:
        if s == 1:
            levels[1] = dict(labels=labels, seen=seen, state=state_of(labels, seen))
            levels[1].update({} if visible is None else {'visible': visible})
            levels[1].update({} if input_occ is None else {'input_occ': input_occ})
            packed[1] = pack_model(labels, seen, visible, input_occ, label_map, empty_value)
        else:
            levels[s] = pool_model(labels, seen, visible, s, fraction)
            packed[s] = pack_model(levels[s]['labels'], levels[s]['state'], label_map=label_map, empty_value=empty_value)
    return {'levels': levels, 'packed': packed}


# ---------------------------------------------------------------------------------------------------------------- scenes
def empty_scene(px, nz):
    return dict(labels=np.full((nz, px, px), 255, dtype=np.uint8), seen=np.zeros((nz, px, px), dtype=np.uint8),
                visible=np.zeros((nz, px, px), dtype=np.uint8))


def fill_block(sc, rng, k0, r0, c0, s, label_list, n_free):
    """The block of scale s at fine (k0, r0, c0): len(label_list) occupied voxels with those labels, n_free free ones, the
    rest unseen, at random places of the block."""
    at = rng.permutation(s ** 3)
    k, r, c = k0 + at // (s * s), r0 + (at // s) % s, c0 + at % s
    sc['labels'][k, r, c] = 255
    sc['seen'][k, r, c] = 0
    n = len(label_list)
    sc['labels'][k[:n], r[:n], c[:n]] = label_list
    sc['seen'][k[n:n + n_free], r[n:n + n_free], c[n:n + n_free]] = 1
    sc['seen'][k[:n:2], r[:n:2], c[:n:2]] = 1                     # (an occupied voxel's seen byte plays no part)


PLANTS = ('at', 'below', 'label_tie', 'free_tie')


def plant(sc, rng, k0, r0, c0, s, kind):
    thr, n = THRESHOLD[s], s ** 3
    if kind == 'at':
        fill_block(sc, rng, k0, r0, c0, s, rng.integers(0, 32, thr), (n - thr) // 3)
    elif kind == 'below':
        fill_block(sc, rng, k0, r0, c0, s, rng.integers(0, 32, thr - 1), n - thr + 1)
    elif kind == 'label_tie':                                     # two labels with as many voxels each, the larger label first
        m = max(thr, 2)
        fill_block(sc, rng, k0, r0, c0, s, [29] * m + [11] * m + [30] * (m - 1), 0)
    else:                                                         # below the threshold, as many free as unseen voxels
        n_occ = {2: 0, 4: 2, 8: 24}[s]
        fill_block(sc, rng, k0, r0, c0, s, rng.integers(0, 32, n_occ), (n - n_occ) // 2)


def random_scene(px, nz, seed=0, planted=True):
    """Occupancy drawn per 4 x 4 x 4 block with p in {0.02, 0.06, 0.4, 0.95}; labels skewed over all 32; seen and visible random
    (non-zero bytes of several values); a few label bytes in 32..254.  planted (px, nz multiples of 8): four blocks of each
    scale are then set to the situations PLANTS names -- for scale 8 only where the volume holds six 8 x 8 x 8 blocks, each
    scale in blocks of its own."""
    rng = np.random.default_rng([seed, px, nz])
    shape = (nz, px, px)
    p4 = rng.choice([0.02, 0.06, 0.4, 0.95], size=((nz + 3) // 4, (px + 3) // 4, (px + 3) // 4))
    p = np.repeat(np.repeat(np.repeat(p4, 4, 0), 4, 1), 4, 2)[:nz, :px, :px]
    skew = np.minimum(rng.geometric(0.3, shape) - 1, 31)
    lab = np.where(rng.random(shape) < 0.8, skew, rng.integers(0, 32, shape))
    labels = np.where(rng.random(shape) < p, lab, 255).astype(np.uint8)
    odd = rng.random(shape) < 0.01
    labels[odd] = rng.integers(32, 255, int(odd.sum()))
    sc = dict(labels=labels, seen=(rng.integers(0, 2, shape) * rng.integers(1, 256, shape)).astype(np.uint8),
              visible=(rng.integers(0, 2, shape) * rng.integers(1, 256, shape)).astype(np.uint8),
              input_occ=(rng.integers(0, 2, shape) * rng.integers(1, 256, shape)).astype(np.uint8))
    if planted:
        supers = [(k, r, c) for k in range(0, nz, 8) for r in range(0, px, 8) for c in range(0, px, 8)]
        rng.shuffle(supers)
        sub = lambda o, s, q: (o[0] + s * (q >> 2), o[1] + s * ((q >> 1) & 1), o[2] + s * (q & 1))      # noqa: E731
        if len(supers) >= 6:
            for q, kind in enumerate(PLANTS):
                plant(sc, rng, *supers[q], 8, kind)
                plant(sc, rng, *sub(supers[4], 4, q), 4, kind)
                plant(sc, rng, *sub(supers[5], 2, q), 2, kind)
        else:
            for q, kind in enumerate(PLANTS):
                plant(sc, rng, *sub(supers[0], 4, q), 4, kind)
                plant(sc, rng, *sub(sub(supers[0], 4, 4), 2, q), 2, kind)
    for v in sc.values():
        v.setflags(write=False)
    return sc


def situations(sc, s):
    """Which of PLANTS' situations the scene holds at scale s: {name: number of coarse voxels}."""
    n_occ, n_free, n_unseen, c = pool_counts(sc['labels'], sc['seen'], s)
    top = np.sort(c, -1)
    occupied = n_occ >= THRESHOLD[s]
    return {'at': int((n_occ == THRESHOLD[s]).sum()), 'below': int((n_occ == THRESHOLD[s] - 1).sum()),
            'label_tie': int((occupied & (top[..., -1] == top[..., -2])).sum()),
            'free_tie': int((~occupied & (n_free == n_unseen) & (n_free > 0)).sum())}


def pack_scene(px, nz, seed=0):
    """One level's volumes for the packer: 40 % occupied, a few label bytes in 32..254, the three byte masks random."""
    rng = np.random.default_rng([seed, px, nz, 7])
    shape = (nz, px, px)
    labels = np.where(rng.random(shape) < 0.4, rng.integers(0, 32, shape), 255).astype(np.uint8)
    odd = rng.random(shape) < 0.05
    labels[odd] = rng.integers(32, 255, int(odd.sum()))
    sc = dict(labels=labels)
    for key in ('seen', 'visible', 'input_occ'):
        sc[key] = (rng.integers(0, 2, shape) * rng.integers(1, 256, shape)).astype(np.uint8)
    for v in sc.values():
        v.setflags(write=False)
    return sc
