"""CPU: the numpy model of pca_bev_elev_partition (tests/elev_partition_common.py) against the reference's
static_obj_partitioning_by_elev as recorded in tests/golden/elev_partition.npz, what the fixture has to contain, and the
public surface (no GPU needed)."""
import numpy as np
import pytest

import elev_partition_common as ec

CASE_NAMES = [c[0] for c in ec.CASES]


def cfg(g):
    view, px, hf, rot, dx, dy = g['cfg']
    return float(view), int(px), float(hf), float(rot), float(dx), float(dy)


@pytest.mark.parametrize('case', CASE_NAMES)
def test_model_reproduces_the_reference_bit_for_bit(golden, case):
    g = golden('elev_partition')
    view, px, _, rot, dx, dy = cfg(g)
    frames, origin, hf, thresh, include_dyn = ec.fixture_case(g, case)
    rows = np.concatenate(frames)
    m = ec.model(rows, origin, ec.rotation(rot), dx, dy, view, px, hf, thresh, include_dyn)
    assert np.array_equal(m['observed'], g[f'mask_{case}'])
    assert np.array_equal(m['elev'].view(np.uint64), g[f'elev_{case}'].view(np.uint64))
    assert np.array_equal(ec.fates(m['flags'], rows[:, 8]), g[f'fate_{case}'])
    # the gridded rows the reference's method was handed are the model's rows in view, in window order, in its cells
    grid = g[ec.grid_name(case)]
    idx = grid[:, 3].astype(int)
    assert np.array_equal(idx, np.flatnonzero(m['flags'] != 255))
    assert np.array_equal((px - 1 - grid[:, 1]) * px + grid[:, 0], m['cell'][idx])
    assert np.array_equal(grid[:, 2], (rows[idx, 2] - origin[2]) + 0.0)
    assert m['counts'][0] == idx.size and m['counts'][1] + m['counts'][2] == idx.size


def test_fixture_holds_the_designed_rows(golden):
    g = golden('elev_partition')
    view, px, hf, rot, dx, dy = cfg(g)
    assert px == 20 and view == 10. and rot == 0.3 and g['origin_a'][2] != 0. and g['origin_z0'][2] == 0.
    frames = [g[f'frame{f}'] for f in range(3)]
    rows = np.concatenate(frames)
    n = rows.shape[0]
    assert 1400 <= n <= 1600 and np.array_equal(rows[:, 3], np.arange(n))
    frame_of = np.repeat(np.arange(3), [f.shape[0] for f in frames])
    for col, vals in ((8, (0., 1., 2.)), (9, (0., 1.))):
        assert set(np.unique(rows[:, col])) == set(vals)
    # every row in view, no static partition, no height filter, threshold 0.2
    grid = g['grid_a_hf0_dyn1']
    assert (grid[:, 0:2] >= 0).all() and (grid[:, 0:2] < px).all()
    idx = grid[:, 3].astype(int)
    cell = ((px - 1 - grid[:, 1]) * px + grid[:, 0]).astype(int)
    z = grid[:, 2]
    fate = {k: g[f'fate_a_hf0_dyn1_t{k}'][idx] for k in range(3)}
    t = ec.THRESHOLDS[0]
    boundary = single = min_last = min_first = 0
    for c in np.unique(cell):
        sel = np.flatnonzero(cell == c)
        zc, m = z[sel], z[sel].min()
        if sel.size == 1:
            if rows[idx[sel[0]], 8] == 0:                        # elevated under the negative threshold, static otherwise
                ok = fate[2][sel[0]] == ec.FATE_DYNAMIC and fate[0][sel[0]] == fate[1][sel[0]] == ec.FATE_STATIC
                single += int(ok)
            continue
        at, up, down = m + t, np.nextafter(m + t, np.inf), np.nextafter(m + t, -np.inf)
        if (zc == at).any() and (zc == up).any() and (zc == down).any():
            f0 = fate[0][sel]
            assert (f0[zc == up] == ec.FATE_DYNAMIC).all()                       # the compare is strict:
            assert (f0[(zc == at) | (zc == down)] != ec.FATE_DYNAMIC).all()      # fl(m + t) itself is not elevated
            boundary += 1
        f_min = frame_of[idx[sel[zc == m]]]
        f_el = frame_of[idx[sel[zc > m + t]]]
        if f_el.size:
            min_last += int((f_min == 2).all() and (f_el == 0).any())
            min_first += int((f_min == 0).all() and (f_el == 2).any())
    assert boundary >= 30 and single >= 10 and min_last >= 5 and min_first >= 5, (boundary, single, min_last, min_first)
    # all four corner cells, both sides of every edge between 8x8 tiles (image rows and columns 7 | 8 and 15 | 16)
    mask = g['mask_a_hf0_dyn1_t0']
    assert mask[0, 0] and mask[0, px - 1] and mask[px - 1, 0] and mask[px - 1, px - 1]
    for k in (7, 8, 15, 16):
        assert mask[k, :].all() and mask[:, k].all()
    # a stored z of -0.0 under origin z 0 is the minimum of its cell: the reference's map holds +0.0 there
    grid0 = g['grid_z0_hf0_dyn1']
    assert not (np.signbit(grid0[:, 2]) & (grid0[:, 2] == 0)).any()
    neg0 = np.flatnonzero(np.signbit(rows[:, 2]) & (rows[:, 2] == 0))
    assert neg0.size >= 3
    emap, emask = g['elev_z0_hf0_dyn1_t0'], g['mask_z0_hf0_dyn1_t0']
    at = {int(r[3]): (int(px - 1 - r[1]), int(r[0])) for r in grid0}
    for k in neg0:
        r, c = at[int(k)]
        assert emask[r, c] and emap[r, c] == 0. and not np.signbit(emap[r, c])
    # the filter and the static partition do remove rows
    assert g['grid_a_hf1_dyn1'].shape[0] < grid.shape[0] and g['grid_a_hf0_dyn0'].shape[0] < grid.shape[0]
    assert (g['fate_a_hf0_dyn1_t0'] == ec.FATE_OUT).sum() > 50 and (g['fate_a_hf0_dyn1_t0'] == ec.FATE_NEITHER).sum() > 50


def test_public_surface():
    """The reference's method under its own name, the device forms, and the two exports (missing before this feature)."""
    import inspect

    from bev_generator.sem_bev import SemBEVGenerator
    from pca_amd import _lib
    from pca_amd.device_store import DeviceStore
    from sem_pc_accum import SemanticPointCloudAccumulator
    assert list(inspect.signature(SemBEVGenerator.static_obj_partitioning_by_elev).parameters) == ['self', 'pc', 'elev_thresh']
    assert list(inspect.signature(SemBEVGenerator.elev_partition_device).parameters)[:8] == \
        ['self', 'pc', 'rot_mat', 'dx', 'dy', 'aug_view_size', 'elev_thresh', 'include_dyn']
    assert list(inspect.signature(DeviceStore.bev_elev_partition).parameters)[:7] == \
        ['self', 'prm', 'elev_thresh', 'first_frame', 'last_frame', 'include_dyn', 'mark_dyn']
    assert list(inspect.signature(SemanticPointCloudAccumulator.partition_by_elev).parameters) == \
        ['self', 'present_idx', 'elev_thresh', 'part', 'mark_dyn']
    assert 'pca_bev_elev_workspace_bytes' in _lib.EXPORTS and 'pca_bev_elev_partition' in _lib.EXPORTS
    lib = _lib.load()
    assert lib.pca_bev_elev_workspace_bytes(1000, 20) > 1000 * 16
    assert _lib.KERNEL_IDS[-2:] == ('bev_elev_bin', 'bev_elev_cells')
