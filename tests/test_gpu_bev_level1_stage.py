"""The tile kernel of the BEV rasteriser without a heavy kernel behind it (the previous calls saw no heavy tile, so the host
launches none): a tile above heavy_min is worked off by the workgroup that finds it, which also tells the host, and no
workgroup counts the others to find the kernel's last.  The 21 planes against the ORACLE (intensity within
assert_planes_match's tolerance, everything else bit for bit), and the launch structure of the call after."""
import numpy as np
import pytest

from test_gpu_kernels import DYNOBJ, T, _skewed_rows, assert_planes_match, dev_store, orc, run_dev_bev, run_orc_bev  # noqa: F401

pytestmark = pytest.mark.gpu

VIEW, INTS = 32., (1., 30., 0.12)


def tile_xy(rng, n, r, c, px):
    """n points inside tile (r, c) of the px grid (8 x 8 cells; row 0 is the top: y runs against the rows)."""
    cell = VIEW / px
    x0, y0 = (8 * c - px / 2) * cell, (px - 8 * r - 8 - px / 2) * cell
    return np.stack([rng.uniform(x0 + 0.01 * cell, x0 + 7.99 * cell, n), rng.uniform(y0 + 0.01 * cell, y0 + 7.99 * cell, n)], 1)


def make_rows(rng, xy, f64_intensity=False):
    n = len(xy)
    rows = np.zeros((n, 10))
    rows[:, :2] = xy
    rows[:, 2] = rng.uniform(-1, 2, n)
    rows[:, 3] = rng.random(n) if f64_intensity else rng.integers(0, 256, n) / 255.
    rows[:, 4:7] = rng.integers(0, 256, (n, 3))
    rows[:, 7] = rng.choice([0, 2, 13], n)
    return rows


def cool_down(T):
    """A context without a heavy launch behind its tile kernel: 70 sparse rasters (the cooldown is 64 calls)."""
    sparse = _skewed_rows(np.random.default_rng(5), 2000, 6.0, 8)
    for _ in range(70):
        run_dev_bev(T, sparse[:800], sparse[800:], VIEW, 64, None, INTS, True, 0.2)


@pytest.mark.parametrize('intensity', ['f32', 'f64'])
def test_heavy_tiles_without_a_heavy_launch_are_worked_off_where_they_are_found(T, orc, intensity):
    """No heavy kernel behind the tile kernel (cooled context), three tiles of 2 561, 3 000 and 5 000 records among sparse ones:
    each is worked off by the workgroup that found it, and the host is told -- the NEXT call of the same raster goes through the
    heavy kernel.  Both equal the oracle.  f64: intensities the store's f32 cannot hold (24-byte records, the other
    instantiation of the tile kernel)."""
    from pca_amd import host_logic as hl
    from pca_amd.device_store import make_bev_params
    px = 64
    rng = np.random.default_rng(2561)
    heavy = {(1, 2): 2561, (4, 4): 3000, (6, 1): 5000}
    xy = [tile_xy(rng, heavy.get((r, c), 20), r, c, px) for r in range(px // 8) for c in range(px // 8)]
    rows = make_rows(rng, np.concatenate(xy), intensity == 'f64')
    rows = rows[rng.permutation(len(rows))]
    cut = int(0.4 * len(rows))
    div255 = intensity == 'f32'                              # (f64: the values as they are, through the side channel)
    if div255:
        ref = run_orc_bev(orc, rows[:cut], rows[cut:], VIEW, px, None, INTS, True, 0.0)
    else:
        oprm = orc.make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.0), 0., 0., VIEW, px, None, *INTS, 0, DYNOBJ, False)
        ref = orc.bev(orc.Store.from_rows(rows), cut, oprm, intensity64=rows[:, 3])
    cool_down(T)
    st = dev_store(capacity=len(rows), max_frames=4, intensity_div255=div255)
    i64 = st.load_rows([rows[:cut], rows[cut:]])
    assert (i64 is None) == (intensity == 'f32')
    prm = make_bev_params((0., 0., 0.), hl.rotation_matrix_3d(0.0), 0., 0., VIEW, px, None, *INTS, 0, DYNOBJ, div255)
    counts = []
    for which in ('worked off by the light kernel', 'heavy kernel'):
        st.ctx.profile(True)
        p16, p64 = st.bev(1, prm, want_f64=True, intensity64=i64)
        counts.append(st.ctx.profile_read()['bev_cells_heavy'][1])
        st.ctx.profile(False)
        st.check_status()
        assert_planes_match(p16.cpu().numpy(), p64.cpu().numpy(), ref, which)
    assert counts[0] == 0 and counts[1] >= 1, counts
