"""Pins the CPU oracle's K1 against the reference on the frustum-edge frames (tests/golden/k1_edges_<camera>.npz: the frames
of k1_edges_common.py run through the reference's velo2img / gen_semantic_pc / filter_semseg_pc), and holds the frames to
what they are meant to contain."""
import numpy as np
import pytest

import k1_edges_common as kc
from oracle import oracle as orc

# Points kept / dropped by the oracle that every plane family (its -3 .. +3 neighbour points) and every ladder rung must hold.
FLOOR = 200
# One family cannot reach it.  A point next to d = 0 is inside the image only next to the camera centre, and KITTI's centre
# (0.80, 0.30, -0.18) has few f32 neighbours: a cone of half-angles 52 and 19 degrees up to 3 steps of x (6e-8 each) holds about
# 1/3 x 3.5 x (2 x 1.27 x 3.5 x 2 ulps of y) x (0.68 x 3.5 x 4 ulps of z) = 200 lattice points.  The family takes every column of the
# lattice with a point inside the image (test_d0_family_holds_the_whole_lattice_next_to_the_centre), which is all there are: 198.
KEPT_FLOOR = {('kitti', 'd0'): 198}
# Ladder rungs: all of a rung's 330 points are inside the image, FLOOR of them also pass the class filter -- but for the 1 x 2 image,
# one of whose two pixels holds a filtered class: half of its rung, 155 on its thinnest rung.
FILTERED_FLOOR = {'tiny': 155}


@pytest.fixture(scope='module', params=kc.CASES)
def case(request):
    """(frame, fixture, the oracle's outputs without and with the class filter): computed once per camera."""
    fr, g = kc.frame(request.param), kc.fixture(request.param)
    pts, P, H, W, filters, seed = fr.case()
    img, sem = fr.images()
    st = orc.Store(len(pts))
    m, mask, u, v = orc.kitti_project_sample_filter(st, pts, P, img, sem, None, H, W, [], want_uv=True)
    stf = orc.Store(len(pts))
    orc.kitti_project_sample_filter(stf, pts, P, img, sem, None, H, W, filters)
    return fr, g, (mask, u, v, st.rows(), stf.rows())


def test_fixture_holds_the_generated_points(case):
    fr, g, _ = case
    assert np.array_equal(g['pts'].view(np.uint32), fr.pts.view(np.uint32))


def test_oracle_matches_the_reference_bit_for_bit(case):
    fr, g, (mask, u, v, rows, rows_f) = case
    img, sem = fr.images()
    assert np.array_equal(mask, g['mask'])
    assert np.array_equal(u[mask], g['u'].astype(np.int64)) and np.array_equal(v[mask], g['v'].astype(np.int64))

    def want_rows(idx):
        """The reference's rows of the points idx: x, y, z, intensity, the pixel's colour and class."""
        where = np.searchsorted(np.flatnonzero(g['mask']), idx)
        uu, vv = g['u'][where].astype(int), g['v'][where].astype(int)
        return np.concatenate([fr.pts[idx].astype(np.float64), img[vv, uu].astype(np.float64), sem[vv, uu, None].astype(np.float64)], 1)
    assert np.array_equal(rows[:, :8], want_rows(np.flatnonzero(g['mask'])))
    assert np.array_equal(rows_f[:, :8], want_rows(g['kept'].astype(np.int64)))
    assert not np.isin(rows_f[:, 7], fr.filters).any() and len(rows_f) < len(rows)
    assert np.isfinite(rows).all()                     # the reference drops NaN and inf: kept points are finite


def test_families_hold_enough_points_on_either_side(case):
    fr, g, (mask, _, _, _, _) = case
    kept_f = np.zeros(len(mask), bool)
    kept_f[g['kept']] = True
    for plane in kc.PLANES:
        i = fr.of(plane)
        kept, dropped = int(mask[i].sum()), int((~mask[i]).sum())
        print(fr.name, plane, 'kept', kept, 'dropped', dropped)
        assert kept >= KEPT_FLOOR.get((fr.name, plane), FLOOR) and dropped >= FLOOR, (fr.name, plane, kept, dropped)
    for e in kc.RUNGS:
        i = fr.of(f'ladder_e{e}')
        print(fr.name, e, 'kept', int(kept_f[i].sum()), 'of', len(i))
        assert mask[i].all() and len(i) >= FLOOR and kept_f[i].sum() >= FILTERED_FLOOR.get(fr.name, FLOOR), (fr.name, e)
        big = np.abs(fr.pts[i, :3]).max(1).astype(np.float64)
        assert (big >= 10.0**e * 0.999).all() or e == 38
        assert (big <= kc.FLT_MAX).all() and np.isfinite(fr.pts[i]).all()
    assert (np.abs(fr.pts[fr.of('ladder_e38'), :3]).max(1) == np.float32(kc.FLT_MAX)).sum() >= 50          # the cap itself
    for fam in kc.OVERFLOWS:
        assert mask[fr.of(fam)].all()
    sp = fr.pts[fr.of('specials'), :3]
    for j in range(3):
        col = sp[:, j]
        assert np.isposinf(col).any() and np.isneginf(col).any() and np.isnan(col).any()
        assert ((col == 0) & np.signbit(col)).any() and (col == np.float32(kc.FLT_MAX)).any()
        assert ((col != 0) & (np.abs(col) < np.finfo(np.float32).tiny)).any()
    assert (~sp.any(1) & ~np.signbit(sp).any(1)).any()                    # the all-zero point


def test_overflow_families_exist_somewhere():
    """Only d, only fx, only fy beyond FLT_MAX: not every camera has such a direction, each kind is there at two or more."""
    for fam in kc.OVERFLOWS:
        assert sum(len(kc.frame(c).of(fam)) >= 20 for c in kc.CASES) >= 2, fam


def test_d0_family_holds_the_whole_lattice_next_to_the_centre():
    """KITTI: every point of the f32 lattice within 12 steps of the camera centre in y and z and within 3 steps of d = 0 in x
    that the generator's own projection puts inside the image is in the d0 family."""
    fr = kc.frame('kitti')
    P, H, W = fr.P, fr.H, fr.W
    C = (-np.linalg.solve(P[:, :3], P[:, 3])).astype(np.float32)
    ab = np.array([(a, b) for a in range(-12, 13) for b in range(-12, 13)])
    base = np.repeat(C[None], len(ab), 0)
    base[:, 1] = [kc.stepped(C[1:2], a)[0] for a, _ in ab]
    base[:, 2] = [kc.stepped(C[2:3], b)[0] for _, b in ab]
    base, j = kc._solve_on_plane(P[2], base)
    assert j == 0
    pts = kc._with_steps(base, 0)
    inside = pts[kc.project(P, pts, H, W)]
    have = {p.tobytes() for p in fr.pts[fr.of('d0'), :3]}
    assert len(inside) >= 150 and all(p.tobytes() in have for p in inside)


def test_placement():
    """Edge points at the lanes, packed-pair halves and tile edges of every tile shape; the frame's last point re-read by idle lanes."""
    for name in kc.CASES:
        fr = kc.frame(name)
        n = len(fr.pts)
        hot = kc.hot_slots(n)
        assert (fr.fam[hot] != kc.FILLER).all()
        for blk, ppt in kc.TILE_SHAPES:
            tile = blk * ppt
            assert n % tile and n % blk
            for t0 in range(0, n, tile):
                k = 2 * ((t0 // tile) % 2)
                for s in (t0, t0 + k * blk + 63, t0 + k * blk + blk - 1, t0 + (k + 1) * blk, t0 + (k + 1) * blk + 63, t0 + tile - 1):
                    assert s >= n - 1 or fr.fam[s] != kc.FILLER, (name, blk, s)
        assert fr.fam[n - 1] == kc.FAMILIES.index('ladder_e36') and kc.fixture(name)['mask'][n - 1]
        wrongly = [f for f in ('ladder_e36', 'ladder_e38') if (fr.fam[hot] == kc.FAMILIES.index(f)).sum() >= 8]
        assert len(wrongly) == 2
        # a plane family lies across a boundary of every tile size
        for fam in kc.PLANES:
            i = fr.of(fam)
            body = i[(i >= 700)]
            assert any(body.min() < b <= body.max() for b in range(4096, n, 4096)) or any(
                body.min() < b <= body.max() for b in range(1024, n, 1024)), (name, fam)
