"""CPU: the numpy model of the camera render (tests/render_camera_common.py) tied to the oracle's projection, which is pinned
to the reference (tests/test_k1_edges_golden.py), and a hand-made image that pins the z-buffer's rules."""
from fractions import Fraction

import numpy as np
import pytest

import k1_edges_common as kc
import render_camera_common as rcc
from oracle import oracle as orc


@pytest.mark.parametrize('name', kc.CASES)
def test_kept_set_and_pixels_equal_the_oracle(name):
    """The frustum-edge frames of K1 (f32-valued points: planes, ladders, specials): the model keeps the points the oracle's
    velo2img keeps and puts them into the same pixels."""
    fr = kc.frame(name)
    pts, P, H, W, _, _ = fr.case()
    img, sem = fr.images()
    st = orc.Store(len(pts))
    m, mask, u, v = orc.kitti_project_sample_filter(st, pts, P, img, sem, None, H, W, [], want_uv=True)
    rows = np.zeros((len(pts), 10))
    rows[:, :3] = pts[:, :3].astype(np.float64)
    kept, mu, mv, _ = rcc.pixels(rows, P, W, H)
    assert m == int(mask.sum()) > 1000
    assert np.array_equal(kept, mask)
    assert np.array_equal(mu[kept], u[mask]) and np.array_equal(mv[kept], v[mask])


def _row(x, y, z, r, g, b, cls, dyn=0):
    return [x, y, z, 0., r, g, b, cls, 0., dyn]


# u = round(x / z), v = round(y / z), d = z
P_UNIT = np.array([[1., 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
FIVE = [np.array([_row(4., 2., 2., 10, 11, 12, 1),               # 0: pixel (u 2, v 1), the bottom right corner, d = 2
                  _row(4., 2., 2., 20, 21, 22, 2)]),             # 1: the same pixel at the same depth: loses to 0
        np.array([_row(0., 0., 4., 30, 31, 32, 3),               # 2: pixel (0, 0), d = 4
                  _row(0., 0., 3., 40, 41, 42, 4, dyn=1),        # 3: pixel (0, 0), d = 3: nearer than 2
                  _row(3., 0., 1., 50, 51, 52, 5)])]             # 4: u = 3, one column outside, the nearest of all: takes no part


def test_five_points_in_a_3_x_2_image():
    W, H = 3, 2
    got = rcc.model(FIVE, P_UNIT, W, H)
    assert got['stats'].tolist() == [5, 4, 2] and got['ties'] == 1 and got['most'] == 2
    assert got['depth'].dtype == np.float32 and got['depth'].tolist() == [[3., 0., 0.], [0., 0., 2.]]
    assert got['index'].tolist() == [[3, -1, -1], [-1, -1, 0]]                      # of equal depths the smallest index
    assert got['sem'].tolist() == [[4, 255, 255], [255, 255, 1]]
    assert got['rgb'][0, 0].tolist() == [40, 41, 42] and got['rgb'][1, 2].tolist() == [10, 11, 12]
    assert not got['rgb'][0, 1:].any() and not got['rgb'][1, :2].any()              # an empty pixel: 0, 0, 0 and class 255
    # radius 1: the corner point's footprint is clipped to 2 x 2 pixels, not wrapped into the next row (pixel (0, 1) would
    # take its depth 2); where the two footprints meet the nearer point wins; point 4 stays out although its footprint
    # would reach column 2
    got = rcc.model(FIVE, P_UNIT, W, H, radius=1)
    assert got['stats'].tolist() == [5, 4, 6]
    assert got['depth'].tolist() == [[3., 2., 2.], [3., 2., 2.]]
    assert got['index'].tolist() == [[3, 0, 0], [3, 0, 0]]
    # without the dynamic point the farther one shows; a class set; a depth range (open at both ends)
    got = rcc.model(FIVE, P_UNIT, W, H, include_dyn=False)
    assert got['stats'].tolist() == [4, 3, 2] and got['index'].tolist() == [[2, -1, -1], [-1, -1, 0]]
    got = rcc.model(FIVE, P_UNIT, W, H, classes=[2, 3, 5])
    assert got['stats'].tolist() == [3, 2, 2] and got['index'].tolist() == [[2, -1, -1], [-1, -1, 1]]
    got = rcc.model(FIVE, P_UNIT, W, H, depth_range=(2., 4.))
    assert got['stats'].tolist() == [5, 1, 1] and got['index'].tolist() == [[3, -1, -1], [-1, -1, -1]]
    # a window cut after three points
    got = rcc.model(FIVE, P_UNIT, W, H, max_points=3)
    assert got['stats'].tolist() == [3, 3, 2] and got['index'].tolist() == [[2, -1, -1], [-1, -1, 0]]
    want = rcc.empty(W, H)
    got = rcc.model(FIVE, P_UNIT, W, H, classes=[])
    assert all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want)


def test_exact_fma_chain_and_the_zero_depth_rule():
    """The chain is fused: a product that the unfused sum would round away survives; d == 0 becomes -1e-6 and drops the point."""
    e = 2.0 ** -30
    assert rcc.row4([-1., 1 + e, 0., 0.], 1., 1 - e, 0.) == -e * e            # -1 + (1 + e)(1 - e), rounded once: -2^-60
    assert -1. + (1 + e) * (1 - e) == 0.                                      # (unfused, the product rounds to 1)
    rng = np.random.default_rng(3)
    for a, b, c in rng.standard_normal((2000, 3)) * 10.0 ** rng.integers(-20, 20, (2000, 3)):
        assert rcc._fma(a, b, c) == float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
    rows = np.array([_row(0., 0., 0., 1, 1, 1, 1), _row(np.nan, 0., 1., 1, 1, 1, 1), _row(0., np.inf, 1., 1, 1, 1, 1)])
    kept, _, _, d = rcc.pixels(rows, P_UNIT, 3, 2)
    assert not kept.any() and d[0] == -1e-6
