"""What the frame-culling tests share (tests/test_gpu_cull_chain.py on the GPU, tests/test_box_encoding.py without one): the
documented encoding of pca_store.frame_box restated in numpy, the expected box of a set of kept rows, the synthetic K1 frames
and the rows of the bin-range window.  CPU only, numpy only, deterministic."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


# ---- the box encoding (include/pca.h, pca_store.frame_box) ----------------------------------------------------------------
def ordered(v):
    """f32 -> u32, order-preserving and never 0 for a number: sign bit set -> all bits flipped, else the sign bit set."""
    u = np.asarray(v, np.float32).view(np.uint32)
    return u ^ np.where(u >> 31 != 0, np.uint32(0xffffffff), np.uint32(0x80000000))


def encode_box(lo, hi):
    """The six words of a row whose lower / upper bounds are lo[3] / hi[3]: word 2k = ~ordered(lo k), word 2k+1 = ordered(hi k)."""
    row = np.zeros(6, np.uint32)
    row[0::2] = ~ordered(lo)
    row[1::2] = ordered(hi)
    return row


def total_order_key(v):
    """IEEE totalOrder of f32 values as int64 keys (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN), written without the
    encoding above: sign-magnitude to two's complement."""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.int64)
    mag = b & 0x7fffffff
    return np.where(b >> 31 != 0, -mag - 1, mag)


def box_of_rows(rows):
    """[lo x, hi x, lo y, hi y, lo z, hi z] (f32) of the kept rows of one frame, or None if there are none.  K1 stores a kept
    point's f32 coordinates as f64, so the cast back is exact.  Minimum and maximum are taken in IEEE total order: for columns
    without NaN that is numpy's min / max (asserted), with -0.0 below +0.0; a NaN kept under per-point labels is the extreme of
    its sign."""
    if len(rows) == 0:
        return None
    out = np.empty(6, np.float32)
    for k in range(3):
        col64 = np.asarray(rows)[:, k]
        col = col64.astype(np.float32)
        assert np.array_equal(col.astype(np.float64).view(np.uint64), np.ascontiguousarray(col64).view(np.uint64))
        key = total_order_key(col)
        out[2 * k], out[2 * k + 1] = col[np.argmin(key)], col[np.argmax(key)]
        if not np.isnan(col).any():
            assert out[2 * k] == col.min() and out[2 * k + 1] == col.max()
    return out


# ---- synthetic K1 frames --------------------------------------------------------------------------------------------------
P_AXIS = np.array([[8., 0, 48, 0], [0, 8, 32, 0], [0, 0, 1, 0]])                 # looks along +z (the 'axis' camera of k1_edges_common)
P_BACK = P_AXIS @ np.diag([-1., -1., -1., 1.])                                    # the same camera looking along -z, x and y mirrored
SYN_H, SYN_W = 64, 96
SYNTHETIC = ('none_kept', 'one_kept', 'all_negative', 'zeros_denormals', 'huge')


def synthetic_frame(name):
    """(pts f32 [n,4], P, sem_gt | None): frames of 2 tiles and a partial one (2500 points).  sem_gt given: the per-point-label
    form (no projection: every point whose class passes is kept)."""
    rng = np.random.default_rng(SYNTHETIC.index(name) + 700)
    n = 2500
    pts = np.zeros((n, 4), np.float32)
    pts[:, 3] = rng.integers(0, 256, n) / np.float32(256.)
    if name in ('none_kept', 'one_kept'):                                         # everything behind the camera
        pts[:, 0:2], pts[:, 2] = rng.uniform(-20, 20, (n, 2)), rng.uniform(-30, -1, n)
        if name == 'one_kept':
            pts[1500, :3] = (0.5, -0.25, 7.)                                      # (in the second tile)
        return pts, P_AXIS, None
    if name == 'all_negative':
        pts[:, 0:2], pts[:, 2] = rng.uniform(-3, -0.1, (n, 2)), rng.uniform(-30, -5, n)
        return pts, P_BACK, None
    if name == 'zeros_denormals':
        d = np.float32(1e-45)
        pts[:, 0] = rng.choice(np.array([-0.0, 0.0, d], np.float32), n)           # lo -0.0 (below +0.0), hi a denormal
        pts[:, 1] = rng.choice(np.array([-d, -0.0, -1e-39], np.float32), n)       # lo -1e-39 (a denormal), hi -0.0
        pts[:, 2] = np.float32(-0.0)                                              # lo = hi = -0.0
        return pts, P_AXIS, rng.integers(0, 19, n).astype(np.uint8)
    assert name == 'huge'                                                         # directions inside the image at 1e35
    uv = np.stack([rng.uniform(2, SYN_W - 3, n), rng.uniform(2, SYN_H - 3, n)], 1)
    z = (1e35 * rng.uniform(1., 3., n))
    pts[:, 0], pts[:, 1], pts[:, 2] = (uv[:, 0] - 48) / 8 * z, (uv[:, 1] - 32) / 8 * z, z
    pts[::7, :3] = rng.uniform(-5, 5, (len(pts[::7]), 3))                         # ordinary points in between
    return pts, P_AXIS, None


def synthetic_images(name):
    rng = np.random.default_rng(SYNTHETIC.index(name) + 900)
    return rng.integers(0, 256, (SYN_H, SYN_W, 3), dtype=np.uint8), rng.integers(0, 10, (SYN_H, SYN_W)).astype(np.uint8)


# ---- the window of the bin-range cases ------------------------------------------------------------------------------------
def skewed_rows(rng, n, sigma=1.5, colour_spread=8):
    """Rows in the style of test_gpu_kernels._skewed_rows: clustered around a driven path, all inside a 32 m view."""
    rows = np.zeros((n, 10))
    rows[:, 0] = rng.uniform(-15.9, 15.9, n)
    rows[:, 1] = np.clip(rng.normal(0, sigma, n), -15.9, 15.9)
    rows[:, 2] = rng.uniform(-1, 2, n)
    rows[:, 3] = rng.integers(0, 256, n) / 255.
    base = rng.integers(0, 256, 3)
    rows[:, 4:7] = np.clip(base + rng.integers(-colour_spread, colour_spread + 1, (n, 3)), 0, 255)
    rows[:, 7] = rng.choice([0, 1, 2, 13], n, p=[0.6, 0.2, 0.15, 0.05])
    rows[:, 9] = rng.random(n) < 0.02
    return rows


def window_frames(n_frames=8, base=2800, step=150, seed=2024):
    """F frames of about 3000 points (2800, 2950, ...: no two alike, none a multiple of a tile), every one inside the view."""
    rng = np.random.default_rng(seed)
    return [skewed_rows(rng, base + step * f) for f in range(n_frames)]
