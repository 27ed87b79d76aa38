"""pca_f32_box_decode on the host (no GPU): rows of pca_store.frame_box assembled in numpy from the documented encoding
(tests/cull_chain_common.py: upper bounds as an order-preserving code of the f32, lower bounds as its complement, 0 = nothing
yet) decode to the very bounds, bit for bit; the code is strictly monotone over the f32 line and never 0."""
import ctypes as C

import numpy as np

import cull_chain_common as cc

D, N = np.float32(1e-45), np.float32(1.17549435e-38)       # the smallest denormal, the smallest normal
EDGE_VALUES = np.array([0.0, -0.0, D, -D, np.float32(1e-39), np.float32(-1e-39), N, -N, 1.0, -1.0, 0.1, -0.1, 3.5e10, -7.25e-12,
                        1e35, -1e35, cc.FLT_MAX, -cc.FLT_MAX, np.inf, -np.inf], np.float32)


def decode(rows):
    from pca_amd import _lib
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 6)
    out = np.full((len(rows), 6), np.nan, np.float32)
    lib.pca_f32_box_decode(rows.ctypes.data_as(C.c_void_p), len(rows), out.ctypes.data_as(C.c_void_p))
    return out


def test_rows_built_from_the_documented_encoding_decode_to_their_bounds():
    v = EDGE_VALUES
    rows, want = [], []
    for i in range(len(v)):                                 # every value as lower and as upper bound, in every coordinate
        lo = np.array([v[i], v[(i + 3) % len(v)], v[(i + 7) % len(v)]], np.float32)
        hi = np.array([v[(i + 1) % len(v)], v[(i + 5) % len(v)], v[(i + 11) % len(v)]], np.float32)
        rows.append(cc.encode_box(lo, hi))
        want.append(np.stack([lo, hi], 1).ravel())
    got = decode(np.stack(rows))
    assert np.array_equal(got.view(np.uint32), np.stack(want).view(np.uint32))       # bit for bit: -0.0 stays -0.0, denormals stay


def test_a_row_of_zeros_decodes_as_unknown_coordinate_by_coordinate():
    got = decode(np.zeros((2, 6), np.uint32))
    assert (got[:, 0::2] > got[:, 1::2]).all()              # lo > hi
    row = cc.encode_box(np.array([-2., 0., 0.], np.float32), np.array([3., 0., 0.], np.float32))
    row[2:] = 0                                             # x known, y and z never written
    got = decode(row)[0]
    assert got[0] == -2. and got[1] == 3. and got[2] > got[3] and got[4] > got[5]


def test_the_code_is_monotone_and_never_zero():
    rng = np.random.default_rng(5)
    bits = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32), EDGE_VALUES.view(np.uint32)])
    v = bits.view(np.float32)
    v = np.unique(v[~np.isnan(v)].view(np.uint32)).view(np.float32)      # distinct bit patterns (-0.0 and +0.0 both stay)
    v = v[np.argsort(cc.total_order_key(v), kind='stable')]
    assert (np.diff(v.astype(np.float64)) >= 0).all()       # (sorted as numbers; -0.0 before +0.0)
    o = cc.ordered(v).astype(np.int64)
    assert (np.diff(o) > 0).all() and (o != 0).all() and ((~cc.ordered(v)) != 0).all()
    # and the library agrees with the restatement on all of them: decode(encode(v)) = v
    pad = (-len(v)) % 3
    w = np.concatenate([v, v[:pad]]).reshape(-1, 3)
    rows = np.zeros((len(w), 6), np.uint32)
    rows[:, 0::2], rows[:, 1::2] = ~cc.ordered(w), cc.ordered(w)
    got = decode(rows)
    assert np.array_equal(got[:, 0::2].view(np.uint32), w.view(np.uint32)) and np.array_equal(got[:, 1::2].view(np.uint32), w.view(np.uint32))


def test_the_expected_box_of_rows_takes_the_total_order():
    rows = np.zeros((4, 10))
    rows[:, 0] = np.array([0.0, -0.0, 0.0, 1e-45], np.float32)
    rows[:, 1] = np.array([-1.0, 2.5, -0.0, 1e35], np.float32)
    rows[:, 2] = np.float32(-3.25)
    box = cc.box_of_rows(rows)
    assert np.signbit(box[0]) and box[0] == 0 and box[1] == np.float32(1e-45)
    assert box[2] == -1. and box[3] == np.float32(1e35) and box[4] == box[5] == np.float32(-3.25)
    assert cc.box_of_rows(rows[:0]) is None
