"""WindowPart.frames(): the one place that maps a part's name and future_is_present to live-frame indices of the window's
store; to_numpy slices by it.  A stub store is enough: no device is touched."""
import numpy as np
import pytest

from bev_generator.bev_generator import DeviceWindow


class StubStore:
    n_frames = 7

    def frame_rows(self):
        """Frame k: k + 1 rows, x = y = z = 10 k, the frame's index in column 3."""
        rows = []
        for k in range(self.n_frames):
            f = np.zeros((k + 1, 10))
            f[:, 0:3], f[:, 3] = 10. * k, k
            rows.append(f)
        return rows


CASES = [  # (window's first, split, last), future_is_present -> frames of present, future, full
    ((0, 4, None), False, ((0, 4), (4, 7), (0, 7))),
    ((0, 4, None), True, ((0, 7), (0, 7), (0, 7))),
    ((2, 5, 6), False, ((2, 5), (5, 6), (2, 6))),
    ((2, 5, 6), True, ((2, 6), (2, 6), (2, 6))),
    ((1, 1, 3), False, ((1, 1), (1, 3), (1, 3))),                 # an empty present part
    ((3, 7, None), False, ((3, 7), (7, 7), (3, 7))),              # an empty future part
]


@pytest.mark.parametrize('bounds,all_sets,want', CASES)
def test_frames_and_to_numpy(bounds, all_sets, want):
    first, split, last = bounds
    origin = np.array([1., 2., 3.])
    win = DeviceWindow(StubStore(), split, origin, first=first, last=last, future_is_present=all_sets)
    for name, (lo, hi) in zip(('present', 'future', 'full'), want):
        part = win.part(name)
        assert part.frames() == (lo, hi)
        rows = part.to_numpy()
        assert rows.shape == (sum(k + 1 for k in range(lo, hi)), 10)
        assert rows[:, 3].tolist() == [k for k in range(lo, hi) for _ in range(k + 1)]   # exactly the frames [lo, hi), in order
        assert np.array_equal(rows[:, 0:3], 10. * rows[:, 3:4] - origin)                 # minus the window's origin


def test_an_unknown_part_name_is_a_key_error():
    for all_sets in (False, True):
        with pytest.raises(KeyError):
            DeviceWindow(StubStore(), 3, np.zeros(3), future_is_present=all_sets).part('past').frames()
