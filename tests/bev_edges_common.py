"""The BEV edge fixtures (tests/golden/bev_edges_*.npz, made by tools/make_golden.py --only bev_edges): which files there
are, and one stored case (inputs, parameters, the reference's planes) behind the key names of the bev_a..e fixtures."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# file (without the bev_edges_ prefix) -> cases stored in it (keys k<n>_...)
EDGE_FILES = {f'lattice_{c}_r{r}': 2 for c in ('kitti', 'nusc', 'px30', 'px7') for r in range(5)}
EDGE_FILES.update({'counts': 1, 'intensity_kitti': 1, 'intensity_nusc': 1, 'empty_sets': 3})
EDGE_CASES = [f'{name}/k{k}' for name, n in EDGE_FILES.items() for k in range(n)]

_cache = {}


class EdgeCase:
    """g[key] / key in g as for a bev_a..e fixture; the case's parameters as attributes."""

    def __init__(self, case):
        name, self.pfx = case.split('/')
        if name not in _cache:
            with np.load(os.path.join(GOLDEN, f'bev_edges_{name}.npz'), allow_pickle=False) as f:
                _cache[name] = {k: f[k] for k in f.files}
        self.file = _cache[name]
        assert int(self.file['n_cases']) == EDGE_FILES[name]
        self.name = case
        c = self['cfg']
        self.view, self.px = float(c[0]), int(c[1])
        self.hf = None if np.isnan(c[2]) else float(c[2])
        self.ints = (float(c[3]), float(c[4]), float(c[5]))
        self.div255 = bool(c[6])
        self.rot, self.dx, self.dy, self.zoom = (float(v) for v in c[7:11])

    def __getitem__(self, key):
        return self.file[f'{self.pfx}_{key}']

    def __contains__(self, key):
        return f'{self.pfx}_{key}' in self.file
