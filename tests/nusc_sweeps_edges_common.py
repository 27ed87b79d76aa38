"""Edge cases of the NuScenes sweep merger, shared by tools/make_golden.py (case_sweeps_edges runs the REFERENCE's
inst_centric_get_sweeps on them -> tests/golden/nusc_sweeps_edges.npz) and the tests of the host and the device form.

Two scenarios on tests/fake_nuscenes.py tables (only numpy and fake_nuscenes are imported here: the generator also runs
where `datasets` is the reference's package):

  'a'  synth_tables(seed, 3, 3000), three sweeps, rows of every record overwritten with
         * points ON BOX FACES: for the boxes of instances 0 and 1, every axis and sign, 12 points whose box coordinate
           on that axis is +-inside_limit * size, pushed back to raw sweep coordinates, each stored with its -3..+3 f32
           neighbours along the raw coordinate that moves the box coordinate most (2 x 3 x 2 x 12 x 7 = 1008 rows);
         * points ON THE center_radius CIRCLE: 60 angles, half of them on radius 2 (1 + 2^-22), each with the -3..+3 f32
           neighbours of x (420 rows);
  'b'  synth_tables(seed + 1, 4, 600), four sweeps: a record whose file is empty, a sweep without candidate box, sweeps of
       exactly 512, 511 and 513 kept points, face points in lanes 0 and 63 and in the first and last row of a tile, points
       inside two overlapping boxes, a track whose first candidate box has no point but whose later one has.
"""
import numpy as np

import fake_nuscenes as fk

SEED = 23
CENTER_RADIUS = 2.0
INSIDE_LIMIT = 0.5 + 5e-2
FACE_ROW0, N_FACE = 100, 1008                 # scenario a: rows of the face points of every record
CIRCLE_ROW0, N_CIRCLE = 1200, 420             # ... and of the circle points
SCENARIOS = {'a': dict(n_sweeps=3), 'b': dict(n_sweeps=4)}
KEPT_B = (0, 512, 511, 513)                   # scenario b: kept points per record
PLANT_ROWS_B = (0, 63, 64, 255, 256, 319, 511, 512, 575, 599, 1, 62, 510, 513)


def cfg(scenario):
    return dict(fk.SWEEP_CFG, **SCENARIOS[scenario])


def _rigid(t, q):
    T = np.eye(4)
    T[:3, :3] = fk.FakeQuaternion(q).rotation_matrix
    T[:3, 3] = t
    return T


def _sensor(t, k):
    return _rigid(t['ego_t'][k], t['ego_q'][k]) @ _rigid(t['cs_t'][k], t['cs_q'][k])


def _box_from_sweep(t, k, b):
    """box frame <- raw sweep coordinates of record k (4x4), and the box's (l, w, h)"""
    box_in_glob = _rigid(t['box_center'][b], t['box_q'][b])
    wlh = t['box_wlh'][b]
    return np.linalg.inv(box_in_glob) @ _sensor(t, k), np.array([wlh[1], wlh[0], wlh[2]])


def _box_of(t, k, inst):
    return int(np.nonzero((t['box_record'] == k) & (t['box_instance'] == inst))[0][0])


def face_points(t, k, inst, rng, per_face=12):
    """(6 * per_face * 7, 3) f32 raw points of record k around the faces of the box of `inst`"""
    M, size = _box_from_sweep(t, k, _box_of(t, k, inst))
    Minv = np.linalg.inv(M)
    out = []
    for axis in range(3):
        coord = int(np.argmax(np.abs(M[axis, :3])))          # the raw coordinate that moves this box coordinate most
        for sign in (-1.0, 1.0):
            for _ in range(per_face):
                local = rng.uniform(-0.4, 0.4, 3) * size
                local[axis] = sign * INSIDE_LIMIT * size[axis]
                p = (Minv @ np.append(local, 1.0))[:3].astype(np.float32)
                for step in range(-3, 4):
                    q = p.copy()
                    for _ in range(abs(step)):
                        q[coord] = np.nextafter(q[coord], np.float32(np.inf if step > 0 else -np.inf))
                    out.append(q)
    return np.stack(out)


def circle_points(rng, n_angles=60):
    out = []
    for j in range(n_angles):
        ang = rng.uniform(0, 2 * np.pi)
        r = CENTER_RADIUS * (1 + 2.0 ** -22) if j % 2 else CENTER_RADIUS
        p = np.array([r * np.cos(ang), r * np.sin(ang), rng.uniform(-2, 2)]).astype(np.float32)
        for step in range(-3, 4):
            q = p.copy()
            for _ in range(abs(step)):
                q[0] = np.nextafter(q[0], np.float32(np.inf if step > 0 else -np.inf))
            out.append(q)
    return np.stack(out)


def _ragged(t):
    t['points'] = [np.ascontiguousarray(p, dtype=np.float32) for p in t['points']]
    for p in t['points']:
        p[:, 4] = 0.0                                        # never read by the merger (and it keeps the fixture small)
    return t


def tables_a():
    t = fk.synth_tables(SEED, 3, 3000)
    rng = np.random.default_rng(SEED + 100)
    for k in range(3):
        face = np.concatenate([face_points(t, k, inst, rng) for inst in (0, 1)])
        assert face.shape[0] == N_FACE
        t['points'][k, FACE_ROW0:FACE_ROW0 + N_FACE, :3] = face
        t['points'][k, CIRCLE_ROW0:CIRCLE_ROW0 + N_CIRCLE, :3] = circle_points(rng)
    return _ragged(t)


def tables_b():
    t = fk.synth_tables(SEED + 1, 4, 600)
    rng = np.random.default_rng(SEED + 200)
    t['points'][:, :, :2] = rng.uniform(5, 30, (4, 600, 2)) * rng.choice([-1.0, 1.0], (4, 600, 2))   # all outside the radius
    t['points'][:, :, 2] = 20.0                              # ... and above every box: only planted points get labels
    t['box_lidar_pts'][t['box_record'] == 1] = 0             # the sweep of record 1 has no candidate box
    for k in (1, 2, 3):
        drop = 600 - KEPT_B[k]
        rows = np.arange(100, 100 + drop)                    # next to the sensor axis: dropped
        t['points'][k, rows, :2] = rng.uniform(-1.0, 1.0, (drop, 2))
    for k in (2, 3):
        face = face_points(t, k, 1, rng, per_face=1)         # 42 rows around the faces of the truck
        for j, row in enumerate(PLANT_ROWS_B):
            t['points'][k, row, :3] = face[(3 * j) % face.shape[0]]
        M, _ = _box_from_sweep(t, k, _box_of(t, k, 0))       # the car's centre lies inside the bus as well
        centre = (np.linalg.inv(M) @ np.array([0.1, 0.1, 0.1, 1.0]))[:3]
        t['points'][k, 300:304, :3] = centre + rng.uniform(-0.05, 0.05, (4, 3))
    M, _ = _box_from_sweep(t, 3, _box_of(t, 3, 2))           # the pedestrian: no point in record 2, one in record 3
    t['points'][3, 320, :3] = (np.linalg.inv(M) @ np.array([0.0, 0.0, 0.0, 1.0]))[:3]
    t = _ragged(t)
    t['points'][0] = np.zeros((0, 5), np.float32)            # the file of record 0 is empty
    return t


TABLES = {'a': tables_a, 'b': tables_b}
OUT_KEYS = ('points', 'instances_token', 'instances_center', 'instances_last_box', 'instances_name')


def store_tables(out, scenario, t):
    """the tables of a scenario as npz entries (the point files one entry each: their lengths differ)"""
    for key, v in t.items():
        if key == 'points':
            for k, p in enumerate(v):
                out[f'{scenario}_in_points_{k}'] = p
        else:
            out[f'{scenario}_in_{key}'] = np.asarray(v)


def load_tables(g, scenario):
    pre = scenario + '_in_'
    t = {key[len(pre):]: g[key] for key in g.files if key.startswith(pre) and not key.startswith(pre + 'points_')}
    t['points'] = [g[f'{pre}points_{k}'] for k in range(int(t['n_records']))]
    return t


def expected(g, scenario):
    return {key: g[f'{scenario}_{key}'] for key in OUT_KEYS}


def kept_mask(raw_xy):
    """which raw rows survive the radius filter, exactly as the merger decides it (un-fused f32)"""
    x, y = raw_xy[:, 0].astype(np.float32), raw_xy[:, 1].astype(np.float32)
    return np.sqrt(x * x + y * y) > np.float32(CENTER_RADIUS)


def coverage_a(t, points):
    """per record of scenario a: (face points labelled, face points unlabelled, circle points kept, circle points dropped),
    read off the merged rows `points` (sweep k = record k)"""
    out = []
    for k in range(3):
        raw = t['points'][k]
        keep = kept_mask(raw[:, :2])
        rows = points[points[:, 5] == k]
        assert rows.shape[0] == keep.sum()
        pos = np.cumsum(keep) - 1                            # raw row -> merged row of the sweep
        face = np.arange(FACE_ROW0, FACE_ROW0 + N_FACE)
        assert keep[face].all()
        lab = rows[pos[face], 6] >= 0
        circ = keep[CIRCLE_ROW0:CIRCLE_ROW0 + N_CIRCLE]
        out.append((int(lab.sum()), int((~lab).sum()), int(circ.sum()), int((~circ).sum())))
    return out


def contract_model(inputs, center_radius, in_box_tolerance, chain):
    """The device contract (include/pca.h, pca_nusc_merge_sweeps) evaluated with numpy: `chain(T, pts)` is the f64 FMA chain
    in k order (oracle.homo_transform).  Returns (points, tokens, centres)."""
    limit = 0.5 + in_box_tolerance
    cand, clouds = [], []                                    # cand: (sweep position, box dict, hits)
    for sw in inputs['sweeps']:
        raw = sw['raw']
        x, y = raw[:, 0], raw[:, 1]
        keep = np.sqrt(x * x + y * y) > np.float32(center_radius)
        pts = np.full((raw.shape[0], 8), -1.0, np.float32)
        pts[:, :3] = chain(sw['target_from_sweep'], raw[:, :3].astype(np.float64)).astype(np.float32)
        pts[:, 3], pts[:, 4], pts[:, 5] = raw[:, 3], np.float32(sw['lag']), np.float32(sw['sweep'])
        pts = pts[keep]
        last = np.full(pts.shape[0], -1)
        for box in sw['boxes']:
            local = chain(np.linalg.inv(box['target_from_box']), pts[:, :3].astype(np.float64))
            with np.errstate(all='ignore'):
                inside = np.all(np.abs(local / box['size']) < limit, axis=1)
            last[inside] = len(cand)
            cand.append((box, int(inside.sum())))
        clouds.append((pts, last))
    # box b opens a track iff it has a hit and no earlier box of its token has; tracks count up in box order
    track, tokens, centres = {}, [], []
    for box, hits in cand:
        if hits > 0:
            track.setdefault(box['instance_token'], len(track))
            tokens.append(box['instance_token'])
            centres.append(box['center'])
    for pts, last in clouds:
        for j in np.nonzero(last >= 0)[0]:
            box = cand[last[j]][0]
            pts[j, 6], pts[j, 7] = track[box['instance_token']], box['cls']
    points = np.concatenate([p for p, _ in clouds], axis=0) if clouds else np.zeros((0, 8), np.float32)
    return points, tokens, centres
