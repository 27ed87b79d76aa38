"""Merging the lidar sweeps of a NuScenes sample and labelling points with their ground-truth boxes.

What the reference does in ``inst_centric_get_sweeps`` (datasets/nuscenes_utils.py:246-531) followed by
``load_data_to_tensor`` (:533-545), restated for the observation loader (ingest):

  * the keyframe's LIDAR_TOP record and its ``n_sweeps - 1`` predecessors (a record without predecessor repeats), oldest
    first, each with its time lag [s] and sweep index (newest = n_sweeps - 1);
  * every sweep: f32 points of the .bin file, points within ``center_radius`` of the sensor axis dropped, moved into the
    keyframe's lidar frame (f64 product, stored back as f32), columns [x, y, z, intensity, lag, sweep, instance, class];
  * every annotated box of the sweep whose class is wanted and that has lidar points: the points inside the box (with
    tolerance) get the instance index of the box's track and its class index; later boxes overwrite earlier ones;
  * per labelled box occurrence: the track token and the box centre (global frame), in encounter order.

The dataset object only has to offer what the devkit's ``NuScenes`` offers: ``get(table, token)``, ``get_sample_data_path``,
``get_boxes`` (boxes with .name .token .center .orientation .wlh) and ``box_velocity``.  Quaternions are turned into
rotation matrices by ``rotation_matrix`` below (the textbook formula pyquaternion also implements; an ``orientation``
object that carries its own ``rotation_matrix`` is used as is).
"""
import numpy as np

# devkit category -> detection class (nuscenes-devkit eval/detection; the reference keeps a copy at :14-38)
DETECTION_NAME = {
    'human.pedestrian.adult': 'pedestrian', 'human.pedestrian.child': 'pedestrian',
    'human.pedestrian.police_officer': 'pedestrian', 'human.pedestrian.construction_worker': 'pedestrian',
    'vehicle.car': 'car', 'vehicle.motorcycle': 'motorcycle', 'vehicle.bicycle': 'bicycle',
    'vehicle.bus.bendy': 'bus', 'vehicle.bus.rigid': 'bus', 'vehicle.truck': 'truck',
    'vehicle.construction': 'construction_vehicle', 'vehicle.trailer': 'trailer',
    'movable_object.barrier': 'barrier', 'movable_object.trafficcone': 'traffic_cone',
}   # every other category is 'ignore'


def rotation_matrix(q):
    """3x3 rotation of a unit quaternion (w, x, y, z), or of an object with a ``rotation_matrix`` attribute."""
    if hasattr(q, 'rotation_matrix'):
        return np.asarray(q.rotation_matrix, dtype=np.float64)
    w, x, y, z = (float(v) for v in (q.elements if hasattr(q, 'elements') else q))
    n = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rigid(translation, rotation):
    T = np.eye(4)
    T[:3, :3] = rotation_matrix(rotation)
    T[:3, 3] = translation
    return T


def sensor_in_global(nusc, sd_token):
    """4x4 pose of a sample_data's sensor in the global frame: ego pose x calibrated sensor pose."""
    rec = nusc.get('sample_data', sd_token)
    cs = nusc.get('calibrated_sensor', rec['calibrated_sensor_token'])
    ego = nusc.get('ego_pose', rec['ego_pose_token'])
    return rigid(ego['translation'], ego['rotation']) @ rigid(cs['translation'], cs['rotation'])


def sweep_chain(nusc, keyframe_sd_token, n_sweeps):
    """[(token, time lag in s, sweep index)] oldest first; a record without 'prev' is repeated."""
    t_ref = nusc.get('sample_data', keyframe_sd_token)['timestamp'] * 1e-6
    chain, token = [], keyframe_sd_token
    for back in range(n_sweeps):
        rec = nusc.get('sample_data', token)
        chain.append((token, t_ref - rec['timestamp'] * 1e-6, n_sweeps - 1 - back))
        if rec['prev'] != '':
            token = rec['prev']
    return chain[::-1]


def _apply(T, xyz):
    """rows of [xyz 1] @ T.T, first three columns (f64 whatever the point dtype)."""
    h = np.concatenate([xyz, np.ones((xyz.shape[0], 1), dtype=xyz.dtype)], axis=1)
    return (h @ T.T)[:, :3]


def inst_centric_get_sweeps(nusc, sample_token, n_sweeps, center_radius, in_box_tolerance, return_instances_last_box,
                            point_cloud_range, detection_classes, map_point_feat2idx):
    """Returns {'points' (N,8) f32, 'instances_token' list, 'instances_center' list, and with
    return_instances_last_box 'instances_last_box' (n_inst,9) f32 + 'instances_name' (n_inst,) f32} -- the values the
    reference holds after load_data_to_tensor (f32 arrays instead of f32 tensors)."""
    key_sd = nusc.get('sample', sample_token)['data']['LIDAR_TOP']
    target_from_glob = np.linalg.inv(sensor_in_global(nusc, key_sd))
    col_inst, col_cls = map_point_feat2idx['inst_idx'], map_point_feat2idx['cls_idx']

    track_index = {}                      # instance token -> instance index (order of first labelled appearance)
    tracks = []                           # per instance: dict(poses, sweeps, size, cls, anno)
    tokens, centres, clouds = [], [], []
    for sd_token, lag, sweep in sweep_chain(nusc, key_sd, n_sweeps):
        raw = np.fromfile(nusc.get_sample_data_path(sd_token), dtype=np.float32).reshape(-1, 5)
        pts = np.full((raw.shape[0], 8), -1.0, dtype=np.float32)
        pts[:, :4] = raw[:, :4]
        pts[:, 4], pts[:, 5] = lag, sweep
        pts = pts[np.linalg.norm(pts[:, :2], axis=1) > center_radius]
        pts[:, :3] = _apply(target_from_glob @ sensor_in_global(nusc, sd_token), pts[:, :3])
        for box in nusc.get_boxes(sd_token):
            cls_name = DETECTION_NAME.get(box.name, 'ignore')
            if cls_name not in detection_classes:
                continue
            anno = nusc.get('sample_annotation', box.token)
            if anno['num_lidar_pts'] < 1:
                continue
            target_from_box = target_from_glob @ rigid(box.center, box.orientation)
            size = np.array([box.wlh[1], box.wlh[0], box.wlh[2]])            # length, width, height = dx, dy, dz
            local = _apply(np.linalg.inv(target_from_box), pts[:, :3])
            inside = np.all(np.abs(local / size) < (0.5 + in_box_tolerance), axis=1)
            if not inside.any():
                continue
            itok = anno['instance_token']
            if itok not in track_index:
                track_index[itok] = len(tracks)
                tracks.append({'poses': [], 'sweeps': [], 'size': size.tolist(),
                               'cls': detection_classes.index(cls_name), 'anno': None})
            tr = tracks[track_index[itok]]
            tr['poses'].append(target_from_box)
            tr['sweeps'].append(sweep)
            tr['anno'] = anno['token']
            pts[inside, col_inst] = track_index[itok]
            pts[inside, col_cls] = detection_classes.index(cls_name)
            tokens.append(itok)
            centres.append(box.center)
        clouds.append(pts)

    out = {'points': np.concatenate(clouds, axis=0) if clouds else np.zeros((0, 8), np.float32),
           'instances_token': tokens, 'instances_center': centres}
    if return_instances_last_box:
        out.update(_last_boxes(nusc, tracks, target_from_glob, point_cloud_range))
    return out


def _last_boxes(nusc, tracks, target_from_glob, point_cloud_range):
    """'instances_last_box' (n_inst,9) f32 and 'instances_name' (n_inst,) f32 of the tracks a merge found."""
    assert point_cloud_range is not None
    rng = np.asarray(point_cloud_range, dtype=np.float64)
    last = np.zeros((len(tracks), 9))
    for k, tr in enumerate(tracks):
        # newest pose whose centre lies inside the range, else the oldest one
        pick = tr['poses'][0]
        for pose in reversed(tr['poses']):
            c = pose[:3, 3]
            if np.all((c >= rng[:3]) & (c < rng[3:] - 1e-2)):
                pick = pose
                break
        last[k, :3] = pick[:3, 3]
        last[k, 3:6] = tr['size']
        last[k, 6] = np.arctan2(pick[1, 0], pick[0, 0])
        vel = np.asarray(nusc.box_velocity(tr['anno']), dtype=np.float64).reshape(1, 3)     # global frame
        last[k, 7:9] = _apply(target_from_glob, vel).reshape(3)[:2]
    return {'instances_last_box': last.astype(np.float32),
            'instances_name': np.array([tr['cls'] for tr in tracks]).astype(np.float32)}


# ---------------------------------------------------------------------------------------------------------------------
#  The same merge with the per-point work on the device (kernel K0s, pca_nusc_merge_sweeps; opt-in, bit-identical)
# ---------------------------------------------------------------------------------------------------------------------
MAX_SWEEPS, MAX_BOXES = 32, 4096              # PCA_NUSC_MAX_SWEEPS / PCA_NUSC_MAX_SWEEP_BOXES of include/pca.h
_SWEEP_DTYPE = np.dtype([('row0', 'i4'), ('n_rows', 'i4'), ('box0', 'i4'), ('n_boxes', 'i4'), ('lag', 'f4'), ('sweep', 'f4'),
                         ('T', 'f8', (12, ))])                                        # pca_nusc_sweep
_BOX_DTYPE = np.dtype([('inv', 'f8', (12, )), ('size', 'f8', (3, )), ('cls', 'i4'), ('track_key', 'i4')])   # pca_nusc_sweep_box
assert _SWEEP_DTYPE.itemsize == 120 and _BOX_DTYPE.itemsize == 128


def collect_sweep_inputs(nusc, sample_token, n_sweeps, detection_classes):
    """Everything of a merge that only needs the host (no HIP call: reader threads may run it): the sweep chain, the
    files' rows, target_from_sweep, and per sweep the candidate boxes -- wanted class, at least one lidar point -- in
    get_boxes order, with the expressions `inst_centric_get_sweeps` evaluates."""
    key_sd = nusc.get('sample', sample_token)['data']['LIDAR_TOP']
    target_from_glob = np.linalg.inv(sensor_in_global(nusc, key_sd))
    sweeps = []
    for sd_token, lag, sweep in sweep_chain(nusc, key_sd, n_sweeps):
        raw = np.fromfile(nusc.get_sample_data_path(sd_token), dtype=np.float32).reshape(-1, 5)
        boxes = []
        for box in nusc.get_boxes(sd_token):
            cls_name = DETECTION_NAME.get(box.name, 'ignore')
            if cls_name not in detection_classes:
                continue
            anno = nusc.get('sample_annotation', box.token)
            if anno['num_lidar_pts'] < 1:
                continue
            boxes.append({'target_from_box': target_from_glob @ rigid(box.center, box.orientation),
                          'size': np.array([box.wlh[1], box.wlh[0], box.wlh[2]]), 'center': box.center,
                          'cls': detection_classes.index(cls_name), 'instance_token': anno['instance_token'],
                          'anno_token': anno['token']})
        sweeps.append({'raw': raw, 'lag': lag, 'sweep': sweep,
                       'target_from_sweep': target_from_glob @ sensor_in_global(nusc, sd_token), 'boxes': boxes})
    return {'target_from_glob': target_from_glob, 'sweeps': sweeps}


def sweep_tables(inputs):
    """(raw rows of all sweeps (n,5) f32, sweep table, box table) as pca_nusc_merge_sweeps takes them."""
    sweeps = inputs['sweeps']
    n_boxes = sum(len(sw['boxes']) for sw in sweeps)
    st, bt = np.zeros(len(sweeps), _SWEEP_DTYPE), np.zeros(n_boxes, _BOX_DTYPE)
    keys = {}
    row0 = b = 0
    for k, sw in enumerate(sweeps):
        st[k] = (row0, sw['raw'].shape[0], b, len(sw['boxes']), sw['lag'], sw['sweep'], sw['target_from_sweep'][:3].ravel())
        row0 += sw['raw'].shape[0]
        for box in sw['boxes']:
            key = keys.setdefault(box['instance_token'], len(keys))
            bt[b] = (np.linalg.inv(box['target_from_box'])[:3].ravel(), box['size'], box['cls'], key)
            b += 1
    raws = [sw['raw'] for sw in sweeps]
    raw = np.concatenate(raws, axis=0) if raws else np.zeros((0, 5), np.float32)
    return np.ascontiguousarray(raw, dtype=np.float32), st, bt


_PINS = {}


class _PendingMerge:
    """A merge whose launches and read-back are enqueued; finish() waits (once) and does the host bookkeeping."""

    def __init__(self, ctx, inputs, n_sweeps, n_boxes, res, pin, ticket, device_points):
        self.ctx, self.inputs, self.n_sweeps, self.n_boxes = ctx, inputs, n_sweeps, n_boxes
        self.res, self.pin, self.ticket, self.device_points = res, pin, ticket, device_points

    def finish(self):
        ctx, ns = self.ctx, self.n_sweeps
        ctx.check(ctx.lib.pca_host_d2h_wait(ctx.h, self.ticket))
        ctx.poll_status()
        host = self.pin.numpy()
        n_kept = int(host[ns])
        hits = host[ns + 1:ns + 1 + self.n_boxes]
        pad = _tally_words(ns, self.n_boxes)
        if self.device_points:
            points = self.res[pad:pad + 8 * n_kept].view(n_kept, 8)
            import torch
            points = points.view(torch.float32)
        else:
            points = host[pad:pad + 8 * n_kept].view(np.float32).reshape(n_kept, 8).copy()
        track_index, tracks, tokens, centres = {}, [], [], []
        b = 0
        for sw in self.inputs['sweeps']:
            for box in sw['boxes']:
                b += 1
                if not hits[b - 1] > 0:
                    continue
                itok = box['instance_token']
                if itok not in track_index:
                    track_index[itok] = len(tracks)
                    tracks.append({'poses': [], 'sweeps': [], 'size': box['size'].tolist(), 'cls': box['cls'], 'anno': None})
                tr = tracks[track_index[itok]]
                tr['poses'].append(box['target_from_box'])
                tr['sweeps'].append(sw['sweep'])
                tr['anno'] = box['anno_token']
                tokens.append(itok)
                centres.append(box['center'])
        return {'points': points, 'instances_token': tokens, 'instances_center': centres, 'tracks': tracks,
                'sweep_off': host[:ns + 1].copy()}


def _tally_words(n_sweeps, n_boxes):
    """int32 words of the tally in front of the point rows (rounded up: the rows are stored 16 bytes at a time)"""
    return (n_sweeps + 1 + n_boxes + 3) // 4 * 4


def merge_sweeps_launch(inputs, center_radius, in_box_tolerance, device_points=False, raw_dev=None, tables=None):
    """Uploads the raw rows (unless `raw_dev`, a device f32 tensor (n,5), holds them already), enqueues the launches and the
    read-back -- the tally alone with device_points, else the rows with it -- and returns the pending merge."""
    import torch
    from pca_amd import _lib
    raw, st, bt = tables if tables is not None else sweep_tables(inputs)
    ctx = _lib.Context.get()
    lib = ctx.lib
    dev = torch.device('cuda', ctx.device_index)
    n, ns, nb = int(raw.shape[0]), int(st.shape[0]), int(bt.shape[0])
    if ns < 1:
        raise ValueError('merge_sweeps_device: no sweep')
    if raw_dev is None:
        raw_dev = torch.from_numpy(raw).to(dev)
    assert raw_dev.dtype == torch.float32 and raw_dev.is_contiguous() and raw_dev.numel() == 5 * n
    pad = _tally_words(ns, nb)
    res = torch.empty(pad + 8 * n, dtype=torch.int32, device=dev)
    ws_bytes = lib.pca_nusc_merge_sweeps_workspace_bytes(n, nb)
    ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=dev)
    limit = 0.5 + float(in_box_tolerance)                    # added in f64, as the host form does
    ctx.check(lib.pca_nusc_merge_sweeps(ctx.h, raw_dev.data_ptr(), n, st.ctypes.data, ns, bt.ctypes.data, nb,
                                        float(np.float32(center_radius)), limit, ws.data_ptr(), ws.numel(),
                                        res.data_ptr() + 4 * pad, res.data_ptr(), ctx.stream()))
    words = pad if device_points else pad + 8 * n
    pins = _PINS.setdefault(id(ctx), [None, None, 0])         # page-locked landing blocks of the context, two in turn
    turn = pins[2] = 1 - pins[2]
    if pins[turn] is None or pins[turn].numel() < words:
        pins[turn] = torch.empty(max(words + words // 4, 1024), dtype=torch.int32).pin_memory()
    pin = pins[turn][:words]
    ticket = lib.pca_host_d2h_async(ctx.h, res.data_ptr(), pin.data_ptr(), 4 * words, ctx.stream())
    if ticket < 0:
        ctx.check(-1)
    return _PendingMerge(ctx, inputs, ns, nb, res, pin, ticket, device_points), (raw_dev, ws)


def merge_sweeps_device(inputs, center_radius, in_box_tolerance, device_points=False, raw_dev=None):
    """The merge of `collect_sweep_inputs`' result on the device: one upload of the raw rows, the launches, ONE wait (for the
    per-box hit counts and the rows kept per sweep), then the host bookkeeping of the host form's loop with `hits[b] > 0`
    in place of `inside.any()`.  Returns {'points' (n_kept,8) f32 -- a device tensor with device_points, else a host
    array --, 'instances_token', 'instances_center', 'tracks', 'sweep_off'}."""
    pending, keep = merge_sweeps_launch(inputs, center_radius, in_box_tolerance, device_points, raw_dev)
    out = pending.finish()
    del keep                                                 # (the launches that read them have run: the wait is behind them)
    return out


def inst_centric_get_sweeps_device(nusc, sample_token, n_sweeps, center_radius, in_box_tolerance, return_instances_last_box,
                                   point_cloud_range, detection_classes, map_point_feat2idx):
    """`inst_centric_get_sweeps` with the per-point work on the device: same signature, same dict, bit for bit (usable as
    NuScenesDataloader.sweep_provider; PCA_NUSC_SWEEPS=device selects it)."""
    if (map_point_feat2idx['inst_idx'], map_point_feat2idx['cls_idx']) != (6, 7):
        raise ValueError('the device merge writes the instance / class columns 6 / 7')
    inputs = collect_sweep_inputs(nusc, sample_token, n_sweeps, detection_classes)
    res = merge_sweeps_device(inputs, center_radius, in_box_tolerance)
    out = {'points': res['points'], 'instances_token': res['instances_token'], 'instances_center': res['instances_center']}
    if return_instances_last_box:
        out.update(_last_boxes(nusc, res['tracks'], inputs['target_from_glob'], point_cloud_range))
    return out
