"""What SemanticPointCloudAccumulator.track_instances carries from one sample of a sequence to the next: the previous
sample's instance volume, its rows and their tracks, the device counter of track numbers, the grid the volume lives on and
the store-frame mark of its moment.  Nothing here touches the device beyond holding tensors."""
import numpy as np


def grid_geom(origin, rot_mat, dx, dy, view, px, z_lo, z_step):
    """The `geom` of pca_amd.host_logic.voxel_index_map: where a voxel grid lies in store coordinates."""
    return (np.array(origin, dtype=np.float64).reshape(3), np.array(rot_mat, dtype=np.float64).reshape(3, 3), float(dx), float(dy),
            float(view), int(px), float(z_lo), float(z_step))


class TrackState:
    """One sample's side of a match, kept for the next sample.
    inst: cuda int32 [nz, px, px], a CLONE of the sample's instance volume (-1 = none); n_rows: its rows; track: cuda int32
    [n_rows], the track of every row (-1 for a row without a voxel); counter: cuda int32 [1], the next unused track number,
    moved on by the device; geom: grid_geom(...) of the volume; frame: f64 4 x 4, the accumulator's store_frame() at the
    sample's moment.  samples: how many samples the sequence has seen."""
    __slots__ = ('inst', 'n_rows', 'track', 'counter', 'geom', 'frame', 'samples')

    def __init__(self, inst, n_rows, track, counter, geom, frame, samples=1):
        self.inst, self.n_rows, self.track, self.counter = inst, int(n_rows), track, counter
        self.geom, self.frame, self.samples = geom, np.array(frame, dtype=np.float64).reshape(4, 4), int(samples)

    def record(self):
        """(inst, rows, geom): the record SemBEVGenerator.voxel_instance_match_device takes."""
        return self.inst, self.n_rows, self.geom

    def next_track(self):
        """The next unused track number (reads the device counter back: synchronises)."""
        return int(self.counter.item())
