"""Semantic-scene-completion samples as files, in SemanticKITTI-SSC's form (SSCBench-KITTI-360 uses the same): what
SemanticPointCloudAccumulator.voxel_ssc_sample / SemBEVGenerator.voxel_pyramid_device pack on the device (pca_voxel_pack)
written as it is, and the host inverse for tests and for users who want to check a file.

A volume of px x px x nz voxels is stored x-major, then y, z fastest: voxel (i, j, k) of this project's grid -- which lives at
[k, px - 1 - j, i] of a [nz, px, px] volume -- sits at place t = (i px + j) nz + k.  `.label` holds one little-endian uint16
per place (0 = empty under the default label_map); `.invalid`, `.occluded` and `.bin` hold one BIT per place, most significant
bit first, eight places per byte (np.packbits)."""
import os

import numpy as np

LEVEL1_FILES = (('label', 'label'), ('invalid', 'invalid'), ('occluded', 'occluded'), ('bin', 'bin'))     # (payload, extension)
POOLED_FILES = (('label', 'label'), ('invalid', 'invalid'))


def ssc_paths(directory, frame_id, scale):
    """{payload name: path} of one level's files: <id>.<ext> for scale 1, <id>_1_<s>.<ext> for a pooled one."""
    stem = '%06d' % int(frame_id) if int(scale) == 1 else '%06d_1_%d' % (int(frame_id), int(scale))
    return {key: os.path.join(str(directory), f'{stem}.{ext}') for key, ext in (LEVEL1_FILES if int(scale) == 1 else POOLED_FILES)}


def write_ssc_sample(sample, directory, frame_id, writer=None):
    """Writes the payloads of sample['packed'] (voxel_ssc_sample's or voxel_pyramid_device's dict; cuda tensors, or anything
    bytes-like) into `directory`: <id>.label, <id>.invalid, <id>.occluded, <id>.bin for level 1 -- those the sample holds --
    and <id>_1_<s>.label, <id>_1_<s>.invalid for every pooled level s, <id> = '%06d' % frame_id.  The '_1_<s>' scale tag of the
    coarse files is the one LMSCNet's preprocessing gives its down-scaled labels (1_2, 1_4, 1_8).
    The files go through AsyncBevWriter.submit_files of `writer` (None: the process-wide shared writer): the copy off the
    device is enqueued here, worker threads write; PCA_ASYNC_WRITE=0 waits until the files are on disk.  Returns the paths."""
    from .writer import shared_writer
    writer = shared_writer() if writer is None else writer
    files = []
    for scale, payloads in sample['packed'].items():
        for key, path in ssc_paths(directory, frame_id, scale).items():
            if key in payloads:
                files.append((path, payloads[key]))
    writer.submit_files(files)
    if os.environ.get('PCA_ASYNC_WRITE', '1') == '0':
        writer.flush()
    return [path for path, _ in files]


def unpack_bits(data, px, nz):
    """A bit stream of px px nz places (bytes-like or a uint8 array) as a uint8 0 / 1 volume [nz, px, px]."""
    n = int(px) * int(px) * int(nz)
    raw = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.astype(np.uint8, copy=False).ravel()
    if raw.size != (n + 7) // 8:
        raise ValueError(f'a bit stream of {px} x {px} x {nz} places holds {(n + 7) // 8} bytes, not {raw.size}')
    return places_to_volume(np.unpackbits(raw)[:n], px, nz)


def places_to_volume(flat, px, nz):
    """Values in place order t = (i px + j) nz + k as a [nz, px, px] volume, voxel (i, j, k) at [k, px - 1 - j, i]."""
    return np.ascontiguousarray(np.asarray(flat).reshape(px, px, nz).transpose(2, 1, 0)[:, ::-1, :])


def read_ssc_sample(directory, frame_id, px, nz, scales=(1, 2, 4, 8)):
    """The host inverse of write_ssc_sample: {s: {'label': uint16, 'invalid' | 'occluded' | 'bin': uint8 0 / 1}}, each
    [nz / s, px / s, px / s] in this project's layout, for the files of frame_id that exist; px, nz: level 1's."""
    out = {}
    for s in scales:
        p, n = int(px) // int(s), int(nz) // int(s)
        level = {}
        for key, path in ssc_paths(directory, frame_id, s).items():
            if not os.path.exists(path):
                continue
            with open(path, 'rb') as f:
                data = f.read()
            if key == 'label':
                flat = np.frombuffer(data, dtype='<u2')
                if flat.size != p * p * n:
                    raise ValueError(f'{path}: {flat.size} labels, not {p} x {p} x {n}')
                level[key] = places_to_volume(flat, p, n).astype(np.uint16)
            else:
                level[key] = unpack_bits(data, p, n)
        out[int(s)] = level
    return out
