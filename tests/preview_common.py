"""A numpy model of the preview sheet (include/pca.h, KP), written from its definition and not imported from pca_amd, the
crafted inputs the GPU tests render, and the PNG plumbing the tests share: scanline filters, their inverse, IDAT access."""
import struct
import zlib

import numpy as np

SETS = ('present', 'future', 'full')
ELEV_RANGE = (-0.5, 2.0)
CHUNK_MAX = 32768


def stream_bytes(px):
    return (1 + 15 * px) * 3 * px


# ---- the pixel definition
def model_lut():
    """The default table from matplotlib itself."""
    import matplotlib
    return (matplotlib.colormaps['viridis'](np.arange(256))[:, :3] * 255).round().astype(np.uint8)


def scalar_panel(plane, lo, hi, lut):
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(256) / (hi - lo)
    v = np.asarray(plane).astype(np.float32)
    with np.errstate(all='ignore'):
        t = np.floor((v - lo) * scale)
    assert t.dtype == np.float32
    idx = np.where(t >= 255, 255, np.where(t > 0, t, 0)).astype(np.int64)            # NaN: both comparisons are false -> 0
    return lut[idx]


def rgb_panel(planes3):
    v = np.asarray(planes3).astype(np.float32)
    c = np.where(v > 0, np.where(v < 1, v, np.float32(1)), np.float32(0)).astype(np.float32)
    b = np.floor(c * np.float32(255) + np.float32(0.5))
    assert b.dtype == np.float32
    return np.transpose(b.astype(np.uint8), (1, 2, 0))


def model_polylines(trajs):
    out = []
    for t in trajs:
        t = np.asarray(t, dtype=np.float64)
        if t.ndim != 2 or t.shape[0] == 0:
            continue
        xy = t[:, :2]
        if not np.isfinite(xy).all():
            continue
        out.append([(int(x), int(y)) for x, y in np.floor(xy)])
    return out


def segment_points(x0, y0, x1, y1):
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return [(x0, y0)]
    return [(x0 + (2 * s * dx + n) // (2 * n), y0 + (2 * s * dy + n) // (2 * n)) for s in range(n + 1)]      # // floors


def overlay_mask(trajs, px):
    """bool [px,px] in panel pixels: grid point (x, y) is column x, row px - 1 - y."""
    m = np.zeros((px, px), dtype=bool)
    for line in model_polylines(trajs):
        pts = [line[0]] if len(line) == 1 else [p for a, b in zip(line[:-1], line[1:]) for p in segment_points(*a, *b)]
        for x, y in pts:
            if 0 <= x < px and 0 <= y < px:
                m[px - 1 - y, x] = True
    return m


def model_sheet(planes, trajs3, lut, elev_range=ELEV_RANGE):
    """planes: float16 [21,px,px]; trajs3: (trajs_present, trajs_future, trajs_full) -> uint8 [3 px, 5 px, 3]."""
    px = planes.shape[-1]
    img = np.zeros((3 * px, 5 * px, 3), dtype=np.uint8)
    for s in range(3):
        p = planes[7 * s:7 * s + 7]
        panels = [scalar_panel(p[0], 0, 1, lut), scalar_panel(p[1], 0, 1, lut), rgb_panel(p[2:5]), scalar_panel(p[5], 0, 1, lut),
                  scalar_panel(p[6], *elev_range, lut)]
        m = overlay_mask(trajs3[s], px)
        for c, panel in enumerate(panels):
            panel = panel.copy()
            panel[m] = (255, 0, 0)
            img[s * px:(s + 1) * px, c * px:(c + 1) * px] = panel
    return img


def model_of_bev(bev, lut, elev_range=ELEV_RANGE):
    """The sheet of a sample's dict: its 15 arrays and its trajectories."""
    planes = np.concatenate([np.asarray(bev[f'{name}_{s}'], dtype=np.float16).reshape(-1, *np.asarray(bev[f'road_{s}']).shape)
                             for s in SETS for name in ('road', 'intensity', 'rgb', 'dynamic', 'elevation')])
    return model_sheet(planes, [bev[f'trajs_{s}'] for s in SETS], lut, elev_range)


# ---- scanlines
def filter_rows(img, ftype):
    """uint8 [H,W,3] -> the PNG scanline stream with filter `ftype` (0 None, 1 Sub, 2 Up) on every row."""
    raw = img.reshape(img.shape[0], -1).astype(np.int64)
    if ftype == 1:
        left = np.concatenate([np.zeros((raw.shape[0], 3), np.int64), raw[:, :-3]], axis=1)
        raw = raw - left
    elif ftype == 2:
        raw = raw - np.concatenate([np.zeros((1, raw.shape[1]), np.int64), raw[:-1]])
    rows = np.concatenate([np.full((raw.shape[0], 1), ftype, np.int64), raw], axis=1)
    return (rows % 256).astype(np.uint8).tobytes()


def unfilter(stream, height, width):
    """The scanline stream -> (uint8 [H,W,3], the filter types of the rows)."""
    rows = np.frombuffer(stream, dtype=np.uint8).reshape(height, 1 + 3 * width)
    out = np.zeros((height, 3 * width), dtype=np.uint8)
    for r in range(height):
        f, line = int(rows[r, 0]), rows[r, 1:].astype(np.int64)
        if f == 1:
            for ch in range(3):
                line[ch::3] = np.cumsum(line[ch::3])
        elif f == 2:
            line = line + (out[r - 1] if r else 0)
        else:
            assert f == 0, f
        out[r] = line % 256
    return out.reshape(height, width, 3), rows[:, 0].copy()


def png_chunks(png):
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    at, out = 8, []
    while at < len(png):
        n, kind = struct.unpack('>I4s', png[at:at + 8])
        data = png[at + 8:at + 8 + n]
        assert struct.unpack('>I', png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data), kind
        out.append((kind, data))
        at += 12 + n
    assert at == len(png)
    return out


def decode_png(png):
    """(pixels by PIL, the scanline stream by zlib) of a PNG that PIL verifies."""
    import io

    from PIL import Image
    Image.open(io.BytesIO(png)).verify()
    pixels = np.asarray(Image.open(io.BytesIO(png)).convert('RGB'))
    chunks = png_chunks(png)
    assert [k for k, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0) and pixels.shape == (h, w, 3)
    body = chunks[1][1]
    assert body[:2] == b'\x78\x01'
    return pixels, zlib.decompress(body)


# ---- crafted inputs
def f16_neighbours(v):
    v = np.float16(v)
    return [np.nextafter(v, np.float16(-np.inf)), np.nextafter(v, np.float16(np.inf))]


def scalar_specials(lo, hi):
    """lo, hi, their float16 neighbours, NaN, +-inf, and LUT bin edges with their neighbours: 24 values."""
    vals = [np.float16(lo), np.float16(hi)] + f16_neighbours(lo) + f16_neighbours(hi) + [np.float16(np.nan), np.float16(np.inf),
                                                                                          np.float16(-np.inf)]
    for i in (1, 2, 127, 128, 255):
        e = np.float16(lo + i * (hi - lo) / 256)
        vals += [e] + f16_neighbours(e)
    return np.array(vals, dtype=np.float16)


def rgb_specials():
    vals = [-0.5, -0.0, 0.0, 1.0, 1.5, np.nan, np.inf, -np.inf]
    vals += [k / 255 for k in (1, 2, 127, 128, 254)] + [(k + 0.5) / 255 for k in (1, 2, 127, 128, 254)]
    return np.array(vals, dtype=np.float16)


def crafted_planes(px, k, seed=3, elev_range=ELEV_RANGE):
    """float16 [k,21,px,px] (px >= 5): every scalar panel holds its specials at scattered cells, every rgb channel its own;
    the other cells hold values around the panel's range."""
    rng = np.random.default_rng(seed)
    out = np.empty((k, 21, px, px), dtype=np.float16)
    for i in range(k):
        for p in range(21):
            kind = p % 7
            lo, hi = elev_range if kind == 6 else (0., 1.)
            special = rgb_specials() if 2 <= kind <= 4 else scalar_specials(lo, hi)
            plane = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), px * px).astype(np.float16)
            plane[rng.random(px * px) < 0.3] = 0          # flat areas, as empty cells are
            cells = rng.permutation(px * px)[:len(special)]
            plane[cells] = special
            out[i, p] = plane.reshape(px, px)
    return out


def crafted_trajs(px):
    """(trajs_present, trajs_future, trajs_full): every polyline case of the pixel definition; `future` has none."""
    m, e = px // 2, px - 1
    present = [
        np.array([[m + 0.5, m + 0.25]]),                                      # a single point, fractional
        np.array([[1., 1.], [e - 1., 1.]]),                                   # horizontal
        np.array([[1., 1., 7.], [1., e - 1., 7.]]),                           # vertical, (N, 3)
        np.array([[0., 0.], [e, e]]),                                         # +45 degrees
        np.array([[0., e], [e, 0.]]),                                         # -45 degrees: crosses the one above
        np.array([[0., 1.], [e, 3.]]),                                        # shallow
        np.array([[2., 0.], [4., e]]),                                        # steep
        np.array([[e, 3.], [0., 1.]]),                                        # the shallow one drawn the other way
        np.array([[m, m], [px + 7., m + 2.]]),                                # partly outside
        np.array([[-9., -3.], [-2., -20.]]),                                  # wholly outside
        np.array([[px, 2.], [px - 3., 4.]]),                                  # a vertex at x == px
        np.array([[3., -1.], [1., 2.], [0.5, 2.5]]),                          # a vertex at y == -1, then a fractional tail
        np.array([[-0.5, 0.5], [2.5, -0.5]]),                                 # negative fractions: floor, not truncation
        np.zeros((0, 2)),                                                     # empty
        np.array([[1., np.nan], [2., 2.]]),                                   # a non-finite vertex: dropped whole
    ]
    full = [np.array([[0., m], [e, m + 1.], [m, e], [m, 0.]]), np.array([[e, e]])]
    return present, [], full


def crafted_block(px, k):
    """(planes [k,21,px,px], trajs per sample): sample 1 of a block has no polylines at all, sample 2 a shifted set."""
    planes = crafted_planes(px, k)
    trajs = []
    for i in range(k):
        if i == 1:
            trajs.append(([], [], []))
        elif i == 0:
            trajs.append(crafted_trajs(px))
        else:
            p, f, u = crafted_trajs(px)
            trajs.append((u, [t + 1.5 for t in p if t.shape[0]], f))
    return planes, trajs
