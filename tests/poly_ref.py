"""A deliberately plain restatement of the polygon rasteriser (pycocotools' rleFrPoly + merge + decode), loop by loop with
Python ints and floats, an explicit sort of the crossing positions and run-length differencing as the original does.  It is the THIRD
implementation beside the host codec (abr_iod_amd/structures/polygon.py, vectorised numpy, parity by cumulative sum) and the kernels
(abr_iod_amd/csrc/poly.hip, integer crossing test, toggle planes), so that a shared misunderstanding cannot hide.  Not a test module."""
import math
import struct

SCALE = 5.0
LIMIT = 5.0 * 32768.0


def f32(x):
    """the float32 nearest to x, as a Python float (polygon coordinates are stored as float32)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def c_int(x):
    """C's (int) of a double: truncation toward zero"""
    return int(math.floor(x)) if x >= 0 else int(math.ceil(x))


def guarded(xy):
    for c in xy:
        if math.isnan(c) or math.isinf(c) or abs(5.0 * c) > LIMIT:
            return True
    return False


def rle_counts_from_polygon(xy, h, w):
    """xy: flat [x0, y0, x1, y1, ...] of float32-representable numbers -> the run lengths of the polygon's mask in column-major order (the
    first run is of zeros), as rleFrPoly builds them"""
    k = len(xy) // 2
    # upsample and get discrete points densely along the entire boundary
    x = [c_int(SCALE * xy[2 * j] + 0.5) for j in range(k)]
    y = [c_int(SCALE * xy[2 * j + 1] + 0.5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx == 0 and dy == 0:
            u.append(xs)            # the single point; 0 / 0 is never formed
            v.append(ys)
            continue
        s = (ye - ys) / dx if dx >= dy else (xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(c_int(ys + s * t + 0.5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(c_int(xs + s * t + 0.5))
    # get points along y-boundary and downsample
    a = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + 0.5) / SCALE - 0.5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + 0.5) / SCALE - 0.5
            if yd < 0:
                yd = 0.0
            elif yd > h:
                yd = float(h)
            yd = math.ceil(yd)
            a.append(int(xd * h + yd))
    # compute rle encoding given y-boundary points
    a.append(h * w)
    a.sort()
    p = 0
    b = []
    for pos in a:
        b.append(pos - p)
        p = pos
    # merge the zero-length runs away: a zero run joins its two neighbours
    counts = []
    j = 0
    if b:
        counts.append(b[0])
        j = 1
    while j < len(b):
        if b[j] > 0:
            counts.append(b[j])
            j += 1
        else:
            j += 1
            if j < len(b):
                counts[-1] += b[j]
                j += 1
    return counts


def decode_counts(counts, h, w):
    """run lengths (column-major, first run zeros) -> [h][w] list of 0 / 1; runs past h * w are cut"""
    flat = []
    value = 0
    for c in counts:
        flat.extend([value] * c)
        value ^= 1
    flat = (flat + [0] * (h * w))[: h * w]
    return [[flat[xx * h + yy] for xx in range(w)] for yy in range(h)]


def rasterize_polygon(xy, h, w):
    """one polygon (flat coordinate list) -> [h][w] list of 0 / 1; a guarded polygon gives zeros"""
    xy = [f32(c) for c in xy]
    if guarded(xy) or len(xy) < 2:
        return [[0] * w for _ in range(h)]
    return decode_counts(rle_counts_from_polygon(xy, h, w), h, w)


def rasterize_instance(polygons, h, w):
    """an instance = the OR of its polygons (merge with intersect = 0)"""
    out = [[0] * w for _ in range(h)]
    for xy in polygons:
        m = rasterize_polygon(xy, h, w)
        for yy in range(h):
            row, mr = out[yy], m[yy]
            for xx in range(w):
                row[xx] |= mr[xx]
    return out
