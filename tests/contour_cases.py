"""The label planes the contour tests share (tests/test_contours_cpu.py runs
their masks through the host core, tests/test_gpu_contours.py the planes
through the kernels); every literal result is computed once per process."""
import functools

import numpy as np

import contours_literal as cl
import objects_literal as ol


def blob(rng, h, w, p=0.85):
    """h x w random pixels at density p with the first and last row and column
    set, so that the bounding box is h x w whatever the draw."""
    a = rng.random((h, w)) < p
    a[0, :] = a[-1, :] = True
    a[:, 0] = a[:, -1] = True
    return a


def put(plane, y, x, shape, label):
    h, w = shape.shape
    view = plane[y:y + h, x:x + w]
    view[shape] = label


def ring(h, w, holes):
    a = np.ones((h, w), bool)
    for (y, x, hh, hw) in holes:
        a[y:y + hh, x:x + hw] = False
    return a


def widths_plane():
    """boxes 63, 64, 65 and 130 columns wide and one starting at column 62"""
    rng = np.random.default_rng(2101)
    p = np.zeros((40, 150), np.int32)
    put(p, 2, 1, blob(rng, 6, 63), 1)
    put(p, 9, 3, blob(rng, 6, 64), 2)
    put(p, 16, 5, blob(rng, 6, 65), 3)
    put(p, 23, 10, blob(rng, 7, 130), 4)
    put(p, 32, 62, blob(rng, 6, 40), 5)
    put(p, 32, 120, blob(rng, 6, 9, 0.7), 9)
    return p


def border_plane():
    """an object cut by the zeroed lines, objects wholly on them, neighbours"""
    rng = np.random.default_rng(2102)
    p = np.zeros((30, 60), np.int32)
    put(p, 0, 0, blob(rng, 6, 8, 0.9), 1)       # cut by row 0 and column 0
    p[0, 20:27] = 2                              # wholly on row 0
    put(p, 1, 19, blob(rng, 5, 9, 0.9), 3)      # its neighbour
    p[10:15, 59] = 4                             # wholly on the last column
    put(p, 9, 50, blob(rng, 7, 9, 0.9), 5)
    put(p, 24, 30, blob(rng, 6, 12, 0.9), 6)    # cut by the last row
    p[29, 0] = 7                                 # a corner pixel
    return p


def small_plane():
    """one pixel, two pixels, one-pixel-wide lines"""
    rng = np.random.default_rng(2103)
    p = np.zeros((24, 50), np.int32)
    p[3, 4] = 1
    p[3, 10:12] = 2
    p[8, 5:14] = 3
    p[5:16, 20] = 4
    put(p, 12, 30, blob(rng, 8, 10, 0.9), 5)
    p[20, 3] = 6
    p[21, 4] = 6                                 # two pixels on a diagonal
    return p


def rings_plane():
    """one hole, three holes, a dumbbell, and a label inside another's hole"""
    p = np.zeros((40, 90), np.int32)
    put(p, 2, 2, ring(9, 9, [(3, 3, 3, 3)]), 1)
    put(p, 2, 15, ring(9, 23, [(3, 3, 3, 3), (3, 10, 3, 3), (3, 16, 3, 4)]), 2)
    dumb = np.zeros((7, 18), bool)
    dumb[1:6, 0:5] = True
    dumb[3, 5:11] = True
    dumb[0:7, 11:18] = True
    put(p, 14, 2, dumb, 3)
    put(p, 14, 30, ring(11, 11, [(3, 3, 5, 5)]), 4)
    put(p, 18, 34, np.ones((3, 3), bool), 5)
    put(p, 27, 50, ring(10, 30, [(3, 4, 4, 3), (3, 20, 3, 6)]), 6)
    p[31, 62:66] = 0                             # a notch in label 6
    return p


def maxlabel_plane():
    rng = np.random.default_rng(2104)
    p = np.zeros((20, 40), np.int32)
    put(p, 2, 2, blob(rng, 6, 7, 0.9), 7)
    put(p, 10, 12, blob(rng, 7, 9, 0.9), 50000)
    put(p, 3, 25, blob(rng, 9, 8, 0.9), 100000)
    return p


def switch_plane(lds_pixels):
    """padded boxes of exactly lds_pixels pixels and of one column more"""
    side = int(round(lds_pixels ** 0.5))
    assert side * side == lds_pixels
    rng = np.random.default_rng(2105)
    p = np.zeros((side + 6, 2 * side + 12), np.int32)
    put(p, 2, 2, blob(rng, side - 2, side - 2, 0.8), 1)
    put(p, 2, side + 6, blob(rng, side - 2, side - 1, 0.8), 2)
    return p


def single_label_plane():
    """300 x 700 of one label, with a few enclosed zeros"""
    rng = np.random.default_rng(2106)
    p = np.ones((300, 700), np.int32)
    p[rng.random(p.shape) < 0.01] = 0
    return p


def voronoi_planes(n_planes=5, h=240, w=320, cells=150, seed=2107):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n_planes, h, w), np.int32)
    for i in range(n_planes):
        sy, sx = rng.integers(0, h, cells), rng.integers(0, w, cells)
        d = (yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2
        lab = np.argmin(d, axis=0).astype(np.int32) + 1
        lab[rng.random((h, w)) < 0.03] = 0       # ragged edges and pinholes
        out[i] = lab
    return out


def polygon_value():
    """a (t, z) = (2, 3) value [H, W, 3, 2]"""
    planes = [rings_plane()[:40, :60], small_plane()[:, :50], border_plane()[:, :50]]
    v = np.zeros((24, 50, 3, 2), np.int32)
    for t in range(2):
        for z in range(3):
            src = planes[(t + z) % 3][:24, :50]
            v[:, :, z, t] = np.roll(src, t * 2, axis=1) if t else src
    return v


SMALL_PLANES = [("widths", widths_plane), ("border", border_plane), ("small", small_plane),
                ("rings", rings_plane), ("maxlabel", maxlabel_plane)]


@functools.lru_cache(maxsize=None)
def literal(name, lds_pixels=4096):
    """(planes [n, H, W], (objects, contours, points) of the literal)."""
    if name == "switch":
        planes = switch_plane(lds_pixels)[None]
    elif name == "single":
        planes = single_label_plane()[None]
    elif name == "voronoi":
        planes = voronoi_planes()
    else:
        planes = dict(SMALL_PLANES)[name]()[None]
    planes = np.ascontiguousarray(planes)
    planes.setflags(write=False)
    return planes, cl.object_contours(planes)


def masks_of(planes):
    """[(mask before the opening, open flag)] of every object of the planes."""
    out = []
    for plane in planes:
        rows = ol.object_rows(plane)
        plane0 = cl.zero_border(plane)
        for label in np.unique(plane0[plane0 > 0]):
            r = rows[label]
            cut = plane0[r["y0"]:r["y1"], r["x0"]:r["x1"]]
            mask = np.pad(cut, 1, mode="constant", constant_values=0) == label
            out.append((mask, 1 if np.sum(mask) > 1 else 0))
    return out
