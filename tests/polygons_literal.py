"""create_from_polygons in plain loops, and the rings the polygon tests draw.

``fill_ring`` restates skimage.draw.polygon of scikit-image 0.13.0 (``_polygon``
-> ``point_in_polygon``) as DESIGN.md section 25.1 records it: every pixel of
the ring's clipped bounding box against every vertex, in f64, multiply, divide,
add.  ``create_from_polygons`` is tmlib/image.py:766-776 around it.  Nothing
here is shared with the library's code.
"""
import math

import numpy as np


def transformed(ring, y_offset, x_offset):
    """(xs, ys) of a stored ring as floats: astype(int), y negated, offsets subtracted."""
    pts = np.array(ring).astype(int).reshape(-1, 2)
    xs = [float(int(x) - x_offset) for x in pts[:, 0]]
    ys = [float(-int(y) - y_offset) for y in pts[:, 1]]
    return xs, ys


def fill_ring(array, label, xs, ys):
    """array[r, c] = label for the pixels skimage.draw.polygon(ys, xs, array.shape) gives."""
    H, W = array.shape
    n = len(xs)
    if n == 0:
        raise ValueError("an empty ring")
    minr = int(max(0, min(ys)))
    maxr = min(H - 1, int(math.ceil(max(ys))))
    minc = int(max(0, min(xs)))
    maxc = min(W - 1, int(math.ceil(max(xs))))
    for r in range(minr, maxr + 1):
        for c in range(minc, maxc + 1):
            inside = False
            j = n - 1
            for i in range(n):
                if ((ys[i] <= r < ys[j]) or (ys[j] <= r < ys[i])) and \
                        (c < (xs[j] - xs[i]) * (r - ys[i]) / (ys[j] - ys[i]) + xs[i]):
                    inside = not inside
                j = i
            if inside:
                array[r, c] = label


def create_from_polygons(polygons, y_offset, x_offset, dimensions):
    """tmlib/image.py:766-776 for (label, ring) pairs: the int32 plane."""
    array = np.zeros(dimensions, dtype=np.int32)
    for label, ring in polygons:
        xs, ys = transformed(ring, y_offset, x_offset)
        fill_ring(array, label, xs, ys)
    return array


def ring_of(xs, ys, y_offset=0, x_offset=0):
    """Plane coordinates (xs, ys) as a stored ring: global (x, y), y negated."""
    return np.array([[int(x) + x_offset, -(int(y) + y_offset)] for x, y in zip(xs, ys)],
                    dtype=np.int32).reshape(-1, 2)


# the four hand anchors: (ring in plane coordinates (x, y), plane shape, filled pixels (r, c))
ANCHORS = [
    ([(1, 1), (3, 1), (3, 3), (1, 3), (1, 1)], (5, 5),
     [(r, c) for r in (1, 2) for c in (1, 2)]),
    ([(2, 0), (4, 2), (2, 4), (0, 2)], (5, 5),
     [(1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2)]),
    ([(0, 0), (4, 0), (0, 4)], (5, 5),
     [(r, c) for r in range(4) for c in range(4 - r)]),
    ([(-2, -2), (2, -2), (2, 2), (-2, 2)], (4, 4),
     [(r, c) for r in (0, 1) for c in (0, 1)]),
]


def anchor_plane(shape, pixels, label=1):
    a = np.zeros(shape, np.int32)
    for r, c in pixels:
        a[r, c] = label
    return a


def star(rng, cy, cx, radius, n_vertices):
    """A star-shaped ring around (cx, cy) with integer vertices, plane coordinates,
    unclosed: angles ascending, radii between 0.35 and 1 of `radius`."""
    angles = np.sort(rng.uniform(0.0, 2.0 * np.pi, n_vertices))
    radii = rng.uniform(0.35, 1.0, n_vertices) * radius
    xs = np.rint(cx + radii * np.cos(angles)).astype(int)
    ys = np.rint(cy + radii * np.sin(angles)).astype(int)
    return list(zip(xs.tolist(), ys.tolist()))


def random_polygons(seed, n, shape, y_offset=0, x_offset=0, max_radius=9.0, labels=None):
    """n (label, stored ring) pairs of stars in and around a plane of `shape`
    (some cross its edges), labels 1..n unless given."""
    rng = np.random.default_rng(seed)
    H, W = shape
    out = []
    for k in range(n):
        cy, cx = rng.uniform(-3, H + 3), rng.uniform(-3, W + 3)
        pts = star(rng, cy, cx, rng.uniform(1.5, max_radius), int(rng.integers(3, 13)))
        label = k + 1 if labels is None else labels[k]
        out.append((label, ring_of([p[0] for p in pts], [p[1] for p in pts], y_offset, x_offset)))
    return out


def rectangle(x0, y0, x1, y1, y_offset=0, x_offset=0):
    """The closed ring of a rectangle with corners (x0, y0), (x1, y1), plane coordinates."""
    return ring_of([x0, x1, x1, x0, x0], [y0, y0, y1, y1, y0], y_offset, x_offset)


def blobs_plane(seed, shape, n):
    """An int32 label plane of about n discs that do not touch (labels 1..)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    plane = np.zeros(shape, np.int32)
    yy, xx = np.mgrid[:H, :W]
    label = 0
    for _ in range(20 * n):
        if label == n:
            break
        r = int(rng.integers(3, 8))
        cy, cx = int(rng.integers(r + 2, H - r - 2)), int(rng.integers(r + 2, W - r - 2))
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        grown = (yy - cy) ** 2 + (xx - cx) ** 2 <= (r + 2) ** 2
        if plane[grown].any():
            continue
        label += 1
        plane[disc] = label
    return plane


def spanning(w, h, x0=3, y0=2):
    """A five-vertex ring whose box is exactly w columns x h rows at (x0, y0),
    every edge slanted."""
    return [(x0, y0 + h // 2), (x0 + w // 3, y0), (x0 + w - 1, y0 + h // 4),
            (x0 + w - 5, y0 + h - 1), (x0 + 5, y0 + (3 * h) // 4)]


def _build_cases():
    """name -> (plane_polygons, y_offset, x_offset, (height, width)): what the
    host core and the device are held to the literal on.  plane_polygons[i] is
    the (label, stored ring) list of plane i."""
    cases = {}

    def add(name, planes, dims, y_offset=0, x_offset=0):
        cases[name] = (planes, y_offset, x_offset, dims)

    def plane_ring(pts, y_offset=0, x_offset=0):
        return ring_of([p[0] for p in pts], [p[1] for p in pts], y_offset, x_offset)

    for k, (pts, shape, _) in enumerate(ANCHORS):
        add("anchor%d" % k, [[(1, plane_ring(pts))]], shape)
    # rings of one and of two vertices, wholly outside, over each plane edge, all four
    add("one_vertex", [[(5, plane_ring([(2, 2)]))]], (6, 7))
    add("two_vertices", [[(5, plane_ring([(1, 1), (4, 5)]))]], (6, 7))
    add("outside", [[(5, plane_ring([(20, 3), (30, 3), (25, 9)])),
                     (6, plane_ring([(2, -9), (5, -2), (1, -3)]))]], (6, 7))
    tri = [(0, 0), (9, 2), (3, 8)]
    for name, dx, dy in (("cross_left", -4, 3), ("cross_right", 14, 3), ("cross_top", 5, -4),
                         ("cross_bottom", 5, 9)):
        add(name, [[(7, plane_ring([(x + dx, y + dy) for x, y in tri]))]], (16, 20))
    add("cross_all", [[(7, plane_ring([(-3, 5), (8, -4), (25, 6), (11, 21)]))]], (16, 20))
    sq = [(2, 1), (9, 3), (7, 10), (1, 6)]
    add("unclosed", [[(3, plane_ring(sq))]], (12, 12))
    add("closed", [[(3, plane_ring(sq + sq[:1]))]], (12, 12))
    add("reversed", [[(3, plane_ring(sq[::-1]))]], (12, 12))
    add("bowtie", [[(4, plane_ring([(1, 1), (11, 9), (11, 1), (1, 9)]))]], (12, 14))
    # random stars on a 64 x 64 plane, with map offsets
    for n in (1, 2, 300):
        add("random%d" % n, [random_polygons(100 + n, n, (64, 64), 7000, -1234)], (64, 64),
            7000, -1234)
    # two overlapping rings, both list orders
    a = (11, plane_ring([(2, 2), (20, 4), (17, 19), (4, 15)]))
    b = (22, plane_ring([(10, 8), (27, 10), (25, 26), (8, 22)]))
    add("overlap_ab", [[a, b]], (30, 32))
    add("overlap_ba", [[b, a]], (30, 32))
    # equal labels on different rings, label 0, negative and extreme labels
    rings = [r for _, r in random_polygons(7, 8, (40, 48), max_radius=12.0)]
    add("labels", [list(zip([5, 5, 0, -3, 2 ** 31 - 1, -2 ** 31, 5, 1], rings))], (40, 48))
    # a 3 x 2 (t x z) stack of 96 x 80 planes, one of them empty
    stack = [random_polygons(200 + i, 12, (96, 80), -50, 300, max_radius=14.0) for i in range(6)]
    stack[4] = []
    add("stack", stack, (96, 80), -50, 300)
    # box widths across the bit rows' word boundaries, in LDS and through memory
    for w in (63, 64, 65, 129):
        add("width%d_lds" % w, [[(9, plane_ring(spanning(w, 12)))]], (16, w + 6))
        add("width%d_mem" % w, [[(9, plane_ring(spanning(w, 600)))]], (604, w + 6))
    # an edge spanning every row with a non-integer slope
    add("full_height", [[(2, plane_ring([(3, -2), (37, 99), (1, 80)]))]], (97, 41))
    # just below and just above the LDS threshold: 64 columns x 512 and x 513 rows
    add("threshold_below", [[(8, plane_ring([(0, 0), (63, 40), (40, 511), (10, 300)]))]], (513, 64))
    add("threshold_above", [[(8, plane_ring([(0, 0), (63, 40), (40, 512), (10, 300)]))]], (513, 64))
    # 20,005 vertices retracing a small box an odd number of times
    add("retrace", [[(6, plane_ring([(1, 0), (6, 2), (5, 6), (2, 5), (0, 3)] * 4001))]], (8, 8))
    # coordinates up to the limit, far outside the plane
    big = 2 ** 24 - 1
    add("extreme", [[(3, plane_ring([(-big, 3), (big, -big), (5, big), (-7, 11)], big - 9, 40 - big))]],
        (9, 10), big - 9, 40 - big)
    return cases


CASES = _build_cases()
_LITERAL = {}


def literal(name):
    """int32 [n_planes, H, W] of a case by the plain loops (computed once)."""
    if name not in _LITERAL:
        planes, y_offset, x_offset, dims = CASES[name]
        out = np.zeros((len(planes),) + tuple(dims), np.int32)
        for i, polygons in enumerate(planes):
            out[i] = create_from_polygons(polygons, y_offset, x_offset, dims)
        out.setflags(write=False)
        _LITERAL[name] = out
    return _LITERAL[name]


def box_words(ring, y_offset, x_offset, dims):
    """Bit-row words of a ring's clipped box: rows x ceil(columns / 64)."""
    xs, ys = transformed(ring, y_offset, x_offset)
    H, W = dims
    rows = min(H - 1, int(max(ys))) - int(max(0, min(ys))) + 1
    cols = min(W - 1, int(max(xs))) - int(max(0, min(xs))) + 1
    return max(rows, 0) * ((max(cols, 0) + 63) // 64)
