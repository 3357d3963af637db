"""Plain-loop literal of SegmentationImage.extract_polygons (tmlib/image.py:778-917).

Restated from reading the reference and from the definitions of what it calls
(neither cv2 nor mahotas is installed here):
  rule 1  the border-zeroed plane and the label loop          image.py:796-808
  rule 2  the padded bounding-box mask and mh.open            image.py:809-821
  rule 3  cv2.findContours(RETR_CCOMP, CHAIN_APPROX_NONE):    image.py:824-828
          Suzuki and Abe (1985), Algorithm 1, pixel by pixel
  rule 4  the choice of shell and holes                       image.py:829-869
  rule 5  the two fallback squares                            image.py:829-841, 871-882
  rule 6  offsets and the y flip                              image.py:886-893
The opening is scipy's.  Slow and obviously right.
"""
import numpy as np
from scipy import ndimage as ndi

import objects_literal as ol

CONTOUR_DTYPE = np.dtype([("plane", np.int32), ("label", np.int32), ("is_hole", np.int32),
                          ("parent", np.int32), ("point_offset", np.int64),
                          ("n_points", np.int64)])
OBJECT_DTYPE = np.dtype([("plane", np.int32), ("label", np.int32), ("first_contour", np.int64),
                         ("first_point", np.int64), ("n_contours", np.int32),
                         ("opened", np.int32), ("n_points", np.int64), ("n_interior", np.int64),
                         ("sum_y", np.int64), ("sum_x", np.int64)])

CROSS = ndi.generate_binary_structure(2, 1)

# clockwise with y pointing down, as (dy, dx): W, NW, N, NE, E, SE, S, SW
CLOCKWISE = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]


def open_cross(mask):
    """mh.open(mask): erosion, then dilation, by the 3x3 cross."""
    return ndi.binary_opening(mask, CROSS)


def find_contours(mask):
    """Rule 3 on a mask whose outermost rows and columns are zero.  Returns
    [(points int32 [n, 2] as (x, y), is_hole, parent)] in discovery order."""
    f = (np.asarray(mask) != 0).astype(np.int64)
    h, w = f.shape
    assert not f[0].any() and not f[-1].any() and not f[:, 0].any() and not f[:, -1].any()
    borders = []      # border number NBD is index + 2 (1 is the frame)
    nbd = 1
    for i in range(h):
        lnbd = 1
        for j in range(w):
            if f[i, j] == 0:
                continue
            if f[i, j] == 1 and f[i, j - 1] == 0:
                is_hole, start = 0, CLOCKWISE.index((0, -1))
            elif f[i, j] >= 1 and f[i, j + 1] == 0:
                is_hole, start = 1, CLOCKWISE.index((0, 1))
                if f[i, j] > 1:
                    lnbd = f[i, j]
            else:
                if f[i, j] != 1:
                    lnbd = abs(f[i, j])
                continue
            nbd += 1
            if is_hole:
                if lnbd == 1:
                    parent = -1
                else:
                    b = borders[lnbd - 2]
                    parent = b[2] if b[1] else lnbd - 2
            else:
                parent = -1
            points = []
            # (3.1) clockwise around (i, j) from the start neighbour
            first = None
            for t in range(8):
                dy, dx = CLOCKWISE[(start + t) % 8]
                if f[i + dy, j + dx] != 0:
                    first = (i + dy, j + dx)
                    break
            if first is None:
                f[i, j] = -nbd
                points.append((j, i))
            else:
                prev, cur = first, (i, j)
                while True:
                    # (3.3) counter-clockwise around cur, from one past prev
                    at = CLOCKWISE.index((prev[0] - cur[0], prev[1] - cur[1]))
                    east_zero = False
                    for t in range(1, 9):
                        dy, dx = CLOCKWISE[(at - t) % 8]
                        if f[cur[0] + dy, cur[1] + dx] != 0:
                            nxt = (cur[0] + dy, cur[1] + dx)
                            break
                        if (dy, dx) == (0, 1):
                            east_zero = True
                    # (3.4)
                    if east_zero:
                        f[cur] = -nbd
                    elif f[cur] == 1:
                        f[cur] = nbd
                    points.append((cur[1], cur[0]))
                    # (3.5)
                    if nxt == (i, j) and cur == first:
                        break
                    prev, cur = cur, nxt
            borders.append((np.array(points, dtype=np.int32).reshape(-1, 2), is_hole, parent))
            # (4)
            if f[i, j] != 1:
                lnbd = abs(f[i, j])
    return borders


def cv2_order(n):
    """List position -> discovery index of the cv2-shaped list: reverse
    discovery order (rests on reading)."""
    return list(range(n - 1, -1, -1))


def cv2_shaped(borders):
    """(contours, hierarchy) as cv2.findContours returns them: contours a list
    of int32 [n, 1, 2], hierarchy [1, n, 4] of [next, previous, first child,
    parent] list positions, -1 for none."""
    n = len(borders)
    order = cv2_order(n)
    pos = {d: p for p, d in enumerate(order)}
    contours = [borders[d][0].reshape(-1, 1, 2).copy() for d in order]
    hier = np.full((1, n, 4), -1, dtype=np.int32)
    for p, d in enumerate(order):
        parent = borders[d][2]
        hier[0, p, 3] = pos[parent] if parent >= 0 else -1
    for p in range(n):
        same = [q for q in range(n) if hier[0, q, 3] == hier[0, p, 3]]
        at = same.index(p)
        hier[0, p, 0] = same[at + 1] if at + 1 < len(same) else -1
        hier[0, p, 1] = same[at - 1] if at > 0 else -1
        kids = [q for q in range(n) if hier[0, q, 3] == p]
        hier[0, p, 2] = kids[0] if kids else -1
    return contours, hier


def square(x, y):
    return np.array([[x - 1, x + 1, x + 1, x - 1, x - 1],
                     [y - 1, y - 1, y + 1, y + 1, y - 1]]).T.astype(np.int32)


def zero_border(plane):
    out = np.array(plane, copy=True)
    out[0, :] = 0
    out[-1, :] = 0
    out[:, 0] = 0
    out[:, -1] = 0
    return out


def object_mask(plane0, bbox, label):
    """Rule 2: (mask, opened)."""
    cut = plane0[bbox[0]:bbox[1], bbox[2]:bbox[3]]
    mask = np.pad(cut, 1, mode="constant", constant_values=0) == label
    if np.sum(mask > 0) > 1:
        return open_cross(mask), 1
    return mask, 0


def extract_polygons(plane, y_offset, x_offset):
    """[(label, shell, holes)]: shell int32 [n, 2], holes a list of such or None."""
    plane = np.asarray(plane)
    bboxes = ol.bbox(plane)
    plane0 = zero_border(plane)
    out = []
    for label in np.unique(plane0[plane0 > 0]):
        bbox = bboxes[label]
        mask, _ = object_mask(plane0, bbox, label)
        contours, hierarchy = cv2_shaped(find_contours(mask))
        if len(contours) == 0:
            coords = np.array(np.where(plane0 == label)).T
            y, x = np.mean(coords, axis=0).astype(int)
            shell = square(x, y)
            holes = None
        elif len(contours) > 1:
            holes = list()
            for i in range(len(contours)):
                child_idx = hierarchy[0][i][2]
                parent_idx = hierarchy[0][i][3]
                if parent_idx >= 0:
                    shell = np.squeeze(contours[parent_idx])
                elif child_idx >= 0:
                    holes.append(np.squeeze(contours[child_idx]))
                else:
                    lengths = [len(c) for c in contours]
                    idx = lengths.index(np.max(lengths))
                    shell = np.squeeze(contours[idx])
                    break
        else:
            shell = np.squeeze(contours[0])
            holes = None
        if shell.ndim < 2 or shell.shape[0] < 3:
            y, x = np.array(mask.shape) // 2
            shell = square(x, y)
        add_y = y_offset + bbox[0] - 1
        add_x = x_offset + bbox[2] - 1
        shell[:, 0] = shell[:, 0] + add_x
        shell[:, 1] = -1 * (shell[:, 1] + add_y)
        if holes is not None:
            for i in range(len(holes)):
                holes[i][:, 0] = holes[i][:, 0] + add_x
                holes[i][:, 1] = -1 * (holes[i][:, 1] + add_y)
        out.append((int(label), shell, holes))
    return out


def iter_polygons(value, y_offset, x_offset):
    """handles.py:457-479: [(t, z, label, shell, holes)] in plane order."""
    out = []
    for (t, z), plane in ol.iter_planes(value):
        for label, shell, holes in extract_polygons(plane, y_offset, x_offset):
            out.append((t, z, label, shell, holes))
    return out


def object_contours(planes, max_label=None):
    """What tmh_object_contours reports for int32 planes [n, H, W]: (objects
    [n, max_label + 1], contours, points int32 [n_points, 2]) -- every label's
    borders in discovery order, objects in (plane, label) order."""
    planes = np.asarray(planes)
    if max_label is None:
        max_label = max(int(planes.max()), 0)
    objects = np.zeros((planes.shape[0], max_label + 1), dtype=OBJECT_DTYPE)
    contours, points = [], []
    n_points = 0
    for p, plane in enumerate(planes):
        rows = ol.object_rows(plane, max_label)
        plane0 = zero_border(plane)
        for label in range(max_label + 1):
            o = objects[p, label]
            o["plane"], o["label"] = p, label
            o["first_contour"], o["first_point"] = len(contours), n_points
            if label == 0 or rows[label]["n"] == 0:
                continue
            ys, xs = np.nonzero(plane0 == label)
            o["n_interior"], o["sum_y"], o["sum_x"] = ys.size, ys.sum(), xs.sum()
            if ys.size == 0:
                continue
            r = rows[label]
            mask, o["opened"] = object_mask(plane0, (r["y0"], r["y1"], r["x0"], r["x1"]), label)
            for pts, is_hole, parent in find_contours(mask):
                contours.append((p, label, is_hole, parent, n_points, len(pts)))
                points.append(pts)
                n_points += len(pts)
                o["n_contours"] += 1
                o["n_points"] += len(pts)
    table = np.array(contours, dtype=CONTOUR_DTYPE) if contours else np.zeros(0, CONTOUR_DTYPE)
    pts = np.concatenate(points) if points else np.zeros((0, 2), np.int32)
    return objects, table, pts.astype(np.int32)
