"""numpy literal of the reference's per-object rules (jterator's output loop).

Restated from reading tmlib/workflow/jterator/handles.py:399-551 and
tmlib/image.py:796 (mahotas itself is not installed here):
  labels      np.unique(value[value > 0])
  bbox        mh.labeled.bbox(plane): per label 0..max [min_y, max_y + 1,
              min_x, max_x + 1], zeros for a label without pixels
  centroids   mh.center_of_mass(plane, labels=plane): the plane's own values
              are the weights, so label L has sum(L * y) / sum(L)
  is_border   _find_border_objects: the label occurs in the first / last row
              or the first / last column
Plain loops over the labels: slow and obviously right.
"""
from functools import reduce

import numpy as np

ROW_DTYPE = np.dtype([("n", np.int64), ("sum_y", np.int64), ("sum_x", np.int64),
                      ("y0", np.int32), ("y1", np.int32), ("x0", np.int32), ("x1", np.int32),
                      ("border", np.int32), ("pad", np.int32)])


def object_rows(plane, max_label=None):
    """One row per label 0..max_label of a 2-D int32 plane."""
    plane = np.asarray(plane)
    H, W = plane.shape
    if max_label is None:
        max_label = max(int(plane.max()), 0)
    rows = np.zeros(max_label + 1, dtype=ROW_DTYPE)
    edge = set(plane[0, :].tolist()) | set(plane[-1, :].tolist()) | \
        set(plane[:, 0].tolist()) | set(plane[:, -1].tolist())
    for label in np.unique(plane).tolist():
        ys, xs = np.nonzero(plane == label)
        r = rows[label]
        r["n"] = ys.size
        r["sum_y"] = int(ys.astype(np.int64).sum())
        r["sum_x"] = int(xs.astype(np.int64).sum())
        r["y0"], r["y1"] = ys.min(), ys.max() + 1
        r["x0"], r["x1"] = xs.min(), xs.max() + 1
        r["border"] = 1 if label in edge else 0
    return rows


def bbox(plane):
    """mh.labeled.bbox(plane) as an [max_label + 1, 4] array."""
    r = object_rows(plane)
    return np.stack([r["y0"], r["y1"], r["x0"], r["x1"]], axis=1).astype(np.intp)


def iter_planes(value):
    """handles.py:220-235."""
    array = value
    if array.ndim == 2:
        array = array[..., np.newaxis, np.newaxis]
    elif array.ndim == 3:
        array = array[..., np.newaxis]
    for t in range(array.shape[-1]):
        for z in range(array[..., t].shape[-1]):
            yield ((t, z), array[:, :, z, t])


def labels(value):
    """handles.py:424."""
    return np.unique(value[value > 0]).astype(int).tolist()


def center_of_mass(plane):
    """mh.center_of_mass(plane, labels=plane): [max_label + 1, 2] float64,
    NaN for a label without weight (label 0 and absent labels)."""
    plane = np.asarray(plane)
    n = max(int(plane.max()), 0) + 1
    out = np.full((n, 2), np.nan)
    yy, xx = np.indices(plane.shape)
    for label in range(1, n):
        m = plane == label
        w = float(label) * float(np.count_nonzero(m))
        if w == 0.0:
            continue
        out[label, 0] = float(label * int(yy[m].sum())) / w
        out[label, 1] = float(label * int(xx[m].sum())) / w
    return out


def centroids_before_int(value, y_offset, x_offset):
    """The float (y, x) pairs handles.py:447-450 holds just before int():
    {(t, z): [max_label + 1, 2]}."""
    out = dict()
    for key, plane in iter_planes(value):
        c = center_of_mass(plane)
        c[:, 1] += x_offset
        c[:, 0] += y_offset
        c[:, 0] *= -1
        out[key] = c
    return out


def iter_points(value, y_offset, x_offset):
    """handles.py:444-455 with (x, y) in place of shapely's Point.  int() of a
    NaN centroid (a label absent from the plane) raises ValueError; so does,
    here, a label above the plane's own maximum (the reference indexes past
    mahotas' array there and raises IndexError: the same place, another type)."""
    labs = labels(value)
    cents = centroids_before_int(value, y_offset, x_offset)
    for key, _ in iter_planes(value):
        c = cents[key]
        for label in labs:
            if label >= len(c):
                raise ValueError("cannot convert float NaN to integer")
            y = int(c[label, 0])
            x = int(c[label, 1])
            yield (key[0], key[1], label, (x, y))


def find_border_objects(img):
    """handles.py:528-551."""
    edges = [np.unique(img[0, :]), np.unique(img[-1, :]), np.unique(img[:, 0]),
             np.unique(img[:, -1])]
    border_ids = list(reduce(set.union, map(set, edges)).difference({0}))
    object_ids = np.unique(img[img != 0])
    return {int(o): True if o in border_ids else False for o in object_ids}


def is_border(value):
    """handles.py:518-526."""
    mapping = dict()
    for (t, z), plane in iter_planes(value):
        for label, flag in find_border_objects(plane).items():
            mapping[(t, z, label)] = bool(flag)
    return mapping
