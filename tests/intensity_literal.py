"""The intensity rule of DESIGN.md section 27.1 in plain numpy and Python ints.

Rows by boolean masks, ``num = n * sum_sq - sum ** 2`` as a Python ``int``,
``float(num)`` (CPython rounds to nearest once), ``math.sqrt`` and ``/``.
"""
import math

import numpy as np

ROW_DTYPE = np.dtype([("sum", np.uint64), ("sum_sq", np.uint64), ("n", np.int64),
                      ("min", np.uint32), ("max", np.uint32)])
FEATURES = ("max", "mean", "min", "sum", "std")
EMPTY = (0, 0, 0, 0, 0)   # (sum, sum_sq, n, min, max)


def row_of(values):
    """(sum, sum_sq, n, min, max) of an iterable of pixel values, as Python ints"""
    v = [int(x) for x in values]
    if not v:
        return EMPTY
    return (sum(v), sum(x * x for x in v), len(v), min(v), max(v))


def plane_rows(labels, image, max_label):
    """rows [max_label + 1] of one label plane and one intensity plane; labels
    outside 0..max_label are skipped"""
    out = np.zeros(max_label + 1, ROW_DTYPE)
    for l in np.unique(labels):
        if 0 <= l <= max_label:
            out[l] = row_of(image[labels == l])
    return out


def table(labels, images, max_label):
    """rows [n_planes][max_label + 1][n_channels] of labels [n_planes][H][W] and
    images [n_channels][n_planes][H][W]"""
    out = np.zeros((labels.shape[0], max_label + 1, images.shape[0]), ROW_DTYPE)
    for p in range(labels.shape[0]):
        for c in range(images.shape[0]):
            out[p, :, c] = plane_rows(labels[p], images[c, p], max_label)
    return out


def as_ints(row):
    return tuple(int(row[k]) for k in ("sum", "sum_sq", "n", "min", "max"))


def merge(rows):
    """the planes of a group as one object: sums add, min / max over the
    planes that hold a pixel (empty rows store 0 and are skipped)"""
    rows = [r for r in rows if r[2] > 0]
    if not rows:
        return EMPTY
    return (sum(r[0] for r in rows), sum(r[1] for r in rows), sum(r[2] for r in rows),
            min(r[3] for r in rows), max(r[4] for r in rows))


def features(row):
    """[max, mean, min, sum, std] of (sum, sum_sq, n, min, max)"""
    s, q, n, lo, hi = row
    if n == 0:
        return [math.nan] * 5
    num = n * q - s * s
    return [float(hi), float(s) / float(n), float(lo), float(s), math.sqrt(float(num)) / float(n)]


def feature_table(rows, n_groups):
    """f64 [n_groups][n_labels][n_channels][5] of rows [n_planes][n_labels][n_channels]"""
    n_planes, n_labels, n_channels = rows.shape
    per = n_planes // n_groups
    assert per * n_groups == n_planes
    out = np.zeros((n_groups, n_labels, n_channels, 5), np.float64)
    for g in range(n_groups):
        for l in range(n_labels):
            for c in range(n_channels):
                out[g, l, c] = features(merge([as_ints(rows[g * per + z, l, c])
                                               for z in range(per)]))
    return out


def same_bits(a, b):
    """equal bit for bit; NaN equals NaN whatever its payload"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))
