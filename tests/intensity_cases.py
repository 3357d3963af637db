"""Label planes, intensity planes and rows the intensity tests share."""
import numpy as np

import intensity_literal as il

TILE = (16, 512)     # the table kernel's tile (measure_kernels.hip)
SHAPES = [(1, 1), (1, 65), (17, 513), (33, 1030)]


def cells(H, W, seed):
    """random cells 5 to 40 pixels across on background 0, later ones on top"""
    rng = np.random.default_rng(seed)
    plane = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    n = max(1, H * W // 400)
    for label in range(1, n + 1):
        ry, rx = rng.integers(5, 41, 2) / 2.0
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        plane[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = label
    return plane


def checkerboard(H, W):
    """labels 1 and 2 alternating: every pixel is a run of its own"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (1 + ((yy + xx) & 1)).astype(np.int32)


def image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def label_planes(kind, H, W, seed=0):
    if kind == "cells":
        return cells(H, W, seed)
    if kind == "checkerboard":
        return checkerboard(H, W)
    if kind == "full":
        return np.full((H, W), 3, np.int32)
    if kind == "background":
        return np.zeros((H, W), np.int32)
    raise KeyError(kind)


def many_labels_tile(n_labels=700):
    """one tile with n_labels distinct labels (1 ..), each a few short runs"""
    H, W = TILE
    idx = np.arange(H * W).reshape(H, W)
    return (1 + idx * n_labels // (H * W)).astype(np.int32)


def bucket_of(label, slots):
    """The LDS entry a label hashes to in both table kernels (label_tile.h, as
    include/tmhip.h documents it): the top log2(slots) bits of the label times
    the constant below, mod 2**32.  The hash restated here is a condition on
    the input: with another hash the labels of same_bucket_labels would spread
    over the table and the probe-limit tests would pass without reaching the
    probe limit."""
    bits = slots.bit_length() - 1
    assert 1 << bits == slots
    return ((label * 2654435761) & 0xFFFFFFFF) >> (32 - bits)


def same_bucket_labels(bucket, count, slots):
    """the first `count` labels (from 1) whose LDS entry is `bucket`"""
    out, label = [], 1
    while len(out) < count:
        if bucket_of(label, slots) == bucket:
            out.append(label)
        label += 1
    return out


def colliding_tile(slots, probe, extra=8):
    """(plane, labels): one tile whose probe + extra labels all hash to entry 7,
    in vertical stripes (many runs each), the rest of the table empty"""
    labels = same_bucket_labels(7, probe + extra, slots)
    H, W = TILE
    xx = np.mgrid[0:H, 0:W][1]
    plane = np.asarray(labels, np.int32)[(xx // 3) % len(labels)]
    return np.ascontiguousarray(plane), labels


def row(values):
    return il.row_of(values)


def scaled(n, value, minus_one_at=None):
    """the row of n pixels of `value` (optionally one of them `minus_one_at`
    instead), without building them"""
    if minus_one_at is None:
        return (n * value, n * value * value, n, value, value)
    v = minus_one_at
    return ((n - 1) * value + v, (n - 1) * value * value + v * v, n, min(v, value), max(v, value))


N_MAX = 2 ** 31 - 1
#: rows no small image gives, one per group: (sum, sum_sq, n, min, max)
EXTREME_ROWS = [
    scaled(N_MAX, 65535),                 # std exactly 0
    scaled(N_MAX, 65535, minus_one_at=0),
    scaled(N_MAX, 1, minus_one_at=65535),
    scaled(N_MAX // 2, 65535, minus_one_at=65534),
    row([12345]),                         # n = 1
    il.EMPTY,                             # n = 0: NaN
    row([0, 0, 0]),
    row([65534, 65535] * 50),
    (N_MAX // 2 * 65535, N_MAX // 2 * 65535 ** 2, N_MAX, 0, 65535),  # half 0, half 65,535
]
#: groups of three planes: an empty middle plane, an empty first plane, all empty, a zero minimum
MERGE_GROUPS = [
    [row([5, 9, 70]), il.EMPTY, row([3, 65535])],
    [il.EMPTY, row([7]), row([8, 2])],
    [il.EMPTY, il.EMPTY, il.EMPTY],
    [row([0, 4]), row([9]), il.EMPTY],
]


def rows_array(rows):
    out = np.zeros(len(rows), il.ROW_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def finalize_cases():
    """[(rows [n_planes][n_labels][1], n_groups)]: the extreme rows one plane per
    group, then the merge groups (planes of a group consecutive)"""
    extreme = rows_array(EXTREME_ROWS).reshape(1, len(EXTREME_ROWS), 1)
    merged = np.zeros((3, len(MERGE_GROUPS), 1), il.ROW_DTYPE)
    for l, group in enumerate(MERGE_GROUPS):
        for z, r in enumerate(group):
            merged[z, l, 0] = r
    return [(extreme, 1), (merged, 1), (np.concatenate([merged, merged[::-1]]), 2)]
