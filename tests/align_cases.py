"""Inputs of the align tests that are chosen for what the registration
kernels' host code does with them (pure numpy; test_align_cpu.py checks the
table, test_gpu_align.py runs it).

``geometry`` restates the rule by which ``reg_run`` and ``reg_scratch``
(tmlibrary_amd/csrc/register_kernels.hip) pick a launch's shape.  Like
``intensity_cases.bucket_of`` the restatement is a condition on the inputs:
PLANE_CASES is there to reach every class of that rule, and carries the values
the rule gave when the table was written, so a changed rule fails the CPU test
and the table is looked at again instead of silently covering less.
"""
from collections import namedtuple

import numpy as np

LDS_BYTES = 160 * 1024       # kLdsBytes
CHUNK_BYTES = 128 << 20      # kChunkBytes
MAX_LAUNCH = 32768           # pairs a launch takes, images a k_reg_sums launch takes
CF = 8                       # sizeof(cf)

Geometry = namedtuple("Geometry", "Mh Mw stride half_cols c groups chunk")


def _smooth(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def fft_line_length(L):
    """fft_core.h: L when it is 5-smooth, else the smallest 5-smooth m >= 2 L - 1."""
    if _smooth(L):
        return L
    m = 2 * L - 1
    while not _smooth(m):
        m += 1
    return m


def geometry(H, W, n=1):
    Mh, Mw = fft_line_length(H), fft_line_length(W)
    stride = Mh | 1
    half_cols = Mw // 2 + 1
    c = max(1, min(LDS_BYTES // (4 * stride * CF), 8, half_cols))
    groups = (half_cols + c - 1) // c
    chunk = max(1, min(n, MAX_LAUNCH, CHUNK_BYTES // (H * Mw * CF)))
    return Geometry(Mh, Mw, stride, half_cols, c, groups, chunk)


PlaneCase = namedtuple("PlaneCase", "shape dtype planted Mh Mw c half_cols groups why")
_u8, _u16 = np.uint8, np.uint16

#: one pair each, xcorr_literal.blob_pair(shape, *planted, seed=7, dtype=dtype)
PLANE_CASES = [
    PlaneCase((2, 2), _u16, (1, 0), 2, 2, 2, 2, 1, "everything exact: the bound is the floor alone"),
    PlaneCase((1, 64), _u16, (0, 6), 1, 64, 8, 33, 5, "Mh = 1"),
    PlaneCase((64, 1), _u16, (-5, 0), 64, 1, 1, 1, 1, "Mw = 1, c = half_cols = 1"),
    PlaneCase((30, 12), _u16, (3, -2), 30, 12, 7, 7, 1, "c = half_cols < 8"),
    PlaneCase((30, 13), _u8, (-2, 3), 30, 25, 8, 13, 2, "Mw padded to odd, last group padded"),
    PlaneCase((64, 64), _u8, (0, 9), 64, 64, 8, 33, 5,
              "pure radix 2, groups < 8, 7 padding slots"),
    PlaneCase((48, 81), _u16, (-7, 4), 48, 81, 8, 41, 6, "odd unpadded Mw: no Nyquist column"),
    PlaneCase((125, 128), _u16, (11, 0), 125, 128, 8, 65, 9, "5^3 with 2^7, groups % 8 = 1"),
    PlaneCase((64, 270), _u16, (4, -13), 64, 270, 8, 136, 17,
              "W > 256: the row argmax's thread stride; groups % 8 = 1 with q = 2"),
    PlaneCase((96, 53), _u16, (5, 7), 96, 108, 8, 55, 7, "x fold only"),
    PlaneCase((53, 96), _u16, (-6, -2), 108, 96, 8, 49, 7, "y fold only"),
    PlaneCase((37, 53), _u8, (5, 3), 75, 108, 8, 55, 7, "both folds"),
    PlaneCase((729, 40), _u8, (9, -4), 729, 40, 7, 21, 3, "the LDS limit gives c = 7"),
    PlaneCase((1024, 24), _u16, (-11, 5), 1024, 24, 4, 13, 4, "c = 4"),
    PlaneCase((2048, 20), _u16, (13, 2), 2048, 20, 2, 11, 6, "c = 2"),
    PlaneCase((1031, 20), _u8, (-8, -3), 2160, 20, 2, 11, 6,
              "tall and padded: the y fold at c = 2"),
    PlaneCase((4096, 6), _u16, (7, 1), 4096, 6, 1, 4, 4, "c = 1, the longest column"),
    PlaneCase((6, 4096), _u16, (-1, 12), 6, 4096, 8, 2049, 257, "the longest row, many groups"),
    PlaneCase((20, 2047), _u8, (2, -9), 20, 4096, 8, 2049, 257, "the longest padded row"),
]


def case_id(case):
    return "%dx%d_%s" % (case.shape[0], case.shape[1], np.dtype(case.dtype).name)


# ---- batches whose shifts hold by construction ----------------------------------------
BATCH_SHIFTS = [(3, -5), (0, 0), (-7, 2), (9, 9), (-1, -12), (4, 0), (0, -3)]
BATCH_REF_OF = [0, 2, 1, 1, 0, 2, 2]


def rolled_batch(shape, dtype=np.uint8, seed=90, impulses=40):
    """(targets [7], refs [3], ref_of, shifts): each reference is zeros plus
    ``impulses`` seeded pixels of random height, each target its reference
    rolled cyclically so that T[r, c] = R[r + dy, c + dx] exactly.  The plane's
    value at (dy, dx) is then the reference's autocorrelation at lag 0, which
    no other lag reaches."""
    H, W = shape
    top = np.iinfo(dtype).max
    refs = np.zeros((3, H, W), dtype)
    for k in range(3):
        rng = np.random.default_rng(seed + k)
        refs[k, rng.integers(0, H, impulses), rng.integers(0, W, impulses)] = \
            rng.integers(top // 4, top + 1, impulses)
    ref_of = np.array(BATCH_REF_OF, np.int32)
    targets = np.stack([np.roll(refs[k], (-dy, -dx), axis=(0, 1))
                        for (dy, dx), k in zip(BATCH_SHIFTS, ref_of)])
    return targets, refs, ref_of, list(BATCH_SHIFTS)


def tiny_batch(n=MAX_LAUNCH + 1, seed=5):
    """(targets, refs [n, 4, 4] uint8, ref_of, shifts [n, 2]): each reference
    is one pixel of 200, ``ref_of`` a permutation, target i reference
    ``ref_of[i]`` rolled by a shift from [-1, 2]^2 -- the four signed lags of an
    axis of 4.  One image more than a launch takes."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    pos = rng.integers(0, 4, (n, 2))
    refs = np.zeros((n, 4, 4), np.uint8)
    refs[idx, pos[:, 0], pos[:, 1]] = 200
    ref_of = rng.permutation(n).astype(np.int32)
    shifts = rng.integers(-1, 3, (n, 2))
    at = (pos[ref_of] - shifts) % 4
    targets = np.zeros((n, 4, 4), np.uint8)
    targets[idx, at[:, 0], at[:, 1]] = 200
    return targets, refs, ref_of, shifts


def literal_planes(targets, refs, ref_of):
    """xcorr_literal.plane over a stack: f64 planes [n, H, W], unsigned lags."""
    def centred(a):
        px = a.shape[1] * a.shape[2]
        sums = a.astype(np.int64).sum(axis=(1, 2))
        return a.astype(np.float64) - (sums / px)[:, None, None]
    ft = np.fft.fft2(centred(np.asarray(targets)))
    fr = np.fft.fft2(centred(np.asarray(refs)))[np.asarray(ref_of)]
    return np.fft.ifft2(np.conj(ft) * fr).real


def shifts_of_planes(planes):
    """[n, 2] signed (y, x) of each plane's first maximum."""
    n, H, W = planes.shape
    dy, dx = np.divmod(planes.reshape(n, -1).argmax(axis=1), W)
    return np.stack([np.where(dy <= H // 2, dy, dy - H), np.where(dx <= W // 2, dx, dx - W)],
                    axis=1)
