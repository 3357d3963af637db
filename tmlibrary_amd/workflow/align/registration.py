"""Registration of sites across cycles (tmlib/workflow/align/registration.py).

``calculate_shift`` replaces the reference's ``image_registration.chi2_shift``
call (:23-41) with the GPU cross-correlation of include/tmhip.h
(``tmh_register_shifts``): the argmax of

    C[dy, dx] = sum_{r,c} T[r, c] * R[(r + dy) mod H, (c + dx) mod W]

over the mean-removed images, in signed form (a lag d along an axis of length
L is d if d <= L // 2, else d - L).  (y, x) means T[r, c] ~ R[r + y, c + x],
the sign ``_shift_and_crop`` / ``align_window`` expect.  ``calculate_shifts``
registers many pairs in one call, from numpy arrays or device tensors.
``calculate_overlap`` is the reference's (:44-86).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from tmlibrary_amd import hip


def _is_tensor(x):
    return hasattr(x, "data_ptr")


def _stack(x, name):
    """-> (pointer or host array, n, H, W, elem_bytes, on_device)."""
    if _is_tensor(x):
        if not x.is_cuda:
            x = x.numpy()
        else:
            if x.dim() == 2:
                x = x[None]
            if x.dim() != 3:
                raise ValueError("%s must be [H, W] or [n, H, W]" % name)
            if x.element_size() not in (1, 2) or x.is_floating_point():
                raise TypeError("%s must hold 8- or 16-bit unsigned integers" % name)
            if not x.is_contiguous():
                x = x.contiguous()
            return x, int(x.shape[0]), int(x.shape[1]), int(x.shape[2]), x.element_size(), True
    a = np.asarray(x)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("%s must be [H, W] or [n, H, W]" % name)
    if a.dtype not in (np.uint8, np.uint16):
        raise TypeError("%s must be uint8 or uint16" % name)
    a = np.ascontiguousarray(a)
    return a, a.shape[0], a.shape[1], a.shape[2], a.dtype.itemsize, False


def calculate_shifts(targets, references, ref_of_target=None, return_peak=False):
    """Shifts of ``targets`` [n, H, W] against ``references`` [m, H, W] (numpy
    uint8/uint16 arrays, or CUDA tensors of 8- or 16-bit integers read as
    unsigned): target i is registered against reference ``ref_of_target[i]``
    (default: i, which needs n == m; one reference serves every target).

    Returns (y, x) int32 arrays of length n, and with ``return_peak`` the f32
    correlation at the argmax; a pair in which either image is constant gives
    (0, 0) and a peak of exactly 0.  Raises ValueError for shapes that differ and
    for an axis over the kernels' limit (a transformed line holds 4,096
    values: 4,096 for a 5-smooth length, 2,048 otherwise)."""
    t, n, H, W, es, t_dev = _stack(targets, "targets")
    r, m, rH, rW, res, r_dev = _stack(references, "references")
    if (H, W) != (rH, rW):
        raise ValueError("targets %s and references %s differ in shape" % ((H, W), (rH, rW)))
    if es != res:
        raise TypeError("targets and references differ in element size")
    if t_dev != r_dev:
        raise TypeError("targets and references must both be arrays or both device tensors")
    if ref_of_target is None:
        if m == 1:
            ref_of_target = np.zeros(n, np.int32)
        elif m == n:
            ref_of_target = np.arange(n, dtype=np.int32)
        else:
            raise ValueError("ref_of_target is required for %d targets and %d references" % (n, m))
    rot = np.ascontiguousarray(ref_of_target, dtype=np.int32).reshape(-1)
    if rot.size != n:
        raise ValueError("ref_of_target must name one reference per target")
    if n and (rot.min() < 0 or rot.max() >= m):
        raise ValueError("ref_of_target holds an index outside the references")
    y, x = np.zeros(n, np.int32), np.zeros(n, np.int32)
    peak = np.zeros(n, np.float32)
    L = hip.lib()
    if t_dev:
        import torch
        sb = int(L.tmh_register_scratch_bytes(n, m, H, W))
        if sb < 0:
            hip.check(sb)
        scratch = torch.empty(max(sb, 256), dtype=torch.uint8, device=t.device)
        stream = torch.cuda.current_stream(t.device).cuda_stream
        with torch.cuda.device(t.device):
            hip.check(L.tmh_register_shifts_device(
                C.c_void_p(t.data_ptr()), n, C.c_void_p(r.data_ptr()), m, H, W, es, hip.ptr(rot),
                C.c_void_p(scratch.data_ptr()), sb, hip.ptr(y), hip.ptr(x), hip.ptr(peak),
                C.c_void_p(stream)))
    else:
        hip.check(L.tmh_register_shifts(hip.ptr(t), n, hip.ptr(r), m, H, W, es, hip.ptr(rot),
                                        hip.ptr(y), hip.ptr(x), hip.ptr(peak)))
    return (y, x, peak) if return_peak else (y, x)


def calculate_shift(target_image, reference_image):
    """registration.py:23-41: the displacement (y, x) of ``target_image``
    relative to ``reference_image``, plain ints."""
    t, r = np.asarray(target_image), np.asarray(reference_image)
    if t.ndim != 2 or r.ndim != 2:
        raise ValueError("images must be 2-D")
    y, x = calculate_shifts(t, r)
    return (int(y[0]), int(x[0]))


def xcorr_plane(target_image, reference_image):
    """The f32 correlation plane C[H, W] of one pair in unsigned lag order
    (``tmh_xcorr_plane``), from the mean-removed images."""
    t, _, H, W, es, _ = _stack(np.asarray(target_image), "target")
    r, _, rH, rW, res, _ = _stack(np.asarray(reference_image), "reference")
    if (H, W) != (rH, rW):
        raise ValueError("target %s and reference %s differ in shape" % ((H, W), (rH, rW)))
    if es != res:
        raise TypeError("target and reference differ in element size")
    out = np.empty((H, W), np.float32)
    hip.check(hip.lib().tmh_xcorr_plane(hip.ptr(t), hip.ptr(r), H, W, es, hip.ptr(out)))
    return out


def calculate_overlap(y_shifts, x_shifts):
    """registration.py:44-86: overhanging pixels (top, bottom, right, left) of
    the sites of one position across cycles -- top = |most negative y shift|,
    bottom = largest positive y shift, right = largest positive x shift, left =
    |most negative x shift|, each 0 when there is none."""
    y = np.asarray(y_shifts, dtype=np.int64).reshape(-1)
    x = np.asarray(x_shifts, dtype=np.int64).reshape(-1)
    top = int(-y[y < 0].min()) if np.any(y < 0) else 0
    bottom = int(y[y > 0].max()) if np.any(y > 0) else 0
    right = int(x[x > 0].max()) if np.any(x > 0) else 0
    left = int(-x[x < 0].min()) if np.any(x < 0) else 0
    return (top, bottom, right, left)
