"""The align step's registration rule, written out in numpy f64 (test oracle).

    C[dy, dx] = sum_{r,c} T[r, c] * R[(r + dy) mod H, (c + dx) mod W]

computed from the mean-removed images; the shift is the argmax of C (ties: the
lowest flat index dy * W + dx, np.argmax's choice) taken to signed form: a lag
d along an axis of length L is d if d <= L // 2, else d - L.  So (y, x) means
T[r, c] ~ R[r + y, c + x], the sign tmlib's _shift_and_crop expects.

brute_plane is the direct sum, used on small shapes to pin the FFT form's
sign; plane_c64 is the same FFT form in numpy's single precision, the
yardstick for what f32 arithmetic costs.  blob_pair builds the test inputs.
"""
import numpy as np


def _centered(a):
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("images must be 2-D")
    total = int(a.astype(np.int64).sum()) if a.dtype.kind in "ui" else None
    mean = total / a.size if total is not None else float(a.astype(np.float64).mean())
    return a.astype(np.float64) - mean


def plane(target, reference):
    """C in unsigned lag order, f64."""
    t, r = _centered(target), _centered(reference)
    if t.shape != r.shape:
        raise ValueError("target and reference differ in shape")
    return np.fft.ifft2(np.conj(np.fft.fft2(t)) * np.fft.fft2(r)).real


def plane_c64(target, reference):
    """The same form with every transform in complex64 (numpy >= 2 keeps it)."""
    t = _centered(target).astype(np.complex64)
    r = _centered(reference).astype(np.complex64)
    out = np.fft.ifft2(np.conj(np.fft.fft2(t)) * np.fft.fft2(r))
    assert out.dtype == np.complex64, "numpy promoted the single-precision transform"
    return out.real


def brute_plane(target, reference):
    """The definition as a direct sum (small shapes only)."""
    t, r = _centered(target), _centered(reference)
    H, W = t.shape
    out = np.empty((H, W))
    for dy in range(H):
        for dx in range(W):
            out[dy, dx] = np.sum(t * np.roll(r, (-dy, -dx), axis=(0, 1)))
    return out


def signed_lag(d, L):
    d = int(d)
    return d if d <= L // 2 else d - L


def shift_of_plane(c):
    H, W = c.shape
    dy, dx = divmod(int(np.argmax(c)), W)
    return signed_lag(dy, H), signed_lag(dx, W)


def shift(target, reference):
    return shift_of_plane(plane(target, reference))


def peak_margin(c):
    """(peak - the largest value outside the peak's cyclic 3x3 neighbourhood)
    / (max - min): the condition under which an f32 plane has the same argmax
    up to that neighbourhood.  1.0 for a plane that is one neighbourhood."""
    H, W = c.shape
    dy, dx = divmod(int(np.argmax(c)), W)
    mask = np.ones(c.shape, bool)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            mask[(dy + a) % H, (dx + b) % W] = False
    span = float(c.max() - c.min())
    if not mask.any() or span == 0.0:
        return 1.0
    return float(c.max() - c[mask].max()) / span


def blob_field(height, width, seed):
    """Background 200 plus ~1 Gaussian blob per 400 px (sigma 1.5-3.5 px,
    amplitude 300-3000), f64."""
    rng = np.random.default_rng(seed)
    f = np.full((height, width), 200.0)
    n = max(1, (height * width) // 400)
    ys, xs = rng.uniform(0, height, n), rng.uniform(0, width, n)
    sig, amp = rng.uniform(1.5, 3.5, n), rng.uniform(300.0, 3000.0, n)
    k = 12
    g = np.arange(-k, k + 1)
    for y, x, s, a in zip(ys, xs, sig, amp):
        iy, ix = int(y), int(x)
        r0, r1 = max(0, iy - k), min(height, iy + k + 1)
        c0, c1 = max(0, ix - k), min(width, ix + k + 1)
        gy = np.exp(-0.5 * ((g[r0 - iy + k:r1 - iy + k] + iy - y) / s) ** 2)
        gx = np.exp(-0.5 * ((g[c0 - ix + k:c1 - ix + k] + ix - x) / s) ** 2)
        f[r0:r1, c0:c1] += a * gy[:, None] * gx[None, :]
    return f


def blob_pair(shape, dy, dx, seed=7, dtype=np.uint16, noise=True, pad=16):
    """(target, reference): two H x W windows of one blob field with
    T[r, c] ~ R[r + dy, c + dx] (edges not cyclic; |dy|, |dx| <= pad); with
    `noise`, gain 1.1 on the target and independent sigma = 8 noise on each.
    The reference depends on (shape, seed, dtype, noise, pad) only, so several
    targets of different shifts share it."""
    H, W = shape
    assert abs(dy) <= pad and abs(dx) <= pad
    f = blob_field(H + 2 * pad, W + 2 * pad, seed)
    r = f[pad:pad + H, pad:pad + W]
    t = f[pad + dy:pad + dy + H, pad + dx:pad + dx + W]
    if noise:
        r = r + np.random.default_rng(seed + 1000).normal(0.0, 8.0, r.shape)
        rng = np.random.default_rng([seed + 2000, dy + pad, dx + pad])
        t = 1.1 * t + rng.normal(0.0, 8.0, t.shape)
    top = np.iinfo(dtype).max
    if dtype == np.uint8:
        t, r = t / 24.0, r / 24.0
    return (np.clip(np.rint(t), 0, top).astype(dtype), np.clip(np.rint(r), 0, top).astype(dtype))
