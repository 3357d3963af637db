"""Inputs that fill the f64 fixup list (FixList, csrc/common.h) past its
capacity, and the conditions that make them do so, shared by
test_overflow_cases_cpu.py (the conditions, from the oracle alone) and
test_gpu_fix_overflow.py (the kernels).  Built once per process.

The recipe: a mean plane near 2.5, a std plane of 0.1 except a few pixels (a
row, or one 8-pixel group) with a large std, which lifts mean(std) so that the
gain a = mean(std) / std is about 2.9 everywhere else; pixels uniform in
[20000, 65535] then correct to 6e7 .. 2e9 -- far beyond the f32 error bound
(common.h: |o| (K1 a + K2) < 1), so every pixel off the large-std ones is
flagged, and large enough that an f32 value alone is more than 1 DN off
modulo 2**16: a fixup that skips, truncates or misplaces pixels fails the
suite's own +-1 DN bar.  All of this is checked here from the oracle's f64
arithmetic: conditions on the inputs, not measurements.
"""
import functools

import numpy as np

from oracle import corilla_oracle as orc

K1, K2 = 6.7e-6, 4.2e-6  # csrc/common.h kRefineK1 / kRefineK2


def fix_capacity(n_sites, npx):
    """Entries of a launch's fixup list (csrc/abi_apply.hip:103,
    corrector_fixlist): 1/1024 of the launch's pixels, at least 2**20, at most
    2**30.  A corrector keeps the largest list it has needed, so this holds for
    a fresh corrector.  An entry is a pixel (plain and stack passes) or a group
    of 8 (chain and fused passes); a count above it makes the fixup kernels
    recompute every pixel of the launch."""
    return min(max(1 << 20, n_sites * npx // 1024), 1 << 30)


class Case(object):
    """sites [n, H, W], the (mean, std) planes as passed to the corrector."""

    def __init__(self, sites, mean, std, log=True):
        self.sites, self.mean, self.std, self.log = sites, mean, std, log
        self.n, self.H, self.W = sites.shape
        self.npx = self.H * self.W
        self.bits = 8 * sites.dtype.itemsize

    @functools.lru_cache(maxsize=None)
    def f64(self):
        """The corrected values before the cast, op for op as
        orc.correct_illumination (image.py:619-631) -- tied to it by want()."""
        x = self.sites.astype(np.float64)
        if self.log:
            x[x == 0] = 10 ** -10
            x = np.log10(x)
        x = (x - self.mean) / self.std
        x = (x * np.mean(self.std)) + np.mean(self.mean)
        return 10 ** x if self.log else x

    @functools.lru_cache(maxsize=None)
    def want(self):
        """The oracle's corrected sites (no clip)."""
        w = np.stack([orc.correct_illumination(s, self.mean, self.std, self.log)
                      for s in self.sites])
        assert np.array_equal(w, orc.cast_float_to_uint_x86(self.f64(), self.sites.dtype))
        return w

    @functools.lru_cache(maxsize=None)
    def flagged(self):
        """Pixels every streaming kernel flags: |o| (K1 a + K2) >= 1.01 with the
        pixel's own gain a.  The kernels flag at 1 (plain and stack: |o| >= T
        with the largest a of the image, a lower threshold) or at 0.998 / 1.002
        (fused and chain, the chain with the largest a of the pixel's group);
        their f32 value is within (K1 a + K2) < 1e-4 relative of o, so 1 % of
        margin puts these pixels on the list whatever the rounding."""
        o = self.f64()
        assert np.isfinite(o).all()
        a =np.abs(np.mean(self.std) / self.std)
        return np.abs(o) * (K1 * a + K2) >= 1.01

    @functools.lru_cache(maxsize=None)
    def f32_only(self):
        """The f64 value only rounded to f32 and cast as the oracle casts: the
        best an unrefined pixel can be.  (Beyond int32 the cast gives INT_MIN
        for either value: such pixels never count as wrong here.)"""
        o32 = self.f64().astype(np.float32).astype(np.float64)
        return orc.cast_float_to_uint_x86(o32, self.sites.dtype)

    def flagged_groups(self):
        """[n, ceil(npx / 8)]: groups of 8 consecutive pixels holding a flagged one."""
        f = self.flagged().reshape(self.n, -1)
        pad = (-f.shape[1]) % 8
        f = np.pad(f, ((0, 0), (0, pad)))
        return f.reshape(self.n, -1, 8).any(axis=2)

    def bad_if_unrefined(self, clip=None):
        """Flagged pixels that miss the suite's bar (assert_dn: more than 1 DN
        off, non-modular, a wrap flip included) if left at the f32 value."""
        got, want = self.f32_only(), self.want()
        if clip is not None:
            got, want = np.clip(got, *clip), np.clip(want, *clip)
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        return self.flagged() & (d > 1)


def check_pixel_overflow(case, clip=None, n_launch=None):
    """The conditions of a plain (per pixel) overflow case; returns the counts."""
    cap = fix_capacity(case.n if n_launch is None else n_launch, case.npx)
    fl = case.flagged()
    n_fl = int(np.count_nonzero(fl))
    assert n_fl >= 1.2 * cap, (n_fl, cap)
    bad = case.bad_if_unrefined(clip)
    for i in range(case.n):
        assert 2 * np.count_nonzero(bad[i]) >= np.count_nonzero(fl[i]) > 0, i
        tail = case.npx % 8
        if tail:  # the partial last group of a site in all mode
            assert bad[i].reshape(-1)[-tail:].any(), i
    return dict(flagged=n_fl, capacity=cap, bad=int(np.count_nonzero(bad)))


def check_group_overflow(case, inside=None):
    """The conditions of a fused (per group of 8) overflow case; inside: a
    bool mask [n, H, W] of the pixels that count (the chain's source windows)."""
    assert case.npx % 8 == 0
    cap = fix_capacity(case.n, case.npx)
    g = case.flagged_groups()
    if inside is not None:  # groups wholly inside: a lower bound on what is pushed
        g = g & inside.reshape(case.n, -1, 8).all(axis=2)
    n_g = int(np.count_nonzero(g))
    assert n_g >= 1.2 * cap, (n_g, cap)
    return dict(flagged_groups=n_g, capacity=cap)


def recipe_planes(H, W, seed, big_rows=(), big_std=100.0, big_group=None, mean0=2.5, std0=0.1):
    rng = np.random.default_rng(seed)
    mean = mean0 + 0.01 * rng.random((H, W))
    std = np.full((H, W), std0)
    for r in big_rows:
        std[r] = big_std
    if big_group is not None:  # one 8-pixel group
        std.reshape(-1)[8 * big_group:8 * big_group + 8] = big_std
    return mean, std


def uniform_sites(n, H, W, seed, lo, hi, dtype=np.uint16):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi + 1, (n, H, W)).astype(dtype)


@functools.lru_cache(maxsize=None)
def plain_log(shape=(512, 512)):
    """5 sites, 1,310,720 pixels (512 x 512) against 2**20 entries; 511 x 513
    has npx % 8 == 7 (the scalar streaming kernel, a partial last group)."""
    H, W = shape
    mean, std = recipe_planes(H, W, 11, big_rows=(H // 2,))
    return Case(uniform_sites(5, H, W, 12, 20000, 65535), mean, std)


@functools.lru_cache(maxsize=None)
def plain_nolog():
    """No log transform: o = (x - mean) a + M with a about 6,000 (one row of
    std 3e5 in a plane of 0.1), x in [20000, 65535]: 1.2e8 .. 3.9e8, past 2**25
    (an f32 step of 8 .. 32) and inside int32."""
    H, W = 512, 512
    mean, std = recipe_planes(H, W, 21, big_rows=(H // 2,), big_std=3.0e5, mean0=100.0)
    return Case(uniform_sites(5, H, W, 22, 20000, 65535), mean, std, log=False)


@functools.lru_cache(maxsize=None)
def plain_u8():
    """8-bit sites: pixels in [150, 255], mean near 0.5, a about 4.5 (one row of
    std 180 in a plane of 0.1): 1e8 .. 1.2e9, an f32 step of 8 .. 128 against
    the 8-bit wrap."""
    H, W = 512, 512
    mean, std = recipe_planes(H, W, 31, big_rows=(H // 2,), big_std=180.0, mean0=0.5)
    return Case(uniform_sites(5, H, W, 32, 150, 255, np.uint8), mean, std)


@functools.lru_cache(maxsize=None)
def full_size():
    """2 sites of 2160 x 2560: 1,382,400 groups of 8 against 2**20 entries."""
    H, W = 2160, 2560
    mean, std = recipe_planes(H, W, 41, big_rows=(500, 1000, 1500, 2000))
    return Case(uniform_sites(2, H, W, 42, 20000, 65535), mean, std)


@functools.lru_cache(maxsize=None)
def ordinary():
    """One synthetic 2160 x 2560 site under planes with a dim left edge (a small
    std there: a gain of about 3), where a few bright pixels pass the f32
    bound: a job whose list holds some hundreds of groups."""
    from tmlibrary_amd.synth import synth_exact_host
    H, W = 2160, 2560
    yy, xx = np.mgrid[0:H, 0:W]
    mean = 2.45 + 0.15 * np.exp(-((yy - H / 2.0) ** 2 + (xx - W / 2.0) ** 2) / (0.3 * H * W))
    std = 0.06 + 0.25 * (xx / float(W))
    sites = synth_exact_host(H, W, 707, 0, 0)[None].copy()
    sites[0, ::37, 0:64:9] = 20000
    return Case(sites, mean, std)


@functools.lru_cache(maxsize=None)
def lds_set():
    """6 sites of 240 x 320 (9,600 groups each, 57,600 in all: far under the
    list's capacity), every group but one per site flagged: the large std sits
    in ONE group (1,800 there: a about 2.9 elsewhere)."""
    H, W = 240, 320
    mean, std = recipe_planes(H, W, 51, big_group=4321, big_std=1800.0)
    return Case(uniform_sites(6, H, W, 52, 20000, 65535), mean, std)


FUSED_BANDS = (8, 16, 32, 64)  # tmhip.h TMH_OPT_FUSED_BANDS; fused_bands() doubles 8 / 16 up to 64
FUSED_SPU = (4,)               # sites per unit of both configurations (fused_kernels.hip kNarrowCfg, kWideCfg)
FIX_SH = 256                   # fused_kernels.hip kFixSh: a unit's LDS fixup set


def min_unit_groups(case):
    """The fewest flagged groups any unit of the fused pass holds, over every
    band count and sites-per-unit a configuration can run with: a unit is the
    groups [band * G / n_bands, (band + 1) * G / n_bands) (G groups per site,
    k_correct_hist decode()) of SPU consecutive sites (the last unit of a job
    may hold fewer)."""
    g = case.flagged_groups()
    G = g.shape[1]
    worst = None
    for nb in FUSED_BANDS:
        edges = [b * G // nb for b in range(nb + 1)]
        per = np.stack([g[:, edges[b]:edges[b + 1]].sum(axis=1) for b in range(nb)], axis=1)
        for spu in FUSED_SPU:
            for s0 in range(0, case.n, spu):
                m = int(per[s0:s0 + spu].sum(axis=0).min())
                worst = m if worst is None else min(worst, m)
    return worst


def chain_windows(shape, shifts, residues):
    from tmlibrary_amd.image import align_window
    return np.stack([align_window(shape, y, x, *residues, crop=False)[0] for y, x in shifts])


def window_mask(case, wins):
    """[n, H, W]: the pixels inside each site's SOURCE window."""
    m = np.zeros(case.sites.shape, bool)
    for i, w in enumerate(wins):
        r0, c0 = int(w["src_r0"]), int(w["src_c0"])
        m[i, r0:r0 + int(w["rows"]), c0:c0 + int(w["cols"])] = True
    return m


CHAIN_SHIFTS = [(0, 0), (2, -3)]
CHAIN_RESIDUES = (4, 4, 8, 8)  # as test_chain_overflow_wrap_and_beyond_int32


def chain_bytes(case, v16, i, bounds):
    """Site i's chain output from corrected uint16 values (the oracle's align,
    clip and scale, oracle.illuminati_chain after its correction)."""
    b, t, r, l = CHAIN_RESIDUES
    y, x = CHAIN_SHIFTS[i]
    out = orc.shift_and_crop(v16, y, x, b, t, r, l, crop=False)
    return orc.map_to_uint8(np.clip(out, *bounds), *bounds)


#: pixels per site whose byte must be more than 1 off if left at the f32 value.
#: Bounds (0, 65535) scale by 1 / 257: a byte is 257 DN wide and an f32 step
#: at most 128 DN here, so only values within a step of a multiple of 65,536
#: (byte 255 against 0) can miss the bar -- about 128 / 65536 / 2 of 5.4 M
#: window pixels, some 2,000 a site at the top of the range and fewer below.
CHAIN_BAD_AT_LEAST = {(100, 3000): 10000, (0, 65535): 1000}


def check_chain_overflow(case, bounds):
    """Capacity from the groups inside each source window; CHAIN_BAD_AT_LEAST
    pixels per site whose byte is more than 1 off if left at the f32 value."""
    wins = chain_windows((case.H, case.W), CHAIN_SHIFTS, CHAIN_RESIDUES)
    inside = window_mask(case, wins)
    res = check_group_overflow(case, inside)
    bad = []
    for i in range(case.n):
        fl = np.where(case.flagged()[i], case.f32_only()[i], case.want()[i])
        d = np.abs(chain_bytes(case, fl, i, bounds).astype(np.int32)
                   - chain_bytes(case, case.want()[i], i, bounds).astype(np.int32))
        bad.append(int(np.count_nonzero(d > 1)))
        assert bad[-1] >= CHAIN_BAD_AT_LEAST[bounds], (i, bounds, bad[-1])
    res["bad"] = bad
    return res, wins


STACK_SLOTS = 3
STACK_EXTENT = (508, 506)
#: (site, slot, src_r0, src_c0) of the 5 planes: 2 sites x 3 slots, (1, 1) unmapped
STACK_PLANES = [(0, 0, 1, 3), (1, 2, 4, 6), (0, 2, 2, 0), (1, 0, 3, 5), (0, 1, 0, 1)]


def stack_layout():
    from tmlibrary_amd import hip
    site = np.array([p[0] for p in STACK_PLANES], np.int32)
    slot = np.array([p[1] for p in STACK_PLANES], np.int32)
    win = np.zeros(len(STACK_PLANES), dtype=hip.WINDOW_DTYPE)
    for k, (_, _, r0, c0) in enumerate(STACK_PLANES):
        win[k]["src_r0"], win[k]["src_c0"] = r0, c0
        win[k]["rows"], win[k]["cols"] = STACK_EXTENT
    return site, slot, win


def check_stack_overflow(case):
    """The stack pass pushes the flagged pixels inside each plane's window;
    its list is sized for n_planes sites."""
    site, slot, win = stack_layout()
    inside = window_mask(case, win)
    cap = fix_capacity(case.n, case.npx)
    fl = case.flagged() & inside
    n_fl = int(np.count_nonzero(fl))
    assert n_fl >= 1.2 * cap, (n_fl, cap)
    bad = case.bad_if_unrefined() & inside
    for i in range(case.n):
        assert 2 * np.count_nonzero(bad[i]) >= np.count_nonzero(fl[i]) > 0, i
    return dict(flagged=n_fl, capacity=cap, bad=int(np.count_nonzero(bad)))
