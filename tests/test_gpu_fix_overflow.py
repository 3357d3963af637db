"""GPU: the routes a full fixup structure takes.

A streaming correct kernel appends the pixels whose f32 result may be more
than 1 DN off to a bounded list (FixList, csrc/common.h); when the count ends
above the list's capacity the fixup kernels ignore the list and recompute
every pixel of the launch in f64 ("all" mode).  A unit of the fused pass
stages its flagged groups in a 256-entry LDS set and sends the rest straight
to the list.  The inputs (tests/overflow_cases.py) flag more than the
structure holds, most of the flagged pixels wrong if left at their f32 value;
each test repeats those conditions, from the oracle alone, before it launches
anything.  Results are held to the suite's bars against the oracle on the
planes as passed: +-1 DN non-modular with no wrap flip (uint16 / uint8
corrected values), |byte difference| <= 1 (the chain's uint8).

Input and output of the device entry points must not overlap (the fixups
re-read the input): the last tests check that such calls are refused.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import overflow_cases as oc
from oracle import corilla_oracle as orc
from test_gpu_fullsize import _results, _stats_handle
from tmlibrary_amd import hip
from util import assert_dn, dn_report, keep  # noqa: F401 (keep: a fixture)

pytestmark = pytest.mark.gpu

Q = 100000


@pytest.fixture(scope="module")
def L():
    return hip.lib()


def new_corrector(case):
    """A fresh corrector: its list has the capacity of overflow_cases.fix_capacity."""
    from tmlibrary_amd.image import Corrector
    return Corrector(case.mean, case.std, log_transform=case.log)


def report(name, got, want, bits=16):
    print("%s: (worst DN, flips, at +-1) per site %s, exact pixels %d of %d" % (
        name, [dn_report(g, w, bits) for g, w in zip(got, want)],
        int(np.count_nonzero(got == want)), got.size))


# ---- B: the list above capacity -----------------------------------------------------

PLAIN = {"log": oc.plain_log, "nolog": oc.plain_nolog, "scalar": lambda: oc.plain_log((511, 513))}


@pytest.mark.parametrize("name,clip", [("log", None), ("log", (1000, 60000)), ("nolog", None),
                                       ("nolog", (1000, 60000)), ("scalar", None)])
def test_plain_u16_list_overflow(L, keep, name, clip):
    """k_fix_correct<LOG, uint16_t, 16> (apply_kernels.hip) in all mode after
    k_correct_u16_vec8 (512 x 512) or k_correct_scalar (511 x 513: npx % 8 ==
    7, so every site's last group of the all-mode walk is partial and its
    p >= npx guard decides): 1.3 M flagged pixels of 5 sites against 2**20
    entries, 88 % of them wrong if left unrefined (check_pixel_overflow)."""
    case = PLAIN[name]()
    print(oc.check_pixel_overflow(case, clip))
    assert (case.npx % 8 == 7) == (name == "scalar")
    corr = new_corrector(case)
    d_in = keep(hip.DeviceBuffer(case.sites.nbytes))
    d_out = keep(hip.DeviceBuffer(case.sites.nbytes))
    d_in.put(case.sites)
    d_out.put(np.full(case.sites.shape, 0xA5A5, np.uint16))
    lo, hi = clip or (-1, -1)
    hip.check(L.tmh_correct_u16_device(corr._h, d_in, d_out, case.n, lo, hi, None))
    assert L.tmh_synchronize(None) == 0
    got = d_out.get(case.sites.shape, np.uint16)
    corr.close()
    want = case.want() if clip is None else np.clip(case.want(), *clip)
    report(name, got, want)
    for g, w in zip(got, want):
        assert_dn(g, w)


def test_u8_list_overflow(L):
    """k_fix_correct<true, uint8_t, 8> in all mode through tmh_correct_u8: 5
    uint8 sites of 512 x 512, values past 2**26 against the 8-bit wrap."""
    case = oc.plain_u8()
    print(oc.check_pixel_overflow(case))
    corr = new_corrector(case)
    got = corr.apply(case.sites)
    corr.close()
    report("u8", got, case.want(), 8)
    for g, w in zip(got, case.want()):
        assert_dn(g, w, bits=8)


@functools.lru_cache(maxsize=None)
def site_truth(case):
    """(per-site histograms, percentile sums) of a case's sites from the oracle."""
    q = np.linspace(0, 100, Q)
    hists = [orc.histogram_u16(s) for s in case.sites]
    acc = np.zeros(Q)
    for s in case.sites:
        acc += orc.percentile_linear(s, q)
    return hists, acc


def fused_jobs(L, jobs, mode):
    """jobs [(case, TMH_OPT_FUSED_CONFIG)], each with a corrector made from the
    case's planes and a statistics handle holding its sites as pending; mode:
    "single" / "blocks" (one call per job, contiguous or through a block
    table) or "multi" (tmh_correct_u16_hist_multi_device).  Returns per job
    (corrected sites, per-site histograms, pooled histogram, percentile sums,
    the configuration that ran)."""
    from tmlibrary_amd.image import ZERO_LOG10
    with contextlib.ExitStack() as stack:
        keep = stack.enter_context
        st = []
        for case, cfg in jobs:
            h = _stats_handle(L, case.H, case.W, hip.TMH_STATS_KEEP_SITE_HIST)
            hip.check(L.tmh_stats_set_option(h, hip.TMH_OPT_FUSED_CONFIG, cfg))
            d_in = keep(hip.DeviceBuffer(case.sites.nbytes))
            d_out = keep(hip.DeviceBuffer(case.sites.nbytes))
            mean, std = keep(hip.DeviceBuffer(case.npx * 8)), keep(hip.DeviceBuffer(case.npx * 8))
            d_in.put(case.sites)
            d_out.put(np.full(case.sites.shape, 0xA5A5, np.uint16))
            mean.put(case.mean)
            std.put(case.std)
            c = C.c_void_p()
            hip.check(L.tmh_corrector_create_device(mean, std, case.H, case.W, 1, ZERO_LOG10, None,
                                                    C.byref(c)))
            hip.check(L.tmh_stats_update_welford_device(h, d_in, case.n, 1, None))
            assert L.tmh_synchronize(None) == 0
            st.append((h, c, d_in, d_out))
        if mode == "multi":
            n = len(jobs)
            arr = lambda xs: (C.c_void_p * n)(*[C.c_void_p(x) for x in xs])  # noqa: E731
            hip.check(L.tmh_correct_u16_hist_multi_device(
                arr([s[1].value for s in st]), arr([s[0].value for s in st]), n,
                arr([s[2].ptr.value for s in st]), arr([s[3].ptr.value for s in st]),
                (C.c_int64 * n)(*[case.n for case, _ in jobs]), -1, -1, None))
        for (case, _), (h, c, d_in, d_out) in zip(jobs, st):
            if mode == "single":
                hip.check(L.tmh_correct_u16_hist_device(c, h, d_in, d_out, case.n, -1, -1, None))
            elif mode == "blocks":  # blocks of 4 sites (the smallest): the sites fill part of one
                assert case.n <= 4
                t_in, t_out = keep(hip.DeviceBuffer(8)), keep(hip.DeviceBuffer(8))
                t_in.put(np.array([d_in.ptr.value], np.int64))
                t_out.put(np.array([d_out.ptr.value], np.int64))
                hip.check(L.tmh_correct_u16_hist_blocks_device(c, h, t_in, t_out, 2, case.n, -1, -1,
                                                               None))
        assert L.tmh_synchronize(None) == 0
        res = []
        for (case, _), (h, c, d_in, d_out) in zip(jobs, st):
            r = _results(L, h, case.H, case.W, case.n, Q)
            sh = []
            for i in range(case.n):
                x = np.empty(65536, np.uint32)
                hip.check(L.tmh_stats_site_histogram(h, i, hip.ptr(x)))
                sh.append(x.astype(np.uint64))
            fc = C.c_int()
            hip.check(L.tmh_stats_job_choice(h, None, None, C.byref(fc)))
            res.append((d_out.get(case.sites.shape, np.uint16), sh, r["hist"], r["acc"], fc.value))
            L.tmh_corrector_destroy(c)
            L.tmh_stats_destroy(h)
    return res


def check_fused(name, case, res):
    out, site_hist, hist, acc, cfg = res
    hists, want_acc = site_truth(case)
    report("%s (configuration %d)" % (name, cfg), out, case.want())
    for g, w in zip(out, case.want()):
        assert_dn(g, w)
    for i, (a, b) in enumerate(zip(site_hist, hists)):
        assert np.array_equal(a, b), i
    assert np.array_equal(hist, sum(hists))
    assert np.array_equal(acc, want_acc), "percentile sums not bit-exact"


def test_fused_list_overflow(L):
    """k_fix_correct_jobs (apply_kernels.hip) in all mode after k_correct_hist:
    2 sites of 2160 x 2560, 1.38 M flagged groups of 8 against 2**20 entries
    (check_group_overflow) -- the units' LDS sets and their direct pushes both
    run the counter past the capacity.  Contiguous, and through a block table
    (fix_correct_body's SiteTab branch; a block is at least 4 sites, so the 2
    sites fill part of one block): outputs bit-identical, within 1 DN of the
    oracle; histograms and percentile sums bit-exact."""
    case = oc.full_size()
    print(oc.check_group_overflow(case))
    res = {m: fused_jobs(L, [(case, -1)], m)[0] for m in ("single", "blocks")}
    check_fused("contiguous", case, res["single"])
    check_fused("blocks", case, res["blocks"])
    assert np.array_equal(res["single"][0], res["blocks"][0])


def test_fused_overflow_next_to_an_ordinary_job(L):
    """k_fix_correct_jobs with two jobs in one launch (blockIdx.y), one list
    above its capacity (all mode) and one holding some thousands of entries
    (list mode), after one k_correct_hist launch for both (configuration 3
    forced on each).  The ordinary job's output must be bit-identical to its
    own single-job run; the overflowed job stays within 1 DN of the oracle."""
    big, small = oc.full_size(), oc.ordinary()
    print(oc.check_group_overflow(big))
    n_small = int(np.count_nonzero(small.flagged_groups()))
    assert 100 <= n_small < oc.fix_capacity(small.n, small.npx)
    alone = fused_jobs(L, [(small, 3)], "single")[0]
    both = fused_jobs(L, [(big, 3), (small, 3)], "multi")
    assert both[0][4] == both[1][4] == 3
    check_fused("overflowed job", big, both[0])
    check_fused("ordinary job", small, both[1])
    check_fused("ordinary job alone", small, alone)
    assert np.array_equal(both[1][0], alone[0])


@pytest.mark.parametrize("bounds", [(100, 3000), (0, 65535)])
def test_chain_list_overflow(L, keep, bounds):
    """k_fix_chain (chain_kernels.hip) in all mode after k_chain_u8t: 2 sites of
    2160 x 2560, one unshifted and one shifted by (2, -3), more flagged groups
    inside the source windows alone than the list holds (check_chain_overflow).
    All mode walks every source pixel and must map each through the site's
    window and leave the padding alone: the bytes outside the destination
    window equal the oracle's exactly, the rest within 1."""
    case = oc.full_size()
    cond, wins = oc.check_chain_overflow(case, bounds)
    print(cond)
    corr = new_corrector(case)
    d_in, d_out = keep(hip.DeviceBuffer(case.sites.nbytes)), keep(hip.DeviceBuffer(case.sites.size))
    d_in.put(case.sites)
    d_out.put(np.full(case.sites.shape, 0xA5, np.uint8))
    wins = np.ascontiguousarray(wins)
    hip.check(L.tmh_correct_chain_u8_device(corr._h, d_in, d_out, case.n, hip.ptr(wins),
                                            bounds[0], bounds[1], None))
    assert L.tmh_synchronize(None) == 0
    got = d_out.get(case.sites.shape, np.uint8)
    corr.close()
    for i, (shift, w) in enumerate(zip(oc.CHAIN_SHIFTS, wins)):
        want = orc.illuminati_chain(case.sites[i], case.mean, case.std, shift, oc.CHAIN_RESIDUES,
                                    *bounds)
        d = np.abs(got[i].astype(np.int32) - want.astype(np.int32))
        print("site %d: max |d| %d, exact %d of %d" % (i, d.max(), np.count_nonzero(d == 0), d.size))
        assert d.max() <= 1, (i, int(d.max()), int(np.count_nonzero(d > 1)))
        pad = np.ones((case.H, case.W), bool)
        r0, c0 = int(w["dst_r0"]), int(w["dst_c0"])
        pad[r0:r0 + int(w["rows"]), c0:c0 + int(w["cols"])] = False
        assert pad.any() and np.array_equal(got[i][pad], want[pad])


def test_stack_list_overflow(L):
    """k_fix_stack (chain_kernels.hip) in all mode after k_stack_px<true, true,
    0>: 5 planes of 512 x 512 as 2 sites x 3 slots with (site 1, slot 1)
    unmapped and windows at five different origins; the pass pushes 1.28 M
    pixels (those inside the windows) against 2**20 entries
    (check_stack_overflow).  All mode maps every source pixel of every plane
    through window, site and slot.  Expected: the plain correction of each
    plane, one launch per plane on a corrector of its own (262,144 pixels: its
    list does not overflow), itself within 1 DN of the oracle, cropped and
    interleaved by numpy; the stack must equal it exactly, the unmapped slot
    be 0 and the bytes around the output stay as they were."""
    import torch

    from test_gpu_jterator import expected_stack
    case = oc.plain_log()
    print(oc.check_stack_overflow(case))
    site, slot, win = oc.stack_layout()
    n_sites, (oh, ow) = 2, oc.STACK_EXTENT
    plain = new_corrector(case)
    assert case.npx <= 1 << 20
    corrected = np.stack([plain.apply(p) for p in case.sites])
    plain.close()
    for g, w in zip(corrected, case.want()):
        assert_dn(g, w)
    want = expected_stack(corrected, site, slot, win, n_sites, oc.STACK_SLOTS, 1, (oh, ow))
    corr = new_corrector(case)
    guard, n_out = 256, n_sites * oh * ow * oc.STACK_SLOTS
    d_in = torch.from_numpy(case.sites.view(np.int16)).cuda()
    buf = torch.full((guard + n_out + guard,), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    hip.check(L.tmh_correct_stack_u16_device(
        corr._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(buf.data_ptr() + 2 * guard), case.n,
        case.H, case.W, hip.ptr(site), hip.ptr(slot), hip.ptr(win), n_sites, oc.STACK_SLOTS, oh, ow,
        None))
    assert L.tmh_synchronize(None) == 0
    host = buf.cpu().numpy().view(np.uint16)
    corr.close()
    assert (host[:guard] == 0x5A5A).all() and (host[guard + n_out:] == 0x5A5A).all()
    got = host[guard:guard + n_out].reshape(want.shape)
    assert not got[1, :, :, 1].any()
    print("stack: %d of %d values differ" % (np.count_nonzero(got != want), got.size))
    assert np.array_equal(got, want)


# ---- C: a unit's LDS set full, the list not -------------------------------------------

def test_fused_unit_set_overflow(L):
    """k_correct_hist's `else fix_push8` (fused_kernels.hip, the unit's LDS set
    is full) together with wave 0's append of the staged 256 -- both routes
    into one list that does not overflow.  6 sites of 240 x 320 with every
    8-pixel group but one per site flagged: 57,594 groups against a capacity
    of 2**20.  A unit is one band of at most SPU sites: the groups
    [band * 9600 / n_bands, (band + 1) * 9600 / n_bands) of 2 or 4 sites
    (configurations 3, 5 and 100 take 4, the last unit the 2 sites left), with
    n_bands at most 64 (TMH_OPT_FUSED_BANDS; fused_bands() doubles a
    configuration's 8 or 16 up to that for short launches).  The smallest unit
    therefore holds 2 x 150 groups, less the one unflagged group of each site:
    298 > 256, and min_unit_groups() finds the same from the flagged groups
    themselves, over every band count and unit size.  Dropping the direct push
    loses at least 42 groups of every unit, most of their pixels then more
    than 1 DN off.  Outputs within 1 DN of the oracle and identical across
    configurations; histograms and percentile sums bit-exact."""
    case = oc.lds_set()
    groups = int(np.count_nonzero(case.flagged_groups()))
    assert groups == 6 * 9599 and groups < oc.fix_capacity(case.n, case.npx)
    assert oc.min_unit_groups(case) == 2 * 150 - 2 > oc.FIX_SH
    bad = case.bad_if_unrefined()
    assert 2 * np.count_nonzero(bad) >= np.count_nonzero(case.flagged())
    outs = {}
    for cfg in (3, 5, 100, -1):
        r = fused_jobs(L, [(case, cfg)], "single")[0]
        check_fused("set overflow, asked %d" % cfg, case, r)
        outs[cfg] = r[0]
    for cfg in (5, 100, -1):
        assert np.array_equal(outs[3], outs[cfg]), cfg


# ---- E: input and output must not overlap ----------------------------------------------

def _refused(L, rc):
    assert rc == hip.TMH_EINVAL
    msg = L.tmh_last_error().decode()
    assert "input and output" in msg and "must not overlap" in msg, msg
    assert L.tmh_synchronize(None) == 0


def test_correct_u16_device_refuses_overlap(L, keep):
    """tmh_correct_u16_device (abi_apply.hip): k_fix_correct re-reads the input
    after the streaming kernel stored the output, so an in-place call would be
    wrong on every flagged pixel.  In place and offset by one site either way:
    TMH_EINVAL, the buffer byte for byte as it was."""
    H, W, n = 64, 64, 2
    mean, std = oc.recipe_planes(H, W, 71, big_rows=(H // 2,))
    case = oc.Case(oc.uniform_sites(n + 1, H, W, 72, 20000, 65535), mean, std)
    corr = new_corrector(case)
    buf = keep(hip.DeviceBuffer(case.sites.nbytes))
    buf.put(case.sites)
    at = lambda k: buf.at(2 * k * case.npx)  # noqa: E731
    for i, o in ((0, 0), (0, 1), (1, 0)):
        _refused(L, L.tmh_correct_u16_device(corr._h, at(i), at(o), n, -1, -1, None))
        assert np.array_equal(buf.get(case.sites.shape, np.uint16), case.sites)
    # adjacent runs do not overlap
    assert L.tmh_correct_u16_device(corr._h, at(0), at(1), 1, -1, -1, None) == 0
    assert L.tmh_synchronize(None) == 0
    got = buf.get(case.sites.shape, np.uint16)
    assert_dn(got[1], case.want()[0])
    assert np.array_equal(got[0], case.sites[0]) and np.array_equal(got[2], case.sites[2])
    corr.close()


def test_correct_stack_device_refuses_overlap(L, keep):
    """tmh_correct_stack_u16_device (abi_chain.hip): k_fix_stack re-reads the
    planes.  The stack written over its own planes, and starting one plane in:
    TMH_EINVAL, nothing written."""
    H, W = 64, 64
    mean, std = oc.recipe_planes(H, W, 73, big_rows=(H // 2,))
    case = oc.Case(oc.uniform_sites(3, H, W, 74, 20000, 65535), mean, std)
    corr = new_corrector(case)
    site, slot = np.array([0, 0], np.int32), np.array([0, 1], np.int32)
    win = np.zeros(2, dtype=hip.WINDOW_DTYPE)
    win["src_r0"], win["src_c0"], win["rows"], win["cols"] = 2, 3, 60, 60
    buf = keep(hip.DeviceBuffer(case.sites.nbytes))
    buf.put(case.sites)
    for o in (0, 1):  # 2 planes in, 60 x 60 x 2 values out: inside 2 planes' room
        out = buf.at(2 * o * case.npx)
        _refused(L, L.tmh_correct_stack_u16_device(corr._h, buf, out, 2, H, W, hip.ptr(site),
                                                   hip.ptr(slot), hip.ptr(win), 1, 2, 60, 60, None))
        assert np.array_equal(buf.get(case.sites.shape, np.uint16), case.sites)
    corr.close()
